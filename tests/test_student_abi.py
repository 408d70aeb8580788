"""CPU: the h12student_* C ABI of the deployable ("student") observation group (include/h12student.h,
csrc/h12_student.hip) -- the exported symbols, the config struct against its ctypes mirror, the row layout, the
argument validation (every error is reported before any HIP call, so no GPU is needed), and the compiled kernel's
resource usage read from the library's gfx950 code object as tests/test_priv_abi.py reads its kernel's."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest
import yaml

from h12env import student

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "h1v2-isaac_amd" / "h12env" / "libh12env.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")
KERNEL = "student_obs_kernel"


def test_library_exports_the_student_symbols_and_the_header_declares_them():
    from h12env import build
    from h12env._abi import load_library

    lib = load_library()
    for s in ("h12student_layout", "h12student_observe", "h12student_last_error"):
        assert hasattr(lib, s), s
    assert student.STUDENT_SYMBOLS == ["h12student_layout", "h12student_observe", "h12student_last_error"]
    header = (ROOT / "include" / "h12student.h").read_text()
    assert all(re.search(rf"\b{s}\(", header) for s in student.STUDENT_SYMBOLS)
    assert build.CSRC / "h12_student.hip" in build.UNITS
    assert ROOT / "include" / "h12student.h" in build.sources()
    assert "h12student" not in (ROOT / "include" / "h12env.h").read_text()  # the env's own ABI is untouched


def test_config_struct_mirrors_the_header():
    # 2 x int32, 3 x uint32, 6 + 6 floats: 20 + 48 bytes, 4 of padding, a pointer
    assert C.sizeof(student.StudentConfig) == 80
    assert student.StudentConfig.noise.offset == 20 and student.StudentConfig.scale.offset == 44
    assert student.StudentConfig.fill_mask.offset == 72
    header = (ROOT / "include" / "h12student.h").read_text()
    body = header[header.index("typedef struct h12student_config {"):header.index("} h12student_config;")]
    names = re.findall(r"(\w+)(?:\[\w+\])?[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == ["history", "enable_corruption", "seed_lo", "seed_hi", "env_offset", "noise", "scale", "fill_mask"]
    assert names == [f[0] for f in student.StudentConfig._fields_]
    assert f"#define H12STUDENT_RNG_STREAM {student.RNG_STREAM}" in header and student.RNG_STREAM == 5
    assert len(student.TERMS) == 6 and sum(student.WIDTHS.values()) == student.FRAME == 45


@pytest.mark.parametrize("h", [1, 6, 10])
def test_layout_is_term_major(h):
    w, table = student.layout(h)
    assert w == 45 * h
    assert [t for t, _, _ in table] == list(student.TERMS)
    assert [o for _, o, _ in table] == [0, 3 * h, 6 * h, 9 * h, 21 * h, 33 * h]
    assert [k for _, _, k in table] == [student.WIDTHS[t] * h for t in student.TERMS]


def test_layout_refuses_a_history_out_of_range_and_every_output_is_optional():
    lib = student.student_library()
    for h in (0, 11, -1):
        assert lib.h12student_layout(h, None, None, None) == -1 and b"history" in lib.h12student_last_error()
    assert lib.h12student_layout(3, None, None, None) == 0


def make_cfg(**kw):
    c = student.StudentConfig()
    c.history, c.enable_corruption = 2, 1
    for i in range(6):
        c.noise[i], c.scale[i] = 0.1, 1.0
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(c, k)[v[0]] = v[1]
        else:
            setattr(c, k, v)
    return c


def test_observe_reports_bad_arguments_before_any_hip_call():
    lib = student.student_library()
    buf = (C.c_float * 2048)()
    p = C.addressof(buf)
    q = p + 4096  # a second buffer that [4][90] rows at p do not reach
    ok = make_cfg()
    cases = [
        ((None, 4, C.byref(ok), None, p, 1, None), b"workspace: null"),
        ((p + 1, 4, C.byref(ok), None, p, 1, None), b"workspace: not 4-byte aligned"),
        ((p, 0, C.byref(ok), None, p, 1, None), b"n: 0"),
        ((p, -3, C.byref(ok), None, p, 1, None), b"n: -3"),
        ((p, 4, None, None, p, 1, None), b"cfg: null"),
        ((p, 4, C.byref(make_cfg(history=0)), None, p, 1, None), b"cfg.history: 0"),
        ((p, 4, C.byref(make_cfg(history=11)), None, p, 1, None), b"cfg.history: 11"),
        ((p, 4, C.byref(make_cfg(noise=(4, -0.5))), None, p, 1, None), b"cfg.noise[4]"),
        ((p, 4, C.byref(make_cfg(noise=(1, float("nan")))), None, p, 1, None), b"cfg.noise[1]"),
        ((p, 4, C.byref(make_cfg(noise=(0, float("inf")))), None, p, 1, None), b"cfg.noise[0]"),
        ((p, 4, C.byref(make_cfg(scale=(5, float("nan")))), None, p, 1, None), b"cfg.scale[5]"),
        ((p, 4, C.byref(ok), None, None, 1, None), b"out: null"),
        ((p, 4, C.byref(ok), None, p + 2, 1, None), b"out: not 4-byte aligned"),
        ((p, 4, C.byref(ok), q + 2, p, 1, None), b"prev: not 4-byte aligned"),
        ((p, 4, C.byref(ok), p, p, 1, None), b"out: overlaps prev"),
        ((p, 4, C.byref(ok), p + 4 * 90 * 4 - 4, p, 1, None), b"out: overlaps prev"),  # by one float
        ((p, 4, C.byref(ok), p, p + 4 * 90 * 4 - 4, 1, None), b"out: overlaps prev"),
    ]
    for args, msg in cases:
        assert lib.h12student_observe(*args) == -1, msg
        assert msg in lib.h12student_last_error(), (msg, lib.h12student_last_error())


def test_python_config_follows_the_env_cfg():
    from h12env import cfg as K

    c = K.H12RoughEnvCfg()
    assert c.observations.student is None
    with pytest.raises(AttributeError):
        student.student_config(c)
    c.observations.student = K.StudentObsCfg(history_length=6)
    c.seed = (7 << 32) | 9
    s = student.student_config(c, env_offset=128)
    assert (s.history, s.enable_corruption, s.seed_lo, s.seed_hi, s.env_offset) == (6, 1, 9, 7, 128)
    assert [round(x, 6) for x in s.noise] == [0.2, 0.05, 0.0, 0.01, 1.5, 0.0]  # the Flat task's noise
    assert list(s.scale) == [1.0] * 6
    flat = K.H12FlatEnvCfg().observations.policy
    for t in student.TERMS:
        u, v = getattr(flat, t), getattr(c.observations.student, t)
        assert (u is None) == (v is None) and (u is None or (u.n_min, u.n_max) == (v.n_min, v.n_max)), t
    c.observations.student.scales = {"base_ang_vel": 0.25, "joint_vel": 0.05}
    assert list(student.student_config(c).scale) == pytest.approx([0.25, 1, 1, 1, 0.05, 1])
    c.observations.student.scales = {"height_scan": 1.0}
    with pytest.raises(ValueError, match="height_scan"):
        student.student_config(c)
    c.observations.student = K.StudentObsCfg(history_length=11)
    with pytest.raises(ValueError, match="history_length"):
        student.student_config(c)
    c.observations.student = K.StudentObsCfg(enable_corruption=False)
    assert student.student_config(c).enable_corruption == 0


def _code_objects(d: Path):
    """Every gfx950 code object of the library: its .hip_fatbin section holds one offload bundle per source file."""
    tools = [LLVM / t for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")]
    assert LIB.exists(), "libh12env.so is not built"
    if not all(t.exists() for t in tools):
        pytest.skip("the ROCm LLVM tools are missing")
    subprocess.run([str(tools[0]), f"--dump-section=.hip_fatbin={d / 'fatbin'}", str(LIB), str(d / "lib.o")],
                   check=True, capture_output=True)
    blob = (d / "fatbin").read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [i for i in range(len(blob)) if blob.startswith(magic, i)]
    out = []
    for k, s in enumerate(starts):
        part = d / f"bundle{k}"
        part.write_bytes(blob[s:starts[k + 1] if k + 1 < len(starts) else len(blob)])
        co = d / f"k{k}.co"
        subprocess.run([str(tools[1]), "--unbundle", "--type=o", f"--input={part}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True, capture_output=True)
        out.append(co)
    return out


def test_student_kernel_uses_no_scratch_and_stores_16_bytes(tmp_path):
    found = []
    for co in _code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True,
                               text=True).stdout
        md = yaml.safe_load(notes[notes.index("---"):notes.index("...", notes.index("---"))])
        found += [(k, co) for k in md["amdhsa.kernels"] if KERNEL in k[".name"]]
    assert len(found) == 1 and found[0][0][".max_flat_workgroup_size"] == 256, [k[".name"] for k, _ in found]
    kd, co = found[0]
    assert kd.get(".vgpr_spill_count", 0) == 0 and kd.get(".sgpr_spill_count", 0) == 0
    assert kd[".private_segment_fixed_size"] == 0
    assert kd[".group_segment_fixed_size"] == 0  # every LDS region is carved from the dynamic one: a 16-byte aligned base
    dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", f"--disassemble-symbols={kd['.name']}", str(co)],
                         check=True, capture_output=True, text=True).stdout
    assert dis.count("\n") > 200  # the kernel was found
    assert "scratch_" not in dis
    assert "global_store_dwordx4" in dis and "ds_read_b128" in dis  # the block's span leaves in 16-byte stores
    assert "atomic" not in dis

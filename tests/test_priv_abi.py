"""CPU: the h12priv_* C ABI of the privileged observation group (include/h12priv.h, csrc/h12_priv.hip) -- the exported
symbols, the argument validation (every error is reported before any HIP call, so no GPU is needed), the row layout
against the Python term list, and the compiled kernel's resource usage read from the library's gfx950 code object."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest
import yaml

from h12env import priv

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "h1v2-isaac_amd" / "h12env" / "libh12env.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")
KERNEL = "priv_obs_kernel"


def test_library_exports_the_priv_symbols():
    from h12env._abi import load_library

    lib = load_library()
    for s in ("h12priv_layout", "h12priv_observe", "h12priv_last_error"):
        assert hasattr(lib, s), s
    assert priv.PRIV_SYMBOLS == ["h12priv_layout", "h12priv_observe", "h12priv_last_error"]
    header = (ROOT / "include" / "h12priv.h").read_text()
    assert all(s in header for s in priv.PRIV_SYMBOLS)


def test_abi_version_and_the_env_header_are_untouched():
    from h12env._abi import ABI_VERSION, load_library

    assert ABI_VERSION == 9 and load_library().h12env_abi_version() == 9
    assert "h12priv" not in (ROOT / "include" / "h12env.h").read_text()


def test_config_struct_mirrors_the_header():
    # int32, pointer, 2 x int32, 3 floats, 2 floats, 2 x int32, 2 floats, 16 floats: the C compiler's layout of
    # h12priv_config (4 + pad 4 + 8 + 8 + 12 + 8 + 8 + 8 + 64)
    assert C.sizeof(priv.PrivConfig) == 124 + 4
    assert priv.PrivConfig.heights.offset == 8 and priv.PrivConfig.scale.offset == 60
    assert len(priv.TERMS) == 16


def test_layout_matches_the_python_term_list():
    for terrain, width in ((False, 65), (True, 252)):
        w, table = priv.layout(terrain)
        assert w == width == (priv.W_TERRAIN if terrain else priv.W_PLANE)
        names = priv.term_names(terrain)
        assert [t for t, _, _ in table] == names
        off = 0
        for name, o, k in table:
            assert (o, k) == (off, priv.WIDTHS[name]), name
            off += k
        assert off == w
        assert ("height_scan" in names) == terrain
    lib = priv.priv_library()
    assert lib.h12priv_layout(2, None, None, None) == -1 and b"terrain" in lib.h12priv_last_error()
    assert lib.h12priv_layout(0, None, None, None) == 0  # every output is optional


def test_observe_reports_bad_arguments_before_any_hip_call():
    lib = priv.priv_library()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def cfg(**kw):
        c = priv.PrivConfig()
        for i in range(len(priv.TERMS)):
            c.scale[i] = 1.0
        c.mu_static, c.mu_dynamic = 0.8, 0.6
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    terrain = dict(terrain=1, heights=p, nx=4, ny=4, hscale=0.1, scan_offset=0.5, scan_clip=1.0)
    nan_scale = cfg()
    nan_scale.scale[12] = float("nan")
    cases = [
        ((None, 4, C.byref(cfg()), None, p, None), b"workspace: null"),
        ((p, 0, C.byref(cfg()), None, p, None), b"n: 0"),
        ((p, -3, C.byref(cfg()), None, p, None), b"n: -3"),
        ((p, 4, None, None, p, None), b"cfg: null"),
        ((p, 4, C.byref(cfg()), None, None, None), b"out: null"),
        ((p, 4, C.byref(cfg()), None, p + 2, None), b"out: not 4-byte aligned"),
        ((p, 4, C.byref(cfg(terrain=1)), None, p, None), b"cfg.heights: null"),
        ((p, 4, C.byref(cfg(terrain=3)), None, p, None), b"cfg.terrain: 3"),
        ((p, 4, C.byref(cfg(**{**terrain, "nx": 1})), None, p, None), b"cfg.nx, ny"),
        ((p, 4, C.byref(cfg(**{**terrain, "hscale": 0.0})), None, p, None), b"cfg.hscale"),
        ((p, 4, C.byref(cfg(**{**terrain, "hscale": float("nan")})), None, p, None), b"cfg.hscale"),
        ((p, 4, C.byref(cfg(**{**terrain, "x0": float("inf")})), None, p, None), b"cfg.x0, y0"),
        ((p, 4, C.byref(cfg(**{**terrain, "scan_clip": -1.0})), None, p, None), b"scan_clip"),
        ((p, 4, C.byref(cfg(mu_static=float("nan"))), None, p, None), b"mu_static"),
        ((p, 4, C.byref(nan_scale), None, p, None), b"cfg.scale[12]"),
    ]
    for args, msg in cases:
        assert lib.h12priv_observe(*args) == -1, msg
        assert msg in lib.h12priv_last_error(), (msg, lib.h12priv_last_error())


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


def test_priv_kernel_uses_no_scratch_and_stores_16_bytes(tmp_path):
    found = []
    for co in _code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True,
                               text=True).stdout
        md = yaml.safe_load(notes[notes.index("---"):notes.index("...", notes.index("---"))])
        found += [(k, co) for k in md["amdhsa.kernels"] if KERNEL in k[".name"]]
    # the plane kernel (64 envs per block) and the heightfield kernel (16 envs per block)
    assert len(found) == 2 and all(k[".max_flat_workgroup_size"] == 256 for k, _ in found), [k[".name"] for k, _ in found]
    for kd, co in found:
        assert kd.get(".vgpr_spill_count", 0) == 0 and kd.get(".sgpr_spill_count", 0) == 0
        assert kd[".private_segment_fixed_size"] == 0
        assert kd[".group_segment_fixed_size"] == 0  # the staged rows are the dynamic region: a 16-byte aligned base
        dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", f"--disassemble-symbols={kd['.name']}", str(co)],
                             check=True, capture_output=True, text=True).stdout
        assert dis.count("\n") > 200  # the kernel was found
        assert "scratch_" not in dis
        assert "global_store_dwordx4" in dis and "ds_read_b128" in dis  # the block's span leaves in 16-byte stores

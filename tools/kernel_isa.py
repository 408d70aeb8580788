#!/usr/bin/env python3
"""Static ISA report of libh12env's kernels (gfx950): register allocation from the code-object metadata and
instruction counts from the compiler's own assembly.

    python tools/kernel_isa.py [kernel-name-substring ...] [--source h12_policy.hip] [--json profiles/latest_isa.json]

Builds one translation unit of csrc/ (--source, default h12env.hip) with -save-temps into a temp dir (same flags as
h12env.build), then for each kernel (of another source than h12env.hip: every kernel unless substrings are given)
prints .vgpr_count / .agpr_count / .sgpr_count / scratch, the instruction mix (VALU, v_accvgpr moves, SALU,
vector / scalar memory, s_waitcnt) and every loop body (backward branch) with its VALU count.  For the Flat step kernel
it also splits each wave role's loop (physics, helper, contact, self) at its three barriers and prints, per segment, the
instruction classes and a weighted issue-slot figure (segments_report; --json key "segments").

Register accounting on gfx950: one wave has up to 512 registers per lane, arch VGPRs first then AGPRs (unified
file; .agpr_count > 0 only when the allocator spills into AGPRs, each use costing a v_accvgpr_read/write).
rocprofv3's "VGPR_Count" / "Accum_VGPR_Count" columns report the dispatch's granule-rounded arch VGPR /
AGPR fields, which is why they can differ from the metadata here.
"""
from __future__ import annotations

import re
import subprocess
import sys
import tempfile
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd"))


DEFAULT_SOURCE = "h12env.hip"


def build_asm(tmp: Path, source: str = DEFAULT_SOURCE) -> Path:
    from h12env.build import ARCH, CSRC, FLAGS, hipcc

    # -c: the other translation units' symbols stay unresolved
    cmd = [hipcc(), *FLAGS, "-c", "-save-temps", "-o", str(tmp / "tu.o"), str(CSRC / source)]
    subprocess.run(cmd, check=True, cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    s = sorted(tmp.glob(f"*{ARCH}*.s"))
    if not s:
        raise RuntimeError("no device assembly produced")
    return s[0]


def metadata(text: str) -> dict:
    import yaml

    y = text.split("\n\t.amdgpu_metadata", 1)[1].split("\t.end_amdgpu_metadata", 1)[0]
    out = {}
    for k in yaml.safe_load(y)["amdhsa.kernels"]:
        out[k[".name"]] = {key[1:]: v for key, v in k.items() if isinstance(v, int)}
    return out


def report(text: str, name: str) -> dict:
    lines = text.splitlines()
    i0 = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[i0:i1]
    ins = [l.strip().split()[0] for l in body if l.startswith("\t") and l.strip() and not l.strip().startswith((".", ";"))]
    c = Counter(ins)
    r = {"total": len(ins), "valu": sum(v for k, v in c.items() if k.startswith("v_")),
         "accvgpr": sum(v for k, v in c.items() if k.startswith("v_accvgpr")),
         "salu": sum(v for k, v in c.items() if k.startswith("s_") and not k.startswith(("s_waitcnt", "s_load",
                                                                                          "s_buffer"))),
         "vmem": sum(v for k, v in c.items() if k.startswith(("buffer_", "global_", "flat_"))),
         "smem": sum(v for k, v in c.items() if k.startswith(("s_load", "s_buffer_load"))),
         "waitcnt": c["s_waitcnt"], "loops": []}
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB[\d_]+):", l)
        if m:
            labels[m.group(1)] = i
    for i, l in enumerate(body):
        m = re.search(r"s_cbranch_\w+\s+(\.LBB[\d_]+)|s_branch\s+(\.LBB[\d_]+)", l)
        if m:
            tgt = m.group(1) or m.group(2)
            if tgt in labels and labels[tgt] < i:
                seg = [x.strip().split()[0] for x in body[labels[tgt]:i]
                       if x.startswith("\t") and x.strip() and not x.strip().startswith((".", ";"))]
                cc = Counter(seg)
                r["loops"].append((tgt, len(seg), sum(v for k, v in cc.items() if k.startswith("v_")),
                                   sum(v for k, v in cc.items() if k.startswith("v_accvgpr")), cc["s_waitcnt"]))
    return r


# ---- per-segment issue accounting of the Flat step kernel's four wave roles
# One wave alone on a SIMD pays for every instruction it issues, not only the VALU ones (MI355X_MICROARCH.md,
# constants table, row "vector-instruction ISSUE cost": ~4 cycles per issued instruction of any kind for a lone wave,
# s_nop 0 included, and 8 for the transcendentals).  SLOT_WEIGHT is that row in units of one plain instruction; the
# scalar rows were priced in this kernel (profiles/slot_diet/slot_price.txt).
TRANS = ("v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_", "v_exp_", "v_log_")
SLOT_WEIGHT = {"trans": 2, "other": 1}
SEGMENT_NAMES = ("S->R1", "R1->R2", "R2->S")
CLASSES = ("valu", "v_mov_b32", "v_accvgpr", "trans", "ds", "vmem", "smem", "s_waitcnt", "s_nop", "exec_mask", "branch",
           "salu_other")


def _ops(lines):
    """(mnemonic, operand text) of every instruction line (directives, labels and comments skipped)."""
    out = []
    for l in lines:
        if not l.startswith("\t"):
            continue
        t = l.split(";")[0].strip()
        if t and not t.startswith("."):
            m, _, rest = t.partition(" ")
            out.append((m, rest))
    return out


def is_exec_mask(m: str, rest: str) -> bool:
    """A scalar instruction of the divergent-branch scaffolding around a predicated region: s_*_saveexec_*, and
    s_or / s_xor / s_andn2 / s_and / s_mov that write exec or keep a copy of it in an SGPR pair.  Not the vcc-destined
    forms (s_and_b64 vcc, exec, x: the condition of a wave-uniform scalar branch)."""
    if not m.startswith("s_") or m.startswith("s_cbranch"):
        return False
    if "saveexec" in m:
        return True
    ops = [o.strip() for o in rest.split(",")]
    return "exec" in ops and ops[0] != "vcc"


def classify(ops) -> dict:
    """Instruction counts per class of CLASSES (valu includes the v_mov_b32, v_accvgpr and transcendental rows) and
    the weighted issue_slots figure (SLOT_WEIGHT)."""
    c = dict.fromkeys(CLASSES, 0)
    n = 0
    for m, rest in ops:
        if m == "s_barrier":
            continue
        n += 1
        if m.startswith("v_"):
            c["valu"] += 1
            if m.startswith("v_mov_b32"):
                c["v_mov_b32"] += 1
            elif m.startswith("v_accvgpr"):
                c["v_accvgpr"] += 1
            elif m.startswith(TRANS):
                c["trans"] += 1
        elif m.startswith("ds_"):
            c["ds"] += 1
        elif m.startswith(("buffer_", "global_", "flat_", "scratch_")):
            c["vmem"] += 1
        elif m.startswith(("s_load", "s_buffer_load")):
            c["smem"] += 1
        elif m == "s_waitcnt":
            c["s_waitcnt"] += 1
        elif m == "s_nop":
            c["s_nop"] += 1
        elif m.startswith(("s_cbranch", "s_branch")):
            c["branch"] += 1
        elif is_exec_mask(m, rest):
            c["exec_mask"] += 1
        else:
            c["salu_other"] += 1
    c["instructions"] = n
    c["issue_slots"] = SLOT_WEIGHT["other"] * (n - c["trans"]) + SLOT_WEIGHT["trans"] * c["trans"]
    return c


def loop_segments(loop_lines) -> list:
    """Split one loop body (the assembly lines from the loop's label to its back-edge) at its s_barriers into the
    cyclic segments between them: with b barriers, b segments, the one that crosses the back-edge being the tail
    behind the last barrier followed by the head before the first.  The list starts at the state barrier S -- the
    barrier nearest the back-edge (it closes the physics wave's body and opens the helper roles') -- so a three-barrier
    loop gives SEGMENT_NAMES.  Each entry: the segment's lines.  Static counts: both sides of a branch count."""
    bars = [i for i, l in enumerate(loop_lines) if l.split(";")[0].strip() == "s_barrier"]
    if not bars:
        return [list(loop_lines)]
    n = len(loop_lines)
    s = min(range(len(bars)), key=lambda k: min(bars[k], n - 1 - bars[k]))
    order = bars[s:] + bars[:s]
    segs = []
    for a, b in zip(order, order[1:] + order[:1]):
        segs.append(loop_lines[a + 1:b] if b > a else loop_lines[a + 1:] + loop_lines[:b])
    return segs


def role_loops(text: str, name: str) -> dict:
    """{role: (label, loop lines)} of the Flat step kernel's four roles.  The physics wave's loop is the one with the
    most v_accvgpr moves (as physics_wave_json); the other three are the innermost AGPR-free loops with three barriers:
    the helper wave's draws the Philox blocks (most v_mul_hi_u32), the self wave's polls for its release (s_sleep),
    the contact wave's is the third."""
    lines = text.splitlines()
    i0 = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[i0:i1]
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB[\d_]+):", l)
        if m:
            labels[m.group(1)] = i
    loops = {}  # barrier positions -> (start, end): the widest loop around the same barriers
    for i, l in enumerate(body):
        m = re.search(r"s_cbranch_\w+\s+(\.LBB[\d_]+)|s_branch\s+(\.LBB[\d_]+)", l)
        tgt = m and (m.group(1) or m.group(2))
        if tgt in labels and labels[tgt] < i:
            a = labels[tgt]
            bars = tuple(k for k in range(a, i) if body[k].split(";")[0].strip() == "s_barrier")
            if len(bars) == 3 and (bars not in loops or (i - a) > loops[bars][2] - loops[bars][1]):
                loops[bars] = (tgt, a, i)
    cnt = lambda a, b, p: sum(1 for m, _ in _ops(body[a:b]) if m.startswith(p))  # noqa: E731
    phys = max(loops.values(), key=lambda x: cnt(x[1], x[2], "v_accvgpr"))
    rest = [x for x in loops.values() if x is not phys and cnt(x[1], x[2], "v_accvgpr") == 0]
    if len(rest) != 3:
        raise RuntimeError(f"expected three helper-role loops with three barriers, found {len(rest)}")
    helper = max(rest, key=lambda x: cnt(x[1], x[2], "v_mul_hi_u32"))
    self_ = max(rest, key=lambda x: cnt(x[1], x[2], "s_sleep"))
    other = [x for x in rest if x is not helper and x is not self_]
    if helper is self_ or len(other) != 1:
        raise RuntimeError("the helper / self / contact loops are not told apart by their traits")
    return {r: (x[0], body[x[1]:x[2]]) for r, x in (("physics", phys), ("helper", helper), ("contact", other[0]),
                                                    ("self", self_))}


def segments_report(text: str, name: str) -> dict:
    """{role: {"loop": label, "segments": {segment name: classify()}}} for the Flat step kernel."""
    out = {}
    for role, (label, lines) in role_loops(text, name).items():
        segs = loop_segments(lines)
        out[role] = {"loop": label, "segments": {n: classify(_ops(s)) for n, s in zip(SEGMENT_NAMES, segs)}}
    return out


def exec_mask_after_last_ds_read(seg_lines) -> list:
    """The exec-mask instructions of a segment behind its last ds_read (the physics wave's R2->S segment: behind the
    state read-back, i.e. in the integration and the joint-limit projection)."""
    ops = _ops(seg_lines)
    last = max((i for i, (m, _) in enumerate(ops) if m.startswith("ds_read")), default=-1)
    return [f"{m} {r}" for m, r in ops[last + 1:] if is_exec_mask(m, r)]


def isa_sha256(text: str) -> str:
    """sha256 of the device assembly with comments and the per-source compile-unit id (__hip_cuid_*) removed: equal
    for two sources that compile to the same machine code (e.g. after a comment-only or dead-macro edit)."""
    import hashlib
    import re

    lines = []
    for ln in text.splitlines():
        if ln.lstrip().startswith(";") or ln.startswith("\t.file") or ".ident" in ln:
            continue
        lines.append(re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", ln.split(";")[0].rstrip()))
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def physics_wave_json(text: str, meta: dict, out: Path) -> None:
    """profiles/latest_isa.json for bench.py's issue roofline: the Flat step_kernel's register allocation and the
    VALU count of its physics wave's physics-step loop, keyed by the kernel source's sha256 like latest_pmc.json.
    The physics wave is the one whose registers overflow into AGPRs, so its loop is the one with the most
    v_accvgpr moves (largest VALU count among ties); the helper / self-contact loops use none and, with the fused
    observation stores, the helper loop has more VALU than the physics loop."""
    import json

    from h12env.build import source_sha256

    name = next(k for k in meta if "step_kernelILi0E" in k)
    g, r = meta[name], report(text, name)
    top = max(r["loops"], key=lambda x: (x[3], x[2]))
    res = {"source_sha256": source_sha256(),
           "kernel": name,
           "registers": {"vgpr_count_total": g.get("vgpr_count"), "agpr_count": g.get("agpr_count"),
                         "arch_vgpr": (g.get("vgpr_count") or 0) - (g.get("agpr_count") or 0),
                         "sgpr_count": g.get("sgpr_count"), "scratch_bytes": g.get("private_segment_fixed_size"),
                         "note": "gfx950 unified file: .vgpr_count is arch + acc registers; rocprofv3's VGPR_Count "
                                 "column decodes the descriptor's granulated field with a granule of 4 instead of 8 "
                                 "(half the allocated count)"},
           "physics_step_loop": {"label": top[0], "instructions": top[1], "valu": top[2], "v_accvgpr": top[3]},
           "valu_total_static": r["valu"], "isa_sha256": isa_sha256(text),
           "segments": {"slot_weight": SLOT_WEIGHT, "roles": segments_report(text, name)}}
    out.write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", out)


def print_segments(seg: dict) -> None:
    cols = ("issue_slots", "instructions") + CLASSES
    print("  per role and barrier-to-barrier segment of one inner step (static; valu includes the next three columns):")
    print("  " + f"{'role':8} {'segment':7} " + " ".join(f"{c:>11}" for c in cols))
    for role, r in seg.items():
        for n, c in r["segments"].items():
            print("  " + f"{role:8} {n:7} " + " ".join(f"{c[k]:>11}" for k in cols))


def main():
    args = sys.argv[1:]
    js = None
    if "--json" in args:
        i = args.index("--json")
        js = Path(args[i + 1])
        del args[i:i + 2]
    source = DEFAULT_SOURCE
    if "--source" in args:
        i = args.index("--source")
        source = args[i + 1]
        del args[i:i + 2]
    if js is not None and source != DEFAULT_SOURCE:
        sys.exit(f"--json describes {DEFAULT_SOURCE}'s step kernel: not with --source {source}")
    subs = args or (["step_kernelILi0E", "obs_assemble_kernelILi10E"] if source == DEFAULT_SOURCE else [""])
    with tempfile.TemporaryDirectory() as td:
        text = build_asm(Path(td), source).read_text()
    meta = metadata(text)
    print("isa_sha256", isa_sha256(text))
    if js is not None:
        physics_wave_json(text, meta, js)
    for name, g in sorted(meta.items()):
        if not any(s in name for s in subs):
            continue
        r = report(text, name)
        print(f"{name}: vgpr {g.get('vgpr_count')} agpr {g.get('agpr_count')} sgpr {g.get('sgpr_count')} "
              f"scratch {g.get('private_segment_fixed_size')} B (spills vgpr {g.get('vgpr_spill_count', 0)} "
              f"sgpr {g.get('sgpr_spill_count', 0)})")
        print(f"  instructions {r['total']}: VALU {r['valu']} (v_accvgpr {r['accvgpr']}), SALU {r['salu']}, "
              f"VMEM {r['vmem']}, SMEM {r['smem']}, s_waitcnt {r['waitcnt']}")
        for tgt, n, v, a, w in r["loops"]:
            print(f"  loop {tgt}: {n} instructions, VALU {v}, v_accvgpr {a}, s_waitcnt {w}")
        if "step_kernelILi0E" in name:
            print_segments(segments_report(text, name))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Record tests/golden/step_planted.npz on the GPU: every output of the planted env steps of
tests/helpers/planted_step.py (Flat with self-collision; 33 and 64 envs, and a fixed-base handle), bit for bit.

    python tools/gen_step_planted_golden.py [--out tests/golden/step_planted.npz]
    H12ENV_LIB=tools/_variants/lib_<tag>.so python tools/gen_step_planted_golden.py   # from a variant library

The golden pins the kernel's results across edits that must not change them (tests/test_gpu_step_planted.py): record it
from the library BEFORE such an edit, never from the edited one.  The recording run also holds the kernel to the fp64
oracle (ForcedParity.check), so a golden is only ever written from a kernel that is right."""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in ("h1v2-isaac_amd", "oracle", "tests/helpers"):
    sys.path.insert(0, str(ROOT / p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "step_planted.npz"))
    a = ap.parse_args()
    import planted_step as PS

    out = {}
    for n, fix in PS.CASES:
        gpu, _, cl, acts, fp = PS.run_case(n, fix)
        fp.check()
        empty = [k for k, m in cl.items() if not m.any()]
        if empty:
            sys.exit(f"{PS.case_key(n, fix)}: planted classes without an env: {empty}")
        for k, v in gpu.items():
            out[f"{PS.case_key(n, fix)}_{k}"] = v
        print(PS.case_key(n, fix), "projection acts in envs", np.nonzero(acts)[0].tolist(), "|", fp.report()[:300])
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, Path(a.out).stat().st_size, "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Regenerate tests/golden/eval_safety.json: a small synthetic metrics.json and what the reference's evaluators
(biped_deploy/eval/safety_checker.py SafetyChecker, eval/eval_policy.py extract_data / check_position_limits) make of it.

    python tools/gen_golden_eval.py <path to the reference checkout>

The fixture is data only: the input records and the reference's outputs (after a JSON round trip, as its save_data
writes them).  h12env.safety restates the evaluators; tests/test_safety_host.py compares against this file.
"""
from __future__ import annotations

import json
import sys
import tempfile
import types
from dataclasses import asdict
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
OUT = ROOT / "tests" / "golden" / "eval_safety.json"
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd"))

FEET = ["left_ankle_roll_link", "right_ankle_roll_link"]


def synthetic_metrics() -> list:
    """12 joints, 40 records; planted: positions exactly on a limit, one ulp outside, well outside; foot forces at the
    weight, one ulp above, 0 (single and both feet); a joint key missing from some records; a foot key missing."""
    from h12env.safety import model_limits

    lim = model_limits()
    names = list(lim["joint_pos_limits"])
    weight = lim["total_mass_force"]
    rng = np.random.default_rng(2024)
    recs = [lim]
    prev_q, prev_tau = {}, {}
    for k in range(40):
        q = {}
        for n in names:
            lo, hi = lim["joint_pos_limits"][n]
            q[n] = float(lo + (hi - lo) * rng.uniform(0.1, 0.9))
        tau = {n: float(rng.normal(0, 20)) for n in names}
        force = {FEET[0]: float(rng.uniform(100, 500)), FEET[1]: float(rng.uniform(100, 500))}
        lo0, hi0 = lim["joint_pos_limits"][names[0]]
        lo7, hi7 = lim["joint_pos_limits"][names[7]]
        if k == 3:
            q[names[0]] = lo0                               # exactly on the lower limit: inside
        if k == 4:
            q[names[0]] = float(np.nextafter(lo0, -np.inf))  # one ulp below
        if k == 5:
            q[names[7]] = hi7                               # exactly on the upper limit: inside
        if k == 6:
            q[names[7]] = float(np.nextafter(hi7, np.inf))   # one ulp above
        if k in (10, 11, 12):
            q[names[4]] = lim["joint_pos_limits"][names[4]][1] + 0.3   # well outside, three records
        if k == 13:
            q[names[10]] = lim["joint_pos_limits"][names[10]][0] - 1.0
        if k == 15:
            force[FEET[0]] = weight                          # exactly the weight: no violation
        if k == 16:
            force[FEET[1]] = float(np.nextafter(weight, np.inf))
        if k == 17:
            force = {FEET[0]: 3.0 * weight, FEET[1]: 0.0}
        if k in (0, 1, 20, 21):
            force = {FEET[0]: 0.0, FEET[1]: 0.0}             # flight: skipped by the force average
        if k == 22:
            force = {FEET[0]: 0.0, FEET[1]: 250.0}
        if k == 25:
            force = {FEET[1]: 300.0}                         # left foot key missing
        ar = {n: tau[n] - prev_tau.get(n, tau[n]) for n in names}
        pr = {n: q[n] - prev_q.get(n, q[n]) for n in names}
        prev_q, prev_tau = dict(q), dict(tau)
        rec = {"timestamp": round(0.001 * (k + 1), 6), "base_lin_pos": [0.0, 0.0, 1.0], "base_quat_pos": [1.0, 0.0, 0.0, 0.0],
               "joint_pos": q, "base_lin_vel": [0.0, 0.0, 0.0], "base_quat_vel": [0.0, 0.0, 0.0],
               "joint_vel": {n: float(rng.normal(0, 1)) for n in names}, "applied_torques": tau,
               "foot_contact_forces": force, "action_rate": ar, "joint_pos_rate": pr}
        if k in (30, 31):                                    # a joint key missing from every per-joint dict
            for key in ("joint_pos", "joint_vel", "applied_torques", "action_rate", "joint_pos_rate"):
                del rec[key][names[2]]
        recs.append(rec)
    return recs


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_eval = Path(sys.argv[1]) / "packages" / "biped_deploy" / "biped_deploy" / "eval"
    if not ref_eval.is_dir():
        sys.exit(f"{ref_eval} not found")
    try:
        import tabulate  # noqa: F401
    except ImportError:  # only the reference's table printing needs it
        stub = types.ModuleType("tabulate")
        stub.tabulate = lambda *a, **k: ""
        sys.modules["tabulate"] = stub
    sys.path.insert(0, str(ref_eval))
    import eval_policy as ref_eval_policy
    from safety_checker import SafetyChecker

    metrics = synthetic_metrics()
    with tempfile.TemporaryDirectory() as td:
        mf = Path(td) / "metrics.json"
        mf.write_text(json.dumps(metrics, indent=2))
        chk = SafetyChecker()
        chk.check_safety(mf)
        violations = json.loads(json.dumps([asdict(v) for v in chk.safety_violations]))
        sf = Path(td) / "safety_check.json"
        sf.write_text(json.dumps(violations))
        extracted = json.loads(json.dumps(ref_eval_policy.extract_data(str(mf))))
        pos_counts = ref_eval_policy.check_position_limits(sf)
    OUT.write_text(json.dumps({"metrics": metrics, "safety_check": violations, "extract_data": extracted,
                               "position_violations": pos_counts}, indent=1) + "\n")
    print(f"wrote {OUT}: {len(metrics) - 1} records, {len(violations)} violations")


if __name__ == "__main__":
    main()

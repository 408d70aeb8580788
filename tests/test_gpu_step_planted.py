"""The step kernel on planted states that take each side of its per-env switches (tests/helpers/planted_step.py): per
joint an env beyond QHI + lproj and one beyond QLO - lproj with outward velocity and envs inside the range; the torso
corner and the knee in contact and clear of the floor; one foot in the air; a fixed-base handle.  Flat with
self-collision, 33 envs (a partial second block) and 64 envs, two env steps.

(i) every planted class occurs; (ii) state, observations, rewards, flags, applied torque and foot force are
bit-identical to tests/golden/step_planted.npz (tools/gen_step_planted_golden.py, recorded before the physics wave's
issue-slot diet: the diet may not change a bit); (iii) the same outputs agree with the fp64 oracle inside the
tolerances of tests/helpers/forced.py (env-steps off them must be threshold-sensitive in the oracle itself), applied
torque and foot force inside those of test_gpu_parity.test_contact_force_and_torque_parity."""
from pathlib import Path

import numpy as np
import pytest

import planted_step as PS

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "step_planted.npz"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("n,fix_base", PS.CASES, ids=[PS.case_key(*c) for c in PS.CASES])
def test_planted_step(gpu, golden, n, fix_base):
    gpu_out, ref, cl, acts, fp = PS.run_case(n, fix_base)
    # (i) no planted class is empty, and the limit projection acts beyond each side of the range in each leg
    counts = {k: int(m.sum()) for k, m in cl.items()}
    print("classes", counts, "projection acts in envs", np.nonzero(acts)[0].tolist())
    assert all(c > 0 for c in counts.values()), counts
    for leg in (0, 1):
        for side in ("over", "under"):
            m = np.zeros(n, bool)
            for k in range(6 * leg, 6 * leg + 6):
                m |= cl[f"joint{k}_{side}"]
            assert (m & acts).any(), (leg, side)
    inside = np.ones(n, bool)
    for k in range(12):
        inside &= cl[f"joint{k}_inside"]
    assert inside.any()
    # (ii) bit-identical to the golden
    key = PS.case_key(n, fix_base)
    for k in PS.OUTPUTS:
        want, got = golden[f"{key}_{k}"], gpu_out[k]
        assert want.shape == got.shape and want.dtype == got.dtype, k
        same = want.view(np.uint8).reshape(-1) == got.view(np.uint8).reshape(-1)
        assert same.all(), f"{key} {k}: {int((~same).sum())} bytes differ from the golden"
    # (iii) against the fp64 oracle
    fp.check()
    from forced import TOL_PHYS, phys_err

    for t in range(PS.STEPS):
        # the envs inside forced.py's tolerances in this step (the others: explained by fp.check above)
        ok = (np.abs(gpu_out["rew"][t] - ref["rew"][t]) <= 1e-3 * np.abs(ref["rew"][t]) + 1e-5) \
            & (gpu_out["term"][t] == ref["term"][t]) & (gpu_out["trunc"][t] == ref["trunc"][t])
        ok &= phys_err(gpu_out["F"][t], ref["F"][t]) <= TOL_PHYS
        ef = np.abs(gpu_out["foot_force"][t] - ref["foot_force"][t]) / (1e-2 * np.maximum(10.0, np.abs(ref["foot_force"][t])))
        et = np.abs(gpu_out["applied_torque"][t] - ref["applied_torque"][t]) \
            / (2e-3 * np.maximum(1.0, np.abs(ref["applied_torque"][t])))
        bad = ok & ((ef.max(axis=1) > 1.0) | (et.max(axis=1) > 1.0))
        print("step", t, "envs inside the tolerances", int(ok.sum()), "worst foot force / torque error (x tolerance)",
              float(ef[ok].max(initial=0.0)), float(et[ok].max(initial=0.0)))
        assert not bad.any(), (t, np.nonzero(bad)[0].tolist())

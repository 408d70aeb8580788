"""CPU: the host side of the safety report (h12env.safety, scripts/eval_policy.py).

check_safety / extract_data / check_position_limits against tests/golden/eval_safety.json (the reference evaluators'
outputs on a synthetic metrics.json, tools/gen_golden_eval.py); the MJLogger schema written from a hand-made trace; the
numpy emulation of the accumulators (tests/helpers/monitor_emulation.py) on a hand-made trace with planted violations;
eval_policy.py's tables and eval.json from canned monitor output."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from h12env import safety as S
from h12env._abi import MON, MON_WORDS, SUM_EXTRA, TRACE, TRACE_WORDS
from monitor_emulation import emulate

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd" / "scripts"))

f32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return json.loads((ROOT / "tests" / "golden" / "eval_safety.json").read_text())


def test_check_safety_equals_reference(golden, tmp_path):
    got = S.check_safety(golden["metrics"])
    assert got == golden["safety_check"]
    kinds = [v["check_type"] for v in got]
    assert kinds.count("position") == 6 and kinds.count("contact_force") == 2  # on-limit / at-weight records pass
    p = tmp_path / "metrics.json"  # the path form reads the same file the reference would
    p.write_text(json.dumps(golden["metrics"]))
    assert S.check_safety(p) == golden["safety_check"]
    assert S.check_position_limits(got) == golden["position_violations"]


def test_extract_data_equals_reference(golden):
    got = S.extract_data(golden["metrics"])
    assert got == golden["extract_data"]  # exact: same operations in the same order
    # "max_force" is the reference's running-total assignment, not a maximum
    pairs = [sum(r["foot_contact_forces"].values()) for r in golden["metrics"][1:]]
    assert got["max_force"] > max(pairs)


def hand_trace():
    """4 substeps x 2 envs; env 0 clean, env 1 with planted violations."""
    lim = S.model_limits()
    names = list(lim["joint_pos_limits"])
    lo = np.array([lim["joint_pos_limits"][n][0] for n in names], f32)
    hi = np.array([lim["joint_pos_limits"][n][1] for n in names], f32)
    tr = np.zeros((4, 2, TRACE_WORDS), f32)
    q = tr[..., TRACE["Q"][0]:TRACE["Q"][0] + 12]
    qd = tr[..., TRACE["QD"][0]:TRACE["QD"][0] + 12]
    tau = tr[..., TRACE["TAU"][0]:TRACE["TAU"][0] + 12]
    force = tr[..., TRACE["FORCE"][0]:TRACE["FORCE"][0] + 2]
    tr[..., TRACE["POS"][0] + 2] = 1.0
    tr[..., TRACE["QUAT"][0]] = 1.0
    q[:] = 0.5 * (lo + hi)
    q[1, 1, 3] = hi[3]                       # on the limit: inside
    q[2, 1, 3] = hi[3] + f32(0.25)           # outside by 0.25
    q[3, 1, 8] = lo[8] - f32(0.5)            # the mirrored leg's lower limit
    tau[:, 0, :] = [[1.0] * 12, [3.0] * 12, [2.0] * 12, [2.0] * 12]
    tau[:, 1, 5] = [0.0, 40.0, -40.0, 10.0]  # clamp 40: saturated twice
    qd[2, 1, 0] = -7.0
    force[:, 0] = [[0, 0], [100, 0], [100, 200], [0, 0]]
    force[:, 1] = [[0, 0], [900, 100], [0, 0], [50, 50]]
    return tr, lo, hi


def test_emulation_known_answers():
    tr, lo, hi = hand_trace()
    clamp = np.full(12, 40.0, f32)
    vel = np.zeros(12, f32)
    vel[0] = 5.0
    mon = emulate(tr, lo, hi, clamp, vel, 800.0)
    I = lambda name: mon[MON[name][0]:MON[name][0] + MON[name][1]]  # noqa: E731
    F = lambda name: mon.view(f32)[MON[name][0]:MON[name][0] + MON[name][1]]  # noqa: E731
    assert mon.shape == (MON_WORDS, 2)
    assert (I("SUBSTEPS")[0] == 4).all()
    assert (I("POS_VIOL_COUNT")[:, 0] == 0).all() and I("POS_VIOL_COUNT")[:, 1].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0]
    assert F("POS_EXCESS_MAX")[3, 1] == (hi[3] + f32(0.25)) - hi[3] and F("POS_EXCESS_MAX")[8, 1] == lo[8] - (lo[8] - f32(0.5))
    assert F("POS_EXCESS_MAX")[:, 0].max() == 0
    assert I("TAU_SAT_COUNT")[5, 1] == 2 and I("TAU_SAT_COUNT").sum() == 2
    assert F("TAU_ABS_MAX")[5, 1] == 40 and F("TAU_ABS_MAX")[0, 0] == 3
    # rates: the first record has rate 0; env 0: |3-1| + |2-3| + 0 = 3, max 2; env 1 joint 5: 40 + 80 + 50
    assert F("TAU_RATE_SUM")[0, 0] == 3 and F("TAU_RATE_MAX")[0, 0] == 2
    assert F("TAU_RATE_SUM")[5, 1] == 170 and F("TAU_RATE_MAX")[5, 1] == 80
    assert F("TAU_PREV")[5, 1] == 10 and F("Q_PREV")[8, 1] == lo[8] - f32(0.5)
    mid3 = (f32(0.5) * (lo + hi))[3]  # joint 3 of env 1: mid, hi, hi + 0.25, mid
    assert F("Q_RATE_MAX")[3, 1] == np.abs(mid3 - (hi[3] + f32(0.25)))
    assert F("Q_RATE_SUM")[3, 1] == (np.abs(hi[3] - mid3) + np.abs((hi[3] + f32(0.25)) - hi[3])) + np.abs(mid3 - (hi[3] + f32(0.25)))
    assert I("QD_VIOL_COUNT")[0, 1] == 1 and I("QD_VIOL_COUNT").sum() == 1 and F("QD_ABS_MAX")[0, 1] == 7
    assert F("FORCE_MAX")[:, 0].tolist() == [100, 200] and F("FORCE_MAX")[:, 1].tolist() == [900, 100]
    assert F("FORCE_SUM")[:, 0].tolist() == [200, 200] and F("FORCE_SUM")[:, 1].tolist() == [950, 150]
    assert I("FORCE_VIOL_COUNT")[:, 1].tolist() == [1, 0] and I("FORCE_VIOL_COUNT")[:, 0].tolist() == [0, 0]
    assert I("CONTACT_SUBSTEPS")[0].tolist() == [2, 2]
    assert F("FORCE_PAIR_SUM")[0].tolist() == [400, 1100] and F("FORCE_PAIR_MAX")[0].tolist() == [300, 1000]
    # persistence: two halves continued equal the whole; a zeroed env restarts with rate 0
    half = emulate(tr[2:], lo, hi, clamp, vel, 800.0, mon=emulate(tr[:2], lo, hi, clamp, vel, 800.0))
    assert (half == mon).all()
    again = mon.copy()
    again[:, 1] = 0
    again = emulate(tr[:1], lo, hi, clamp, vel, 800.0, mon=again)
    assert again.view(f32)[MON["TAU_RATE_SUM"][0] + 5, 1] == 0 and again[MON["SUBSTEPS"][0], 1] == 1
    assert again[MON["SUBSTEPS"][0], 0] == 5

    # the host fold of these accumulators and the report dict
    words = S.fold_monitor_host(mon)
    d = S.summary_from_words(words)
    names = list(d["joints"])
    assert d["num_envs"] == 2 and d["substeps"] == 8 and d["contact_substeps"] == 4
    assert d["joints"][names[3]]["pos_viol_count"] == 1 and d["joints"][names[5]]["tau_sat_count"] == 2
    assert d["joints"][names[5]]["tau_rate_avg"] == (3 + 170) / 8 and d["joints"][names[5]]["tau_rate_max"] == 80
    assert d["feet"]["left_ankle_roll_link"] == {"force_max": 900.0, "force_viol_count": 1, "force_avg": 1150 / 8}
    assert d["force_pair_avg"] == 1500 / 4 and d["force_pair_max"] == 1000
    assert (d["envs_pos_viol"], d["envs_force_viol"], d["envs_vel_viol"], d["envs_any_viol"]) == (1, 1, 1, 1)
    assert d["share_any_viol"] == 0.5
    assert words[SUM_EXTRA["ENVS"]] == 2


def test_mjlogger_schema_from_trace(tmp_path):
    tr, lo, hi = hand_trace()
    m = S.metrics_from_trace(tr[:, 1], 0.001)
    assert set(m[0]) == {"joint_pos_limits", "total_mass_force"} and len(m) == 1 + 4
    keys = {"timestamp", "base_lin_pos", "base_quat_pos", "joint_pos", "base_lin_vel", "base_quat_vel", "joint_vel",
            "applied_torques", "foot_contact_forces", "action_rate", "joint_pos_rate"}
    names = list(m[0]["joint_pos_limits"])
    for k, rec in enumerate(m[1:]):
        assert set(rec) == keys
        assert all(list(rec[x]) == names for x in ("joint_pos", "joint_vel", "applied_torques", "action_rate", "joint_pos_rate"))
        assert list(rec["foot_contact_forces"]) == S.FOOT_NAMES
        assert rec["timestamp"] == pytest.approx(0.001 * (k + 1))
        assert len(rec["base_lin_pos"]) == 3 and len(rec["base_quat_pos"]) == 4 and len(rec["base_quat_vel"]) == 3
    assert [r["applied_torques"][names[5]] for r in m[1:]] == [0.0, 40.0, -40.0, 10.0]
    assert [r["action_rate"][names[5]] for r in m[1:]] == [0.0, 40.0, -80.0, 50.0]  # signed, first 0 (MJLogger)
    assert m[2]["foot_contact_forces"] == {"left_ankle_roll_link": 900.0, "right_ankle_roll_link": 100.0}
    # the evaluators on the written file: q on the limit passes, the two planted positions and the 900 N foot do not
    mf, sf = S.write_env_logs(tmp_path, 1, m)
    v = json.loads(sf.read_text())
    assert v == S.check_safety(mf)
    assert [(x["joint_name"], x["check_type"]) for x in v] == [
        ("left_ankle_roll_link", "contact_force"), (names[3], "position"), (names[8], "position")]
    ex = S.extract_data(mf)
    assert ex["avg_force"] == 1100 / 2 and ex["max_action_rate"][names[5]] == 80


def test_eval_policy_tables_and_json_from_canned_monitor(tmp_path):
    import eval_policy

    tr, lo, hi = hand_trace()
    vel = np.zeros(12, f32)
    mon = emulate(tr, lo, hi, np.full(12, 40.0, f32), vel, 800.0)
    summary = S.summary_from_words(S.fold_monitor_host(mon))
    text = eval_policy.format_tables(summary, label="toy")
    names = list(summary["joints"])
    assert "Avg Action Rate:" in text and "Avg Force and Max Force:" in text and "Position Violations:" in text
    lines = text.splitlines()
    row = next(l for l in lines if l.startswith(f"| {names[5]} "))
    assert f"{173 / 8:.3f}" in row
    assert any(l.startswith("| Avg Force") and " 375 " in l for l in lines)
    assert any(l.startswith("| Max Force ") and " 1000 " in l for l in lines)
    viol = lines[lines.index("Position Violations:"):]
    assert sum(l.startswith("| ") for l in viol) == 1 + 2  # header + the two violating joints only
    assert "envs with any violation: 1 of 2 (50.00 %" in text
    p = eval_policy.write_eval(tmp_path / "out", summary, {"num_envs": 2})
    back = json.loads(p.read_text())
    assert back["summary"] == summary and back["run"] == {"num_envs": 2}
    # the command grid covers all 27 combinations once num_envs allows it
    g = eval_policy.command_grid(64)
    assert g.shape == (64, 3) and len({tuple(r) for r in g.tolist()}) == 27

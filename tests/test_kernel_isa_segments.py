"""CPU: tools/kernel_isa.py's per-segment issue accounting -- the splitter and the instruction classes on a hand-written
loop, then the real build of csrc/h12env.hip: every wave role of the Flat step kernel splits into the three
barrier-to-barrier segments, the physics wave's last segment has no exec-mask instruction behind its last LDS read
(the joint-limit projection and the quaternion integration are selects), and the register / scratch allocation stays
inside the bounds the issue-slot diet was accepted under."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

import kernel_isa as K  # noqa: E402

# scratch bytes (private_segment_fixed_size) of step_kernel<0..2> before the diet (commit 7b14028): the SGPR allocator's
# unused slots (tests/test_code_object.py)
PARENT_SCRATCH = {0: 68, 1: 100, 2: 0}
STEP = "_ZN12_GLOBAL__N_111step_kernelILi{}EEEvNS_7KParamsENS_9WorkspaceENS_8StepArgsE"

# a loop in the physics wave's shape: the state barrier S closes the body, so the S->R1 segment is the tail behind S
# plus the head before R1
PHYSICS_LIKE = """\
.LBB0_1:
\tv_add_f32_e32 v0, v0, v9
\tv_add_f32_e32 v0, v0, v9
\tv_sin_f32_e32 v1, v0
\tv_mov_b32_e32 v2, v1
\ts_nop 0
\ts_barrier
\tds_read2st64_b32 v[4:5], v3 offset0:1 offset1:2
\ts_waitcnt lgkmcnt(0)
\tv_pk_fma_f32 v[6:7], v[4:5], v[4:5], v[6:7]
\tv_rcp_f32_e32 v8, v6
\tv_accvgpr_write_b32 a0, v8
\ts_barrier
\tv_cmp_gt_f32_e32 vcc, 0, v8
\ts_and_saveexec_b64 s[6:7], vcc
\ts_cbranch_execz .LBB0_3
; %bb.2:
\tv_min_f32_e32 v8, 0, v8
.LBB0_3:
\ts_or_b64 exec, exec, s[6:7]
\ts_and_b64 vcc, exec, s[8:9]
\ts_cbranch_vccnz .LBB0_4
\tds_write2st64_b32 v3, v8, v8 offset0:1 offset1:2
\ts_barrier
.LBB0_4:
\ts_add_i32 s4, s4, 1
\ts_cmp_lt_i32 s4, s5
\ts_cbranch_scc1 .LBB0_1
"""


def _body(text):
    lines = text.splitlines()
    return lines[1:-1]  # between the loop's label and its back-edge


def test_splitter_and_classes_on_a_hand_written_loop():
    segs = K.loop_segments(_body(PHYSICS_LIKE))
    assert len(segs) == 3
    c = [K.classify(K._ops(s)) for s in segs]
    # S->R1: two scalar instructions behind S, then two adds, sin, mov, nop before R1
    assert c[0]["instructions"] == 7 and c[0]["valu"] == 4 and c[0]["trans"] == 1 and c[0]["v_mov_b32"] == 1
    assert c[0]["s_nop"] == 1 and c[0]["salu_other"] == 2 and c[0]["issue_slots"] == 8
    # R1->R2: read, wait, packed fma, rcp, accvgpr write
    assert c[1] == dict(K.classify([]), valu=3, trans=1, v_accvgpr=1, ds=1, s_waitcnt=1, instructions=5, issue_slots=6)
    # R2->S: compare, saveexec, execz branch, min, exec restore, vcc-destined and (not exec-mask), vccnz branch, write
    assert c[2]["valu"] == 2 and c[2]["exec_mask"] == 2 and c[2]["branch"] == 2 and c[2]["salu_other"] == 1
    assert c[2]["ds"] == 1 and c[2]["instructions"] == 8 and c[2]["issue_slots"] == 8
    # every non-barrier instruction lands in exactly one segment
    assert sum(x["instructions"] for x in c) == len([m for m, _ in K._ops(_body(PHYSICS_LIKE)) if m != "s_barrier"])
    assert K.exec_mask_after_last_ds_read(segs[1]) == []
    assert len(K.exec_mask_after_last_ds_read(segs[2])) == 2  # no ds_read in it: the whole segment counts


def test_splitter_starts_at_the_state_barrier_in_a_helper_shaped_loop():
    # the helper roles' loops open with S: rotate the body so that a barrier comes first
    body = ["\ts_barrier", "\tv_add_f32_e32 v0, v0, v1", "\ts_barrier", "\tv_add_f32_e32 v0, v0, v1",
            "\tv_add_f32_e32 v0, v0, v1", "\ts_barrier", "\ts_add_i32 s4, s4, 1", "\ts_add_i32 s4, s4, 1",
            "\ts_add_i32 s4, s4, 1", "\ts_cmp_lt_i32 s4, s5"]
    segs = K.loop_segments(body)
    assert [K.classify(K._ops(s))["valu"] for s in segs] == [1, 2, 0]
    assert K.classify(K._ops(segs[2]))["salu_other"] == 4


@pytest.fixture(scope="module")
def real(tmp_path_factory):
    try:
        from h12env.build import hipcc

        hipcc()
    except Exception:  # noqa: BLE001
        pytest.skip("hipcc is missing")
    text = K.build_asm(tmp_path_factory.mktemp("isa")).read_text()
    return text, K.metadata(text)


def test_every_role_splits_into_three_segments(real):
    text, _ = real
    seg = K.segments_report(text, STEP.format(0))
    assert set(seg) == {"physics", "helper", "contact", "self"}
    assert len({r["loop"] for r in seg.values()}) == 4
    for role, r in seg.items():
        assert tuple(r["segments"]) == K.SEGMENT_NAMES, role
        for name, c in r["segments"].items():
            assert c["instructions"] > 20 and c["issue_slots"] >= c["instructions"], (role, name, c)
    assert seg["physics"]["segments"]["R1->R2"]["v_accvgpr"] + seg["physics"]["segments"]["S->R1"]["v_accvgpr"] > 0


def test_physics_tail_has_no_exec_mask_behind_its_last_lds_read(real):
    text, _ = real
    _, lines = K.role_loops(text, STEP.format(0))["physics"]
    tail = K.loop_segments(lines)[2]
    assert any(m.startswith("ds_read") for m, _ in K._ops(tail))
    assert K.exec_mask_after_last_ds_read(tail) == []


def test_registers_and_scratch_stay_inside_the_diet_bounds(real):
    _, meta = real
    assert meta[STEP.format(0)]["vgpr_count"] <= 312
    for k, parent in PARENT_SCRATCH.items():
        g = meta[STEP.format(k)]
        assert g.get("vgpr_spill_count", 0) == 0
        assert g["private_segment_fixed_size"] <= parent, (k, g["private_segment_fixed_size"])

"""CPU: the gates of the rms_forward depth tests (tests/test_gpu_cleanrl.py) bite, shown on a numpy fp32 stand-in
for the kernel (tests/helpers/rms_emulation.py) with the GPU tests' own inputs, references and gate function.

(a) The clean stand-in stays inside the gates on every depth and late-training case: inputs and gates are attainable.
(b) Five planted errors each break a gate where the fold's geometry says they change the result:
      batch_restart        every case with more than FOLD_BATCH chunks per segment: (2049, 64), (4033, 70)
      drop_partial_batch   every case with a partial fetch batch after a segment's first: (2049, 64)
      skip_tree_top        every shape with more than nseg / 2 occupied segments: all six
      full_last_chunk      every shape with a ragged last chunk: all but (32768, 1)
      single_sample_shift  found, not derived: (4033, 70) alone (3.0x the y and mean bounds on a zero-mean column;
                           the other new shapes stay inside, at most 0.7x), (300, 450), (64, 70), (129, 70) of the
                           old shapes (1.7x, 1.2x, 1.3x): the gates resolve a rounding-level defect
    On rms_batches' d = 1 column (1e3 + 1e-2 randn, gates of 0.05 sigma and 2e-3 var) the one-row last chunk of
    (16385, 1) is invisible: skip_tree_top and full_last_chunk pass there, and skip_tree_top misses the var bound at
    (32768, 1) by a mere 1.7x with half the batch lost.  On the zero-mean column of the same shapes they miss the
    mean bound 400x / 25000x (16385) and 45000x (32768): that column is why RMS_DEPTH_CASES has the d = 1 shapes
    twice.  From a late-training state (count = 2^24 + 2) a batch weighs 1e-3 to 1e-4 of the statistics:
    (2049, 64) still rejects the four data-flow plants (16x to 105x); (16385, 1) rejects none of them on the
    standard column and only full_last_chunk (5.8x) on the zero-mean one: there it is a check of the count
    arithmetic and of the clean path at that state.
(c) The shapes the suite had before (_rms_shapes) cannot see batch_restart or drop_partial_batch on any shape:
    the stand-in with either plant is bit-identical to the clean one there.  That is the gap the depth shapes close.
"""
import functools

import numpy as np
import pytest

from rms_emulation import FOLD_BATCH, PLANTS, ROWS, RmsEmu, fold_geometry, rms_normalise, rms_update
from test_gpu_cleanrl import (EPS, RMS_DEPTH_CASES, RMS_DEPTH_SHAPES, RMS_LATE_CASES, Rms64, _rms_shapes,
                              check_rms_gates, check_rms_one_step, rms_case_batches, rms_late_case)

OLD_CASES = [(n, d, None) for n, d in dict.fromkeys(_rms_shapes())]


def test_depth_shapes_reach_the_paths_they_were_chosen_for():
    """The (chunks, per, nseg, occupied) figures of RMS_DEPTH_SHAPES, from the library's row chunk, 64 columns per
    pass and 256 folding threads.  A failure here means R or the block size changed: choose the depth shapes anew
    (tests/test_gpu_cleanrl.py), or the depth tests no longer run the second fetch batch and the wide tree."""
    from h12env._learn import rms_row_chunk

    R = rms_row_chunk()
    assert R == ROWS, "the stand-in's chunk size is not the kernel's"
    for (n, d), figures in RMS_DEPTH_SHAPES.items():
        assert fold_geometry(n, d, rows=R, block=256, cols=64) == figures, (n, d, "re-choose the depth shapes")
    per = {s: f[1] for s, f in RMS_DEPTH_SHAPES.items()}
    assert per[(2049, 64)] == FOLD_BATCH + 1 and per[(4033, 70)] == 2 * FOLD_BATCH  # one partial, two full batches
    assert all(n % R == 1 for n, _ in [(2049, 64), (4033, 70), (2113, 12), (16385, 1)])  # one-row last chunks
    for n, d in _rms_shapes():  # what the shallow shapes reach: one fetch batch, at most 3 occupied segments
        chunks, p, nseg, occupied = fold_geometry(n, d, rows=R)
        assert p <= 2 and occupied <= 3


@functools.lru_cache(maxsize=None)
def _fresh(case, plant):
    """None if the stand-in passes every gate over the four calls from the initial state, else the message."""
    n, d, kind = case
    emu, ref = RmsEmu(d, plant, EPS), Rms64(d)
    try:
        for i, xb in enumerate(rms_case_batches(n, d, kind)):
            y = emu(xb)
            y64 = ref(xb, True)
            check_rms_gates(y, emu.mean, emu.var, float(emu.count), y64, ref, f"{plant} {case} call {i}")
    except AssertionError as e:
        return str(e).splitlines()[0]
    return None


@functools.lru_cache(maxsize=None)
def _late(case, plant):
    mean, var, count, batches = rms_late_case(*case)
    try:
        for i, xb in enumerate(batches):
            before = (mean, var, count)
            mean, var, count = rms_update(xb, mean, var, count, plant)
            check_rms_one_step(rms_normalise(xb, mean, var, EPS), mean, var, float(count), xb, before,
                               f"{plant} late {case} call {i}")
    except AssertionError as e:
        return str(e).splitlines()[0]
    return None


def _identical_to_clean(case, plant):
    n, d, kind = case
    a, b = RmsEmu(d, plant, EPS), RmsEmu(d, None, EPS)
    for xb in rms_case_batches(n, d, kind):
        ya, yb = a(xb), b(xb)
        if any(s.tobytes() != t.tobytes() for s, t in ((ya, yb), (a.mean, b.mean), (a.var, b.var))):
            return False
    return True


def test_clean_stand_in_stays_inside_the_gates():
    for case in RMS_DEPTH_CASES + OLD_CASES:
        assert _fresh(case, None) is None, _fresh(case, None)
    for case in RMS_LATE_CASES:
        assert _late(case, None) is None, _late(case, None)


def _geometry(case):
    return dict(zip(("chunks", "per", "nseg", "occupied"), fold_geometry(case[0], case[1])), n=case[0], d=case[1],
                kind=case[2])


# which fresh-state cases each plant must break, from the geometry of the fold; the d = 1 standard column cannot see
# one lost or overweighted row in 16385 (module docstring)
BLIND = {(16385, 1, None)}
MUST_FAIL = {
    "batch_restart": lambda g: g["per"] > FOLD_BATCH,
    "drop_partial_batch": lambda g: g["per"] > FOLD_BATCH and g["per"] % FOLD_BATCH != 0,
    "skip_tree_top": lambda g: g["occupied"] > g["nseg"] // 2 and (g["n"], g["d"], g["kind"]) not in BLIND,
    "full_last_chunk": lambda g: g["n"] % ROWS != 0 and g["chunks"] > 1 and (g["n"], g["d"], g["kind"]) not in BLIND,
    "single_sample_shift": lambda g: (g["n"], g["d"]) in {(4033, 70), (300, 450), (64, 70), (129, 70)},
}
# the shapes each plant is required to fail on; a shape counts as failed when one of its cases fails
NAMED = {
    "batch_restart": [(2049, 64), (4033, 70)],
    "drop_partial_batch": [(2049, 64)],
    "skip_tree_top": [s for s, f in RMS_DEPTH_SHAPES.items() if f[3] > f[2] // 2],
    "full_last_chunk": [s for s in RMS_DEPTH_SHAPES if s[0] % ROWS != 0],
    "single_sample_shift": [(4033, 70)],
}
LATE_FAIL = {"batch_restart": {(2049, 64, None)}, "drop_partial_batch": {(2049, 64, None)},
             "skip_tree_top": {(2049, 64, None)}, "full_last_chunk": {(2049, 64, None), (16385, 1, 3)},
             "single_sample_shift": set()}


@pytest.mark.parametrize("plant", PLANTS)
def test_planted_error_breaks_a_gate_where_it_changes_the_result(plant):
    assert len(NAMED["skip_tree_top"]) == 6 and len(NAMED["full_last_chunk"]) == 5
    failed = {case for case in RMS_DEPTH_CASES if _fresh(case, plant) is not None}
    for shape in NAMED[plant]:
        assert any(c[:2] == shape for c in failed), (plant, shape, "not rejected")
    for case in RMS_DEPTH_CASES:
        assert (case in failed) == MUST_FAIL[plant](_geometry(case)), (plant, case, _fresh(case, plant))
    assert {case for case in RMS_LATE_CASES if _late(case, plant) is not None} == LATE_FAIL[plant], plant


@pytest.mark.parametrize("plant", PLANTS)
def test_what_the_shallow_shapes_could_see(plant):
    """(c) of the module docstring: batch_restart and drop_partial_batch do not change a bit on the old shapes."""
    for case in OLD_CASES:
        seen = _fresh(case, plant)
        assert (seen is not None) == MUST_FAIL[plant](_geometry(case)), (plant, case, seen)
    if plant in ("batch_restart", "drop_partial_batch"):
        assert all(_identical_to_clean(case, plant) for case in OLD_CASES)
        assert not any(_identical_to_clean(case, plant) for case in RMS_DEPTH_CASES if case[:2] == (2049, 64))

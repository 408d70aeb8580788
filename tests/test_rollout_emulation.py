"""CPU: the planted-record cases of the HIP row rebuild (tests/test_gpu_rollout_decode.py) bite, shown on a numpy
restatement of rollout_decode_kernel's own window algorithm (rollout_ref.decode_windowed) with the GPU tests' own
inputs and reference.

(a) The kernel's geometry (DEC_ENVS, DEC_BLOCK, DEC_WT, DEC_MAX_BLOCKS, read from csrc/h12env.hip) is what the
    stand-in and the case table assume, and every case reaches the path it was chosen for.
(b) The faithful stand-in equals decode_ref bit for bit on every GPU case (decode_ref itself is pinned to the
    CircularBuffer model by tests/test_rollout.py), and reads nothing its window did not stage.
(c) Eight planted mistakes (rollout_ref.MUTANTS): each differs from decode_ref on at least one case, and every case
    whose call spans more than one window -- B, C, E, F -- and the chunked case D, whose lead-in frames come from
    earlier chunks, is failed by the short lead-in and by the done search over the window's own rows.  One exception
    is arithmetic, not a weak case: the done search over [w0, w1) alone computes the same rows as the kernel for
    history 1 and 2 (a done step s < w0 changes a slot of row t >= w0 only if t - (H - 1) < s, i.e. H >= 3), so
    F1 and F2 are required to be bit-identical under that mutant instead.  The mutant x case table is printed.
(d) h12env_rollout_decode refuses bad arguments with the argument error and a message before any launch."""
import ctypes as C
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import rollout_ref as R
from rollout_ref import DECODE_CASES, FRAME, MUTANTS, case_calls, case_inputs, decode_windowed

ROOT = Path(__file__).resolve().parents[1]
H12_E_ARG = -1  # include/h12env.h


def test_kernel_geometry_is_what_the_cases_assume():
    src = (ROOT / "h1v2-isaac_amd" / "csrc" / "h12env.hip").read_text()
    line = re.search(r"^constexpr int DEC_ENVS\b[^;]*;", src, re.M).group(0)
    got = {k: int(v) for k, v in re.findall(r"\b(DEC_\w+)\s*=\s*(\d+)\b", line)}
    assert got == {"DEC_ENVS": 8, "DEC_BLOCK": 256, "DEC_WT": 16, "DEC_MAX_BLOCKS": 96}, \
        "the decode's geometry changed: choose the cases of rollout_ref.DECODE_CASES anew"
    assert re.search(r"\bDEC_FR\s*=\s*DEC_WT\s*\+\s*H12_NHIST\s*-\s*1\b", line)
    assert (R.DEC_ENVS, R.DEC_BLOCK, R.DEC_WT, R.DEC_MAX_BLOCKS) == (8, 256, 16, 96)
    from h12env._abi import NHIST

    assert NHIST == R.NHIST == 10 and R.DEC_FR == 25
    assert R.DEC_FR * R.DEC_ENVS <= R.DEC_BLOCK  # one thread per staged done flag


def _windows(case):
    return [len(range(t0, t1, R.DEC_WT)) for t0, t1 in case_calls(case)]


def test_cases_reach_the_paths_they_were_chosen_for():
    c = DECODE_CASES
    groups = {k: v["shards"] * -(-v["n"] // R.DEC_ENVS) for k, v in c.items()}
    assert _windows(c["A"]) == [1] and _windows(c["B"]) == [2] and _windows(c["C"]) == [3]
    assert _windows(c["E"]) == [2] and all(_windows(c[f"F{h}"]) == [2] for h in range(1, 11))
    assert case_calls(c["D"]) == [(0, 7), (7, 14), (14, 21), (21, 28), (28, 35), (35, 41)]
    assert c["B"]["n"] % R.DEC_ENVS == 1 and groups["B"] == 2                   # groups of 8 and of 1
    row = 4 * FRAME * c["C"]["H"]
    assert (c["C"]["n"] * row) % 16 == 8 and (R.DEC_ENVS * row) % 16 == 0       # shard 1: scalar stores, shard 0: float4
    assert groups["E"] == 99 > R.DEC_MAX_BLOCKS and c["E"]["n"] % R.DEC_ENVS == 5
    assert c["D"]["H"] == 6 and c["D"]["T"] % c["D"]["G"] == 6
    assert [c[f"F{h}"]["H"] for h in range(1, 11)] == list(range(1, 11)) and c["F1"]["T"] % c["F1"]["G"] == 2
    assert R.ALIAS_SMALL["T"] < R.ALIAS_SMALL["H"] - 1
    # the done patterns: every listed one exists where its step does, and nine envs see every reset around w0 = 16
    names = [s[0] for s in R.done_specs(41, 10)]
    assert len(names) == 18 and len(set(names)) == 18
    assert {"16:w0-H", "16:w0-(H-1)", "16:w0-1", "16:w0", "never", "every", "first", "last", "three"} <= set(names[:9])
    assert [s[0] for s in R.done_specs(24, 10) if s[0].startswith("32:")] == []
    for name, case in c.items():
        d = case_inputs(case)
        assert set(np.unique(d["terminated"])) | set(np.unique(d["truncated"])) <= {0, 1}, name
        specials = np.isin(d["frames"], R.SPECIAL_WORDS).mean()
        assert d["frames"].size < 50000 or 0.005 < specials < 0.02, (name, specials)  # about 1 % (C, D, E: enough words)
    d = case_inputs(c["C"])
    for k, (te, tr) in {"terminated": (1, 0), "truncated": (0, 1), "both": (1, 1)}.items():
        j = [s[0] for s in R.done_specs(41, 10)].index(k)
        assert d["terminated"][:, j].any() == bool(te) and d["truncated"][:, j].any() == bool(tr), k
        assert d["done"][:, j].any()


def test_decode_ref_keeps_every_bit_pattern():
    """On uint32 views decode_ref is a gather of words; on float32 it gives the same bits as before wherever the
    words are ordinary numbers (existing callers)."""
    d = case_inputs(DECODE_CASES["B"])
    assert d["ref"].dtype == np.uint32 and np.isin(d["ref"], d["frames"]).sum() + np.isin(d["ref"], d["tail"]).sum() >= d["ref"].size
    rng = np.random.default_rng(3)
    f = rng.normal(size=(24, 9, FRAME)).astype(np.float32)
    tl = rng.normal(size=(9, FRAME * 10)).astype(np.float32)
    a = R.decode_ref(f, d["done"], tl, 10)
    b = R.decode_ref(f.view(np.uint32), d["done"], tl.view(np.uint32), 10)
    assert a.dtype == np.float32 and a.view(np.uint32).tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _emulated(name, mutant):
    """The case's rows from the stand-in, over the case's own calls into a sentinel-filled buffer."""
    case = DECODE_CASES[name]
    d = case_inputs(case)
    out = np.full(d["ref"].shape, R.SENTINEL, np.uint32)
    for t0, t1 in case_calls(case):
        decode_windowed(d["records"], case["shards"], case["n"], case["T"], case["G"], case["H"], t0, t1, d["tail"],
                        out, d["layout"], mutant)
    return out


def _caught(name, mutant):
    return _emulated(name, mutant).tobytes() != case_inputs(DECODE_CASES[name])["ref"].tobytes()


@pytest.mark.parametrize("name", list(DECODE_CASES))
def test_faithful_stand_in_equals_the_closed_form(name):
    np.testing.assert_array_equal(_emulated(name, None), case_inputs(DECODE_CASES[name])["ref"])


def test_faithful_stand_in_on_sub_ranges_and_an_aliased_tail():
    """The GPU tests' other calls: row ranges that are no whole chunk (only their rows are written), and a second
    rollout whose tail is the first one's last row, in the output buffer itself."""
    case = DECODE_CASES["B"]
    d = case_inputs(case)
    for t0, t1 in [(0, 1), (3, 20), (15, 17), (16, 17), (23, 24)]:
        out = np.full(d["ref"].shape, R.SENTINEL, np.uint32)
        decode_windowed(d["records"], 1, case["n"], case["T"], case["G"], case["H"], t0, t1, d["tail"], out, d["layout"])
        want = np.full_like(out, R.SENTINEL)
        want[t0:t1] = d["ref"][t0:t1]
        np.testing.assert_array_equal(out, want)
    case = R.ALIAS_SMALL
    first, second = case_inputs(case, 0), case_inputs(case, 1)
    out = first["ref"].copy()
    for t0, t1 in case_calls(case):
        decode_windowed(second["records"], case["shards"], case["n"], case["T"], case["G"], case["H"], t0, t1,
                        out[case["T"] - 1], out, second["layout"])
    np.testing.assert_array_equal(out, R.decode_ref(second["frames"], second["done"], first["ref"][-1], case["H"]))


MULTI_WINDOW = ["B", "C", "E"] + [f"F{h}" for h in range(1, 11)]
EQUIVALENT = {("done_in_window_rows", "F1"), ("done_in_window_rows", "F2")}  # module docstring (c)


def test_every_planted_mistake_is_caught():
    assert len(MUTANTS) >= 6 and MUTANTS[:2] == ("short_lead_in", "done_in_window_rows")
    assert all(max(_windows(DECODE_CASES[n])) > 1 for n in MULTI_WINDOW)
    names = list(DECODE_CASES)
    print("\nmutant x case (X: differs from decode_ref, .: identical)")
    print(f"{'':22s}" + " ".join(f"{n:>3s}" for n in names))
    for m in MUTANTS:
        print(f"{m:22s}" + " ".join(f"{'X' if _caught(n, m) else '.':>3s}" for n in names))
    for m in MUTANTS:
        assert any(_caught(n, m) for n in names), (m, "no case notices it")
    for m in MUTANTS[:2]:
        for n in MULTI_WINDOW + ["D"]:
            if (m, n) in EQUIVALENT:
                assert not _caught(n, m), (m, n, "expected to be the same computation")
            else:
                assert _caught(n, m), (m, n, "change the case's done pattern")
    # where each of the others must show: the clamp, the tail slot and the truncated flag in every case with more than
    # one row; the last chunk's length where a shard other than 0 has a short last chunk; the group base where a later
    # shard follows a ragged one; the flags' env offset wherever a shard has a second group
    for n in names:
        c = DECODE_CASES[n]
        assert _caught(n, "no_clamp") == (c["T"] > 1 and c["H"] > 1), n
        assert _caught(n, "tail_offset_t") == (c["H"] > 1), n
        assert _caught(n, "ignore_truncated") == (c["T"] > 1 and c["H"] > 1), n
        assert _caught(n, "last_chunk_len_G") == (c["shards"] > 1 and c["T"] % c["G"] != 0), n
        assert _caught(n, "group_base_padded") == (c["shards"] > 1 and c["n"] % R.DEC_ENVS != 0), n
        assert _caught(n, "flags_without_e0") == (c["n"] > R.DEC_ENVS and c["H"] > 1), n


def test_one_window_calls_cannot_see_the_window_mistakes():
    """What the suite had before: calls of at most 5 rows from step 0 of a rollout whose chunks the env had just
    produced.  On case B's records, the first chunk of five rows is blind to both window mistakes; the gap the
    multi-window cases close."""
    case = DECODE_CASES["B"]
    d = case_inputs(case)
    for m in MUTANTS[:2]:
        out = np.full(d["ref"].shape, R.SENTINEL, np.uint32)
        decode_windowed(d["records"], 1, case["n"], case["T"], case["G"], case["H"], 0, 5, d["tail"], out, d["layout"], m)
        assert out[:5].tobytes() == d["ref"][:5].tobytes(), m


# ---------------------------------------------------------------- argument refusals (no launch: each returns first)
def _decode_rc(**kw):
    from h12env._abi import load_library

    lib = load_library()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)  # never dereferenced: every call below returns before the launch
    a = dict(records=p, n_shards=2, n=9, T=24, G=6, history=10, t0=0, t1=24, tail=p, obs_out=p)
    a.update(kw)
    rc = lib.h12env_rollout_decode(a["records"], a["n_shards"], a["n"], a["T"], a["G"], a["history"], a["t0"], a["t1"],
                                   a["tail"], a["obs_out"], None)
    return rc, (lib.h12env_last_error() or b"").decode()


@pytest.mark.parametrize("bad,word", [
    (dict(history=0), "history 0"), (dict(history=11), "history 11"),
    (dict(t0=-1), "rows [-1, 24)"), (dict(t1=25), "rows [0, 25)"), (dict(t0=7, t1=6), "rows [7, 6)"),
    (dict(n_shards=0), ">= 1"), (dict(n=0), ">= 1"), (dict(T=0, t1=0), ">= 1"), (dict(G=0), ">= 1"),
    (dict(records=None), "required"), (dict(tail=None), "required"), (dict(obs_out=None), "required"),
])
def test_decode_refuses_bad_arguments(bad, word):
    rc, msg = _decode_rc(**bad)
    assert rc == H12_E_ARG and word in msg, (bad, rc, msg)


def test_decode_of_an_empty_range_returns_zero():
    for t in (0, 3, 24):
        assert _decode_rc(t0=t, t1=t)[0] == 0

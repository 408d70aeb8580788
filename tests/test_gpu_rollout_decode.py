"""GPU: the HIP row rebuild (rollout_decode_kernel, h12env.rollout.decode) on planted records, at every window path.

The rebuild is a gather, so every output word has one correct bit pattern: each test compares uint32 views against
rollout_ref.decode_ref, with no tolerance.  No env and no subprocess: the records are built on the host
(rollout_ref.plant) from random bit patterns (about 1 % NaNs with payloads, signed zeros, infinities, denormals) and
done flags whose env columns cycle through a fixed list (rollout_ref.done_specs: never, every step, first, last,
three in a row, terminated / truncated / both, single resets at w0 - H, w0 - (H - 1), w0 - 1 and w0 of the windows
at 16 and 32, random at 0.15 and 0.5).  Every output buffer is filled with a sentinel and sits between two guard
rows; rows outside [t0, t1) and the guard rows must still hold the sentinel afterwards.

The shapes are rollout_ref.DECODE_CASES (what each reaches is written there); tests/test_rollout_emulation.py shows
on the CPU that they catch eight planted mistakes in the kernel's algorithm, the window ones in every multi-window
case.  Beyond the cases: sub-ranges of rows, the tail aliasing the output's last row over two rollouts (as
RolloutGather._last_row does), output and tail bases 4 bytes off a 16-byte boundary, and repeatability."""
import numpy as np
import pytest
import torch

from rollout_ref import ALIAS_SMALL, DECODE_CASES, SENTINEL, case_calls, case_inputs, decode_ref

pytestmark = pytest.mark.gpu


def _words(a: np.ndarray, gpu, lead: int = 0) -> torch.Tensor:
    """The words of a uint32 array as a contiguous fp32 device tensor that starts ``lead`` words into its allocation."""
    buf = torch.empty(lead + a.size, dtype=torch.int32, device=gpu)
    buf[lead:].copy_(torch.from_numpy(a.view(np.int32).reshape(-1).copy()))
    return buf[lead:].view(torch.float32).view(a.shape)


def _guarded(case, gpu, lead: int = 0) -> torch.Tensor:
    """(T + 2, N_global, 45H) fp32 sentinel words: the output rows between one guard row before and one after."""
    T, NG, row = case["T"], case["shards"] * case["n"], 45 * case["H"]
    buf = torch.full((lead + (T + 2) * NG * row,), int(np.uint32(SENTINEL).view(np.int32)), dtype=torch.int32,
                     device=gpu)
    return buf[lead:].view(torch.float32).view(T + 2, NG, row)


def _decode(case, records, calls, tail, guarded):
    from h12env.rollout import decode

    T = case["T"]
    for t0, t1 in calls:
        decode(records, case["shards"], case["n"], T, case["G"], case["H"], t0, t1, tail, guarded[1:T + 1])


def _host(guarded: torch.Tensor) -> np.ndarray:
    return guarded.view(torch.int32).cpu().numpy().view(np.uint32)


def _expect(ref: np.ndarray, calls) -> np.ndarray:
    """The guarded buffer after the calls: the reference's rows where a call covers them, the sentinel elsewhere."""
    want = np.full((ref.shape[0] + 2,) + ref.shape[1:], SENTINEL, np.uint32)
    for t0, t1 in calls:
        want[1 + t0:1 + t1] = ref[t0:t1]
    return want


def _assert_words(got: np.ndarray, want: np.ndarray, what):
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        t, e, col = bad[0]
        pytest.fail(f"{what}: {len(bad)} words differ, first at (t, env, col) = ({t - 1}, {e}, {col}) "
                    f"[t = -1 / T: a guard row]: got {got[t, e, col]:#010x}, want {want[t, e, col]:#010x}")


def _run_case(gpu, case, lead=0, variant=0):
    d = case_inputs(case, variant)
    g = _guarded(case, gpu, lead)
    calls = case_calls(case)
    _decode(case, torch.from_numpy(d["records"].copy()).to(gpu), calls, _words(d["tail"], gpu, lead), g)
    return _host(g), _expect(d["ref"], calls)


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_planted_case(gpu, name):
    got, want = _run_case(gpu, DECODE_CASES[name])
    _assert_words(got, want, name)


@pytest.mark.parametrize("H", range(1, 11))
def test_every_instantiated_history(gpu, H):
    got, want = _run_case(gpu, DECODE_CASES[f"F{H}"])
    _assert_words(got, want, f"history {H}")


@pytest.mark.parametrize("t0,t1", [(0, 1), (3, 20), (15, 17), (16, 17), (23, 24)])
def test_sub_range_writes_exactly_its_rows(gpu, t0, t1):
    case = DECODE_CASES["B"]
    d = case_inputs(case)
    g = _guarded(case, gpu)
    _decode(case, torch.from_numpy(d["records"].copy()).to(gpu), [(t0, t1)], _words(d["tail"], gpu), g)
    _assert_words(_host(g), _expect(d["ref"], [(t0, t1)]), f"rows [{t0}, {t1})")


@pytest.mark.parametrize("name", ["B", "small"])
def test_tail_aliasing_the_output(gpu, name):
    """Two consecutive rollouts into one buffer, the second with tail = obs_out[T - 1] (RolloutGather._last_row):
    its rows must be the reference's fed the first rollout's last row.  At the small shape T < H - 1, so every chunk
    of the second rollout reads the tail, the last one while it overwrites that very row."""
    case = DECODE_CASES["B"] if name == "B" else ALIAS_SMALL
    T, H = case["T"], case["H"]
    first, second = case_inputs(case, 0), case_inputs(case, 1)
    calls = case_calls(case)
    g = _guarded(case, gpu)
    _decode(case, torch.from_numpy(first["records"].copy()).to(gpu), calls, _words(first["tail"], gpu), g)
    _assert_words(_host(g), _expect(first["ref"], calls), f"{name}: first rollout")
    _decode(case, torch.from_numpy(second["records"].copy()).to(gpu), calls, g[T], g)
    want = decode_ref(second["frames"], second["done"], first["ref"][T - 1], H)
    assert want.tobytes() != second["ref"].tobytes()  # the tail matters
    _assert_words(_host(g), _expect(want, calls), f"{name}: second rollout")


@pytest.mark.parametrize("name", ["B", "C"])
def test_unaligned_bases(gpu, name):
    """obs_out and tail are contiguous views that start 4 bytes into their allocations."""
    case = DECODE_CASES[name]
    got, want = _run_case(gpu, case, lead=1)
    _assert_words(got, want, name)
    g = _guarded(case, gpu, 1)
    assert g.data_ptr() % 16 == 4 and _words(case_inputs(case)["tail"], gpu, 1).data_ptr() % 16 == 4


def test_second_call_gives_identical_bits(gpu):
    case = DECODE_CASES["E"]
    d = case_inputs(case)
    rec, tail = torch.from_numpy(d["records"].copy()).to(gpu), _words(d["tail"], gpu)
    g = _guarded(case, gpu)
    _decode(case, rec, case_calls(case), tail, g)
    once = _host(g)
    _decode(case, rec, case_calls(case), tail, g)
    twice = _host(g)
    other = _guarded(case, gpu)
    _decode(case, rec, case_calls(case), tail, other)
    _assert_words(once, _expect(d["ref"], case_calls(case)), "E")
    assert once.tobytes() == twice.tobytes() == _host(other).tobytes()

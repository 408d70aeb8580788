"""CPU: the safety monitor's C ABI -- the three entry points are exported, the H12_MON_* / H12_TRACE_* / H12_SUM_*
tables of include/h12env.h equal the _abi.py mirror, h12env_monitor_layout returns the sizes they imply, and the entry
points reject bad arguments before any HIP call (there is no GPU here) with a message naming the field."""
import ctypes as C
import re
from pathlib import Path

import pytest

from h12env import _abi
from h12env._abi import load_library

ROOT = Path(__file__).resolve().parents[1]


def header_enums():
    """Every enumerator of include/h12env.h with its value (C rules: previous + 1 unless assigned)."""
    src = (ROOT / "include" / "h12env.h").read_text()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    vals = {}
    for body in re.findall(r"enum\s*\{(.*?)\}", src, flags=re.S):
        nxt = 0
        for item in (x.strip() for x in body.split(",")):
            if not item:
                continue
            name, _, expr = (p.strip() for p in item.partition("="))
            v = eval(expr, {}, vals) if expr else nxt  # expressions only name earlier enumerators
            vals[name] = v
            nxt = v + 1
    return vals


def test_symbols_exported():
    lib = load_library()
    for name in ("h12env_monitor_layout", "h12env_step_physics_monitored", "h12env_monitor_reduce"):
        assert name in _abi.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    assert lib.h12env_abi_version() == 9  # additive


def test_tables_equal_python_mirror():
    E = header_enums()
    mon = {k[len("H12_MON_"):]: v for k, v in E.items() if k.startswith("H12_MON_") and "LIMIT" not in k}
    assert mon.pop("WORDS") == _abi.MON_WORDS
    assert mon == {k: off for k, (off, _) in _abi.MON.items()}
    # the fields tile [0, WORDS) without gaps, in the mirror's (offset, count) pairs
    end = 0
    for name, (off, cnt) in sorted(_abi.MON.items(), key=lambda kv: kv[1][0]):
        assert off == end, name
        end = off + cnt
    assert end == _abi.MON_WORDS
    tr = {k[len("H12_TRACE_"):]: v for k, v in E.items() if k.startswith("H12_TRACE_")}
    assert tr.pop("WORDS") == _abi.TRACE_WORDS == 3 + 4 + 3 + 3 + 12 + 12 + 12 + 2
    assert tr == {k: off for k, (off, _) in _abi.TRACE.items()}
    sm = {k[len("H12_SUM_"):]: v for k, v in E.items() if k.startswith("H12_SUM_")}
    assert sm.pop("WORDS") == _abi.SUM_WORDS
    assert sm == _abi.SUM_EXTRA
    assert (E["H12_MON_LIMIT_QD"], E["H12_MON_LIMIT_FORCE"], E["H12_MON_LIMIT_WORDS"]) == \
        (_abi.MON_LIMIT_QD, _abi.MON_LIMIT_FORCE, _abi.MON_LIMIT_WORDS)
    assert set(_abi.MON_COUNTS) | set(_abi.MON_SUMS) | set(_abi.MON_PREV) <= set(_abi.MON)


@pytest.mark.parametrize("n,n_trace,n_sub", [(1, 0, 0), (37, 37, 60), (4096, 1, 20), (4097, 2, 20), (200000, 0, 20)])
def test_layout_sizes(n, n_trace, n_sub):
    lib = load_library()
    E = header_enums()
    mb, tb, sb = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.h12env_monitor_layout(n, n_trace, n_sub, C.byref(mb), C.byref(tb), C.byref(sb)) == 0
    assert mb.value == E["H12_MON_WORDS"] * n * 4
    assert tb.value == n_sub * n_trace * E["H12_TRACE_WORDS"] * 4
    # the summary record, then one partial record per block of max(64, ceil(n / 1024)) envs
    chunk = max(64, -(-n // 1024))
    assert sb.value == (1 + -(-n // chunk)) * E["H12_SUM_WORDS"] * 8


def test_layout_rejects_bad_arguments():
    lib = load_library()
    z = C.c_size_t()
    for args, word in (((0, 0, 0), "n_envs"), ((4, -1, 0), "n_trace"), ((4, 5, 0), "n_trace"), ((4, 0, -1), "n_substeps")):
        assert lib.h12env_monitor_layout(*args, C.byref(z), C.byref(z), C.byref(z)) == -1
        assert word in lib.h12env_last_error().decode()


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    lib = load_library()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    step = lib.h12env_step_physics_monitored
    #            h     q_ref n  monitor limits trace env0 n_trace
    cases = [((None, p, 20, p, p, None, 0, 0), "null handle"),
             ((None, None, 20, p, p, None, 0, 0), "q_ref"),
             ((None, p, -1, p, p, None, 0, 0), "n_substeps"),
             ((None, p, 20, None, p, None, 0, 0), "monitor"),
             ((None, p, 20, p, None, None, 0, 0), "limits"),
             ((None, p, 20, p, p, p, 0, -1), "n_trace"),
             ((None, p, 20, p, p, p, -1, 1), "trace_env0"),
             ((None, p, 20, p, p, None, 0, 1), "trace is required"),
             # a range past the largest env count of any handle is beyond n whatever the handle
             ((None, p, 20, p, p, p, 2 ** 31 - 2, 2 ** 31 - 2), "beyond n")]
    for args, word in cases:
        assert step(*args, None) == -1, word
        assert word in lib.h12env_last_error().decode(), (word, lib.h12env_last_error())
    red = lib.h12env_monitor_reduce
    for args, word in (((None, p, p), "null handle"), ((None, None, p), "monitor"), ((None, p, None), "summary")):
        assert red(*args, None) == -1
        assert word in lib.h12env_last_error().decode()

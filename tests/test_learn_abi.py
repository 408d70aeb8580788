"""CPU: libh12env.so exports every h12learn_* function include/h12learn.h declares, the env ABI is untouched, the
build knows the new translation unit, and the entry points validate their arguments before any HIP call."""
import ctypes as C
import re
from pathlib import Path

from h12env import build
from h12env._abi import LIB_PATH, load_library
from h12env._learn import LEARN_SYMBOLS, learn_library

ROOT = Path(__file__).resolve().parents[1]


def header_functions():
    src = (ROOT / "include" / "h12learn.h").read_text()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(h12learn_[a-z_]+)\s*\(", src)))


def test_library_exports_learn_header_symbols():
    assert LIB_PATH.exists(), "build the extension first (__graft_entry__.build())"
    lib = load_library()
    names = header_functions()
    assert set(names) == set(LEARN_SYMBOLS), (names, LEARN_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.h12env_abi_version() == 9


def test_build_sources_list_the_new_files():
    names = {p.name for p in build.sources()}
    assert {"h12_learn.hip", "h12learn.h", "h12env.hip", "h12env.h"} <= names
    assert all(p.exists() for p in build.sources())


def test_workspace_query_and_argument_validation_without_gpu():
    lib = learn_library()
    R = lib.h12learn_rms_row_chunk()
    assert R >= 1
    assert lib.h12learn_rms_workspace_bytes(0, 5) == 0 and lib.h12learn_rms_workspace_bytes(5, 0) == 0
    one = lib.h12learn_rms_workspace_bytes(R, 70)
    assert lib.h12learn_rms_workspace_bytes(1, 70) == one
    assert lib.h12learn_rms_workspace_bytes(R + 1, 70) == 2 * one - 64  # a 64-byte header + per-chunk partials
    # null pointers / empty shapes are rejected before anything is launched
    assert lib.h12learn_rms_forward(None, None, None, None, None, 4, 4, 1e-8, 1, None, 0, None) == -1
    assert b"null" in lib.h12learn_last_error()
    buf = (C.c_float * 4)()
    p = C.addressof(buf)
    assert lib.h12learn_rms_forward(p, p, p, p, p, 0, 4, 1e-8, 0, None, 0, None) == -1
    assert b"n = 0" in lib.h12learn_last_error()
    assert lib.h12learn_rms_forward(p, p, p, p, p, 1, 4, 1e-8, 1, None, 0, None) == -1
    assert b"workspace" in lib.h12learn_last_error()
    assert lib.h12learn_gae_soft(p, p, p, p, p, p, p, 0.99, 0.94, 0, 4, p, p, None) == -1
    assert b"T = 0" in lib.h12learn_last_error()

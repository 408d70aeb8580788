"""CPU: the h12learn_lstm_* entry points (csrc/h12_policy_rnn.hip) are declared, bound and exported, their structs have
the C layout, and every invalid argument returns H12LEARN_E_ARG with a message before anything touches a device."""
import ctypes as C
import re
from pathlib import Path

from h12env import _learn, build
from h12env._abi import load_library
from h12env._learn import LEARN_SYMBOLS, LstmDesc, LstmIo, MlpDesc, learn_library

ROOT = Path(__file__).resolve().parents[1]
LSTM_NAMES = {"h12learn_lstm_max_hidden", "h12learn_lstm_packed_bytes", "h12learn_lstm_pack", "h12learn_lstm_step"}


def shape_desc(d_in, hidden, mlps, ptr=0):
    """A descriptor of the given shapes with every pointer set to ``ptr`` (never dereferenced on the host)."""
    d = LstmDesc()
    d.d_in, d.hidden = d_in, hidden
    d.mlp.n_nets, d.mlp.d_in = len(mlps), hidden
    for i, dims in enumerate(mlps[:_learn.MLP_MAX_NETS]):
        if i < _learn.LSTM_MAX_NETS:
            c = d.cells[i]
            c.w_ih = c.w_hh = c.b_ih = c.b_hh = ptr or None
        d.mlp.nets[i].n_layers = len(dims) - 1
        for k, w in enumerate(dims):
            d.mlp.nets[i].dims[k] = w
        for k in range(len(dims) - 1):
            d.mlp.nets[i].W[k] = d.mlp.nets[i].b[k] = ptr or None
    return d


def test_header_bindings_exports_and_layout():
    src = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "h12learn.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(h12learn_[a-z_]+)\s*\(", src))
    assert LSTM_NAMES <= declared and LSTM_NAMES <= set(LEARN_SYMBOLS)
    lib = load_library()
    for n in LSTM_NAMES:
        assert hasattr(lib, n), n
    assert "h12_policy_rnn.hip" in {p.name for p in build.sources()}
    assert C.sizeof(LstmDesc) == 32 + 2 * 32 + C.sizeof(MlpDesc)  # the C structs' layout on LP64
    assert C.sizeof(LstmIo) == 24 + 5 * 2 * 8
    assert "h_out == h_in and c_out == c_in (in place) is" in " ".join((ROOT / "include" / "h12learn.h").read_text().split())


def test_max_hidden_and_packed_bytes():
    lib = learn_library()
    assert lib.h12learn_lstm_max_hidden() == 256
    assert lib.h12learn_lstm_packed_bytes(None) == 0 and b"desc" in lib.h12learn_last_error()
    one = lib.h12learn_lstm_packed_bytes(C.byref(shape_desc(450, 256, [[256, 512, 256, 128, 12]])))
    two = lib.h12learn_lstm_packed_bytes(C.byref(shape_desc(450, 256, [[256, 512, 256, 128, 12],
                                                                       [256, 512, 256, 128, 1]])))
    # x padded to 464 and h to 256 columns, 1024 gate rows and their bias, then the MLP as mlp_pack lays it out
    mlp = lib.h12learn_mlp_packed_bytes(C.byref(shape_desc(450, 256, [[256, 512, 256, 128, 12]]).mlp))
    assert mlp > 0 and one == 4 * ((464 + 256) * 1024 + 1024) + mlp
    assert one < two < 2 * one + 1 and one % 16 == 0
    # the K axis is padded per segment
    small = lib.h12learn_lstm_packed_bytes(C.byref(shape_desc(3, 24, [[24, 12]])))
    assert small == 4 * ((16 + 32) * 96 + 96 + 32 * 16 + 16)


def test_argument_validation_without_gpu():
    lib = learn_library()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    good = [[8, 6, 3]]

    def io_of(n=4, x=p, nets=2, **null):
        io = LstmIo()
        io.x, io.n = x, n
        for i in range(nets):
            for name in ("h_in", "c_in", "h_out", "c_out", "y"):
                getattr(io, name)[i] = None if null.get(name) == i else p
        return io

    def step(desc, packed=p, io=None, no_io=False):
        io = io_of() if io is None else io
        return lib.h12learn_lstm_step(C.byref(desc) if desc is not None else None, packed,
                                      None if no_io else C.byref(io), None)

    def pack(desc, packed=p):
        return lib.h12learn_lstm_pack(C.byref(desc) if desc is not None else None, packed, None)

    def err():
        return lib.h12learn_last_error()

    ok = shape_desc(5, 8, good, p)
    assert step(None) == -1 and b"desc is null" in err()
    assert pack(None) == -1 and b"desc is null" in err()
    assert step(shape_desc(5, 8, [], p)) == -1 and b"n_nets = 0" in err()
    three = shape_desc(5, 8, good * 3, p)
    assert step(three) == -1 and b"n_nets = 3" in err()
    assert pack(three) == -1 and b"n_nets = 3" in err()
    assert lib.h12learn_lstm_packed_bytes(C.byref(three)) == 0 and b"n_nets = 3" in err()
    big = lib.h12learn_lstm_max_hidden() + 1
    assert step(shape_desc(5, big, [[big, 3]], p)) == -1 and b"hidden = 257" in err()
    assert pack(shape_desc(5, big, [[big, 3]], p)) == -1 and b"hidden = 257" in err()
    assert step(shape_desc(5, 0, [[0, 3]], p)) == -1 and b"hidden = 0" in err()
    assert step(shape_desc(0, 8, good, p)) == -1 and b"d_in = 0" in err()
    assert step(shape_desc(lib.h12learn_mlp_max_width() + 1, 8, good, p)) == -1 and b"d_in" in err()
    assert step(shape_desc(5, 8, [[7, 3]], p)) == -1 and b"dims[0]" in err()  # the MLP must read the hidden state
    wrong = shape_desc(5, 8, good, p)
    wrong.mlp.d_in = 5
    assert step(wrong) == -1 and b"mlp.d_in = 5" in err()
    assert step(shape_desc(5, 8, [[8, 0, 3]], p)) == -1 and b"dims[1] = 0" in err()
    norm = shape_desc(5, 8, good, p)
    norm.norm_kind = _learn.MLP_NORM_STD
    assert step(norm) == -1 and b"norm_mean" in err()
    norm.norm_kind = 7
    assert step(norm) == -1 and b"norm_kind = 7" in err()
    inner = shape_desc(5, 8, good, p)
    inner.mlp.norm_kind = _learn.MLP_NORM_VAR
    assert step(inner) == -1 and b"mlp.norm_kind" in err()
    # null parameters: pack reads them, step does not
    assert pack(shape_desc(5, 8, good, 0)) == -1 and b"cells[0]" in err()
    no_w = shape_desc(5, 8, good, p)
    no_w.mlp.nets[0].W[1] = None
    assert pack(no_w) == -1 and b"W[1]" in err()
    assert pack(ok, packed=None) == -1 and b"packed is null" in err()
    assert pack(ok, packed=p + 4) == -1 and b"16-byte aligned" in err()
    assert step(ok, packed=None) == -1 and b"packed is null" in err()
    assert step(ok, packed=p + 8) == -1 and b"16-byte aligned" in err()
    assert step(ok, no_io=True) == -1 and b"io is null" in err()
    assert step(ok, io=io_of(x=None)) == -1 and b"x is null" in err()
    assert step(ok, io=io_of(n=0)) == -1 and b"n = 0" in err()
    for name in ("h_in", "c_in", "h_out", "c_out", "y"):
        assert step(ok, io=io_of(**{name: 0})) == -1 and b"[0] is null" in err(), name
    two = shape_desc(5, 8, good * 2, p)
    assert step(two, io=io_of(y=1)) == -1 and b"[1] is null" in err()

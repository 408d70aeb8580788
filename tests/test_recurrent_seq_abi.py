"""CPU: the h12learn_lstm_seq_* entry points (csrc/h12_policy_rnn_train.hip) are declared, bound and exported, their
structs have the C layout, and every invalid argument returns H12LEARN_E_ARG with a message before anything touches a
device."""
import ctypes as C
import re
from pathlib import Path

from h12env import _learn, build
from h12env._abi import load_library
from h12env._learn import LEARN_SYMBOLS, LstmSeqDesc, LstmSeqGradIo, LstmSeqIo, learn_library

ROOT = Path(__file__).resolve().parents[1]
SEQ_NAMES = {"h12learn_lstm_seq_packed_bytes", "h12learn_lstm_seq_pack", "h12learn_lstm_seq_forward",
             "h12learn_lstm_seq_backward"}


def test_header_bindings_exports_and_layout():
    src = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "h12learn.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(h12learn_[a-z_]+)\s*\(", src))
    assert SEQ_NAMES <= declared and SEQ_NAMES <= set(LEARN_SYMBOLS)
    lib = load_library()
    for n in SEQ_NAMES:
        assert hasattr(lib, n), n
    assert "h12_policy_rnn_train.hip" in {p.name for p in build.sources()}
    assert build.UNITS.index(build.CSRC / "h12_policy_rnn_train.hip") > 0
    # the C structs' layout on LP64
    assert C.sizeof(LstmSeqDesc) == 8 + 2 * 8
    assert C.sizeof(LstmSeqIo) == 8 + 8 + 8 + 6 * 2 * 8
    assert C.sizeof(LstmSeqGradIo) == 8 + 8 + 8 + 7 * 2 * 8
    for name in ("h12learn_lstm_seq_desc", "h12learn_lstm_seq_io", "h12learn_lstm_seq_grad_io"):
        assert re.search(r"typedef struct %s \{" % name, src), name
    assert lib.h12env_abi_version() == 9


def desc_of(hidden=8, n_nets=1, ptr=0):
    d = LstmSeqDesc()
    d.n_nets, d.hidden = n_nets, hidden
    for i in range(min(n_nets, _learn.LSTM_MAX_NETS)):
        d.w_hh[i] = ptr or None
    return d


def test_packed_bytes():
    lib = learn_library()
    assert lib.h12learn_lstm_seq_packed_bytes(None) == 0 and b"desc is null" in lib.h12learn_last_error()
    # W_hh [4H][pad16(H)] and W_hh^T [pad16(H)][pad16(4H)], per network
    assert lib.h12learn_lstm_seq_packed_bytes(C.byref(desc_of(256))) == 4 * 2 * 256 * 1024
    assert lib.h12learn_lstm_seq_packed_bytes(C.byref(desc_of(256, 2))) == 4 * 4 * 256 * 1024
    assert lib.h12learn_lstm_seq_packed_bytes(C.byref(desc_of(20))) == 4 * 2 * 32 * 80
    assert lib.h12learn_lstm_seq_packed_bytes(C.byref(desc_of(1))) == 4 * 2 * 16 * 16
    big = lib.h12learn_lstm_max_hidden() + 1
    assert lib.h12learn_lstm_seq_packed_bytes(C.byref(desc_of(big))) == 0 and b"hidden = 257" in lib.h12learn_last_error()


def test_argument_validation_without_gpu():
    lib = learn_library()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    fwd_fields = ("zx", "h0", "c0", "h_seq", "c_seq", "gates")
    bwd_fields = ("dh_seq", "gates", "c_seq", "c0", "dz")

    def io_of(cls, fields, T=3, n=4, dones=p, nets=2, **null):
        io = cls()
        io.T, io.n, io.dones = T, n, dones
        for i in range(nets):
            for name in fields:
                getattr(io, name)[i] = None if null.get(name) == i else p
        return io

    def err():
        return lib.h12learn_last_error()

    def pack(desc, packed=p):
        return lib.h12learn_lstm_seq_pack(C.byref(desc) if desc is not None else None, packed, None)

    ok = desc_of(8, 1, p)
    big = lib.h12learn_lstm_max_hidden() + 1
    assert pack(None) == -1 and b"desc is null" in err()
    assert pack(desc_of(0, 1, p)) == -1 and b"hidden = 0" in err()
    assert pack(desc_of(big, 1, p)) == -1 and b"hidden = 257" in err()
    assert pack(desc_of(8, 0, p)) == -1 and b"n_nets = 0" in err()
    assert pack(desc_of(8, 3, p)) == -1 and b"n_nets = 3" in err()
    assert pack(desc_of(8, 1, 0)) == -1 and b"w_hh[0] is null" in err()
    half = desc_of(8, 2, p)
    half.w_hh[1] = None
    assert pack(half) == -1 and b"w_hh[1] is null" in err()
    assert pack(ok, packed=None) == -1 and b"packed is null" in err()
    assert pack(ok, packed=p + 4) == -1 and b"16-byte aligned" in err()

    for fn, cls, fields in ((lib.h12learn_lstm_seq_forward, LstmSeqIo, fwd_fields),
                            (lib.h12learn_lstm_seq_backward, LstmSeqGradIo, bwd_fields)):
        def call(desc=ok, packed=p, io=None, no_io=False):
            io = io_of(cls, fields) if io is None else io
            return fn(C.byref(desc) if desc is not None else None, packed, None if no_io else C.byref(io), None)

        assert call(desc=None) == -1 and b"desc is null" in err()
        assert call(desc=desc_of(0, 1, p)) == -1 and b"hidden = 0" in err()
        assert call(desc=desc_of(big, 1, p)) == -1 and b"hidden = 257" in err()
        assert call(desc=desc_of(8, 3, p)) == -1 and b"n_nets = 3" in err()
        assert call(packed=None) == -1 and b"packed is null" in err()
        assert call(packed=p + 8) == -1 and b"16-byte aligned" in err()
        assert call(no_io=True) == -1 and b"io is null" in err()
        assert call(io=io_of(cls, fields, T=0)) == -1 and b"T = 0" in err()
        assert call(io=io_of(cls, fields, T=4097)) == -1 and b"T = 4097" in err()
        assert call(io=io_of(cls, fields, n=0)) == -1 and b"n = 0" in err()
        assert call(io=io_of(cls, fields, dones=None)) == -1 and b"dones is null" in err()
        for name in fields:
            assert call(io=io_of(cls, fields, **{name: 0})) == -1 and b"[0] is null" in err(), name
        assert call(desc=desc_of(8, 2, p), io=io_of(cls, fields, **{fields[0]: 1})) == -1 and b"[1] is null" in err()

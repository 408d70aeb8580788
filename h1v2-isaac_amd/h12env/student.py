"""The deployable ("student") observation group (include/h12student.h, csrc/h12_student.hip): what
a distilled student policy reads as ``extras["observations"]["student"]``.  Only what the robot measures -- the Flat
policy frame (base_ang_vel, projected_gravity, velocity_commands, joint_pos, joint_vel, actions), with noise and a
term-major history of ``history_length`` frames, the row the deploy stack's observation handler rebuilds.
"""
from __future__ import annotations

import ctypes as C

# row order
TERMS = ("base_ang_vel", "projected_gravity", "velocity_commands", "joint_pos", "joint_vel", "actions")
WIDTHS = dict(zip(TERMS, (3, 3, 3, 12, 12, 12)))
FRAME = 45
MAX_HISTORY = 10
RNG_STREAM = 5

STUDENT_SYMBOLS = ["h12student_layout", "h12student_observe", "h12student_last_error"]


class StudentConfig(C.Structure):
    """h12student_config"""
    _fields_ = [("history", C.c_int32), ("enable_corruption", C.c_int32), ("seed_lo", C.c_uint32),
                ("seed_hi", C.c_uint32), ("env_offset", C.c_uint32), ("noise", C.c_float * len(TERMS)),
                ("scale", C.c_float * len(TERMS)), ("fill_mask", C.c_void_p)]


_bound = None


def student_library():
    """libh12env.so with the h12student_* prototypes set.  A library without them is an error (no fallback)."""
    global _bound
    if _bound is not None:
        return _bound
    from ._abi import H12EnvError, load_library

    lib = load_library()
    for s in STUDENT_SYMBOLS:
        if not hasattr(lib, s):
            raise H12EnvError(f"libh12env.so lacks {s}; rebuild it (csrc/h12_student.hip)")
    i32p = C.POINTER(C.c_int32)
    lib.h12student_layout.argtypes = [C.c_int, i32p, C.c_void_p, i32p]
    lib.h12student_layout.restype = C.c_int
    lib.h12student_observe.argtypes = [C.c_void_p, C.c_int, C.POINTER(StudentConfig), C.c_void_p, C.c_void_p,
                                       C.c_int64, C.c_void_p]
    lib.h12student_observe.restype = C.c_int
    lib.h12student_last_error.argtypes = []
    lib.h12student_last_error.restype = C.c_char_p
    _bound = lib
    return lib


def check(lib, rc: int, what: str):
    if rc != 0:
        from ._abi import H12EnvError

        msg = lib.h12student_last_error()
        raise H12EnvError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def layout(history: int):
    """(W, [(term name, offset, width)]) as the library lays the row out (h12student_layout: host only)."""
    lib = student_library()
    w, k = C.c_int32(), C.c_int32()
    table = (C.c_int32 * (3 * len(TERMS)))()
    check(lib, lib.h12student_layout(int(history), C.byref(w), table, C.byref(k)), "h12student_layout")
    return w.value, [(TERMS[table[3 * i]], table[3 * i + 1], table[3 * i + 2]) for i in range(k.value)]


def term_noise(sc) -> dict:
    """term -> noise half-width of a StudentObsCfg (a term without a Unoise takes none)."""
    out = {}
    for t in TERMS:
        u = getattr(sc, t)
        if u is not None and u.n_min != -u.n_max:
            raise ValueError(f"student observation noise of {t} must be symmetric (U(-n, n)), got ({u.n_min}, {u.n_max})")
        out[t] = 0.0 if u is None else float(u.n_max)
    return out


def term_scales(sc) -> dict:
    unknown = set(sc.scales) - set(TERMS)
    if unknown:
        raise ValueError(f"student observation scales for unsupported terms: {sorted(unknown)} (terms: {TERMS})")
    return {t: float(sc.scales.get(t, 1.0)) for t in TERMS}


def student_config(cfg, env_offset: int = 0) -> StudentConfig:
    """h12student_config of an env cfg whose observations have a student group."""
    sc = cfg.observations.student
    h = int(sc.history_length)
    if not 1 <= h <= MAX_HISTORY:
        raise ValueError(f"the student observation's history_length is 1 .. {MAX_HISTORY}, got {sc.history_length}")
    if not sc.concatenate_terms:
        raise ValueError("the student observation is one concatenated row (concatenate_terms=True)")
    c = StudentConfig()
    c.history = h
    c.enable_corruption = int(bool(sc.enable_corruption))
    seed = (cfg.seed if cfg.seed is not None else 0) & 0xFFFFFFFFFFFFFFFF
    c.seed_lo, c.seed_hi = seed & 0xFFFFFFFF, seed >> 32
    c.env_offset = int(env_offset) & 0xFFFFFFFF
    nz, s = term_noise(sc), term_scales(sc)
    for i, name in enumerate(TERMS):
        c.noise[i] = nz[name]
        c.scale[i] = s[name]
    return c

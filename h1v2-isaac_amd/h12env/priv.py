"""The privileged ("critic") observation group (include/h12priv.h, csrc/h12_priv.hip): what
rsl_rl's asymmetric actor-critic reads as ``extras["observations"]["critic"]``.  One noise-free row per env, no history:
the policy's terms without corruption, the base linear velocity, and what only the simulator knows (base height, foot
contacts / timers / forces, the randomised actuator lags, sole friction and added torso mass).
"""
from __future__ import annotations

import ctypes as C

# row order; height_scan only on a heightfield task
TERMS = ("base_lin_vel", "base_ang_vel", "projected_gravity", "velocity_commands", "joint_pos", "joint_vel", "actions",
         "height_scan", "base_height", "feet_contact", "feet_air_time", "feet_contact_time", "feet_force",
         "actuator_lag", "sole_friction", "added_mass")
WIDTHS = dict(zip(TERMS, (3, 3, 3, 3, 12, 12, 12, 187, 1, 2, 2, 2, 2, 3, 4, 1)))
POLICY_SCALED = ("base_ang_vel", "projected_gravity", "velocity_commands", "joint_pos", "joint_vel", "actions")
# the terms the policy group does not have: their scales come from CriticObsCfg.scales
OWN_TERMS = TERMS[TERMS.index("base_height"):]
W_PLANE, W_TERRAIN = 65, 252

PRIV_SYMBOLS = ["h12priv_layout", "h12priv_observe", "h12priv_last_error"]
# a subset of the row's terms, compacted: the rnd_state group (h12env.rnd)
PRIV_TERMS_SYMBOLS = ["h12priv_layout_terms", "h12priv_observe_terms"]


class PrivConfig(C.Structure):
    """h12priv_config"""
    _fields_ = [("terrain", C.c_int32), ("heights", C.c_void_p), ("nx", C.c_int32), ("ny", C.c_int32),
                ("hscale", C.c_float), ("x0", C.c_float), ("y0", C.c_float), ("mu_static", C.c_float),
                ("mu_dynamic", C.c_float), ("per_env_friction", C.c_int32), ("per_env_mass", C.c_int32),
                ("scan_offset", C.c_float), ("scan_clip", C.c_float), ("scale", C.c_float * len(TERMS))]


_bound = None


def priv_library():
    """libh12env.so with the h12priv_* prototypes set.  A library without them is an error (no fallback)."""
    global _bound
    if _bound is not None:
        return _bound
    from ._abi import H12EnvError, load_library

    lib = load_library()
    for s in PRIV_SYMBOLS + PRIV_TERMS_SYMBOLS:
        if not hasattr(lib, s):
            raise H12EnvError(f"libh12env.so lacks {s}; rebuild it (csrc/h12_priv.hip)")
    i32p = C.POINTER(C.c_int32)
    lib.h12priv_layout.argtypes = [C.c_int, i32p, C.c_void_p, i32p]
    lib.h12priv_layout.restype = C.c_int
    lib.h12priv_observe.argtypes = [C.c_void_p, C.c_int, C.POINTER(PrivConfig), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.h12priv_observe.restype = C.c_int
    lib.h12priv_layout_terms.argtypes = [C.c_int, C.c_uint32, i32p, C.c_void_p, i32p]
    lib.h12priv_layout_terms.restype = C.c_int
    lib.h12priv_observe_terms.argtypes = [C.c_void_p, C.c_int, C.POINTER(PrivConfig), C.c_void_p, C.c_uint32,
                                          C.c_void_p, C.c_void_p]
    lib.h12priv_observe_terms.restype = C.c_int
    lib.h12priv_last_error.argtypes = []
    lib.h12priv_last_error.restype = C.c_char_p
    _bound = lib
    return lib


def check(lib, rc: int, what: str):
    if rc != 0:
        from ._abi import H12EnvError

        msg = lib.h12priv_last_error()
        raise H12EnvError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def term_names(terrain: bool) -> list[str]:
    """The group's terms in row order."""
    return [t for t in TERMS if terrain or t != "height_scan"]


def layout(terrain: bool):
    """(W, [(term name, offset, width)]) as the library lays the row out (h12priv_layout: host only)."""
    lib = priv_library()
    w, k = C.c_int32(), C.c_int32()
    table = (C.c_int32 * (3 * len(TERMS)))()
    check(lib, lib.h12priv_layout(int(bool(terrain)), C.byref(w), table, C.byref(k)), "h12priv_layout")
    return w.value, [(TERMS[table[3 * i]], table[3 * i + 1], table[3 * i + 2]) for i in range(k.value)]


def term_mask(terms) -> int:
    """The h12priv_observe_terms mask of a collection of term names (bit i: TERMS[i]); ValueError for a name that is
    not a term or for none at all."""
    terms = list(terms)
    unknown = [t for t in terms if t not in TERMS]
    if unknown:
        raise ValueError(f"unknown observation terms {unknown} (terms: {TERMS})")
    if not terms:
        raise ValueError("no observation terms")
    mask = 0
    for t in terms:
        mask |= 1 << TERMS.index(t)
    return mask


def layout_terms(terrain: bool, mask: int):
    """(W, [(term name, offset, width)]) of the compacted row of ``mask`` (h12priv_layout_terms: host only)."""
    lib = priv_library()
    w, k = C.c_int32(), C.c_int32()
    table = (C.c_int32 * (3 * len(TERMS)))()
    check(lib, lib.h12priv_layout_terms(int(bool(terrain)), mask, C.byref(w), table, C.byref(k)),
          "h12priv_layout_terms")
    return w.value, [(TERMS[table[3 * i]], table[3 * i + 1], table[3 * i + 2]) for i in range(k.value)]


def default_force_scale() -> float:
    """1 / (total model mass x g): a foot force in body weights (the raw ~700 N would swamp a critic that runs
    without empirical normalisation)."""
    from .model import model_dict

    d = model_dict()
    mass = float(d["base"]["mass"]) + sum(float(j["mass"]) for j in d["joints"])
    return 1.0 / (mass * float(d["gravity"]))


def term_scales(cfg) -> dict:
    """term -> scale of the critic row of an env cfg: the policy group's scales for the terms they share, the critic
    group's for its own (feet_force defaults to default_force_scale(), every other term to 1)."""
    crit = cfg.observations.critic
    if crit is None:  # the rnd_state group without a critic group: the critic row's default scales
        from .cfg import CriticObsCfg

        crit = CriticObsCfg()
    unknown = set(crit.scales) - set(OWN_TERMS)
    if unknown:
        raise ValueError(f"critic observation scales for unsupported terms: {sorted(unknown)} (own terms: {OWN_TERMS})")
    out = {t: 1.0 for t in TERMS}
    for t in POLICY_SCALED:
        out[t] = float(cfg.observations.policy.scales.get(t, 1.0))
    out["feet_force"] = default_force_scale()
    for t, v in crit.scales.items():
        out[t] = float(v)
    return out


def priv_config(env) -> PrivConfig:
    """h12priv_config of an H12VelocityEnv whose cfg has a critic group or an rnd_state group."""
    cfg, cc = env.cfg, env._ccfg
    crit = cfg.observations.critic
    if crit is not None and crit.history_length not in (0, 1, None):
        raise ValueError("the critic observation has no history (history_length 0)")
    if crit is not None and not crit.concatenate_terms:
        raise ValueError("the critic observation is one concatenated row (concatenate_terms=True)")
    t = env.terrain
    if (t is None) != (cfg.scene.height_scanner is None):
        raise ValueError("the critic / rnd_state group needs the heightfield and the height scanner together (a "
                         "terrain task) or neither (a plane task)")
    c = PrivConfig()
    if t is not None:
        c.terrain = 1
        c.heights, c.nx, c.ny = env._t_heights.data_ptr(), t.shape[0], t.shape[1]
        c.hscale, c.x0, c.y0 = t.hscale, t.x0, t.y0
    c.mu_static, c.mu_dynamic = cc.mu_static, cc.mu_dynamic
    c.per_env_friction, c.per_env_mass = cc.per_env_friction, cc.per_env_mass
    c.scan_offset, c.scan_clip = cc.scan_offset, cc.scan_clip
    s = term_scales(cfg)
    for i, name in enumerate(TERMS):
        c.scale[i] = s[name]
    return c

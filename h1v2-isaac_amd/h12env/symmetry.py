"""Mirror symmetry of the H1-2 tasks: the reflection about the sagittal x-z plane as a column map of the observation
and action vectors, for rsl_rl 2.3's symmetry options (data augmentation and mirror loss, h12env/ppo.py).

A ``MirrorTable`` of width D is ``src`` (int32 [D]) and ``flip`` (bool [D]): ``mirror(x)[..., j] = +-x[..., src[j]]``.
It is built from the env's observation term list and history length, never from hard-coded offsets.  The history is
term-major ([term][slot][component], oldest slot first), so the per-frame rule of a term applies to each of its slots.

    term                                         rule
    base_lin_vel, projected_gravity  (polar)     (x, -y, z)
    base_ang_vel                     (axial)     (-x, y, -z)
    velocity_commands (vx, vy, wz)               (vx, -vy, -wz)
    joint_pos, joint_vel, actions                left_* <-> right_* by joint name; yaw and roll joints negated
    height_scan (17 x 11 rays, x fastest)        out[iy * 17 + ix] = in[(10 - iy) * 17 + ix]

and, of the privileged ("critic") group (h12env.priv):

    base_height, actuator_lag, added_mass        unchanged (the three actuator groups span both legs)
    feet_contact, feet_air_time,
    feet_contact_time, feet_force (left, right)  left <-> right
    sole_friction (static L, dynamic L,
                   static R, dynamic R)          the left sole's pair <-> the right sole's

The joint rule is checked against the model's joint axes when a table is built (a rotation about z or x changes sign
under the reflection, one about y does not).  The legs of the model are exact mirrors of each other; the base body
is not, so the simulated robot has this symmetry only approximately.

CPU tensors go through plain torch indexing; CUDA tensors through ``h12learn_mirror_rows`` (csrc/h12_learn.hip), which
also fuses the minibatch gather and the concatenation of ``augment``.  Both move the values bit for bit (the sign is
a sign-bit flip), and both are differentiable: the map is a signed permutation and an involution, so its transpose is
itself.

An env other than the H1-2 env can supply its own tables as ``env.unwrapped.mirror_tables``: a dict of
``MirrorTable`` by observation group name, plus the key ``"actions"``.
"""
from __future__ import annotations

from functools import lru_cache

import torch

from . import model as _model

SCAN_NX, SCAN_NY = 17, 11  # RayCasterCfg grid pattern 1.6 x 1.0 m at 0.1 m, x fastest (csrc/h12env.hip, rough row)

_POLAR = ((0, False), (1, True), (2, False))   # (x, -y, z)
_AXIAL = ((0, True), (1, False), (2, True))    # (-x, y, -z)
_COMMAND = ((0, False), (1, True), (2, True))  # (vx, -vy, -wz)
_SAME = {"base_height": 1, "actuator_lag": 3, "added_mass": 1}  # term -> width, components unchanged
_FEET = ("feet_contact", "feet_air_time", "feet_contact_time", "feet_force")  # (left, right)


class MirrorTable:
    """``mirror(x)[..., j] = (-1 if flip[j] else 1) * x[..., src[j]]``."""

    def __init__(self, src, flip):
        self.src = torch.as_tensor(src, dtype=torch.int32).contiguous()
        self.flip = torch.as_tensor(flip, dtype=torch.bool).contiguous()
        if self.src.dim() != 1 or self.src.shape != self.flip.shape or self.src.numel() < 1:
            raise ValueError("MirrorTable: src and flip must be 1-D and of one length")
        d = self.width
        if int(self.src.min()) < 0 or int(self.src.max()) >= d:
            raise ValueError(f"MirrorTable: a source column is outside [0, {d})")
        s = self.src.long()
        if not (torch.equal(s[s], torch.arange(d)) and torch.equal(self.flip[s], self.flip)):
            raise ValueError("MirrorTable: the map is not an involution")
        self._dev: dict = {}

    @property
    def width(self) -> int:
        return self.src.numel()

    def packed(self, device) -> torch.Tensor:
        """int32 [D] on ``device``: src | flip << 31, the table h12learn_mirror_rows reads."""
        key = str(device)
        if key not in self._dev:
            t = self.src.clone()
            t[self.flip] |= torch.iinfo(torch.int32).min
            self._dev[key] = t.to(device)
        return self._dev[key]

    def _on(self, device):
        key = ("torch", str(device))
        if key not in self._dev:
            self._dev[key] = (self.src.long().to(device), self.flip.to(device))
        return self._dev[key]

    def mirror(self, x: torch.Tensor) -> torch.Tensor:
        return self.apply(x, both=False)

    def apply(self, x: torch.Tensor, idx: torch.Tensor | None = None, both: bool = False) -> torch.Tensor:
        """The mirror of the rows ``idx`` of x (every row when None); ``both``: cat([rows, mirror(rows)]) along the
        first dimension."""
        if x.shape[-1] != self.width:
            raise ValueError(f"mirror: the last dimension is {x.shape[-1]}, the table is {self.width} wide")
        if x.is_cuda and x.dtype == torch.float32:
            return _MirrorRows.apply(x, idx, self, both)
        src, flip = self._on(x.device)
        rows = x if idx is None else x[idx]
        g = rows[..., src]
        m = torch.where(flip, -g, g)  # a negation flips the sign bit and nothing else
        return torch.cat([rows, m], dim=0) if both else m


class _MirrorRows(torch.autograd.Function):
    """h12learn_mirror_rows on a float32 CUDA tensor of any leading shape.  Backward: the map is its own transpose, so
    the gradient of the mirrored rows is mirrored back and scattered to the gathered rows."""

    @staticmethod
    def forward(ctx, x, idx, table, both):
        from ._learn import mirror_rows

        x2 = x.detach().contiguous().view(-1, table.width)
        if idx is not None and x.dim() != 2:
            raise ValueError("mirror: a row index needs a 2-D tensor")
        out = mirror_rows(x2, table.packed(x.device), idx, both)
        ctx.table, ctx.both, ctx.idx, ctx.shape = table, both, idx, x.shape
        if idx is None:
            lead = x.shape[0]
            out = out.view((2 * lead if both else lead,) + tuple(x.shape[1:])) if x.dim() >= 1 else out.view(x.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        from ._learn import mirror_rows

        t, w = ctx.table, ctx.table.width
        g = g.contiguous()
        if ctx.both:
            n = g.shape[0] // 2
            gx = g[:n].reshape(-1, w) + mirror_rows(g[n:].reshape(-1, w), t.packed(g.device))
        else:
            gx = mirror_rows(g.view(-1, w), t.packed(g.device))
        if ctx.idx is None:
            return gx.view(ctx.shape), None, None, None
        full = torch.zeros(ctx.shape, dtype=g.dtype, device=g.device)
        return full.index_add_(0, ctx.idx, gx), None, None, None


# ---------------------------------------------------------------------------------------------- the tables
def _joint_rule():
    """Per joint j: (index of its mirror partner, negate), from the joint names; checked against the joint axes."""
    names = list(_model.joint_names())
    pos = {n: i for i, n in enumerate(names)}
    axes = {jd["name"]: int(jd["axis"]) for jd in _model.model_dict()["joints"]}
    rule = []
    for n in names:
        if n.startswith("left_"):
            partner = "right_" + n[len("left_"):]
        elif n.startswith("right_"):
            partner = "left_" + n[len("right_"):]
        else:
            raise ValueError(f"joint {n!r} is neither left_* nor right_*: no mirror partner")
        if partner not in pos:
            raise ValueError(f"joint {n!r} has no mirror partner {partner!r}")
        negate = "_yaw_" in n or "_roll_" in n
        # the model's joint axes: 0 = x (roll), 1 = y (pitch), 2 = z (yaw); rotations about z and x change sign
        assert n in axes and axes[n] == axes[partner], f"{n}: the mirror partner turns about another axis"
        assert negate == (axes[n] in (0, 2)), f"{n}: the name says negate={negate}, the model's axis is {axes[n]}"
        rule.append((pos[partner], negate))
    return rule


def _term_rule(term: str):
    """The per-frame rule of one observation term: a list of (source component, negate)."""
    if term in ("base_lin_vel", "projected_gravity"):
        return list(_POLAR)
    if term == "base_ang_vel":
        return list(_AXIAL)
    if term == "velocity_commands":
        return list(_COMMAND)
    if term in ("joint_pos", "joint_vel", "actions"):
        return _joint_rule()
    if term == "height_scan":
        return [((SCAN_NY - 1 - iy) * SCAN_NX + ix, False) for iy in range(SCAN_NY) for ix in range(SCAN_NX)]
    if term in _SAME:
        return [(k, False) for k in range(_SAME[term])]
    if term in _FEET:
        return [(1, False), (0, False)]
    if term == "sole_friction":  # H12_F_MU: [static L, dynamic L, static R, dynamic R] (h12env.startup)
        return [(2, False), (3, False), (0, False), (1, False)]
    raise ValueError(f"no mirror rule for the observation term {term!r}")


_tables: dict = {}


def table_from_terms(terms, history_length: int = 1) -> MirrorTable:
    """The table of a term-major observation row: for every term, ``history_length`` slots of its frame.  One object
    per (terms, history, joint order): its device copy is then made once, outside any graph capture that uses it."""
    h = max(1, int(history_length or 0))
    key = (tuple(terms), h, tuple(_model.joint_names()))
    if key in _tables:
        return _tables[key]
    src, flip, off = [], [], 0
    for term in terms:
        rule = _term_rule(term)
        w = len(rule)
        for slot in range(h):
            base = off + slot * w
            src += [base + s for s, _ in rule]
            flip += [f for _, f in rule]
        off += h * w
    _tables[key] = MirrorTable(src, flip)
    return _tables[key]


def action_table() -> MirrorTable:
    """The table of the 12-wide action / action-mean vector."""
    return table_from_terms(["actions"], 1)


def _cfg_terms(cfg, obs_type: str):
    group = getattr(cfg.observations, obs_type, None)
    if group is None:
        raise ValueError(f"the env cfg has no observation group {obs_type!r}")
    if obs_type == "critic":  # the privileged row: its own term list, no history
        from .priv import term_names

        return term_names(cfg.scene.height_scanner is not None), group.history_length
    terms = ["base_ang_vel", "projected_gravity", "velocity_commands", "joint_pos", "joint_vel", "actions"]
    if getattr(group, "base_lin_vel", None) is not None:
        terms = ["base_lin_vel"] + terms
    if getattr(group, "height_scan", None) is not None:
        terms = terms + ["height_scan"]
    return terms, group.history_length


def _unwrap(env):
    return getattr(env, "unwrapped", env)


def mirror_table(env_or_cfg, obs_type: str = "policy") -> MirrorTable:
    """The table of the observation group ``obs_type`` (or of ``"actions"``) of an env, a wrapped env or an env cfg."""
    u = _unwrap(env_or_cfg)
    own = getattr(u, "mirror_tables", None)
    if own is not None:
        if obs_type not in own:
            raise ValueError(f"the env's mirror_tables have no entry {obs_type!r}")
        return own[obs_type]
    if obs_type == "actions":
        return action_table()
    om = getattr(u, "observation_manager", None)
    if om is not None:  # an env
        active = getattr(om, "active_terms", None)
        if active is None or obs_type not in active:
            raise ValueError(f"the env's observation manager lists no terms for the group {obs_type!r}")
        terms, h = list(active[obs_type]), getattr(u.cfg.observations, obs_type).history_length
    else:
        terms, h = _cfg_terms(u, obs_type)
    t = table_from_terms(terms, h)
    dims = getattr(om, "group_obs_dim", {}).get(obs_type) if om is not None else None
    if dims is not None and int(dims[0]) != t.width:
        raise ValueError(f"the mirror table of {terms} x {h} is {t.width} wide, the observation is {dims[0]}")
    return t


@lru_cache(maxsize=None)
def _layout_tables() -> dict:
    """width -> table of the shipped H1-2 task layouts (Flat, Rsl, CaT, Rough), for calls that give no env."""
    from . import cfg as K

    out: dict = {}
    for c in (K.H12FlatEnvCfg, K.H12RslEnvCfg, K.H12CaTEnvCfg, K.H12RoughEnvCfg):
        t = table_from_terms(*_cfg_terms(c(), "policy"))
        prev = out.setdefault(t.width, t)
        if not (torch.equal(prev.src, t.src) and torch.equal(prev.flip, t.flip)):
            raise ValueError(f"two task layouts of width {t.width} mirror differently: pass the env")
    return out


def _obs_table(x, env, obs_type):
    if env is not None:
        return mirror_table(env, obs_type)
    tables = _layout_tables()
    if x.shape[-1] not in tables:
        raise ValueError(f"no H1-2 task has a {x.shape[-1]}-wide observation ({sorted(tables)}): pass the env")
    return tables[x.shape[-1]]


def _action_table(env):
    return action_table() if env is None else mirror_table(env, "actions")


def mirror_obs(x: torch.Tensor, env=None, obs_type: str = "policy") -> torch.Tensor:
    """The mirror image of observation rows; without ``env`` the layout is the H1-2 task layout of x's width."""
    return _obs_table(x, env, obs_type).mirror(x)


def mirror_actions(a: torch.Tensor, env=None) -> torch.Tensor:
    return _action_table(env).mirror(a)


def augment(obs=None, actions=None, env=None, obs_type: str = "policy", idx=None):
    """rsl_rl's ``data_augmentation_func``: (cat([obs, mirror(obs)]), cat([actions, mirror(actions)])); None stays
    None.  ``idx`` (an extension the runner uses): the rows to gather from ``obs`` / ``actions`` first, fused into the
    same launch on the device."""
    o = None if obs is None else _obs_table(obs, env, obs_type).apply(obs, idx, both=True)
    a = None if actions is None else _action_table(env).apply(actions, idx, both=True)
    return o, a


def resolve_func(f):
    """A callable, or the callable a ``"module:func"`` string names."""
    if callable(f):
        return f
    if isinstance(f, str) and ":" in f:
        import importlib

        mod, _, name = f.partition(":")
        return getattr(importlib.import_module(mod), name)
    raise ValueError(f"data_augmentation_func must be a callable or a 'module:func' string, got {f!r}")

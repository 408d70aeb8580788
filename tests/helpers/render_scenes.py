"""The renderer's test scenes: workspace states for n = 5 envs (host arrays), cameras and view lists, shared by the
CPU tests (sensitive-pixel share, gates) and the GPU tests.  Everything here is host data; the float64 reference of
a scene is computed once per process (``reference``).

    python tests/helpers/render_scenes.py --write-gates     # regenerates tests/golden/render_gates.json
"""
from __future__ import annotations

import json
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT / "h1v2-isaac_amd", ROOT / "tests" / "helpers"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import render_reference as RR  # noqa: E402

N_ENVS = 5
GATES = ROOT / "tests" / "golden" / "render_gates.json"
SENSITIVE_CAP = 0.01          # the GPU condition (share of skipped pixels per frame)
SENSITIVE_REF_CAP = 0.005     # what the scenes are chosen for: the reference alone stays under half the cap

SCENES = {
    # name: views, (W, H), camera, overlays, heightfield
    "batch_asset": dict(views=[4, 0, 2], res=(96, 64), origin_type="asset_root", eye=(2.0, 1.2, 0.4),
                        lookat=(0.0, 0.0, -0.3), overlays=True, rough=False),
    "fallen_world": dict(views=[1], res=(50, 37), origin_type="world", eye=(2.4, -2.1, 1.6), lookat=(0.0, 0.0, 0.2),
                         overlays=True, rough=False),
    "above_plain": dict(views=[2], res=(96, 64), origin_type="world", eye=(0.3, 0.25, 3.4), lookat=(0.0, 0.0, 0.5),
                        overlays=False, rough=False),
    "rough": dict(views=[4, 0, 2], res=(96, 64), origin_type="asset_root", eye=(2.7, 1.7, 1.0),
                  lookat=(0.0, 0.0, -0.3), overlays=True, rough=True),
}
FOVY_DEG, SUN, FAR = 45.0, (0.35, -0.25, 0.9), 12.0


def rough_cfg():
    from h12env.cfg import H12RoughEnvCfg

    cfg = H12RoughEnvCfg()
    cfg.scene.num_envs = N_ENVS
    g = cfg.scene.terrain.terrain_generator
    g.num_rows, g.num_cols, g.border_width = 2, 2, 2.0
    g.noise_range, g.noise_step = (0.0, 0.1), 0.02   # visible bumps (the task's own 2 cm noise barely shows)
    cfg.scene.terrain.max_init_terrain_level = 1
    return cfg


def flat_cfg():
    from h12env.cfg import H12FlatEnvCfg

    cfg = H12FlatEnvCfg()
    cfg.scene.num_envs = N_ENVS
    return cfg


def _quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a])


@lru_cache(maxsize=None)
def workspace(rough: bool):
    """(F (NF_FLOAT, 5) float32, I (NF_INT, 5) int32, terrain or None, plane origins (5, 3) or None)."""
    from h12env._abi import F as FIELDS
    from h12env._abi import I as IFIELDS
    from h12env._abi import NF_FLOAT, NF_INT
    from h12env.model import DEFAULT_JOINT_POS

    n = N_ENVS
    F = np.zeros((NF_FLOAT, n), np.float32)
    I = np.zeros((NF_INT, n), np.int32)
    rng = np.random.default_rng(20251019)
    q0 = np.asarray(DEFAULT_JOINT_POS)
    pos = np.zeros((n, 3))
    quat = np.tile([1.0, 0, 0, 0], (n, 1))
    q = np.tile(q0, (n, 1))
    cmd = np.zeros((n, 3))
    vlin = np.zeros((n, 3))
    pack = np.zeros(n, np.int64)
    # env 0: standing, walking command; env 3: standing, no command
    pos[0] = (0.1, -0.2, 1.0)
    cmd[0], vlin[0] = (1.0, 0.0, 0.0), (0.7, 0.1, 0.0)
    pos[3] = (0.0, 0.0, 1.0)
    # env 2, 4: random poses (q0 + 0.3 N(0, 1)), tilted bases
    for e, ax, ang in ((2, (1.0, 0.5, 0.2), 0.35), (4, (-0.3, 1.0, 0.6), -0.5)):
        q[e] = q0 + 0.3 * rng.standard_normal(12)
        quat[e] = _quat(ax, ang)
        pos[e] = (0.2 * rng.standard_normal(), 0.2 * rng.standard_normal(), 1.05)
        cmd[e] = (0.6, -0.4, 0.0)
        vlin[e] = (0.3 * rng.standard_normal(), 0.3 * rng.standard_normal(), 0.0)
    # env 1: fallen (lying on its side), every sole sphere flagged in contact
    quat[1] = _quat((1.0, 0.0, 0.0), 1.45)
    pos[1] = (0.0, 0.1, 0.16)
    q[1] = q0 + 0.2 * rng.standard_normal(12)
    cmd[1], vlin[1] = (0.8, -0.3, 0.0), (0.2, 0.5, 0.0)
    pack[1] = 0xFF << 13
    pack[0] = 0b0011 << 13
    terrain, origins = None, None
    if rough:
        from h12env.startup import apply_to_arrays, startup_state

        st = startup_state(rough_cfg(), n, 0)
        apply_to_arrays(st, F, I)
        terrain = st.terrain
        org = F[FIELDS["ORIGIN"][0]:FIELDS["ORIGIN"][0] + 3].T.astype(np.float64)
        pos = pos + org  # the workspace POS of a terrain task is world
        pos[:, 2] += 0.06  # soles clear of the bumps: a sole face lying in the ground surface is a depth tie
    else:
        import torch

        from h12env.env import env_origins_grid

        origins = env_origins_grid(n, flat_cfg().scene.env_spacing, torch.device("cpu")).numpy().astype(np.float32)
    for name, val in (("POS", pos), ("QUAT", quat), ("Q", q), ("CMD", cmd), ("VLIN", vlin)):
        o, c = FIELDS[name]
        F[o:o + c] = val.T.astype(np.float32)
    I[IFIELDS["PACK"][0]] = pack.astype(np.int32)
    return F, I, terrain, origins


def rows():
    from h12env.model import build_model
    from h12env.render import default_primitives

    return default_primitives(build_model())


def view_of(scene: str, k: int, F=None, I=None) -> RR.View:
    """The reference's description of view k of ``scene`` (optionally on other workspace arrays)."""
    from h12env._abi import F as FIELDS
    from h12env._abi import I as IFIELDS
    from h12env.model import model_dict

    s = SCENES[scene]
    F0, I0, terrain, origins = workspace(s["rough"])
    F = F0 if F is None else F
    I = I0 if I is None else I
    e = s["views"][k]
    col = lambda name: F[FIELDS[name][0]:FIELDS[name][0] + FIELDS[name][1], e]  # noqa: E731
    origin = col("ORIGIN") if s["rough"] else origins[e]
    return RR.View(pos=col("POS"), quat=col("QUAT"), q=col("Q"), vlin=col("VLIN"), cmd=col("CMD")[:2],
                   pack=int(I[IFIELDS["PACK"][0], e]), origin=origin, model=model_dict(), rows=rows(),
                   width=s["res"][0], height=s["res"][1], eye=s["eye"], lookat=s["lookat"],
                   origin_type=s["origin_type"], fovy_deg=FOVY_DEG, sun_dir=SUN, far=FAR, overlays=s["overlays"],
                   terrain=terrain)


def viewer_cfg(scene: str):
    from h12env.render import ViewerCfg

    s = SCENES[scene]
    return ViewerCfg(eye=s["eye"], lookat=s["lookat"], resolution=s["res"], origin_type=s["origin_type"],
                     env_index=s["views"][0], fovy_deg=FOVY_DEG, sun_dir=SUN, overlays=s["overlays"], supersample=1,
                     far=FAR)


@lru_cache(maxsize=None)
def reference(scene: str, k: int):
    """(float64 image dict, sensitive mask) of view k of ``scene``; computed once and left unchanged."""
    v = view_of(scene, k)
    base = RR.render(v, np.float64)
    sens = RR.sensitive(v, base)
    for a in base.values():
        a.setflags(write=False)
    sens.setflags(write=False)
    return base, sens


def measure_gates(scene: str, k: int) -> dict:
    """The reference's own float32-vs-float64 difference over the non-sensitive pixels of a view."""
    base, sens = reference(scene, k)
    lo = RR.render(view_of(scene, k), np.float32)
    ok = ~sens
    same = ok & (lo["id"] == base["id"])
    fin = same & np.isfinite(base["depth"])
    depth = float(np.max(np.abs(lo["depth"][fin].astype(np.float64) - base["depth"][fin]))) if fin.any() else 0.0
    rgb = int(np.max(np.abs(lo["rgb"][same].astype(np.int64) - base["rgb"][same].astype(np.int64)))) if same.any() else 0
    return dict(depth_f32=depth, rgb_levels_f32=rgb, id_mismatch_f32=int((ok & (lo["id"] != base["id"])).sum()),
                sensitive_share=float(sens.mean()))


def all_views():
    return [(s, k) for s in SCENES for k in range(len(SCENES[s]["views"]))]


if __name__ == "__main__":
    out = {f"{s}/{k}": measure_gates(s, k) for s, k in all_views()}
    print(json.dumps(out, indent=1))
    if "--write-gates" in sys.argv:
        GATES.write_text(json.dumps(out, indent=1) + "\n")

"""GPU: the ray-cast renderer (csrc/h12_render.hip) against the float64 numpy reference on the shared scenes
(tests/helpers/render_scenes.py: n = 5 envs, views [4, 0, 2] and single views, 96 x 64 and 50 x 37 frames, standing,
random-pose and fallen states, "world" and "asset_root" cameras, a small heightfield, overlays on and off).

Parity rule: on every pixel the reference itself does not mark threshold-sensitive (its signature -- id, checker
parity, lit flag -- is unchanged under a +-1/256 pixel shift of the pixel centre) the id is equal, the depth is within
4 x the reference's own float32-vs-float64 difference of that view and the rgb within that difference in levels plus
one (tests/golden/render_gates.json).  Sensitive pixels are skipped; their share per frame is capped at 1 %.
Then the bitwise properties, and env.render() / play.py --video / train_cleanrl.py --video end to end at 16 envs."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import render_reference as RR
import render_scenes as S

ROOT = Path(__file__).resolve().parents[1]
SCRIPTS = ROOT / "h1v2-isaac_amd" / "scripts"
sys.path[:0] = [str(ROOT / "h1v2-isaac_amd" / "shims")]

pytestmark = pytest.mark.gpu


def _load(env, rough):
    F, I, _, _ = S.workspace(rough)
    env._fstate.copy_(torch.from_numpy(F).to(env.device))
    env._istate.copy_(torch.from_numpy(I).to(env.device))


@pytest.fixture(scope="module")
def flat_env(gpu):
    from h12env.env import H12VelocityEnv

    cfg = S.flat_cfg()
    cfg.sim.device = "cuda:0"
    env = H12VelocityEnv(cfg)
    env.reset()
    _load(env, False)
    yield env
    env.close()


@pytest.fixture(scope="module")
def rough_env(gpu):
    from h12env.env import H12VelocityEnv

    cfg = S.rough_cfg()
    cfg.sim.device = "cuda:0"
    env = H12VelocityEnv(cfg)
    env.reset()
    _load(env, True)
    yield env
    env.close()


def _renderer(env, scene, **kw):
    from h12env.render import Renderer

    return Renderer(env, viewer=S.viewer_cfg(scene), **kw)


def _render(env, scene, views=None, **kw):
    r = _renderer(env, scene, **kw)
    rgb, ids, depth = r.render(S.SCENES[scene]["views"] if views is None else views, ids=True, depth=True)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), ids.cpu().numpy(), depth.cpu().numpy()


@pytest.mark.parametrize("scene", list(S.SCENES))
def test_matches_the_float64_reference_off_sensitive_pixels(scene, flat_env, rough_env):
    env = rough_env if S.SCENES[scene]["rough"] else flat_env
    rgb, ids, depth = _render(env, scene)
    gates = json.loads(S.GATES.read_text())
    W, H = S.SCENES[scene]["res"]
    assert rgb.shape == (len(S.SCENES[scene]["views"]), H, W, 3) and rgb.dtype == np.uint8
    failures = []
    for k in range(rgb.shape[0]):
        base, sens = S.reference(scene, k)
        g = gates[f"{scene}/{k}"]
        ok = ~sens
        share = float(sens.mean())
        id_bad = int((ok & (ids[k] != base["id"])).sum())
        same = ok & (ids[k] == base["id"])
        fin = same & np.isfinite(base["depth"])
        d_err = float(np.abs(depth[k][fin].astype(np.float64) - base["depth"][fin]).max())
        sky_ok = bool(np.isposinf(depth[k][same & ~np.isfinite(base["depth"])]).all())
        c_err = int(np.abs(rgb[k][same].astype(np.int64) - base["rgb"][same].astype(np.int64)).max())
        d_gate, c_gate = 4.0 * g["depth_f32"], g["rgb_levels_f32"] + 1
        print(f"{scene}/{k}: sensitive {share:.4%}  id mismatches {id_bad}  depth err {d_err:.3e} (gate {d_gate:.3e}, "
              f"fraction {d_err / d_gate:.3f})  rgb err {c_err} levels (gate {c_gate})  "
              f"robot px {(base['id'] >= 0).mean():.3%}")
        if share > S.SENSITIVE_CAP:
            failures.append(f"{k}: sensitive share {share}")
        if id_bad:
            failures.append(f"{k}: {id_bad} id mismatches at {np.argwhere(ok & (ids[k] != base['id']))[:5].tolist()}")
        if not d_err <= d_gate:
            failures.append(f"{k}: depth {d_err} > {d_gate}")
        if not sky_ok:
            failures.append(f"{k}: sky depth is not +inf")
        if c_err > c_gate:
            failures.append(f"{k}: rgb {c_err} > {c_gate}")
    assert not failures, failures


def test_overlay_rows_carry_ids_and_can_be_switched_off(flat_env):
    from h12env.render import Renderer

    n_rows = len(S.rows())
    base, _ = S.reference("fallen_world", 0)
    assert (base["id"] >= n_rows).any()  # the scene does show contact spheres / arrows
    _, ids_on, _ = _render(flat_env, "fallen_world")
    v = S.viewer_cfg("fallen_world")
    v.overlays = False
    out = Renderer(flat_env, viewer=v).render([1], ids=True)
    torch.cuda.synchronize()
    ids_off = out[1].cpu().numpy()
    assert (ids_on >= n_rows).any() and not (ids_off >= n_rows).any()
    assert set(np.unique(ids_on[ids_on >= n_rows])) <= set(range(n_rows, n_rows + 10))


def test_bitwise_run_to_run_batch_invariance_and_culling(flat_env, rough_env):
    for env, scene in ((flat_env, "batch_asset"), (rough_env, "rough")):
        a = _render(env, scene)
        b = _render(env, scene)
        alone = _render(env, scene, views=[0])
        noc = _render(env, scene, cull=False)
        for x, y, z, w in zip(a, b, alone, noc):
            assert np.array_equal(x, y, equal_nan=True)            # run to run
            assert np.array_equal(x[1:2], z, equal_nan=True)       # view [0] alone == inside the batch [4, 0, 2]
            assert np.array_equal(x, w, equal_nan=True)            # the tile mask never changes the image


def test_graph_replay_after_a_state_change_equals_eager(flat_env):
    env = flat_env
    r = _renderer(env, "batch_asset")
    views = S.SCENES["batch_asset"]["views"]
    r.render(views, ids=True, depth=True)  # allocate outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = r.render(views, ids=True, depth=True)
    saved = env._fstate.clone()
    try:
        env._fstate.copy_(saved.roll(1, dims=1))  # every view now shows another env's pose
        g.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in out]
        eager = [t.clone() for t in r.render(views, ids=True, depth=True)]
        torch.cuda.synchronize()
        first = _render(env, "batch_asset")
    finally:
        env._fstate.copy_(saved)
    for a, b in zip(replayed, eager):
        assert torch.equal(a, b)
    assert not np.array_equal(replayed[0].cpu().numpy(), _render(env, "batch_asset")[0])  # the state did change
    assert np.array_equal(first[0], eager[0].cpu().numpy())


def test_nan_base_draws_background_only_and_leaves_other_views_alone(flat_env):
    env = flat_env
    good = _render(env, "batch_asset")
    saved = env._fstate.clone()
    try:
        env._fstate[0, 0] = float("nan")       # POS.x of env 0: view 1 of [4, 0, 2]
        env._fstate[3, 0] = float("inf")       # and its QUAT.w
        bad = _render(env, "batch_asset")
    finally:
        env._fstate.copy_(saved)
    for a, b in zip(good, bad):
        assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[2], b[2], equal_nan=True)
    assert (bad[1][1] < 0).all() and (bad[1][1] == RR.ID_GROUND).any() and (bad[1][1] == RR.ID_SKY).any()
    v = S.view_of("batch_asset", 1)
    ref = RR.render(RR.View(**{**v.__dict__, "pos": np.array([np.nan, 0, 1], np.float32)}))
    assert (bad[1][1] == ref["id"]).mean() > 0.99  # the same background as the reference's


def test_render_leaves_workspace_and_observations_untouched(flat_env):
    env = flat_env
    before = (env._state.clone(), env._obs[0].clone(), env._obs[1].clone())
    _render(env, "batch_asset")
    _render(env, "fallen_world")
    for a, b in zip(before, (env._state, env._obs[0], env._obs[1])):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_supersample_and_mosaic(flat_env):
    from h12env.render import Renderer

    v = S.viewer_cfg("batch_asset")
    v.supersample = 2
    r = Renderer(flat_env, viewer=v)
    rgb = r.render([4, 0, 2])
    m = r.mosaic([4, 0, 2], cols=2)
    torch.cuda.synchronize()
    assert rgb.shape == (3, 64, 96, 3) and rgb.dtype == torch.uint8
    assert m.shape == (2 * 64, 2 * 96, 3) and torch.equal(m[:64, 96:], rgb[1]) and torch.equal(m[64:, :96], rgb[2])
    assert int(m[64:, 96:].max()) == 0
    # supersample = 2 is the 2 x 2 box filter of the frame rendered at twice the size, rounded half up: exact in
    # float32 (a sum of four uint8 values over 4)
    v2 = S.viewer_cfg("batch_asset")
    v2.resolution = (192, 128)
    big = Renderer(flat_env, viewer=v2).render([4, 0, 2]).cpu().numpy().astype(np.int64)
    want = (big.reshape(3, 64, 2, 96, 2, 3).sum(axis=(2, 4)) + 2) // 4
    assert np.array_equal(rgb.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------- end to end, 16 envs
def _frames(path):
    from PIL import Image

    im = Image.open(path)
    return getattr(im, "n_frames", 1), im.size


def _run(script, args, cwd):
    env = dict(os.environ)
    return subprocess.run([sys.executable, str(SCRIPTS / script), *args], cwd=cwd, env=env, capture_output=True,
                          text=True, timeout=300)


def test_env_render_and_play_video(gpu, tmp_path):
    import gymnasium as gym

    import biped_tasks.tasks  # noqa: F401
    from isaaclab_rl.rsl_rl import RslRlVecEnvWrapper
    from isaaclab_tasks.utils.parse_cfg import load_cfg_from_registry
    from rsl_rl.runners import OnPolicyRunner

    task = "Isaac-Velocity-Flat-H12_12dof-Play-v0"
    cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
    agent = load_cfg_from_registry(task, "rsl_rl_cfg_entry_point")
    cfg.scene.num_envs = 16
    cfg.sim.device = "cuda:0"
    raw = gym.make(task, cfg=cfg, render_mode="rgb_array")
    env = RslRlVecEnvWrapper(raw)
    frame = raw.render()
    assert isinstance(frame, np.ndarray) and frame.shape == (360, 640, 3) and frame.dtype == np.uint8
    assert len(np.unique(frame.reshape(-1, 3), axis=0)) > 20  # a picture, not a constant
    runner = OnPolicyRunner(env, agent.to_dict(), log_dir=None, device="cuda:0")
    run = tmp_path / "logs" / "rsl_rl" / agent.experiment_name / "run0"
    runner.save(str(run / "model_0.pt"))
    env.close()
    none_env = gym.make(task, cfg=cfg)
    assert none_env.render() is None
    none_env.close()
    p = _run("play.py", ["--task", task, "--num_envs", "16", "--video", "--video_length", "5", "--steps", "50"], tmp_path)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    (video,) = list((run / "videos" / "play").iterdir())
    assert video.name == "rl-video-step-0.gif"
    assert _frames(video) == (5, (640, 360))


def test_train_cleanrl_video(gpu, tmp_path):
    p = _run("train_cleanrl.py", ["--task", "Isaac-Velocity-CaT-Flat-H12_12dof-v0", "--headless", "--num_envs", "16",
                                  "--num_iterations", "1", "--video", "--video_length", "5", "--video_interval",
                                  "100000"], tmp_path)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    videos = list((tmp_path / "logs" / "clean_rl").glob("*/*/videos_train/*"))
    assert [v.name for v in videos] == ["rl-video-step-0.gif"]
    assert _frames(videos[0]) == (5, (640, 360))

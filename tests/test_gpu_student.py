"""GPU: the deployable ("student") observation group (h12env.student, csrc/h12_student.hip).

Kernel, through the raw ABI on planted workspaces (no env): the noise-free row against h12priv_observe's columns of the
same workspace, bit for bit; the noise against a numpy Philox4x32-10 restatement of its keying; the history against a
numpy ring (fill on reset, else shift) in the term-major layout.  Then the env: the group follows the ring over a Rough
run with resets, only reads, is covered by snapshot / restore, and is pushed by step() and reset() alone."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from h12env import cfg as K
from h12env import priv, student
from h12env._abi import F as FIELDS
from h12env._abi import I as IFIELDS
from h12env._abi import NF_FLOAT, NF_INT

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "h1v2-isaac_amd" / "shims"), str(ROOT / "h1v2-isaac_amd" / "scripts")]

pytestmark = pytest.mark.gpu

OFF = (0, 3, 6, 9, 21, 33)
WID = (3, 3, 3, 12, 12, 12)
TERM_OF_COL = np.repeat(np.arange(6), WID)
NOISE = (0.2, 0.05, 0.0, 0.01, 1.5, 0.0)  # the Flat task's
SEED = (0x9E3779B9 << 32) | 12345


# ---------------------------------------------------------------------------------------------- helpers
def workspace(n, seed, bad_row=None):
    """A planted workspace of n envs: every float field random and finite, PACK random with bits 9-10 non-zero (no row
    was reset).  bad_row: that env's base orientation and position are non-finite."""
    r = np.random.default_rng(seed)
    Fh = r.normal(size=(NF_FLOAT, n)).astype(np.float32)
    Ih = r.integers(0, 1 << 20, size=(NF_INT, n)).astype(np.int32)
    pk = IFIELDS["PACK"][0]
    Ih[pk] = (Ih[pk] & ~(3 << 9)) | (r.integers(1, 4, size=n).astype(np.int32) << 9)
    if bad_row is not None:
        Fh[FIELDS["QUAT"][0] + 1, bad_row] = np.nan
        Fh[FIELDS["POS"][0], bad_row] = np.inf
    return Fh, Ih


def to_device(Fh, Ih):
    buf = torch.empty((NF_FLOAT + NF_INT) * Fh.shape[1], dtype=torch.int32, device="cuda")
    buf[:Fh.size] = torch.from_numpy(Fh.reshape(-1).view(np.int32)).cuda()
    buf[Fh.size:] = torch.from_numpy(Ih.reshape(-1)).cuda()
    return buf


def stu_cfg(history=1, corrupt=True, noise=NOISE, scale=(1.0,) * 6, env_offset=0, seed=SEED):
    c = student.StudentConfig()
    c.history, c.enable_corruption = history, int(corrupt)
    c.seed_lo, c.seed_hi, c.env_offset = seed & 0xFFFFFFFF, seed >> 32, env_offset
    for i in range(6):
        c.noise[i], c.scale[i] = noise[i], scale[i]
    return c


def observe(ws, n, cfg, prev, step, out=None):
    lib = student.student_library()
    out = torch.full((n, 45 * cfg.history), float("nan"), device="cuda") if out is None else out
    rc = lib.h12student_observe(ws.data_ptr(), n, C.byref(cfg), None if prev is None else prev.data_ptr(),
                                out.data_ptr(), step, torch.cuda.current_stream().cuda_stream)
    student.check(lib, rc, "h12student_observe")
    return out


def priv_columns(ws, n, scale=(1.0,) * 6):
    """Columns 3:48 of h12priv_observe (plane layout) of the workspace: the six shared terms, noise-free."""
    lib = priv.priv_library()
    c = priv.PrivConfig()
    for i in range(len(priv.TERMS)):
        c.scale[i] = 1.0
    for i, s in enumerate(scale):
        c.scale[1 + i] = s  # base_ang_vel .. actions follow base_lin_vel
    c.mu_static, c.mu_dynamic = 0.8, 0.6
    out = torch.zeros(n, priv.W_PLANE, device="cuda")
    priv.check(lib, lib.h12priv_observe(ws.data_ptr(), n, C.byref(c), None, out.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream), "h12priv_observe")
    torch.cuda.synchronize()
    return out[:, 3:48].cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def philox4x32_10(k0, k1, c0, c1, c2, c3):
    """Philox4x32-10 on uint32 arrays (Salmon et al. 2011; csrc/h12_math.h)."""
    c = [np.asarray(x, np.uint64) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return [x.astype(np.uint32) for x in c]


def noise_ref(n, step, env_offset=0, noise=NOISE, seed=SEED):
    """[n][45] fp32: fma(2 nz, u, -nz), u = (word >> 8) / 2^24, word c & 3 of
    philox(seed_lo, seed_hi; env_offset + e, step_lo, (5 << 16) | (c >> 2), step_hi)."""
    step &= 0xFFFFFFFFFFFFFFFF
    e = (np.arange(n, dtype=np.uint64) + np.uint64(env_offset))[:, None]
    blk = np.arange(12, dtype=np.uint64)[None, :]
    words = philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, e, step & 0xFFFFFFFF, (5 << 16) | blk, step >> 32)
    w = np.stack(words, -1).reshape(n, 48)[:, :45]  # column c = 4 block + word
    u = (w >> 8).astype(np.float64) / 16777216.0
    nz = np.asarray(noise, np.float32)[TERM_OF_COL].astype(np.float64)
    out = (2.0 * nz * u - nz).astype(np.float32)  # the product and the sum are exact in fp64: one rounding, the fma's
    out[:, nz == 0] = 0.0
    return out


def term_major(ring):
    """[n][H][45] frames, oldest first -> the [n][45 H] row."""
    n, h, _ = ring.shape
    return np.concatenate([ring[:, :, o:o + w].reshape(n, h * w) for o, w in zip(OFF, WID)], axis=1)


def ring_push(ring, frame, fill):
    nxt = np.concatenate([ring[:, 1:], frame[:, None]], axis=1)
    nxt[fill] = frame[fill, None]
    return nxt


# ---------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_noise_free_row_is_the_priv_rows_columns_bit_for_bit(gpu, n):
    bad = n // 2
    Fh, Ih = workspace(n, seed=n, bad_row=bad)
    ws = to_device(Fh, Ih)
    keep = ws.clone()
    want = priv_columns(ws, n)
    for c in (stu_cfg(corrupt=False), stu_cfg(noise=(0.0,) * 6)):  # corruption off, and on with every noise 0
        got = observe(ws, n, c, None, 7).cpu().numpy()
        others = np.arange(n) != bad
        np.testing.assert_array_equal(bits(got[others]), bits(want[others]))
        cols = np.r_[0:3, 6:45]  # the non-finite row may differ only in its own projected_gravity
        np.testing.assert_array_equal(bits(got[bad][cols]), bits(want[bad][cols]))
        assert np.isfinite(got[others]).all() and np.isfinite(got[bad][cols]).all()
    assert torch.equal(ws, keep)  # the call only reads the workspace
    # the terms are what the header says they are
    f = lambda name: Fh[FIELDS[name][0]:FIELDS[name][0] + FIELDS[name][1]].T  # noqa: E731
    np.testing.assert_array_equal(bits(want[:, 0:3]), bits(f("WANG")))
    np.testing.assert_array_equal(bits(want[:, 6:9]), bits(f("CMD")))
    np.testing.assert_array_equal(bits(want[:, 21:33]), bits(f("QD")))
    np.testing.assert_array_equal(bits(want[:, 33:45]), bits(f("ACT")))


def test_scaled_columns_are_the_unscaled_ones_times_the_scale(gpu):
    n, scale = 65, (0.25, 1.0, 2.0, 1.0, 0.05, 1.0)
    ws = to_device(*workspace(n, seed=3))
    plain = observe(ws, n, stu_cfg(corrupt=False), None, 1).cpu().numpy()
    got = observe(ws, n, stu_cfg(corrupt=False, scale=scale), None, 1).cpu().numpy()
    want = plain * np.asarray(scale, np.float32)[TERM_OF_COL]
    np.testing.assert_array_equal(bits(got), bits(want))
    np.testing.assert_array_equal(bits(got), bits(priv_columns(ws, n, scale)))
    # noise, then scale: (value + noise) * scale
    noisy = observe(ws, n, stu_cfg(), None, 1).cpu().numpy()
    both = observe(ws, n, stu_cfg(scale=scale), None, 1).cpu().numpy()
    np.testing.assert_array_equal(bits(both), bits(noisy * np.asarray(scale, np.float32)[TERM_OF_COL]))


# ---------------------------------------------------------------------------------------------- noise
def test_noise_is_bounded_keyed_as_documented_and_independent_of_the_shard(gpu):
    n, step = 257, (3 << 32) | 41
    scale = (0.25, 1.0, 2.0, 1.0, 0.05, 1.0)
    Fh, Ih = workspace(n, seed=17)
    ws = to_device(Fh, Ih)
    clean = priv_columns(ws, n)
    got = observe(ws, n, stu_cfg(), None, step).cpu().numpy()
    nz = np.asarray(NOISE, np.float32)[TERM_OF_COL]
    ref = noise_ref(n, step)
    assert (np.abs(ref) <= nz).all() and np.abs(ref[:, nz > 0]).max() > 0.9 * 1.5
    # up to the one rounding of the add: the row is fp32(value + noise)
    np.testing.assert_array_equal(bits(got), bits(clean + ref))
    scaled = observe(ws, n, stu_cfg(scale=scale), None, step).cpu().numpy()
    d = scaled.astype(np.float64) / np.asarray(scale, np.float64)[TERM_OF_COL] - clean
    ulp = np.spacing(np.maximum(np.abs(clean), np.abs(clean + ref)).astype(np.float32)).astype(np.float64)
    assert (np.abs(d) <= nz + 2 * ulp).all()
    np.testing.assert_array_equal(d[:, nz == 0], 0.0)  # commands and actions take no noise at all
    assert np.abs(d - ref).max() <= 2 * ulp.max() and (np.abs(d - ref) <= 2 * ulp).all()
    for t in (0, 1, 3, 4):  # each noisy term fills its range and is centred
        x = d[:, OFF[t]:OFF[t] + WID[t]] / NOISE[t]
        assert x.min() < -0.9 and x.max() > 0.9 and abs(x.mean()) < 0.1, t
    # rows e >= 64 of a call at env_offset 0 are rows e - 64 of a call at env_offset 64 on the shifted workspace
    m = n - 64
    shifted = to_device(Fh[:, 64:].copy(), Ih[:, 64:].copy())
    part = observe(shifted, m, stu_cfg(env_offset=64), None, step).cpu().numpy()
    np.testing.assert_array_equal(bits(part), bits(got[64:]))
    # another step index, another seed: other noise
    other = observe(ws, n, stu_cfg(), None, step + 1).cpu().numpy()
    np.testing.assert_array_equal(bits(other), bits(clean + noise_ref(n, step + 1)))
    assert (other[:, nz > 0] != got[:, nz > 0]).mean() > 0.99
    neg = observe(ws, n, stu_cfg(), None, -2).cpu().numpy()  # a reset()'s index: any int64 is taken
    np.testing.assert_array_equal(bits(neg), bits(clean + noise_ref(n, -2)))
    seeded = observe(ws, n, stu_cfg(seed=SEED + 1), None, step).cpu().numpy()
    np.testing.assert_array_equal(bits(seeded), bits(clean + noise_ref(n, step, seed=SEED + 1)))


# ---------------------------------------------------------------------------------------------- history
@pytest.mark.parametrize("h", [1, 6, 10])
def test_history_follows_the_ring_restatement(gpu, h):
    n, calls = 65, 12
    # (call, env) pairs whose PACK bits 9-10 are planted as 0: call 0, two consecutive calls, the ragged block's last env
    resets = {(0, 3), (0, 64), (4, 10), (5, 10), (6, 64), (7, 0), (7, 31), (7, 32), (11, 64), (11, 5)}
    bufs = [torch.full((n, 45 * h), float("nan"), device="cuda") for _ in range(2)]
    one, cfg = stu_cfg(history=1), stu_cfg(history=h)
    ring = None
    pk = IFIELDS["PACK"][0]
    for k in range(calls):
        Fh, Ih = workspace(n, seed=100 + k)
        fill = np.zeros(n, bool)
        for (kk, e) in resets:
            if kk == k:
                Ih[pk, e] &= ~(3 << 9)
                fill[e] = True
        ws = to_device(Fh, Ih)
        keep = ws.clone()
        frame = observe(ws, n, one, None, 50 + k).cpu().numpy()  # the frame alone (H = 1: pinned by the tests above)
        prev = None if k == 0 else bufs[(k - 1) & 1]
        got = observe(ws, n, cfg, prev, 50 + k, out=bufs[k & 1]).cpu().numpy()
        assert torch.equal(ws, keep)
        prev_ring = ring
        ring = np.repeat(frame[:, None], h, axis=1) if k == 0 else ring_push(ring, frame, fill)  # prev = NULL: all fill
        np.testing.assert_array_equal(bits(got), bits(term_major(ring)), err_msg=f"call {k}")
    if h > 1:
        assert not np.array_equal(ring[1, 0], ring[1, -1])  # frames differ along the history
        # cfg.fill_mask replaces the PACK rule: exactly its rows fill (env 64's bits say "reset" on this workspace)
        masked = stu_cfg(history=h)
        m = torch.zeros(n, dtype=torch.uint8, device="cuda")
        m[[0, 33]] = 1
        masked.fill_mask = m.data_ptr()
        fill = np.zeros(n, bool)
        fill[[0, 33]] = True
        got = observe(ws, n, masked, bufs[(calls - 2) & 1], 50 + calls - 1).cpu().numpy()
        assert (Ih[pk, 64] >> 9) & 3 == 0
        np.testing.assert_array_equal(bits(got), bits(term_major(ring_push(prev_ring, frame, fill))))
        # prev = NULL fills every row whatever the PACK bits say
        got = observe(ws, n, cfg, None, 50 + calls - 1).cpu().numpy()
        np.testing.assert_array_equal(bits(got), bits(term_major(np.repeat(frame[:, None], h, axis=1))))


# ---------------------------------------------------------------------------------------------- the env
def make(name, n, student_h=None, critic=True, **kw):
    from h12env.env import H12VelocityEnv

    cfg = getattr(K, name)()
    cfg.scene.num_envs = n
    cfg.sim.device = "cuda:0"
    g = cfg.scene.terrain.terrain_generator
    if g is not None:
        g.num_rows, g.num_cols, g.border_width = 6, 8, 5.0
    if critic:
        cfg.observations.critic = K.CriticObsCfg()
    if student_h is not None:
        cfg.observations.student = K.StudentObsCfg(history_length=student_h)
    return H12VelocityEnv(cfg, **kw)


def env_frame(env, step):
    """The student frame (H = 1) of the env's workspace as it stands, by the raw ABI with the env's own keying."""
    sc = env._stu[1]
    one = stu_cfg(history=1, corrupt=bool(sc.enable_corruption), noise=tuple(sc.noise), scale=tuple(sc.scale),
                  env_offset=sc.env_offset, seed=sc.seed_lo | (sc.seed_hi << 32))
    return observe(env._state, env.num_envs, one, None, step).cpu().numpy()


def test_env_group_follows_the_ring_and_only_reads(gpu):
    n, h, steps = 64, 6, 40
    a, b = make("H12RoughEnvCfg", n, student_h=h), make("H12RoughEnvCfg", n)
    assert a.student_obs_dim == 45 * h and b.student_obs_dim is None
    assert a.observation_manager.group_obs_dim["student"] == (45 * h,)
    assert a.observation_manager.active_terms["student"] == list(student.TERMS)
    assert a.observation_manager.group_obs_dim["policy"] == (235,)  # the teacher's row is not touched
    assert a.single_observation_space["student"].shape == (45 * h,)
    assert "student" not in b.observation_manager.group_obs_dim and "student" not in b.single_observation_space.spaces
    oa, _ = a.reset()
    ob, _ = b.reset()
    assert set(oa) == {"policy", "critic", "student"} and set(ob) == {"policy", "critic"}
    assert torch.equal(oa["policy"], ob["policy"]) and torch.equal(oa["critic"], ob["critic"])
    ring = np.repeat(env_frame(a, -1)[:, None], h, axis=1)  # reset(): every row fills, noise index -1
    np.testing.assert_array_equal(bits(oa["student"].cpu().numpy()), bits(term_major(ring)))
    g = torch.Generator(device="cpu").manual_seed(11)
    pk = IFIELDS["PACK"][0]
    n_fill, snap, acts, after = 0, None, [], []
    for t in range(steps):
        if t == 17:
            a.episode_length_buf[n - 1] = a.max_episode_length - 1
            b.episode_length_buf[n - 1] = b.max_episode_length - 1
        act = torch.randn(n, 12, generator=g).cuda()
        if t == 30:
            snap = a.snapshot()
        if t >= 30:
            acts.append(act)
        ra, rb = a.step(act), b.step(act)
        for k in ("policy", "critic"):
            assert torch.equal(ra[0][k], rb[0][k]), (t, k)
        for x, y in zip(ra[1:4], rb[1:4]):
            assert torch.equal(x, y)
        fill = ((a._istate[pk].cpu().numpy() >> 9) & 3) == 0
        assert fill[n - 1] or t != 17  # the forced time-out
        assert np.array_equal(fill, (ra[2] | ra[3]).cpu().numpy())  # the rows the step reset
        n_fill += int(fill.sum())
        ring = ring_push(ring, env_frame(a, a.common_step_counter), fill)
        np.testing.assert_array_equal(bits(ra[0]["student"].cpu().numpy()), bits(term_major(ring)), err_msg=f"step {t}")
        if 30 <= t < 35:
            after.append(ra[0]["student"].clone())
    print(f"rows reset in {steps} steps x {n} envs: {n_fill}")
    assert n_fill >= 2
    assert torch.equal(a._state, b._state)
    # compute() / observe() / get_observations() return the current rows and push nothing
    cur = a.get_observations()["student"]
    keep = cur.clone()
    assert a.observation_manager.compute()["student"].data_ptr() == cur.data_ptr() == a.obs_buf["student"].data_ptr()
    assert a.observe()["student"].data_ptr() == cur.data_ptr() and torch.equal(cur, keep)
    # snapshot / restore: the next 5 steps again, bit for bit
    a.restore(snap)
    for act, want in zip(acts[:5], after):
        assert torch.equal(a.step(act)[0]["student"], want)
    a.close()
    b.close()


def test_returned_rows_live_for_one_further_step_and_bind_rollout_is_refused(gpu):
    from h12env.rollout import RolloutRecorder

    env = make("H12FlatEnvCfg", 64, student_h=3, critic=False)
    env.reset()
    act = torch.zeros(64, 12, device="cuda")
    s_t = env.step(act)[0]["student"]
    keep = s_t.clone()
    env.episode_length_buf[5] = env.max_episode_length - 1  # the next step resets env 5
    s_t1 = env.step(act)[0]["student"]
    assert s_t1.data_ptr() != s_t.data_ptr() and torch.equal(s_t, keep) and not torch.equal(s_t1, keep)
    # a masked reset pushes too: exactly the rows of its mask fill, the others shift -- env 5 as well, which the step
    # before reset (its since-reset bits are still 0: by the bits alone it would fill a second time)
    before = s_t1.clone()
    assert ((env._istate[IFIELDS["PACK"][0]] >> 9) & 3)[[5, 6]].tolist() == [0, 2]
    out, _ = env.reset(env_ids=[2, 63])
    torch.cuda.synchronize()
    frame = env_frame(env, -2)  # the env's second reset()
    ring = before.cpu().numpy()
    fill = np.zeros(64, bool)
    fill[[2, 63]] = True
    want = np.concatenate([np.concatenate([ring[:, 3 * o + w:3 * o + 3 * w], frame[:, o:o + w]], 1)
                           for o, w in zip(OFF, WID)], 1)
    want[fill] = term_major(np.repeat(frame[:, None], 3, axis=1))[fill]
    np.testing.assert_array_equal(bits(out["student"].cpu().numpy()), bits(want))
    assert not np.array_equal(want[5], term_major(np.repeat(frame[:, None], 3, axis=1))[5])  # shifted, not filled
    after = env.step(act)[0]["student"].cpu().numpy()  # and the step after it goes by the bits again
    f2 = env_frame(env, env.common_step_counter)
    shifted = np.concatenate([np.concatenate([want[:, 3 * o + w:3 * o + 3 * w], f2[:, o:o + w]], 1)
                              for o, w in zip(OFF, WID)], 1)
    np.testing.assert_array_equal(bits(after), bits(shifted))
    rec = RolloutRecorder(64, 4, gpu, 10)
    with pytest.raises(ValueError, match="student"):
        env.bind_rollout(rec)
    env.close()
    env = make("H12FlatEnvCfg", 64, student_h=3, critic=False, obs_copy=True)
    env.reset()
    s0 = env.step(act)[0]["student"]
    keep = s0.clone()
    for _ in range(3):
        env.step(act)
    assert torch.equal(s0, keep)  # obs_copy: the returned tensor is the caller's
    env.close()


# ---------------------------------------------------------------------------------------------- distillation end to end
ROUGH = "Isaac-Velocity-Rough-H12_12dof-v0"
SMALL = ["--headless", "--num_envs", "64", "agent.num_steps_per_env=8", "agent.save_interval=1",
         "env.scene.terrain.terrain_generator.num_rows=6", "env.scene.terrain.terrain_generator.num_cols=8",
         "env.scene.terrain.terrain_generator.border_width=5.0"]
DISTILL = ["--distill", "--student_recurrent", "--student_history", "2", "agent.policy.student_hidden_dims=[32]",
           "agent.policy.teacher_hidden_dims=[32,32]", "agent.policy.rnn_hidden_dim=32",
           "agent.algorithm.gradient_length=4"]


@pytest.fixture(scope="module")
def teacher_run(gpu, tmp_path_factory):
    """One PPO iteration on Rough (64 envs x 8 steps, a 32-32 actor), saved: the teacher of the tests below."""
    import os

    import train

    root = tmp_path_factory.mktemp("teacher")
    cwd = os.getcwd()
    os.chdir(root)
    try:
        assert train.main(["--task", ROUGH, "--max_iterations", "1", "--run_name", "teacher",
                           "agent.policy.actor_hidden_dims=[32,32]", "agent.policy.critic_hidden_dims=[32,32]"] + SMALL) == 0
    finally:
        os.chdir(cwd)
    run = next((root / "logs" / "rsl_rl").glob("*/*_teacher"))
    return root, run / "model_1.pt"


def _distill(monkeypatch, root, teacher, fused: bool, name: str):
    import train
    from h12env import distill as DS

    seen = []

    inner = DS.DistillationRunner.learn

    def spy(self, *a, **kw):
        seen.append(self)
        return inner(self, *a, **kw)

    monkeypatch.setattr(DS.DistillationRunner, "learn", spy)
    monkeypatch.chdir(root)
    if fused:
        monkeypatch.setenv("H12_POLICY_FUSED", "1")
    else:
        monkeypatch.delenv("H12_POLICY_FUSED", raising=False)
    argv = ["--task", ROUGH, "--max_iterations", "3", "--run_name", name, "--teacher_checkpoint", str(teacher)]
    assert train.main(argv + DISTILL + SMALL + (["--fused_rnn_update"] if fused else [])) == 0
    run = next((root / "logs" / "rsl_rl").glob(f"*/*_{name}"))
    return seen[0], run


@pytest.mark.parametrize("fused", [False, True], ids=["library", "fused"])
def test_distillation_trains_saves_plays_and_exports(gpu, teacher_run, monkeypatch, fused):
    import copy
    import json
    import os
    import subprocess

    from h12env import distill as DS
    from h12env.export import export_policy_as_jit

    root, teacher = teacher_run
    runner, run = _distill(monkeypatch, root, teacher, fused, "fused" if fused else "library")
    alg, policy = runner.alg, runner.alg.policy
    assert type(runner) is DS.DistillationRunner and type(policy) is DS.StudentTeacherRecurrent
    assert policy.loaded_teacher and alg.fused_rnn_update == fused and alg.gradient_length == 4
    assert policy.memory_s.rnn.input_size == 90 and policy.teacher[0].in_features == 235
    assert (alg._fused is not None) == fused  # the collection ran through the fused wrappers, or never built them
    t_sd = torch.load(teacher, weights_only=True)["model_state_dict"]
    for k, v in policy.teacher.state_dict().items():
        assert torch.equal(v, t_sd["actor." + k].to(v.device)), k
    lines = [json.loads(x) for x in (run / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == 3 and all(np.isfinite(x["Loss/behavior"]) and x["Loss/behavior"] > 0 for x in lines)
    print("behaviour loss per iteration:", [round(x["Loss/behavior"], 5) for x in lines])
    env_yaml = (run / "params" / "env.yaml").read_text()
    assert "student:" in env_yaml and "history_length: 2" in env_yaml
    ck = run / "model_3.pt"
    sd = torch.load(ck, weights_only=True)["model_state_dict"]
    assert DS.is_student_checkpoint(sd) and DS.cfg_from_checkpoint(sd)[1] == 2
    # play.py's path: the checkpoint says what it is, the student group comes on, the student plays and is exported
    envv = dict(os.environ, PYTHONPATH=os.pathsep.join([str(ROOT / "h1v2-isaac_amd"), os.environ.get("PYTHONPATH", "")]))
    envv.pop("H12_POLICY_FUSED", None)
    p = subprocess.run([sys.executable, str(ROOT / "h1v2-isaac_amd" / "scripts" / "play.py"), "--task",
                        "Isaac-Velocity-Rough-H12_12dof-Play-v0", "--num_envs", "16", "--load_run", run.name, "--steps",
                        "5"] + (["--fused"] if fused else []), cwd=root, env=envv, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    import yaml

    y = yaml.safe_load((run / "exported" / "env.yaml").read_text())
    assert [o["name"] for o in y["observations"]] == ["base_ang_vel", "projected_gravity", "generated_commands",
                                                      "joint_pos_rel", "joint_vel_rel", "last_action"]
    assert y["history_length"] == 2
    m = torch.jit.load(str(run / "exported" / "policy.pt"))
    assert hasattr(m, "rnn") and m.rnn.weight_ih_l0.shape[1] == 90
    if fused:  # the Rough-trained student on sim2sim's plane, from the exported directory alone
        p = subprocess.run([sys.executable, str(ROOT / "h1v2-isaac_amd" / "scripts" / "sim2sim.py"),
                            str(run / "exported"), "--num_envs", "16", "--episode_length", "0.2", "--fused"], cwd=root,
                           env=envv, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert "[sim2sim] 16 envs" in p.stdout
    # the TorchScript export against act_inference over a 10-step sequence of one robot with a done in it
    cpu = copy.deepcopy(policy).cpu().eval()
    cpu.load_state_dict(sd)
    m = torch.jit.load(export_policy_as_jit(DS.StudentView(cpu), None, str(run / "again")))
    g = torch.Generator().manual_seed(3)
    cpu.reset()
    with torch.no_grad():
        for t in range(10):
            x = torch.randn(1, 90, generator=g)
            if t == 6:
                cpu.reset(torch.ones(1, dtype=torch.long))
                m.reset()
            want, got = cpu.act_inference(x), m(x)
            assert torch.allclose(got, want, rtol=0, atol=1e-6), t  # tests/test_recurrent.py's for the recurrent export


def test_fused_and_library_updates_agree_on_the_first_update(gpu, teacher_run):
    """One rollout, three updates of the same student from it: float64 (the library LSTM), float32 on the library LSTM
    and float32 on the sequence kernels.  The kernels' distance from float64 is at most FACTOR = 8 times the library's
    own (tests/test_gpu_recurrent_sequence.py's gate for the same kernels; a yardstick below 2^-24 of the tensor's
    largest element is raised to that)."""
    import copy

    from h12env import distill as DS

    T, N, L = 8, 64, 4
    torch.manual_seed(5)
    policy = DS.StudentTeacherRecurrent(90, 235, 12, student_hidden_dims=(32,), teacher_hidden_dims=(32, 32),
                                        rnn_hidden_dim=32)
    policy.load_state_dict(torch.load(teacher_run[1], weights_only=True)["model_state_dict"])
    env = make("H12RoughEnvCfg", N, student_h=2, critic=False)
    algs = {k: DS.Distillation(copy.deepcopy(policy).to(dt), gradient_length=L, device="cuda", fused_rnn_update=f)
            for k, dt, f in (("f64", torch.float64, False), ("lib", torch.float32, False), ("fused", torch.float32, True))}
    for a in algs.values():
        a.init_storage(N, T, [90], [235], [12])
    lib = algs["lib"]
    obs, _ = env.reset()
    with torch.inference_mode():
        for t in range(T):
            act = lib.act(obs["student"], obs["policy"])
            if t == 2:
                env.episode_length_buf[[3, 63]] = env.max_episode_length - 1
            obs, rew, term, trunc, _ = env.step(act)
            lib.process_env_step(rew, (term | trunc).long(), {})
    env.close()
    st = lib.storage
    assert st.dones.sum() >= 2 and st.dones[2, 3] == 1
    for k in ("f64", "fused"):
        s = algs[k].storage
        for name in ("observations", "privileged_observations", "actions", "privileged_actions", "rewards", "dones"):
            getattr(s, name).copy_(getattr(st, name))
        s.step = T
    out = {k: a.update() for k, a in algs.items()}
    ref = dict(algs["f64"].policy.named_parameters())
    worst = 0.0
    for (name, p_lib), p_fused in zip(algs["lib"].policy.named_parameters(), algs["fused"].policy.parameters()):
        r = ref[name].detach()
        yard = max(float((p_lib.detach().double() - r).abs().max()), 2.0 ** -24 * float(r.abs().max()))
        err = float((p_fused.detach().double() - r).abs().max())
        worst = max(worst, err / yard)
        assert err <= 8 * yard, (name, err, yard)
    moved = [n for n, p in algs["fused"].policy.named_parameters() if not torch.equal(p, dict(policy.named_parameters())[n].cuda())]
    assert sorted(moved) == sorted(n for n, _ in policy.named_parameters() if n.startswith(("student.", "memory_s.")))
    yard = max(abs(float(out["lib"]["behavior"]) - float(out["f64"]["behavior"])), 2.0 ** -24 * float(out["f64"]["behavior"]))
    assert abs(float(out["fused"]["behavior"]) - float(out["f64"]["behavior"])) <= 8 * yard
    for a, b, r in zip(*(algs[k].policy.get_hidden_states()[0] for k in ("fused", "lib", "f64"))):  # the carried state
        yard = max(float((b.double() - r).abs().max()), 2.0 ** -24 * float(r.abs().max()))
        assert float((a.double() - r).abs().max()) <= 8 * yard
    print(f"first update, fused against library: largest error / yardstick {worst:.3f}")


def test_fused_collection_leaves_the_next_updates_start_state_alone(gpu, teacher_run, monkeypatch):
    """With H12_POLICY_FUSED=1 the wrapper steps the student's memory and nothing rebinds memory_s.hidden_states, which
    process_env_step still zeroes in place where an env is done.  The state the next update starts from is the one the
    last update ended with, and the one the wrapper started the rollout from -- done or no done."""
    from h12env import distill as DS

    monkeypatch.setenv("H12_POLICY_FUSED", "1")
    T, N = 8, 64
    torch.manual_seed(6)
    policy = DS.StudentTeacherRecurrent(90, 235, 12, student_hidden_dims=(32,), teacher_hidden_dims=(32, 32),
                                        rnn_hidden_dim=32)
    policy.load_state_dict(torch.load(teacher_run[1], weights_only=True)["model_state_dict"])
    alg = DS.Distillation(policy, gradient_length=4, device="cuda", fused_rnn_update=True)
    alg.init_storage(N, T, [90], [235], [12])
    env = make("H12RoughEnvCfg", N, student_h=2, critic=False)
    obs, _ = env.reset()

    def rollout(obs, force):
        with torch.inference_mode():
            for t in range(T):
                act = alg.act(obs["student"], obs["policy"])
                if force and t == 2:
                    env.episode_length_buf[[3, 63]] = env.max_episode_length - 1
                obs, rew, term, trunc, _ = env.step(act)
                alg.process_env_step(rew, (term | trunc).long(), {})
        return obs

    obs = rollout(obs, False)
    assert alg._fused is not None
    assert torch.isfinite(alg.update()["behavior"])
    start = [s.clone() for s in alg._start_state(N)]
    assert all((s[:, [3, 63]] != 0).any() for s in start)
    for w, s in zip(alg._fused[1].state, start):  # the wrapper goes on from the update's end state
        assert torch.equal(w, s)
    obs = rollout(obs, True)
    assert alg.storage.dones[2, 3] == 1 and alg.storage.dones[2, 63] == 1
    assert all((s[:, [3, 63]] == 0).all() for s in policy.memory_s.hidden_states)  # the resets did reach the memory
    for a, b in zip(alg._start_state(N), start):
        assert torch.equal(a, b)
    assert torch.isfinite(alg.update()["behavior"])
    env.close()

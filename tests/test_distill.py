"""CPU: teacher-student distillation (h12env.distill) -- the state-dict rules of StudentTeacher /
StudentTeacherRecurrent, the chunked update against a literal step loop in float64, and the runner.

The literal loop (``literal_update``) is rsl_rl 2.3's Distillation.update restated step by step on nn.LSTM / nn.Sequential:
every epoch restarts from the state the last update ended with; per step the loss of act_inference against the
teacher's action is added to a running sum; every gradient_length steps, counted across the epochs, the sum is
backpropagated, Adam steps, the state is detached and the sum restarts; after every step the state is zeroed where the
step was a done; a trailing remainder is evaluated and never backpropagated.

Gate: the chunked update's distance from the float64 loop, per tensor, is at most FACTOR times the float32 literal
loop's own distance from it (a distance below U = 2^-24 of the tensor's largest element is raised to that: a correctly
rounded fp32 tensor is that far from its fp64 value).  FACTOR = 8 is tests/test_gpu_recurrent_sequence.py's for the
sequence kernels the chunks run on.  Measured here (CPU, torch loop): the largest ratio over the four cases is printed
by the test and recorded in DESIGN.md section 7s."""
import copy
import sys
import warnings
from pathlib import Path

import pytest
import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd" / "shims"))
sys.path.insert(0, str(ROOT / "tests" / "helpers"))

from h12env import distill as DS  # noqa: E402
from h12env import distributed as D  # noqa: E402
from h12env.ppo import ActorCritic, ActorCriticRecurrent, OnPolicyRunner  # noqa: E402
from isaaclab_rl.rsl_rl import (RslRlDistillationAlgorithmCfg, RslRlDistillationStudentTeacherCfg,  # noqa: E402
                                RslRlDistillationStudentTeacherRecurrentCfg, RslRlOnPolicyRunnerCfg,
                                RslRlSymmetryCfg, RslRlVecEnvWrapper)
from toyenv import ToyEnv, ToyEnvCfg  # noqa: E402

U = 2.0 ** -24
FACTOR = 8


# ---------------------------------------------------------------------------------------------- 1: state dicts
def test_ppo_checkpoint_becomes_the_teacher_and_is_no_resume():
    torch.manual_seed(0)
    ppo = ActorCritic(9, 9, 3, actor_hidden_dims=(8, 6), critic_hidden_dims=(5,))
    st = DS.StudentTeacher(4, 9, 3, student_hidden_dims=(7,), teacher_hidden_dims=(8, 6))
    assert not st.loaded_teacher and not st.teacher.training
    student_before = copy.deepcopy(st.student.state_dict())
    std_before = st.std.detach().clone()
    assert st.load_state_dict(ppo.state_dict()) is False
    assert st.loaded_teacher
    x = torch.randn(11, 9)
    assert torch.equal(st.evaluate(x), ppo.actor(x)) and not st.evaluate(x).requires_grad
    for k, v in st.student.state_dict().items():
        assert torch.equal(v, student_before[k])
    assert torch.equal(st.std, std_before) and float(st.std[0]) == pytest.approx(0.1)
    st.train()
    assert st.student.training and not st.teacher.training  # the teacher stays in eval()
    # act samples around the student's mean, act_inference is the mean
    o = torch.randn(5, 4)
    assert torch.equal(st.act_inference(o), st.student(o))
    a = st.act(o)
    assert torch.equal(st.action_mean, st.student(o)) and not torch.equal(a, st.action_mean)
    # a teacher of another shape, or a recurrent one, is refused with a message
    with pytest.raises(ValueError, match="does not match"):
        DS.StudentTeacher(4, 9, 3, teacher_hidden_dims=(8,)).load_state_dict(ppo.state_dict())
    rec = ActorCriticRecurrent(9, 9, 3, actor_hidden_dims=(8, 6), critic_hidden_dims=(5,), rnn_hidden_dim=9)
    with pytest.raises(ValueError, match="teacher_recurrent"):
        DS.StudentTeacher(4, 9, 3, teacher_hidden_dims=(8, 6)).load_state_dict(rec.state_dict())


def test_recurrent_ppo_checkpoint_loads_into_memory_t():
    torch.manual_seed(1)
    ppo = ActorCriticRecurrent(9, 9, 3, actor_hidden_dims=(8,), critic_hidden_dims=(5,), rnn_hidden_dim=6)
    st = DS.StudentTeacherRecurrent(4, 9, 3, student_hidden_dims=(7,), teacher_hidden_dims=(8,), rnn_hidden_dim=6,
                                    teacher_recurrent=True)
    assert st.memory_s.rnn.input_size == 4 and st.memory_t.rnn.input_size == 9
    mem_s = copy.deepcopy(st.memory_s.state_dict())
    assert st.load_state_dict(ppo.state_dict()) is False and st.loaded_teacher
    for k, v in ppo.memory_a.state_dict().items():
        assert torch.equal(st.memory_t.state_dict()[k], v)
    for k, v in st.memory_s.state_dict().items():
        assert torch.equal(v, mem_s[k])
    x = torch.randn(3, 5, 9)
    for t in range(3):  # stepped side by side: the same labels, the same state
        assert torch.equal(st.evaluate(x[t]), ppo.act_inference(x[t]))
    for a, b in zip(st.get_hidden_states()[1], ppo.memory_a.hidden_states):
        assert torch.equal(a, b)
    dones = torch.tensor([0, 1, 0, 0, 1])
    st.act(torch.randn(5, 4))
    st.reset(dones)
    hs, ht = st.get_hidden_states()
    assert all((s[:, dones == 1] == 0).all() and (s[:, dones == 0] != 0).any() for s in hs + ht)
    st.detach_hidden_states()
    assert not any(s.requires_grad for s in st.get_hidden_states()[0])
    st.reset()
    assert st.get_hidden_states() == (None, None)
    # without teacher_recurrent there is no memory_t, and a plain PPO teacher reads the observation
    plain = DS.StudentTeacherRecurrent(4, 9, 3, student_hidden_dims=(7,), teacher_hidden_dims=(8,), rnn_hidden_dim=6)
    assert not hasattr(plain, "memory_t") and plain.teacher[0].in_features == 9 and plain.student[0].in_features == 6
    with pytest.raises(ValueError, match="teacher_recurrent"):
        plain.load_state_dict(ppo.state_dict())


@pytest.mark.parametrize("recurrent", [False, True])
def test_student_checkpoint_resumes_and_an_unknown_dict_raises(recurrent):
    torch.manual_seed(2)
    make = (lambda: DS.StudentTeacherRecurrent(4, 9, 3, student_hidden_dims=(7,), teacher_hidden_dims=(8,),
                                               rnn_hidden_dim=6)) if recurrent else \
        (lambda: DS.StudentTeacher(4, 9, 3, student_hidden_dims=(7,), teacher_hidden_dims=(8,)))
    a, b = make(), make()
    assert b.load_state_dict(a.state_dict()) is True and b.loaded_teacher
    for (k, v), w in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(v, w), k
    assert any(k.startswith("student.") for k in a.state_dict()) and not any("actor" in k for k in a.state_dict())
    assert ("memory_s.rnn.weight_ih_l0" in a.state_dict()) == recurrent
    with pytest.raises(ValueError, match="neither"):
        make().load_state_dict({"critic.0.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="neither"):
        make().load_state_dict({})


# ---------------------------------------------------------------------------------------------- 2: the update
T, N, L, EPOCHS, HID, D_S, D_T, A = 7, 5, 3, 2, 8, 6, 9, 3
LR = 1e-3


def planted_dones():
    """A done at t = 0, one in the middle of a chunk (t = 1, t = 4), one on the step before a chunk boundary (t = 2,
    t = 5) and one on the rollout's last step; the chunks of 3 over 2 x 7 steps are [0-2] [3-5] [6, 0', 1'] [2'-4'] and
    the remainder [5', 6']."""
    d = torch.zeros(T, N, dtype=torch.uint8)
    for t, e in ((0, 0), (1, 1), (4, 2), (2, 3), (5, 0), (6, 4), (2, 1)):
        d[t, e] = 1
    return d


def make_case(recurrent: bool, loss_type: str, seed: int):
    torch.manual_seed(seed)
    if recurrent:
        policy = DS.StudentTeacherRecurrent(D_S, D_T, A, student_hidden_dims=(10,), teacher_hidden_dims=(8,),
                                            rnn_hidden_dim=HID)
    else:
        policy = DS.StudentTeacher(D_S, D_T, A, student_hidden_dims=(10, HID), teacher_hidden_dims=(8,))
    policy.loaded_teacher = True
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        alg = DS.Distillation(policy, num_learning_epochs=EPOCHS, gradient_length=L, learning_rate=LR,
                              loss_type=loss_type, device="cpu")
        alg.init_storage(N, T, [D_S], [D_T], [A])
    assert any("never backpropagated" in str(x.message) for x in w)  # 14 % 3 != 0
    st = alg.storage
    st.observations.copy_(torch.randn(T, N, D_S))
    st.privileged_actions.copy_(2.0 * torch.randn(T, N, A))  # errors on both sides of the huber delta
    st.dones.copy_(planted_dones())
    st.step = T
    start = None
    if recurrent:  # the state a previous update ended with
        start = (0.5 * torch.randn(1, N, HID), 0.5 * torch.randn(1, N, HID))
        alg.last_hidden_states = (start, None)
    return alg, start


def literal_update(policy, st, start, loss_type, dtype):
    """rsl_rl's Distillation.update as a step loop (the module docstring), in ``dtype``.  Returns the parameters after
    it, the mean per-step loss and the carried state."""
    p = copy.deepcopy(policy).to(dtype)
    opt = torch.optim.Adam(p.parameters(), lr=LR)
    loss_fn = nn.functional.mse_loss if loss_type == "mse" else nn.functional.huber_loss
    obs, target = st.observations.to(dtype), st.privileged_actions.to(dtype)
    keep = (st.dones == 0).to(dtype).view(T, 1, N, 1)
    cnt, loss, total, state = 0, 0.0, 0.0, None
    for _ in range(EPOCHS):
        if start is not None:
            state = tuple(s.detach().to(dtype) for s in start)
        for t in range(T):
            feats = obs[t]
            if start is not None:
                out, state = p.memory_s.rnn(obs[t][None], state)
                feats = out[0]
            step_loss = loss_fn(p.student(feats), target[t])
            loss = loss + step_loss
            total += float(step_loss)
            cnt += 1
            if cnt % L == 0:
                opt.zero_grad()
                loss.backward()
                opt.step()
                loss = 0.0
                if state is not None:
                    state = tuple(s.detach() for s in state)
            if state is not None:
                state = tuple(s * keep[t] for s in state)
    params = {k: v.detach().double() for k, v in p.named_parameters()}
    return params, total / cnt, None if state is None else tuple(s.detach().double() for s in state)


def dist(a, b):
    return float((a.double() - b).abs().max())


_ratios = {}


@pytest.mark.parametrize("loss_type", ["mse", "huber"])
@pytest.mark.parametrize("recurrent", [False, True], ids=["plain", "recurrent"])
def test_chunked_update_reproduces_the_literal_step_loop(recurrent, loss_type):
    alg, start = make_case(recurrent, loss_type, seed=3 + recurrent)
    before = {k: v.detach().clone() for k, v in alg.policy.named_parameters()}
    ref_p, ref_loss, ref_state = literal_update(alg.policy, alg.storage, start, loss_type, torch.float64)
    f32_p, f32_loss, f32_state = literal_update(alg.policy, alg.storage, start, loss_type, torch.float32)
    # the trailing remainder: four optimizer steps for 14 steps in chunks of 3, and nothing moves after the fourth
    seen = []
    step = alg.optimizer.step
    alg.optimizer.step = lambda *a, **k: (step(*a, **k), seen.append(
        {n: v.detach().clone() for n, v in alg.policy.named_parameters()}))[0]
    out = alg.update()
    assert len(seen) == (EPOCHS * T) // L == 4
    got_p = dict(alg.policy.named_parameters())
    for k, v in got_p.items():
        assert torch.equal(v, seen[-1][k]), k
    assert set(out) == {"behavior"} and torch.is_tensor(out["behavior"]) and out["behavior"].shape == ()
    assert alg.storage.step == 0
    worst = 0.0
    moved = 0
    for k, v in got_p.items():
        yard = max(dist(f32_p[k], ref_p[k]), U * float(ref_p[k].abs().max()))
        err = dist(v.detach(), ref_p[k])
        worst = max(worst, err / yard)
        moved += int(not torch.equal(v, before[k]))
        assert err <= FACTOR * yard, (k, err, yard)
    trained = [k for k in got_p if k.startswith(("student.", "memory_s."))]
    assert moved == len(trained) and all(not torch.equal(got_p[k], before[k]) for k in trained)
    assert all(torch.equal(got_p[k], before[k]) for k in got_p if k.startswith(("teacher.", "std")))
    yard = max(abs(f32_loss - ref_loss), U * abs(ref_loss))
    worst = max(worst, abs(float(out["behavior"]) - ref_loss) / yard)
    assert abs(float(out["behavior"]) - ref_loss) <= FACTOR * yard
    if recurrent:
        hs, _ = alg.policy.get_hidden_states()
        assert not any(s.requires_grad for s in hs)
        for s, r, f in zip(hs, ref_state, f32_state):
            assert s.shape == (1, N, HID)
            yard = max(dist(f, r), U * float(r.abs().max()))
            worst = max(worst, dist(s, r) / yard)
            assert dist(s, r) <= FACTOR * yard
            assert (s[:, 4] == 0).all() and (s[:, 0] != 0).any()  # env 4 ended on the rollout's last step
        # what the next update starts from is a copy of its own: the resets of the next rollout zero the memory's rows
        # in place (with the fused collection nothing rebinds them first) and must not reach it
        kept = alg.last_hidden_states[0]
        assert all(k is not s and torch.equal(k, s) for k, s in zip(kept, hs))
        want = [k.clone() for k in kept]
        dones = torch.tensor([1, 0, 0, 1, 0])
        alg._obs = alg._teacher_obs = alg._actions = alg._teacher_actions = None
        alg.storage.add = lambda *a: None
        alg.process_env_step(torch.zeros(N), dones, {})
        assert all((s[:, dones == 1] == 0).all() for s in alg.policy.get_hidden_states()[0])
        assert all(torch.equal(k, w) for k, w in zip(alg.last_hidden_states[0], want))
        assert all(torch.equal(k, w) for k, w in zip(alg._start_state(N), want)) and (want[0][:, 0] != 0).any()
    else:
        assert alg.policy.get_hidden_states() == (None, None)
    _ratios[(recurrent, loss_type)] = worst
    print(f"recurrent {recurrent} {loss_type}: largest error / yardstick {worst:.3f} (all cases so far: "
          f"{max(_ratios.values()):.3f})")


def test_update_schedule_counts_steps_across_epochs():
    ch = DS.update_segments(7, 2, 3)
    assert [c[1] for c in ch] == [True, True, True, True, False]
    assert ch[2][0] == [(0, 6, 7), (1, 0, 2)] and ch[4][0] == [(1, 5, 7)]
    assert DS.update_segments(8, 1, 4) == [([(0, 0, 4)], True), ([(0, 4, 8)], True)]
    assert DS.update_segments(2, 3, 15) == [([(0, 0, 2), (1, 0, 2), (2, 0, 2)], False)]
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a whole number of chunks: no warning
        alg = DS.Distillation(DS.StudentTeacher(4, 4, 2, student_hidden_dims=(4,), teacher_hidden_dims=(4,)),
                              gradient_length=4, device="cpu")
        alg.init_storage(3, 8, [4], [4], [2])
    with pytest.raises(ValueError, match="mse or huber"):
        DS.Distillation(DS.StudentTeacher(4, 4, 2), loss_type="l1", device="cpu")
    with pytest.raises(ValueError, match="recurrent student"):
        DS.Distillation(DS.StudentTeacher(4, 4, 2), fused_rnn_update=True, device="cpu")


# ---------------------------------------------------------------------------------------------- 3: the runner
class ToyStudentEnv(ToyEnv):
    """The toy point task with a "student" group: the policy row through noise.  The policy row is what the teacher
    reads."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.observation_manager.group_obs_dim["student"] = (6,)
        self.observation_manager.compute = self._obs

    def _obs(self):
        d = super()._obs()
        d["student"] = d["policy"] + 0.01 * torch.randn(self.num_envs, 6, generator=self.g)
        return d


def toy(cls=ToyStudentEnv, n=64):
    return RslRlVecEnvWrapper(cls(ToyEnvCfg(scene=type(ToyEnvCfg().scene)(num_envs=n))))


def runner_cfg(recurrent=False, **kw):
    c = RslRlOnPolicyRunnerCfg(device="cpu", num_steps_per_env=8, save_interval=1000, experiment_name="toy")
    if recurrent:
        c.policy = RslRlDistillationStudentTeacherRecurrentCfg(student_hidden_dims=[16], teacher_hidden_dims=[16],
                                                               rnn_hidden_dim=8)
    else:
        c.policy = RslRlDistillationStudentTeacherCfg(student_hidden_dims=[16], teacher_hidden_dims=[16])
    c.algorithm = RslRlDistillationAlgorithmCfg(gradient_length=4, learning_rate=3e-3)
    for k, v in kw.items():
        setattr(c, k, v)
    return c.to_dict()


def teacher_checkpoint(path, seed=5):
    torch.manual_seed(seed)
    ppo = ActorCritic(6, 6, 3, actor_hidden_dims=(16,), critic_hidden_dims=(16,))
    torch.save({"model_state_dict": ppo.state_dict(), "iter": 17, "infos": None}, path)
    return ppo


def test_runner_is_built_for_the_distillation_names_and_refuses_the_mismatches():
    r = OnPolicyRunner(toy(), runner_cfg(), log_dir=None, device="cpu")
    assert type(r) is DS.DistillationRunner and isinstance(r, OnPolicyRunner)
    assert isinstance(r.alg, DS.Distillation) and type(r.alg.policy) is DS.StudentTeacher
    assert r.obs_groups == {"student": "student", "teacher": "policy"}
    assert type(OnPolicyRunner(toy(), runner_cfg(True), log_dir=None, device="cpu").alg.policy) is DS.StudentTeacherRecurrent
    only_alg = runner_cfg()
    only_alg["policy"] = RslRlOnPolicyRunnerCfg().to_dict()["policy"]
    with pytest.raises(ValueError, match="needs a StudentTeacher"):
        OnPolicyRunner(toy(), only_alg, log_dir=None, device="cpu")
    only_policy = runner_cfg()
    only_policy["algorithm"] = RslRlOnPolicyRunnerCfg().to_dict()["algorithm"]
    with pytest.raises(ValueError, match="is trained by algorithm.class_name = 'Distillation'"):
        OnPolicyRunner(toy(), only_policy, log_dir=None, device="cpu")
    with pytest.raises(ValueError, match="no such observation group.*--distill"):
        OnPolicyRunner(toy(ToyEnv), runner_cfg(), log_dir=None, device="cpu")
    sym = runner_cfg()
    sym["algorithm"]["symmetry_cfg"] = dict(RslRlSymmetryCfg(use_mirror_loss=True).__dict__)
    with pytest.raises(ValueError, match="symmetry_cfg is not supported with Distillation"):
        OnPolicyRunner(toy(), sym, log_dir=None, device="cpu")
    with pytest.raises(ValueError, match="empirical_normalization is not supported with a recurrent student"):
        OnPolicyRunner(toy(), runner_cfg(True, empirical_normalization=True), log_dir=None, device="cpu")
    env = toy()
    env.shard = D.Shard(0, 2, 0, 0)
    with pytest.raises(ValueError, match="one GPU"):
        OnPolicyRunner(env, runner_cfg(), log_dir=None, device="cpu")
    # the PPO runner is what it was
    ppo = OnPolicyRunner(toy(), RslRlOnPolicyRunnerCfg(device="cpu").to_dict(), log_dir=None, device="cpu")
    assert type(ppo) is OnPolicyRunner
    other = RslRlOnPolicyRunnerCfg(device="cpu").to_dict()
    other["policy"]["class_name"] = "Transformer"
    with pytest.raises(ValueError, match="this runner builds"):
        OnPolicyRunner(toy(), other, log_dir=None, device="cpu")


def test_learn_refuses_without_a_teacher(tmp_path):
    r = OnPolicyRunner(toy(), runner_cfg(), log_dir=None, device="cpu")
    with pytest.raises(ValueError, match="needs a trained teacher"):
        r.learn(1)
    teacher_checkpoint(tmp_path / "teacher.pt")
    r.load(str(tmp_path / "teacher.pt"))
    assert r.alg.policy.loaded_teacher and r.current_learning_iteration == 0  # the teacher's iteration is not resumed
    r.learn(1)


@pytest.mark.parametrize("recurrent", [False, True], ids=["plain", "recurrent"])
def test_behaviour_loss_falls_and_the_checkpoint_round_trips(tmp_path, recurrent):
    torch.manual_seed(0)
    ppo = teacher_checkpoint(tmp_path / "teacher.pt")
    r = OnPolicyRunner(toy(), runner_cfg(recurrent), log_dir=str(tmp_path / "run"), device="cpu")
    r.load(str(tmp_path / "teacher.pt"))
    x = torch.randn(7, 6)
    assert torch.equal(r.alg.policy.evaluate(x), ppo.actor(x))
    r.learn(1)
    first = r.last_iteration_stats["Loss/behavior"]
    assert set(r.last_iteration_stats) >= {"Loss/behavior", "Loss/learning_rate", "Perf/total_fps"}
    assert "Loss/surrogate" not in r.last_iteration_stats
    r.learn(29)
    last = r.last_iteration_stats["Loss/behavior"]
    print(f"behaviour loss: iteration 1 {first:.4f}, iteration 30 {last:.4f}")
    assert last < first and r.current_learning_iteration == 30
    assert torch.equal(r.alg.policy.evaluate(x), ppo.actor(x))  # the teacher never moves
    ck = tmp_path / "run" / "model_30.pt"
    d = torch.load(ck, weights_only=True)
    assert set(d) >= {"model_state_dict", "optimizer_state_dict", "iter", "infos"} and d["iter"] == 30
    assert any(k.startswith("student.") for k in d["model_state_dict"])
    r2 = OnPolicyRunner(toy(), runner_cfg(recurrent), log_dir=None, device="cpu")
    r2.load(str(ck))  # a student checkpoint: a resume
    assert r2.current_learning_iteration == 30 and r2.alg.policy.loaded_teacher
    o = torch.randn(5, 6)
    assert torch.equal(r2.get_inference_policy()(o), r.get_inference_policy()(o))
    assert torch.equal(r2.get_inference_policy()(o), r2.alg.policy.student(
        r2.alg.policy.memory_s.rnn(o[None])[0][0] if recurrent else o))

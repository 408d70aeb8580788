"""CPU: the deploy config of a distilled student (h12env.export.deploy_config(cfg, group="student")) lists exactly the
terms the deploy stack's observation handler serves, with the student's history; the default group's output is what it
was; the cfg field and the scripts' flags."""
import json
import sys
from pathlib import Path

import pytest
import torch
import yaml

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "h1v2-isaac_amd" / "shims"), str(ROOT / "h1v2-isaac_amd" / "scripts")]

from h12env import cfg as K  # noqa: E402
from h12env.export import DeployObservations, deploy_config, write_env_yaml  # noqa: E402

TASKS = ("H12FlatEnvCfg", "H12RoughEnvCfg", "H12RslEnvCfg")
# what biped_deploy's ObservationHandler offers besides the phase terms
DEPLOY_TERMS = ["base_ang_vel", "projected_gravity", "generated_commands", "joint_pos_rel", "joint_vel_rel",
                "last_action"]


@pytest.mark.parametrize("name", TASKS)
@pytest.mark.parametrize("h", [1, 6])
def test_student_deploy_config_lists_the_six_deploy_terms(name, h):
    c = getattr(K, name)()
    before = json.loads(json.dumps(deploy_config(c)))
    with pytest.raises(ValueError, match="observations.student is not set"):
        deploy_config(c, group="student")
    c.observations.student = K.StudentObsCfg(history_length=h)
    d = deploy_config(c, group="student")
    assert [o["name"] for o in d["observations"]] == DEPLOY_TERMS
    assert all(set(o) == {"name"} for o in d["observations"])  # scale 1: no scale entry
    assert d["history_length"] == h and d["history_step"] == 1
    # everything that is not about the observation row is the policy group's
    for k in ("control_dt", "action_scale", "velocity_deadzone", "command_ranges", "joints"):
        assert d[k] == before[k], k
    # the default group is untouched by the new group: what it was before the group was set
    assert json.loads(json.dumps(deploy_config(c))) == before
    assert json.loads(json.dumps(deploy_config(c, group="policy"))) == before
    if name == "H12RoughEnvCfg":
        assert [o["name"] for o in before["observations"]][0] == "base_lin_vel" and \
            before["observations"][-1]["name"] == "height_scan"
    with pytest.raises(ValueError, match="policy or student"):
        deploy_config(c, group="critic")


def test_student_scales_reach_the_deploy_config_and_the_yaml(tmp_path):
    c = K.H12RoughEnvCfg()
    c.observations.student = K.StudentObsCfg(history_length=3, scales={"base_ang_vel": 0.25, "joint_vel": 0.05})
    d = deploy_config(c, group="student")
    assert d["observations"][0] == {"name": "base_ang_vel", "scale": 0.25}
    assert d["observations"][4] == {"name": "joint_vel_rel", "scale": 0.05}
    a = Path(write_env_yaml(c, str(tmp_path / "a" / "env.yaml"))).read_bytes()
    b = Path(write_env_yaml(K.H12RoughEnvCfg(), str(tmp_path / "b" / "env.yaml"))).read_bytes()
    assert a == b  # the default file is byte-identical with and without the group
    s = yaml.safe_load(Path(write_env_yaml(c, str(tmp_path / "s" / "env.yaml"), group="student")).read_text())
    assert s == json.loads(json.dumps(d))
    # the deploy-side handler builds the student's row from it: term-major, 45 H wide
    obs = DeployObservations(s, 4, "cpu")
    st = {"base_orientation": torch.tensor([[1.0, 0, 0, 0]]).repeat(4, 1), "base_angular_vel": torch.randn(4, 3),
          "qpos": torch.randn(4, 12), "qvel": torch.randn(4, 12)}
    row = obs(st, torch.zeros(4, 12), torch.zeros(4, 3))
    assert row.shape == (4, 45 * 3)
    assert torch.equal(row[:, 0:3], st["base_angular_vel"] * 0.25) and torch.equal(row[:, 6:9], row[:, 0:3])  # filled


@pytest.mark.parametrize("name", TASKS + ("H12CaTEnvCfg",))
def test_cfg_field_is_off_by_default_and_left_out_of_the_dumps(name):
    from isaaclab.utils.dict import class_to_dict

    c = getattr(K, name)()
    assert c.observations.student is None
    off = class_to_dict(c)
    assert "student" not in off["observations"]
    raw = bytes(c.to_c())
    K.enable_student_observations(c, 6)
    on = class_to_dict(c)
    assert on["observations"]["student"]["history_length"] == 6
    assert on["observations"]["student"]["base_ang_vel"] == {"n_min": -0.2, "n_max": 0.2}
    del on["observations"]["student"]
    assert on == off and bytes(c.to_c()) == raw  # the env's own config struct does not know the group
    K.enable_student_observations(c)  # again, without a history: the group is kept as it is
    assert c.observations.student.history_length == 6


def test_script_flags(tmp_path, monkeypatch):
    import train
    from isaaclab_rl.rsl_rl import RslRlOnPolicyRunnerCfg
    from toyenv import ToyEnvCfg

    args, _ = train.build_parser().parse_known_args(["--distill", "--teacher_checkpoint", "t.pt", "--student_recurrent",
                                                     "--student_history", "6", "--fused_rnn_update"])
    assert args.distill and args.teacher_checkpoint == "t.pt" and args.student_recurrent and args.student_history == 6
    none = train.build_parser().parse_known_args([])[0]
    assert not none.distill and none.teacher_checkpoint is None and none.student_history is None
    with pytest.raises(ValueError, match="--distill"):
        K.enable_student_observations(ToyEnvCfg())
    # the swap of the agent cfg's sections, from a PPO teacher checkpoint
    from h12env.ppo import ActorCritic

    torch.save({"model_state_dict": ActorCritic(235, 235, 12, actor_hidden_dims=(64, 32)).state_dict()}, tmp_path / "t.pt")
    agent, env_cfg = RslRlOnPolicyRunnerCfg(), K.H12RoughEnvCfg()
    agent.policy.actor_hidden_dims = [64, 32]
    agent.algorithm.learning_rate = 5e-4
    args.teacher_checkpoint = str(tmp_path / "t.pt")
    train.make_distillation(agent, env_cfg, args)
    d = agent.to_dict()
    assert d["policy"]["class_name"] == "StudentTeacherRecurrent" and d["algorithm"]["class_name"] == "Distillation"
    assert d["policy"]["student_hidden_dims"] == d["policy"]["teacher_hidden_dims"] == [64, 32]
    assert d["algorithm"]["learning_rate"] == 5e-4 and d["algorithm"]["gradient_length"] == 15
    assert env_cfg.observations.student.history_length == 6
    train.apply_cli(agent, env_cfg, args)
    assert agent.algorithm.fused_rnn_update is True
    args.teacher_checkpoint = None
    with pytest.raises(SystemExit, match="--teacher_checkpoint"):
        train.make_distillation(RslRlOnPolicyRunnerCfg(), K.H12RoughEnvCfg(), args)
    args.symmetry, args.resume = "both", True
    with pytest.raises(SystemExit, match="--symmetry"):
        train.make_distillation(RslRlOnPolicyRunnerCfg(), K.H12RoughEnvCfg(), args)
    assert "is_student_checkpoint" in (ROOT / "h1v2-isaac_amd" / "scripts" / "play.py").read_text()


def test_resume_and_play_rebuild_the_run_from_its_checkpoint_and_params(tmp_path, monkeypatch):
    """train.py --distill --resume without a teacher checkpoint, and play.py, take the policy sections (a recurrent
    teacher's memory included) and the history from the student checkpoint, and the group's scales and noise from the
    run's params/env.yaml."""
    import train
    from h12env import distill as DS
    from isaaclab.utils.io import dump_yaml
    from isaaclab_rl.rsl_rl import RslRlOnPolicyRunnerCfg

    run = tmp_path / "logs" / "rsl_rl" / "default" / "2026-01-01_00-00-00_student"
    trained = K.H12RoughEnvCfg()
    trained.observations.student = K.StudentObsCfg(history_length=4, scales={"base_ang_vel": 0.25, "joint_vel": 0.05})
    trained.observations.student.joint_vel = K.Unoise(-0.5, 0.5)
    trained.observations.student.projected_gravity = None
    dump_yaml(str(run / "params" / "env.yaml"), trained)
    p = DS.StudentTeacherRecurrent(45 * 4, 235, 12, student_hidden_dims=(32,), teacher_hidden_dims=(64, 32),
                                   rnn_hidden_dim=24, teacher_recurrent=True)
    torch.save({"model_state_dict": p.state_dict(), "iter": 7}, run / "model_7.pt")
    monkeypatch.chdir(tmp_path)
    args, _ = train.build_parser().parse_known_args(["--distill", "--resume", "True"])
    agent, env_cfg = RslRlOnPolicyRunnerCfg(), K.H12RoughEnvCfg()
    train.make_distillation(agent, env_cfg, args)
    d = agent.to_dict()["policy"]
    assert d["class_name"] == "StudentTeacherRecurrent" and d["teacher_recurrent"] is True and d["rnn_hidden_dim"] == 24
    assert d["student_hidden_dims"] == [32] and d["teacher_hidden_dims"] == [64, 32]
    assert agent.to_dict()["algorithm"]["class_name"] == "Distillation"
    g = env_cfg.observations.student
    assert g.history_length == 4 and g.scales == {"base_ang_vel": 0.25, "joint_vel": 0.05} and g.enable_corruption
    assert (g.joint_vel.n_min, g.joint_vel.n_max) == (-0.5, 0.5) and g.projected_gravity is None
    assert (g.base_ang_vel.n_max, g.velocity_commands) == (0.2, None)
    q = DS.StudentTeacherRecurrent(45 * 4, 235, 12, **{k: v for k, v in d.items() if k != "class_name"})
    assert q.load_state_dict(p.state_dict()) is True
    # the exported env.yaml of that group carries the scales
    obs = deploy_config(env_cfg, group="student")["observations"]
    assert obs[0] == {"name": "base_ang_vel", "scale": 0.25} and obs[4] == {"name": "joint_vel_rel", "scale": 0.05}
    args.student_history = 6
    with pytest.raises(SystemExit, match="--student_history 6"):
        train.make_distillation(RslRlOnPolicyRunnerCfg(), K.H12RoughEnvCfg(), args)
    with pytest.raises(ValueError, match="history_length 4"):
        DS.student_group_from_run(run, 6)
    assert DS.student_group_from_run(tmp_path, 3) == K.StudentObsCfg(history_length=3)  # no params file: the defaults
    play = (ROOT / "h1v2-isaac_amd" / "scripts" / "play.py").read_text()
    assert "student_group_from_run" in play and "enable_corruption = False" in play


def test_checkpoint_describes_its_own_policy_cfg():
    from h12env import distill as DS

    for cls, kw in ((DS.StudentTeacher, {}), (DS.StudentTeacherRecurrent, {"rnn_hidden_dim": 12}),
                    (DS.StudentTeacherRecurrent, {"rnn_hidden_dim": 12, "teacher_recurrent": True, "rnn_type": "gru"})):
        p = cls(45 * 6, 235, 12, student_hidden_dims=(32, 16), teacher_hidden_dims=(64,), **kw)
        sd = p.state_dict()
        assert DS.is_student_checkpoint(sd)
        pol, h = DS.cfg_from_checkpoint(sd)
        assert h == 6 and pol["class_name"] == cls.__name__
        assert pol["student_hidden_dims"] == [32, 16] and pol["teacher_hidden_dims"] == [64]
        q = cls(45 * h, 235, 12, **{k: v for k, v in pol.items() if k != "class_name"})
        assert q.load_state_dict(sd) is True
    from h12env.ppo import ActorCritic

    assert not DS.is_student_checkpoint(ActorCritic(45, 45, 12).state_dict())
    v = DS.StudentView(p)
    assert v.actor is p.student and v.memory_a is p.memory_s and v.is_recurrent

"""CPU: scripts/train.py builds the recurrent policy from ``--recurrent`` (with the rnn overrides it makes available) and
from the ``agent.policy.class_name=ActorCriticRecurrent`` override alone, on the toy env of tests/test_train_script.py."""
import torch

from test_train_script import run


def trained(tmp_path, *extra):
    r = run(tmp_path, "--max_iterations", "1", *extra)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    (run_dir,) = sorted((tmp_path / "logs" / "rsl_rl" / "toy_train").iterdir())
    sd = torch.load(run_dir / "model_1.pt", map_location="cpu", weights_only=True)["model_state_dict"]
    return sd, (run_dir / "params" / "agent.yaml").read_text()


def test_recurrent_flag_keeps_the_tasks_hidden_dims_and_opens_the_rnn_overrides(tmp_path):
    sd, agent = trained(tmp_path, "--recurrent", "agent.policy.rnn_hidden_dim=24")
    assert sd["memory_a.rnn.weight_hh_l0"].shape == (96, 24) and sd["memory_c.rnn.weight_ih_l0"].shape == (96, 6)
    assert sd["actor.0.weight"].shape == (16, 24) and sd["critic.0.weight"].shape == (16, 24)  # the task's [16]
    assert "class_name: ActorCriticRecurrent" in agent and "rnn_hidden_dim: 24" in agent


def test_class_name_override_alone_builds_the_recurrent_class(tmp_path):
    sd, agent = trained(tmp_path, "agent.policy.class_name=ActorCriticRecurrent")
    assert sd["memory_a.rnn.weight_hh_l0"].shape == (1024, 256) and sd["actor.0.weight"].shape == (16, 256)
    assert "class_name: ActorCriticRecurrent" in agent

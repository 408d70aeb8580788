"""CPU: the host side of the privileged ("critic") observation group -- the cfg field leaves every default output as it
was, the mirror table of the critic row, the runner with a critic group and symmetry on, and the checkpoint-width
error of OnPolicyRunner.load."""
import hashlib
import json
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd" / "shims"))

from h12env import cfg as K  # noqa: E402
from h12env import priv  # noqa: E402
from h12env import symmetry as S  # noqa: E402
from h12env.ppo import OnPolicyRunner  # noqa: E402

TASKS = ("H12FlatEnvCfg", "H12RoughEnvCfg", "H12RslEnvCfg", "H12CaTEnvCfg")
GOLDEN = json.loads((ROOT / "tests" / "golden" / "default_cfg_surface.json").read_text())


def with_critic(name):
    c = getattr(K, name)()
    c.observations.critic = K.CriticObsCfg()
    return c


# ---------------------------------------------------------------------------------------------- 1. the cfg field
@pytest.mark.parametrize("name", TASKS)
def test_default_cfg_outputs_are_those_of_the_cfg_without_the_field(name):
    """tests/golden/default_cfg_surface.json was written by tools/gen_golden_default_cfg.py before
    ObservationsCfg.critic existed."""
    from isaaclab.utils.dict import class_to_dict

    from h12env.export import deploy_config

    c = getattr(K, name)()
    assert c.observations.critic is None
    want = GOLDEN[name]
    assert json.loads(json.dumps(class_to_dict(c))) == want["to_dict"]
    assert json.loads(json.dumps(deploy_config(c))) == want["env_yaml"]
    assert hashlib.sha256(bytes(c.to_c())).hexdigest() == want["to_c_sha256"]


def test_env_yaml_text_is_the_same_with_and_without_the_group(tmp_path):
    from isaaclab.utils.io import dump_yaml

    from h12env.export import write_env_yaml

    a = Path(write_env_yaml(K.H12FlatEnvCfg(), str(tmp_path / "a" / "env.yaml"))).read_bytes()
    b = Path(write_env_yaml(with_critic("H12FlatEnvCfg"), str(tmp_path / "b" / "env.yaml"))).read_bytes()
    assert a == b  # the deploy file describes the actor's input alone
    dump_yaml(str(tmp_path / "off.yaml"), K.H12FlatEnvCfg())
    dump_yaml(str(tmp_path / "on.yaml"), with_critic("H12FlatEnvCfg"))
    off, on = (tmp_path / "off.yaml").read_text(), (tmp_path / "on.yaml").read_text()
    assert "critic" not in off and "critic:" in on


def test_the_group_is_dumped_when_it_is_on_and_to_c_does_not_change():
    from isaaclab.utils.dict import class_to_dict

    c = with_critic("H12RslEnvCfg")
    d = class_to_dict(c)["observations"]
    assert d["critic"] == {"enable_corruption": False, "concatenate_terms": True, "history_length": 0, "scales": {}}
    assert bytes(c.to_c()) == bytes(K.H12RslEnvCfg().to_c())
    assert K.CriticObsCfg().history_length == 0 and K.CriticObsCfg().concatenate_terms


def test_scales_come_from_the_policy_group_and_the_critic_cfg():
    c = with_critic("H12RslEnvCfg")
    s = priv.term_scales(c)
    assert s["base_ang_vel"] == 0.25 and s["joint_vel"] == 0.05 and s["joint_pos"] == 1.0
    assert s["base_lin_vel"] == 1.0 and s["height_scan"] == 1.0 and s["base_height"] == 1.0
    from h12env.model import model_dict

    d = model_dict()
    mass = d["base"]["mass"] + sum(j["mass"] for j in d["joints"])
    assert 60.0 < mass < 75.0
    assert s["feet_force"] == pytest.approx(1.0 / (mass * 9.81), rel=1e-12)
    assert 600.0 * s["feet_force"] < 1.0  # a standing robot's foot force is below one body weight
    c.observations.critic.scales = {"feet_force": 1.0, "base_height": 2.0}
    s = priv.term_scales(c)
    assert s["feet_force"] == 1.0 and s["base_height"] == 2.0
    c.observations.critic.scales = {"joint_vel": 2.0}  # a shared term: its scale is the policy group's
    with pytest.raises(ValueError, match="joint_vel"):
        priv.term_scales(c)


def test_flag_helper_switches_the_group_on_and_refuses_other_cfgs():
    from toyenv import ToyEnvCfg

    c = K.H12FlatEnvCfg()
    K.enable_privileged_critic(c)
    assert isinstance(c.observations.critic, K.CriticObsCfg)
    with pytest.raises(ValueError, match="privileged_critic"):
        K.enable_privileged_critic(ToyEnvCfg())
    sys.path.insert(0, str(ROOT / "h1v2-isaac_amd" / "scripts"))
    import train

    args, _ = train.build_parser().parse_known_args(["--privileged_critic", "--symmetry", "both"])
    assert args.privileged_critic and args.symmetry == "both"
    assert not train.build_parser().parse_known_args([])[0].privileged_critic
    for script in ("play.py", "eval_policy.py"):
        assert "--privileged_critic" in (ROOT / "h1v2-isaac_amd" / "scripts" / script).read_text()


# ---------------------------------------------------------------------------------------------- 2. the mirror table
@pytest.mark.parametrize("name", TASKS)
def test_critic_mirror_table_is_an_involution_of_the_row_width(name):
    c = with_critic(name)
    t = S.mirror_table(c, "critic")
    terrain = c.scene.height_scanner is not None
    assert t.width == (252 if terrain else 65) == priv.layout(terrain)[0]
    x = torch.randn(5, t.width, generator=torch.Generator().manual_seed(0))
    assert torch.equal(t.mirror(t.mirror(x)), x)
    assert not torch.equal(t.mirror(x), x)
    with pytest.raises(ValueError):
        S.mirror_table(getattr(K, name)(), "critic")  # no group, no table


@pytest.mark.parametrize("terrain", [False, True], ids=["plane", "terrain"])
def test_critic_mirror_rules_term_by_term(terrain):
    """On a row whose entries are their own column index (+ 1, so that a sign flip shows in column 0 too)."""
    c = with_critic("H12RoughEnvCfg" if terrain else "H12FlatEnvCfg")
    t = S.mirror_table(c, "critic")
    w, table = priv.layout(terrain)
    row = torch.arange(1, w + 1, dtype=torch.float32)
    m = t.mirror(row[None])[0]
    off = {name: o for name, o, _ in table}
    col = lambda name, k: float(off[name] + k + 1)  # noqa: E731
    for name, sign in (("base_lin_vel", (1, -1, 1)), ("projected_gravity", (1, -1, 1)), ("base_ang_vel", (-1, 1, -1)),
                       ("velocity_commands", (1, -1, -1))):
        for k in range(3):
            assert m[off[name] + k] == sign[k] * col(name, k), (name, k)
    from h12env.model import joint_names

    names = joint_names()
    for term in ("joint_pos", "joint_vel", "actions"):
        for j, n in enumerate(names):
            partner = names.index(n.replace("left_", "right_") if n.startswith("left_") else n.replace("right_", "left_"))
            sign = -1.0 if ("_yaw_" in n or "_roll_" in n) else 1.0
            assert m[off[term] + j] == sign * col(term, partner), (term, n)
    if terrain:
        for iy in range(11):
            for ix in range(17):
                assert m[off["height_scan"] + iy * 17 + ix] == col("height_scan", (10 - iy) * 17 + ix)
    for name in ("base_height", "added_mass"):
        assert m[off[name]] == col(name, 0)
    for k in range(3):
        assert m[off["actuator_lag"] + k] == col("actuator_lag", k)
    for name in ("feet_contact", "feet_air_time", "feet_contact_time", "feet_force"):
        assert m[off[name]] == col(name, 1) and m[off[name] + 1] == col(name, 0), name
    # H12_F_MU is [static L, dynamic L, static R, dynamic R] (h12env.startup): the soles swap, the pair's order stays
    assert [float(m[off["sole_friction"] + k]) for k in range(4)] == [col("sole_friction", k) for k in (2, 3, 0, 1)]
    startup = (ROOT / "h1v2-isaac_amd" / "h12env" / "startup.py").read_text()
    assert "[mu_s L, mu_d L, mu_s R, mu_d R]" in startup
    with pytest.raises(ValueError):
        S._term_rule("foot_contact")  # not one of the group's names


# ---------------------------------------------------------------------------------------------- 3. the runner
def critic_toy(num_envs=16):
    """The symmetric toy point task with a 9-wide critic group (target - x, x, target): three polar vectors."""
    from toy_sym import POLAR_FLIP, ToyEnvCfg, ToySymEnv

    class ToyCriticEnv(ToySymEnv):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.observation_manager.group_obs_dim["critic"] = (9,)
            self.mirror_tables["critic"] = S.MirrorTable(list(range(9)), POLAR_FLIP * 3)

        def _obs(self):
            d = super()._obs()
            d["critic"] = torch.cat([d["policy"], self.target], dim=1)
            return d

    return ToyCriticEnv(ToyEnvCfg(scene=type(ToyEnvCfg().scene)(num_envs=num_envs)))


def runner_cfg(symmetry=True):
    from isaaclab_rl.rsl_rl import RslRlOnPolicyRunnerCfg, RslRlSymmetryCfg

    c = RslRlOnPolicyRunnerCfg(device="cpu", num_steps_per_env=8, save_interval=1000, experiment_name="toy")
    c.policy.actor_hidden_dims = c.policy.critic_hidden_dims = [16]
    if symmetry:
        c.algorithm.symmetry_cfg = RslRlSymmetryCfg(use_data_augmentation=True, use_mirror_loss=True,
                                                    mirror_loss_coeff=0.3,
                                                    data_augmentation_func="h12env.symmetry:augment")
    return c.to_dict()


def test_runner_iteration_with_a_critic_group_and_symmetry(tmp_path):
    from isaaclab_rl.rsl_rl import RslRlVecEnvWrapper

    env = RslRlVecEnvWrapper(critic_toy())
    assert env.num_privileged_obs == 9
    runner = OnPolicyRunner(env, runner_cfg(), log_dir=str(tmp_path), device="cpu")
    assert runner.alg.policy.critic[0].weight.shape[1] == 9 and runner.alg.policy.actor[0].weight.shape[1] == 6
    assert runner.alg.storage.t["privileged_observations"].shape[-1] == 9
    before = [p.clone() for p in runner.alg.policy.critic.parameters()]
    runner.learn(1)
    line = json.loads((tmp_path / "metrics.jsonl").read_text().splitlines()[0])
    assert all(torch.isfinite(torch.tensor(line[k])) for k in ("Loss/value_function", "Loss/surrogate", "Loss/symmetry"))
    assert any(not torch.equal(p, q) for p, q in zip(before, runner.alg.policy.critic.parameters()))


def test_load_refuses_a_checkpoint_of_another_critic_width(tmp_path):
    from isaaclab_rl.rsl_rl import RslRlVecEnvWrapper
    from toy_sym import ToyEnvCfg, ToySymEnv

    wide = OnPolicyRunner(RslRlVecEnvWrapper(critic_toy()), runner_cfg(False), log_dir=None, device="cpu")
    plain_env = RslRlVecEnvWrapper(ToySymEnv(ToyEnvCfg(scene=type(ToyEnvCfg().scene)(num_envs=16))))
    plain = OnPolicyRunner(plain_env, runner_cfg(False), log_dir=None, device="cpu")
    wide.save(str(tmp_path / "wide.pt"))
    plain.save(str(tmp_path / "plain.pt"))
    with pytest.raises(ValueError, match=r"9-wide.*6 wide.*--privileged_critic"):
        plain.load(str(tmp_path / "wide.pt"))
    with pytest.raises(ValueError, match=r"6-wide.*9 wide.*--privileged_critic"):
        wide.load(str(tmp_path / "plain.pt"))
    wide2 = OnPolicyRunner(RslRlVecEnvWrapper(critic_toy()), runner_cfg(False), log_dir=None, device="cpu")
    wide2.load(str(tmp_path / "wide.pt"))  # the matching width loads as before
    for p, q in zip(wide.alg.policy.parameters(), wide2.alg.policy.parameters()):
        assert torch.equal(p, q)

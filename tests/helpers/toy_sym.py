"""The CPU toy env (toyenv.ToyEnv) with its own mirror tables: the point task is symmetric under y -> -y, so both
halves of the observation (target - x, x) and the action are polar vectors (x, -y, z).  h12env.symmetry reads the
tables from ``env.unwrapped.mirror_tables``, the hook for envs that are not the H1-2 env."""
from __future__ import annotations

from h12env.symmetry import MirrorTable
from toyenv import ToyEnv, ToyEnvCfg  # noqa: F401  (ToyEnvCfg: the registry's cfg entry point)

POLAR_FLIP = [False, True, False]


class ToySymEnv(ToyEnv):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.mirror_tables = {"policy": MirrorTable(list(range(6)), POLAR_FLIP * 2),
                              "actions": MirrorTable(list(range(3)), POLAR_FLIP)}

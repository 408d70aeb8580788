#!/usr/bin/env python3
"""tests/golden/default_cfg_surface.json: what the shipped task cfgs serialise to -- class_to_dict (the params/env.yaml
dump of the training scripts), the deploy env.yaml (h12env.export.deploy_config) and the sha256 of the C config struct
(to_c()) -- per task.  tests/test_priv_host.py pins them: an optional cfg field that is left at None must not change
any of the three.  Regenerate only when a task's default configuration changes on purpose."""
from __future__ import annotations

import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd"))
sys.path.insert(0, str(ROOT / "h1v2-isaac_amd" / "shims"))

TASKS = ("H12FlatEnvCfg", "H12RoughEnvCfg", "H12RslEnvCfg", "H12CaTEnvCfg")


def surface(cfg) -> dict:
    from isaaclab.utils.dict import class_to_dict

    from h12env.export import deploy_config

    return {"to_dict": json.loads(json.dumps(class_to_dict(cfg))), "env_yaml": json.loads(json.dumps(deploy_config(cfg))),
            "to_c_sha256": hashlib.sha256(bytes(cfg.to_c())).hexdigest()}


def main():
    from h12env import cfg as K

    out = {name: surface(getattr(K, name)()) for name in TASKS}
    path = ROOT / "tests" / "golden" / "default_cfg_surface.json"
    path.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()

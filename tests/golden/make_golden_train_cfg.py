"""Generate tests/golden/isfusion_0075voxel_train.txt: the training-recipe variables (`optimizer`, `optimizer_config`,
`lr_config`, `momentum_config`, `total_epochs`) of the REFERENCE's unmodified configs/isfusion/isfusion_0075voxel.py, as
evaluated by isfusion_amd.registry.load_config, written as a Python literal (read back with ast.literal_eval).

    python tests/golden/make_golden_train_cfg.py      # authoring container only

Only the evaluated values are stored, not the config file."""
import ast
import os
import pprint
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from isfusion_amd import registry  # noqa: E402

REF = os.environ.get("ISF_REFERENCE_ROOT", "/root/reference")
KEYS = ("optimizer", "optimizer_config", "lr_config", "momentum_config", "total_epochs")


def main():
    cfg = registry.load_config(os.path.join(REF, "configs", "isfusion", "isfusion_0075voxel.py"))
    train = {k: cfg[k] for k in KEYS}
    text = pprint.pformat(train, width=120, sort_dicts=False) + "\n"
    assert ast.literal_eval(text) == train
    with open(os.path.join(HERE, "isfusion_0075voxel_train.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

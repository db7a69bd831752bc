"""Config-driven entry point for the baseline counters — drop-in for the reference's main_base.py
(main_base.py:35-157): the YAML schema and the factories of `dgvcc_amd.main`, with main_base.py's
model table behind `get_model`:

* 'dgnet' -> models2.DensityRegressorBase (as `dgvcc_amd.main`), 'csrnet' -> baselines.CSRNet,
  'mcnn' -> baselines.MCNN, 'bl' -> baselines.BL_VGG;
* 'sasnet', 'dssinet', 'cctrans' are not built and raise NotImplementedError;
* any other name raises ValueError (main_base.py:50-51).

The reference runs these through BaseTrainer: `model(img)` and the count loss, no `mode`, no
`patch_size`.  Here that is DGTrainer in 'simple' mode with the config's `patch_size` or 10000, for
every model of this table; losses, datasets, optimizers and schedulers are `main`'s, including the
`loss: bl` checks on the train set's crop.

    python -m dgvcc_amd.main_base --config configs/bl.yml --task train
"""
from __future__ import annotations

from . import main as _main
from .main import get_dataset, get_loss, get_optimizer, get_scheduler  # noqa: F401

_NOT_BUILT = ("sasnet", "dssinet", "cctrans")


def get_model(name, params):
    from .models import baselines as B
    from .models import models2 as M2
    table = {"dgnet": M2.DensityRegressorBase, "csrnet": B.CSRNet, "mcnn": B.MCNN, "bl": B.BL_VGG}
    if name in table:
        return table[name](**params)
    if name in _NOT_BUILT:
        raise NotImplementedError(f"model '{name}' is not built yet (DESIGN.md §7)")
    raise ValueError(f"Unknown model: {name}")


def load_config(config_path, task):
    return _main.load_config(config_path, task, model_factory=get_model, simple=True)


def main(argv=None):
    _main.main(argv, loader=load_config)


if __name__ == "__main__":
    main()

"""Drop-in `datasets.jhu_domain_dataset.JHUDomainDataset` (reference
datasets/jhu_domain_dataset.py:18-225): DensityMapDataset's per-sample pipeline (grey, random
rescale, pad, crop, downsample, flip; the rescale on the GPU, see den_dataset.py) over the file
lists of the JHU cross-domain splits, `<root>/domains/<domain_label>_<train|val>.txt` (test reads
the val list).  Train files: `<name>_dmap.npy`; no ROI map, no `gt_dir`, no generated-image root.
"""
from __future__ import annotations

from .den_dataset import _check_crop, collate_rescaled, rescale_train_transform
from .jhu_domain_cls_dataset import JHUDomainClsDataset


class JHUDomainDataset(JHUDomainClsDataset):
    """Constructor arguments as the reference."""
    dmap_suffix = "_dmap"

    def __init__(self, root, domain_label, crop_size, domain_type, domain, downsample, method, is_grey=False,
                 unit_size=0, pre_resize=1):
        super().__init__(root, domain_label, crop_size, domain_type, domain, downsample, method, is_grey=is_grey,
                         unit_size=unit_size, pre_resize=pre_resize)
        _check_crop(self)

    def _train_transform(self, img, gt, dmap):
        return rescale_train_transform(self, img, gt, dmap)

    collate = staticmethod(collate_rescaled)

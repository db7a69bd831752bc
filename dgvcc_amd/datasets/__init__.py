"""Datasets with GPU-side augmentation."""
from .augment import (DeviceAugment, RawDenBatch, RawDenClsBatch, augment_den_cls, block_map,  # noqa: F401
                      resize_crop)
from .den_cls_dataset import DenClsDataset, augment_val_sample  # noqa: F401
from .den_dataset import DensityMapDataset  # noqa: F401
from .jhu_domain_cls_dataset import JHUDomainClsDataset  # noqa: F401
from .jhu_domain_dataset import JHUDomainDataset  # noqa: F401

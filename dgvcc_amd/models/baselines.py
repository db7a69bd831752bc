"""Drop-in MI355X implementation of the reference's baseline counters (models/baselines/).

  CSRNet   models/baselines/CSRNet.py:10-64: the first ten VGG16 convolutions (no BatchNorm, three
           MaxPool2d(2)), six 3x3 convolutions with dilation 2 and a 1x1 64->1 output layer;
           forward(x [B,3,H,W]) -> [B,1,H/8,W/8].

Same sub-module names, and therefore the same `state_dict` keys, as the reference
(`tests/golden/csrnet_keys.json`).  The whole network is one `plans2.ChainPlan`: the dilated back
end runs on the dense 3x3 kernels over the polyphase sub-images of its input.
"""
from __future__ import annotations

import torch.nn as nn

from . import plans2 as P2
from .models import _DGBase

__all__ = ["CSRNet", "make_layers"]


def make_layers(cfg, in_channels=3, batch_norm=False, dilation=False):
    """reference models/baselines/CSRNet.py:47-64."""
    d_rate = 2 if dilation else 1
    layers = []
    for v in cfg:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            continue
        conv = nn.Conv2d(in_channels, v, kernel_size=3, padding=d_rate, dilation=d_rate)
        layers += [conv, nn.BatchNorm2d(v), nn.ReLU(inplace=True)] if batch_norm else [conv, nn.ReLU(inplace=True)]
        in_channels = v
    return nn.Sequential(*layers)


class CSRNet(_DGBase):
    """load_weights=True applies the reference's `_initialize_weights` (normal(0, 0.01) filters, zero
    biases).  The reference then copies torchvision's pretrained VGG16 into the front end, a remote
    download: this package never downloads, load such weights with `load_state_dict`."""

    def __init__(self, load_weights=False):
        super().__init__()
        self._init_precision()
        self.frontend_feat = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512]
        self.backend_feat = [512, 512, 512, 256, 128, 64]
        self.frontend = make_layers(self.frontend_feat)
        self.backend = make_layers(self.backend_feat, in_channels=512, dilation=True)
        self.output_layer = nn.Conv2d(64, 1, kernel_size=1)
        if load_weights:
            self._initialize_weights()
        self._plans = None

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_plans"] = None
        return st

    def _initialize_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, std=0.01)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def forward(self, x):
        if x.shape[-2] % 8 or x.shape[-1] % 8:
            raise ValueError(f"CSRNet: H, W must be multiples of 8 (got {x.shape[-2]}x{x.shape[-1]})")
        if self._plans is None:
            mods = list(self.frontend) + list(self.backend) + [self.output_layer]
            self._plans = {"net": P2.ChainPlan(mods, image_input=True)}
        return P2.run_chain(self._plans["net"], (x,), self.training, self.compute_dtype)

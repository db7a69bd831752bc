"""Drop-in MI355X implementation of the reference's baseline counters (models/baselines/).

  CSRNet   models/baselines/CSRNet.py:10-64: the first ten VGG16 convolutions (no BatchNorm, three
           MaxPool2d(2)), six 3x3 convolutions with dilation 2 and a 1x1 64->1 output layer;
           forward(x [B,3,H,W]) -> [B,1,H/8,W/8].

  MCNN     models/baselines/MCNN.py:7-74: three columns of four convolutions (9/7/7/7, 7/5/5/5 and
           5/3/3/3 filters, 3..48 channels, no BatchNorm, two MaxPool2d(2) each) on the same image,
           and a 1x1 30->1 layer on their concatenation; forward(x [B,3,H,W]) -> [B,1,H/4,W/4].

  BL_VGG   models/baselines/BL.py:11-56: the sixteen VGG19 ("E") convolutions with four MaxPool2d(2)
           (no BatchNorm), a x2 align-corners bilinear upsampling, 512->256->128 in 3x3, a 1x1 128->1
           layer and torch.abs; forward(x [B,3,H,W]) -> [B,1,H/8,W/8], the Bayesian loss's grid.

Same sub-module names, and therefore the same `state_dict` keys, as the reference
(`tests/golden/csrnet_keys.json`, `tests/golden/mcnn_keys.json`, `tests/golden/blvgg_keys.json`).
CSRNet is one `plans2.ChainPlan`:
the dilated back end runs on the dense 3x3 kernels over the polyphase sub-images of its input
(DESIGN.md §3.3).  MCNN's columns are three ChainPlans of small-channel layers on
one padded NHWC image, writing into channel slices of one concatenation buffer that the 1x1 layer
reads as a head.  BL_VGG is one ChainPlan whose head returns |z|.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import engine as E
from .. import kernels as K
from ..kernels import Act
from . import plans2 as P2
from .models import _DGBase, _load_pretrained_vgg

__all__ = ["CSRNet", "MCNN", "VGG", "BL_VGG", "make_layers"]

# reference models/baselines/BL.py:45-47
cfg = {"E": [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512]}


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


class MCNNPlan:
    """MCNN as HIP launches: dg_image_nhwc_pad once, the three columns (ChainPlans of
    engine.SmallConvLayer and MaxPool2d(2)) each writing its last layer into its slice of an
    [N, H/4, W/4, 8 + 16 + 16] buffer (8 / 10 / 12 channels padded to multiples of 8, zeros between),
    and `fuse` as one dg_head_fwd over that buffer with the 30 weights spread to their channels."""

    def __init__(self, model):
        self.chains = [P2.ChainPlan(b, input_grad=False) for b in (model.branch1, model.branch2, model.branch3)]
        self.fuse = model.fuse[0]
        self.widths = [c.ops[-1][1].Cp_out for c in self.chains]
        idx, off = [], 0
        for c, wd in zip(self.chains, self.widths):
            idx += list(range(off, off + c.ops[-1][1].Cout))
            off += wd
        self.idx = idx  # position of each of the 30 concatenated channels in the padded buffer

    def params(self):
        return [p for c in self.chains for p in c.params()] + [self.fuse.weight, self.fuse.bias]

    def _weight(self, dev):
        w = torch.zeros(sum(self.widths), dtype=torch.float32, device=dev)
        w[torch.as_tensor(self.idx, device=dev)] = self.fuse.weight.detach().reshape(-1).float()
        return w

    def forward(self, img, dt, training, tape=None):
        N, _, H, W = img.shape
        x = Act(K.image_nhwc_pad(img, dt))
        cat = K.nhwc(N, H // 4, W // 4, sum(self.widths), dt, img.device)
        off = 0
        for c, wd in zip(self.chains, self.widths):
            c.run(x, dt, training, tape, out=Act(cat, off, wd))
            off += wd
        w = self._weight(img.device)
        y = K.head_fwd(Act(cat), w, self.fuse.bias.detach(), K.ACT_NONE)
        if tape is not None:
            tape[self] = (cat, w, y)
        return y.unsqueeze(1)

    def backward(self, tape, g):
        cat, w, y = tape.pop(self)
        gcat = torch.empty_like(cat)
        gw = torch.empty_like(w)
        gb = torch.empty(1, dtype=torch.float32, device=w.device)
        K.head_bwd(Act(cat), w, K.ACT_NONE, y, g.float().contiguous(), Act(gcat), gw, gb)
        grads = {self.fuse.weight: gw[torch.as_tensor(self.idx, device=w.device)].reshape(self.fuse.weight.shape),
                 self.fuse.bias: gb}
        off = 0
        for c, wd in zip(self.chains, self.widths):
            gr, _ = c.back(tape, Act(gcat, off, wd))
            for p, gp in gr.items():
                E._acc(grads, p, gp)
            off += wd
        return (), grads


class MCNN(_DGBase):
    """The reference's flag is inverted and kept so: load_weights=False runs `_initialize_weights`
    (kaiming_normal_ filters, zero biases); load_weights=True leaves torch's default initialisation for
    a `load_state_dict` to overwrite."""

    def __init__(self, load_weights=False):
        super().__init__()
        self._init_precision()

        def column(cfg):
            layers, cin = [], 3
            for i, (cout, k) in enumerate(cfg):
                layers += [nn.Conv2d(cin, cout, k, padding=k // 2), nn.ReLU(inplace=True)]
                if i < 2:
                    layers.append(nn.MaxPool2d(2))
                cin = cout
            return nn.Sequential(*layers)

        self.branch1 = column([(16, 9), (32, 7), (16, 7), (8, 7)])
        self.branch2 = column([(20, 7), (40, 5), (20, 5), (10, 5)])
        self.branch3 = column([(24, 5), (48, 3), (24, 3), (12, 3)])
        self.fuse = nn.Sequential(nn.Conv2d(30, 1, 1, padding=0))
        if not load_weights:
            self._initialize_weights()
        self._plans = None

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_plans"] = None
        return st

    def _initialize_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def forward(self, x):
        if x.shape[-2] % 4 or x.shape[-1] % 4:
            raise ValueError(f"MCNN: H, W must be multiples of 4 (got {x.shape[-2]}x{x.shape[-1]})")
        if self._plans is None:
            self._plans = {"net": MCNNPlan(self)}
        plan = self._plans["net"]
        dt, training = self.compute_dtype, self.training
        return E.run_plan(plan, lambda img, tape: plan.forward(img, dt, training, tape), (x,), plan.params())


class VGG(_DGBase):
    """reference models/baselines/BL.py:11-27: `features`, bilinear x2 (align_corners=True), `reg_layer`
    and torch.abs, as one ChainPlan: the upsampling is dg_upsample_fwd's UP_BILINEAR_AC and the abs is
    dg_abs_fwd on the head's map, with the signed map on the tape for dg_abs_bwd."""

    def __init__(self, features):
        super().__init__()
        self._init_precision()
        self.features = features
        self.reg_layer = nn.Sequential(
            nn.Conv2d(512, 256, kernel_size=3, padding=1),
            nn.ReLU(inplace=True),
            nn.Conv2d(256, 128, kernel_size=3, padding=1),
            nn.ReLU(inplace=True),
            nn.Conv2d(128, 1, 1))
        self._plans = None

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_plans"] = None
        return st

    def forward(self, x):
        if x.shape[-2] % 16 or x.shape[-1] % 16:
            raise ValueError(f"BL_VGG: H, W must be multiples of 16 (got {x.shape[-2]}x{x.shape[-1]})")
        if self._plans is None:
            up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)  # F.upsample_bilinear
            mods = list(self.features) + [up] + list(self.reg_layer)
            self._plans = {"net": P2.ChainPlan(mods, image_input=True, head_abs=True)}
        return P2.run_chain(self._plans["net"], (x,), self.training, self.compute_dtype)


def BL_VGG(pretrained=False):
    """reference models/baselines/BL.py:49-56: VGG(make_layers(cfg["E"])).  The reference's
    pretrained=True downloads torchvision's VGG19; this package never downloads: as the other models'
    flag, it reads the file from the local torch hub cache if it is there and warns otherwise.  Load
    weights with `load_state_dict`."""
    model = VGG(make_layers(cfg["E"], batch_norm=False))
    if pretrained:
        _load_pretrained_vgg(model.features, "vgg19-dcbb9e9d.pth", "VGG19")
    return model

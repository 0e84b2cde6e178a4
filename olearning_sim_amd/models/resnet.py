"""ResNet-18 (CIFAR variant, GroupNorm) — the flagship FedAvg CNN.

BASELINE config 3: FedAvg ResNet-18 on CIFAR-100 non-IID, 10k clients
across 8 GPUs.  BatchNorm is replaced with GroupNorm(8) as is standard
for federated training (per-client running stats are meaningless when
every client re-starts from the global model each round); all clients'
convs run as one grouped conv per layer in the channel-grouped layout
[B, C*ch, H, W] (models/base.py).
"""

from __future__ import annotations

import os
from typing import Optional

import torch

from .base import (ClientBatchedModel, Params, binit, kaiming,
                   blinear, bconv2d)

_STAGES = (64, 128, 256, 512)
_GN_GROUPS = 8


class ResNet18(ClientBatchedModel):
    name = "resnet18"
    num_classes = 100
    act_elems_per_sample = 1_600_000
    input_shape = (3, 32, 32)

    def __init__(self, num_classes: int = 100, in_ch: int = 3,
                 width_mult: float = 1.0):
        self.num_classes = num_classes
        self.in_ch = in_ch
        self.widths = [int(w * width_mult) for w in _STAGES]
        self.input_shape = (in_ch, 32, 32)

    # ------------------------------------------------------------------
    def init_global(self, device="cpu", dtype=torch.float32,
                    generator: Optional[torch.Generator] = None) -> Params:
        g = generator
        p: Params = {}

        def conv(name, oc, ic, k):
            p[f"{name}.w"] = kaiming((oc, ic, k, k), ic * k * k, device, dtype, g)

        def gn(name, ch):
            p[f"{name}.g"] = torch.ones(ch, device=device, dtype=dtype)
            p[f"{name}.b"] = torch.zeros(ch, device=device, dtype=dtype)

        w = self.widths
        conv("stem", w[0], self.in_ch, 3)
        gn("stem.gn", w[0])
        in_c = w[0]
        for s, out_c in enumerate(w):
            for blk in range(2):
                pre = f"s{s}.b{blk}"
                ic = in_c if blk == 0 else out_c
                conv(f"{pre}.c1", out_c, ic, 3)
                gn(f"{pre}.gn1", out_c)
                conv(f"{pre}.c2", out_c, out_c, 3)
                gn(f"{pre}.gn2", out_c)
                if blk == 0 and (ic != out_c or s > 0):
                    conv(f"{pre}.down", out_c, ic, 1)
                    gn(f"{pre}.gndown", out_c)
            in_c = out_c
        p["fc.w"] = binit((w[3], self.num_classes), w[3], device, dtype, g)
        p["fc.b"] = binit((self.num_classes,), w[3], device, dtype, g)
        return p

    # ------------------------------------------------------------------
    def _block(self, params: Params, x: torch.Tensor, C: int, pre: str,
               stride: int, has_down: bool) -> torch.Tensor:
        from ..ops.fused import groupnorm_act
        h = bconv2d(x, params[f"{pre}.c1.w"], C, stride=stride, padding=1)
        h = groupnorm_act(h, C, _GN_GROUPS, params[f"{pre}.gn1.g"],
                          params[f"{pre}.gn1.b"], relu=True)
        h = bconv2d(h, params[f"{pre}.c2.w"], C, stride=1, padding=1)
        if has_down:
            sc = bconv2d(x, params[f"{pre}.down.w"], C, stride=stride)
            sc = groupnorm_act(sc, C, _GN_GROUPS, params[f"{pre}.gndown.g"],
                               params[f"{pre}.gndown.b"])
        else:
            sc = x
        # fused: relu(gn(h) + sc)
        return groupnorm_act(h, C, _GN_GROUPS, params[f"{pre}.gn2.g"],
                             params[f"{pre}.gn2.b"], res=sc, relu=True)

    # -- fast path: client-channel-first layout + hand-written MFMA
    # conv kernels (ops/conv.py / ops/csrc/client_conv.hip) -------------
    # Activations travel as padded pairs (x, x_pad) (ops/fused.py): every
    # GroupNorm that feeds a 3x3 conv writes the conv's zero-haloed input
    # itself; x is the interior view that keeps the autograd graph dense.
    # x_pad is None wherever a shape falls back to the dense kernels.
    def _block_cbf(self, params: Params, x: torch.Tensor, x_pad, C: int,
                   pre: str, stride: int, has_down: bool,
                   pad_out: bool = True):
        from ..ops.conv import conv3x3_gn_relu, client_conv1x1
        from ..ops.fused import groupnorm_act
        h, h_pad = conv3x3_gn_relu(x, x_pad, params[f"{pre}.c1.w"], stride,
                                   C, _GN_GROUPS, params[f"{pre}.gn1.g"],
                                   params[f"{pre}.gn1.b"])
        if has_down:
            sc = client_conv1x1(x, params[f"{pre}.down.w"], stride,
                                x_pad=x_pad)
            sc = groupnorm_act(sc, C, _GN_GROUPS, params[f"{pre}.gndown.g"],
                               params[f"{pre}.gndown.b"])
            sc_pad = None
        else:
            sc, sc_pad = x, x_pad
        return conv3x3_gn_relu(h, h_pad, params[f"{pre}.c2.w"], 1, C,
                               _GN_GROUPS, params[f"{pre}.gn2.g"],
                               params[f"{pre}.gn2.b"], res=sc,
                               res_pad=sc_pad, pad_out=pad_out)

    def dgrad_wt_params(self, params: Params):
        """{name: (H, W)} of the 3x3 weights forward_cbf convolves at
        stride 1 and whose input needs a gradient (all but the stem and
        each stage's strided c1), with the plane they run at: the
        candidates for a trainer-held flipped copy (ops/conv.py _dgrad_p).
        Whether the shape is eligible is the caller's question to
        conv3x3_v6_ok."""
        if os.environ.get("OLSIM_CONV", "custom") != "custom":
            return {}
        planes = {}
        for s in range(4):
            for blk in range(2):
                for cv in ("c1", "c2"):
                    if s > 0 and blk == 0 and cv == "c1":
                        continue                    # stride 2: dgrad_s2
                    planes[f"s{s}.b{blk}.{cv}.w"] = (32 >> s, 32 >> s)
        return planes

    def forward_cbf(self, params: Params, x: torch.Tensor) -> torch.Tensor:
        from ..ops.conv import client_conv3x3
        from ..ops.fused import groupnorm_relu_pad
        C, B = x.shape[0], x.shape[1]
        h = x.permute(0, 2, 1, 3, 4).contiguous()    # [C, 3, B, 32, 32]
        h = client_conv3x3(h, params["stem.w"], 1)
        h, h_pad = groupnorm_relu_pad(h, C, _GN_GROUPS, params["stem.gn.g"],
                                      params["stem.gn.b"])
        for s in range(4):
            stride = 1 if s == 0 else 2
            h, h_pad = self._block_cbf(params, h, h_pad, C, f"s{s}.b0",
                                       stride, s > 0)
            # the last block's output feeds the pooling and stays dense
            h, h_pad = self._block_cbf(params, h, h_pad, C, f"s{s}.b1", 1,
                                       False, pad_out=s < 3)
        # h: [C, 512, B, 4, 4] -> avg pool -> [C, B, 512]
        h = h.mean(dim=(3, 4)).permute(0, 2, 1)
        return blinear(h, params["fc.w"], params["fc.b"])

    def forward(self, params: Params, x: torch.Tensor) -> torch.Tensor:
        from ..ops.fused import groupnorm_act
        # Default: the hand-written client-batched implicit-GEMM MFMA
        # conv kernels (ops/csrc/client_conv2.hip v6 padded family —
        # mask-free gathers, XCD-aware tiling, parity-decomposed
        # stride-2 dgrad).  Measured vs MIOpen grouped conv at C=250
        # (tools/convbench3.py, profiles/): all-shape conv total
        # 30.9 ms vs 57.1 ms (0.54x).  OLSIM_CONV=miopen forces the
        # grouped-conv reference path.
        if x.is_cuda and x.dtype == torch.bfloat16 and \
                os.environ.get("OLSIM_CONV", "custom") == "custom":
            from ..ops.fused import hip_ops_available
            if hip_ops_available():
                return self.forward_cbf(params, x)
        # x: [C, B, 3, 32, 32]
        C, B = x.shape[0], x.shape[1]
        h = x.permute(1, 0, 2, 3, 4).reshape(B, C * self.in_ch, 32, 32)
        h = bconv2d(h, params["stem.w"], C, stride=1, padding=1)
        h = groupnorm_act(h, C, _GN_GROUPS, params["stem.gn.g"],
                          params["stem.gn.b"], relu=True)
        for s in range(4):
            stride = 1 if s == 0 else 2
            has_down = s > 0
            h = self._block(params, h, C, f"s{s}.b0", stride, has_down)
            h = self._block(params, h, C, f"s{s}.b1", 1, False)
        # h: [B, C*512, 4, 4] -> global average pool -> [C, B, 512]
        h = h.mean(dim=(2, 3)).reshape(B, C, self.widths[3]).permute(1, 0, 2)
        return blinear(h, params["fc.w"], params["fc.b"])

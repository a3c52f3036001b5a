"""Launch builders of the transfer model (TransferSRModel): the RRDB backbone of rrdb.py, then the
face-specific head on the FaceEnhanceNet builders of net.py.

NCHW fp32 in, NCHW fp32 out, NHWC of the compute dtype in between: the backbone's last launch
(conv_body with the `+ feat` epilogue) writes the 64-channel buffer the head's first launch reads,
so there is no layout change and no elementwise launch at the seam.

The head -- num_blocks RCABs, conv_after, `+ x`, the PixelShuffle upsampler, conv_last -- has the
arithmetic of a ResidualGroup followed by FaceEnhanceNet's tail without conv_after_body and with a
conv_last that adds no bicubic skip and never clamps (FEN_EPI_NOSKIP).  It therefore runs through
Forward.group / Forward.tail(skip=False) and, in training, Backward.up / Backward.group, over
weights whose keys are the head's mapped onto the group's (`head_key`).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import lib as L
from . import rrdb as R
from .net import Backward, Forward, NetSpec, Weights
from .program import Ctx, ptr


def head_spec(channels: int, num_blocks: int, scale: int, reduction_ratio: int = 4, res_scale: float = 0.2) -> NetSpec:
    return NetSpec(C=channels, G=1, NB=num_blocks, Cr=max(channels // reduction_ratio, 8), scale=scale,
                   res_scale=res_scale)


def head_key(key: str) -> str:
    """A FaceSpecificHead state_dict key -> the key the group / tail builders use with pre = ''."""
    if key.startswith("rcab_blocks."):
        return "blocks." + key[len("rcab_blocks."):]
    if key.startswith("conv_after."):
        return "conv." + key[len("conv_after."):]
    return key                                   # upsample.stages.N.*, conv_last.*


def backbone(ctx: Ctx, W: Weights, x: torch.Tensor, num_block: int) -> torch.Tensor:
    """x NCHW fp32 [B,3,H,W] -> the head's input, NHWC [B,H,W,64] (inference kernels, nothing saved)."""
    return R.trunk(ctx, W, x, num_block)


def head(spec: NetSpec, ctx: Ctx, W: Weights, feat: torch.Tensor, save: bool, out: Optional[torch.Tensor] = None,
         hr: Optional[torch.Tensor] = None, l1_scale: float = 0.0):
    """feat NHWC [B,H,W,C] -> (NCHW fp32 [B,3,sH,sW], what head_backward needs when save)."""
    fw = Forward(spec, ctx, W, save=save)
    y, gsv = fw.group(feat, 0, pre="")
    out, tsv = fw.tail(y, None, None, training=True, out=out, hr=hr, l1_scale=l1_scale, fb=y, skip=False)
    return out, dict(group=gsv, tail=tsv)


def head_backward(spec: NetSpec, ctx: Ctx, W: Weights, G: Dict[str, torch.Tensor], sv: dict,
                  dout: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fills G (fp32, by mapped key) and returns d(feat), NHWC.  dout: dL/dsr NCHW fp32, or None
    when the forward's L1 epilogue already wrote it (sv['tail']['dout'])."""
    tsv, gsv = sv["tail"], sv["group"]
    if dout is not None:
        B, Co, Ho, Wo = (int(v) for v in dout.shape)
        d16 = ctx.alloc((B, Ho, Wo, 16))
        dd = dout.contiguous().float()
        ctx.emit("nchw_to_nhwc", ctx.lib.fen_nchw_to_nhwc, ctx.code, B, Co, Ho, Wo, 16, ptr(dd), ptr(d16))
        tsv["dout"] = d16
    bw = Backward(spec, ctx, W, G)
    d_y = bw.up(tsv)
    return bw.group(gsv, d_y, 0, pre="")


def forward(spec: NetSpec, ctx: Ctx, Wb: Weights, Wh: Weights, x: torch.Tensor, num_block: int) -> torch.Tensor:
    """TransferSRModel.forward for inference over one Ctx (eager, or recorded for a graph)."""
    L.check_strip_status()
    out, _ = head(spec, ctx, Wh, backbone(ctx, Wb, x, num_block), save=False)
    return out

"""Launch builders of the ESRGAN baseline (RRDBNet) forward over csrc/rrdb.hip.

A dense block lives in one NHWC buffer of 192 channels per pixel (x | x1 | x2 | x3 | x4); four
such buffers rotate, block n in buffer n % 4, its conv5 writing channels 0..63 of buffer
(n + 1) % 4 -- never one of the RRDB's three inputs nor the holder of the RRDB's own input.  No
concatenation, no elementwise launch: every launch below is a convolution.  The builders talk
to a `Ctx` (program.py), so the same code runs eagerly or is recorded for a graph.
"""
from __future__ import annotations

import torch

from . import lib as L
from .net import conv
from .program import Ctx, byref, ptr

FEAT, GROW, STRIDE = 64, 32, 192
SLOPE = 0.2


def rrdb_conv(ctx: Ctx, x, x_stride, wpk, bias, y, y_stride, y_off, B, H, W, Cin, Cout, *, lrelu=0, up2=0,
              r1=None, r1_stride=0, s1=0.0, r2=None, r2_stride=0, s2=0.0, nchw_out=0) -> None:
    """One fen_rrdb_conv launch (include/fen.h); B, H, W are the output's."""
    d = L.RrdbConvDesc()
    d.dtype, d.B, d.H, d.W, d.Cin, d.Cout = ctx.code, B, H, W, Cin, Cout
    d.x, d.x_stride, d.up2 = ptr(x), x_stride, up2
    d.w, d.bias = ptr(wpk), ptr(bias)
    d.y, d.y_stride, d.y_off, d.lrelu = ptr(y), y_stride, y_off, lrelu
    d.r1, d.r1_stride, d.s1 = ptr(r1), r1_stride, float(s1)
    d.r2, d.r2_stride, d.s2 = ptr(r2), r2_stride, float(s2)
    d.nchw_out = nchw_out
    ctx.emit("rrdb_conv", ctx.lib.fen_rrdb_conv, byref(d))


def dense_block(ctx: Ctx, W, pre: str, buf, nxt, x_rrdb, B, H, Wd, num_feat=FEAT, num_grow_ch=GROW) -> None:
    """ResidualDenseBlock `pre` (a state_dict prefix ending in '.') on buf -> channels 0..63 of nxt."""
    d = L.RrdbBlockDesc()
    d.dtype, d.B, d.H, d.W = ctx.code, B, H, Wd
    d.num_feat, d.num_grow_ch = num_feat, num_grow_ch
    d.buf, d.next, d.x_rrdb = ptr(buf), ptr(nxt), ptr(x_rrdb)
    for k in range(5):
        d.w[k] = ptr(W.packed(f"{pre}conv{k + 1}", 0))
        d.bias[k] = ptr(W.p[f"{pre}conv{k + 1}.bias"])
    ctx.emit("rrdb_block", ctx.lib.fen_rrdb_block, byref(d))


def rrdb(ctx: Ctx, W, pre: str, bufs, n: int, B, H, Wd) -> int:
    """RRDB `pre` starting in bufs[n % 4]; returns the index of the buffer holding its output."""
    x_rrdb = bufs[n % 4]
    for j in range(3):
        dense_block(ctx, W, f"{pre}rdb{j + 1}.", bufs[n % 4], bufs[(n + 1) % 4], x_rrdb if j == 2 else None, B, H, Wd)
        n += 1
    return n


def _slopes(ctx: Ctx) -> torch.Tensor:
    """LeakyReLU(0.2) as fen_conv3x3's PReLU epilogue: constant slopes."""
    key = f"rrdb_slopes/{ctx.device}"
    t = ctx._shared.get(key)
    if t is None:
        t = ctx._shared[key] = torch.full((FEAT,), SLOPE, dtype=torch.float32, device=ctx.device)
    return t


def trunk(ctx: Ctx, W, x: torch.Tensor, num_block: int) -> torch.Tensor:
    """feat + conv_body(body(feat)), feat = conv_first(x) (reference esrgan.py:54-57; the transfer
    model's backbone, transfer.py:257-264): x NCHW fp32 [B,Ci,H,W] on the GPU -> NHWC [B,H,W,64] of
    the compute dtype.  W: Weights with the keys conv_first.*, body.N.rdbM.convK.*, conv_body.*."""
    B, Ci, H, Wd = (int(v) for v in x.shape)
    bufs = [ctx.alloc((B, H, Wd, STRIDE)) for _ in range(min(4, 3 * num_block + 1))]
    feat = ctx.alloc((B, H, Wd, FEAT))
    ctx.emit("rrdb_first", ctx.lib.fen_rrdb_first, ctx.code, B, Ci, H, Wd, ptr(x), ptr(W.p["conv_first.weight"]),
             ptr(W.p["conv_first.bias"]), ptr(bufs[0]), STRIDE, ptr(feat))
    n = 0
    for i in range(num_block):
        n = rrdb(ctx, W, f"body.{i}.", bufs, n, B, H, Wd)
    # feat + conv_body(body(feat)): the body's output sits in channels 0..63 at stride 192
    body = ctx.alloc((B, H, Wd, FEAT))
    rrdb_conv(ctx, bufs[n % 4], STRIDE, W.packed("conv_body", 0), W.p["conv_body.bias"], body, FEAT, 0, B, H, Wd,
              FEAT, FEAT, r1=feat, r1_stride=FEAT, s1=1.0)
    return body


def forward(ctx: Ctx, W, x: torch.Tensor, num_block: int, num_out_ch: int) -> torch.Tensor:
    """RRDBNet.forward (reference esrgan.py:54-66): x NCHW fp32 [B,Ci,H,W] on the GPU -> NCHW fp32
    [B,num_out_ch,4H,4W].  W: Weights over the module's state_dict keys."""
    B, _, H, Wd = (int(v) for v in x.shape)
    body = trunk(ctx, W, x, num_block)
    # nearest x2 -> conv -> LeakyReLU, twice: the upsample is the gather's (h >> 1, w >> 1)
    t = body
    for s, name in ((2, "conv_up1"), (4, "conv_up2")):
        y = ctx.alloc((B, s * H, s * Wd, FEAT))
        rrdb_conv(ctx, t, FEAT, W.packed(name, 0), W.p[name + ".bias"], y, FEAT, 0, B, s * H, s * Wd, FEAT, FEAT,
                  lrelu=1, up2=1)
        t = y
    # conv_hr: a dense 64 -> 64 conv + LeakyReLU, exactly fen_conv3x3's bias + PReLU epilogue
    hr = ctx.alloc((B, 4 * H, 4 * Wd, FEAT))
    conv(ctx, t, W.packed("conv_hr", 0), B, 4 * H, 4 * Wd, FEAT, FEAT, bias=W.p["conv_hr.bias"], epi=L.EPI_PRELU,
         alpha=_slopes(ctx), y=hr)
    out = ctx.alloc((B, num_out_ch, 4 * H, 4 * Wd), torch.float32)
    rrdb_conv(ctx, hr, FEAT, W.packed("conv_last", 0), W.p["conv_last.bias"], out, 0, 0, B, 4 * H, 4 * Wd, FEAT,
              num_out_ch, nchw_out=1)
    return out

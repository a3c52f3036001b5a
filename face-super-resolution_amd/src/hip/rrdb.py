"""Launch builders of the ESRGAN baseline (RRDBNet) forward over csrc/rrdb.hip, and of the dense
blocks' backward (trunk(save_from=...) / trunk_backward: the transfer model's stages 2 and 3).

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


def _slopes(ctx: Ctx) -> torch.Tensor:
    """LeakyReLU(0.2) as fen_conv3x3's PReLU epilogue: constant slopes."""
    key = f"rrdb_slopes/{ctx.device}"
    t = ctx._shared.get(key)
    if t is None:
        t = ctx._shared[key] = torch.full((FEAT,), SLOPE, dtype=torch.float32, device=ctx.device)
    return t


def trunk(ctx: Ctx, W, x: torch.Tensor, num_block: int, save_from=None):
    """feat + conv_body(body(feat)), feat = conv_first(x) (reference esrgan.py:54-57; the transfer
    model's backbone, transfer.py:257-264): x NCHW fp32 [B,Ci,H,W] on the GPU -> NHWC [B,H,W,64] of
    the compute dtype.  W: Weights with the keys conv_first.*, body.N.rdbM.convK.*, conv_body.*.

    save_from = i (training with RRDBs i.. unfrozen): RRDBs < i run on the four rotating buffers
    as in inference, nothing kept; from RRDB i on every dense block gets its own 192-channel buffer
    (fen_rrdb_block takes any `next` that is neither its buffer nor the RRDB input's holder), and
    one more holds the body's output.  The same launches on the same values: the result is
    bit-identical to the inference forward.  Returns (body, saved) then, saved = what
    trunk_backward needs."""
    B, Ci, H, Wd = (int(v) for v in x.shape)
    nblk = 3 * num_block
    first = nblk if save_from is None else 3 * max(0, min(int(save_from), num_block))
    rot = [ctx.alloc((B, H, Wd, STRIDE)) for _ in range(min(4, first + (save_from is None)))]
    own = [ctx.alloc((B, H, Wd, STRIDE)) for _ in range(nblk - first + 1)] if save_from is not None else []

    def buf(n):       # the buffer dense block n lives in (n = 3 num_block: the body's output)
        return rot[n % 4] if n < first or save_from is None else own[n - first]
    feat = ctx.alloc((B, H, Wd, FEAT))
    ctx.emit("rrdb_first", ctx.lib.fen_rrdb_first, ctx.code, B, Ci, H, Wd, ptr(x), ptr(W.p["conv_first.weight"]),
             ptr(W.p["conv_first.bias"]), ptr(buf(0)), STRIDE, ptr(feat))
    for n in range(nblk):
        i, j = divmod(n, 3)
        dense_block(ctx, W, f"body.{i}.rdb{j + 1}.", buf(n), buf(n + 1), buf(n - 2) if j == 2 else None, B, H, Wd)
    # feat + conv_body(body(feat)): the body's output sits in channels 0..63 at stride 192
    body = ctx.alloc((B, H, Wd, FEAT))
    rrdb_conv(ctx, buf(nblk), STRIDE, W.packed("conv_body", 0), W.p["conv_body.bias"], body, FEAT, 0, B, H, Wd,
              FEAT, FEAT, r1=feat, r1_stride=FEAT, s1=1.0)
    if save_from is None:
        return body
    return body, dict(bufs=own, first=first // 3, num_block=num_block, B=B, H=H, W=Wd)


def dgrad(ctx: Ctx, dy, dy_stride, dy_off, wpk, dx, dx_stride, B, H, W, Cin, Cout, *, accumulate=0, s=1.0,
          r1=None, r1_stride=0, s1=0.0, r2=None, r2_stride=0, s2=0.0, act=None, act_stride=0) -> None:
    """One fen_rrdb_dgrad launch (include/fen.h)."""
    d = L.RrdbDgradDesc()
    d.dtype, d.B, d.H, d.W, d.Cin, d.Cout = ctx.code, B, H, W, Cin, Cout
    d.dy, d.dy_stride, d.dy_off, d.w = ptr(dy), dy_stride, dy_off, ptr(wpk)
    d.dx, d.dx_stride, d.accumulate, d.s = ptr(dx), dx_stride, accumulate, float(s)
    d.r1, d.r1_stride, d.s1 = ptr(r1), r1_stride, float(s1)
    d.r2, d.r2_stride, d.s2 = ptr(r2), r2_stride, float(s2)
    d.act, d.act_stride = ptr(act), act_stride
    ctx.emit("rrdb_dgrad", ctx.lib.fen_rrdb_dgrad, byref(d))


def strided_wgrad(ctx: Ctx, x, x_stride, dy, dy_stride, dy_off, B, H, W, Cin, Cout, dw, db, *, scale=1.0,
                  accumulate=0) -> None:
    """One fen_rrdb_wgrad launch pair (include/fen.h)."""
    d = L.RrdbWgradDesc()
    d.dtype, d.B, d.H, d.W, d.Cin, d.Cout = ctx.code, B, H, W, Cin, Cout
    d.x, d.x_stride, d.dy, d.dy_stride, d.dy_off = ptr(x), x_stride, ptr(dy), dy_stride, dy_off
    d.scale, d.dw, d.db, d.accumulate = float(scale), ptr(dw), ptr(db), accumulate
    work = ctx.scratch("rrdb_wgrad_work", (ctx.lib.fen_rrdb_wgrad_work_floats(byref(d)),), torch.float32)
    d.work = ptr(work)
    ctx.emit("rrdb_wgrad", ctx.lib.fen_rrdb_wgrad, byref(d))


def dense_block_backward(ctx: Ctx, W, G, pre: str, buf, D, g, g_stride, third, g_rrdb, g_rrdb_stride, B, H, Wd,
                         weights=True) -> None:
    """ResidualDenseBlock `pre` backwards (fen_rrdb_block_bwd): D[..., 0:64] becomes the gradient of
    the block's input; G[pre + 'convK.weight' / '.bias'] (fp32) are filled when `weights`."""
    d = L.RrdbBlockBwdDesc()
    d.dtype, d.B, d.H, d.W = ctx.code, B, H, Wd
    d.num_feat, d.num_grow_ch = FEAT, GROW
    d.buf, d.D, d.g, d.g_stride, d.third = ptr(buf), ptr(D), ptr(g), g_stride, int(third)
    d.g_rrdb, d.g_rrdb_stride = ptr(g_rrdb), g_rrdb_stride
    for k in range(5):
        d.wt[k] = ptr(W.packed(f"{pre}conv{k + 1}", 2))
        if weights:
            d.dw[k] = ptr(G[f"{pre}conv{k + 1}.weight"])
            d.db[k] = ptr(G[f"{pre}conv{k + 1}.bias"])
    if weights:
        nwork = ctx.lib.fen_rrdb_block_bwd_work_floats(ctx.code, B, H, Wd)
        d.work = ptr(ctx.scratch("rrdb_wgrad_work", (nwork,), torch.float32))
    ctx.emit("rrdb_block_bwd", ctx.lib.fen_rrdb_block_bwd, byref(d))


def trunk_backward(ctx: Ctx, W, G, saved: dict, d_feat: torch.Tensor) -> torch.Tensor:
    """The backward of trunk(save_from=i) from d_feat, NHWC [B,H,W,64]: the gradient of `feat +
    conv_body(t)` w.r.t. what conv_body and RRDBs i.. hold.  Fills G (fp32 tensors keyed by
    state-dict name: conv_body.*, body.N.rdbM.convK.* for N >= i) and returns the gradient buffer
    whose channels 0..63 (pixel stride 192; dense for an empty range) are the gradient of RRDB i's
    input.  conv_first is frozen and the skip `+ feat` feeds only it: neither gets a gradient.

    Four gradient buffers rotate as the forward's do: block n's holds the next block's incoming
    gradient in channels 0..63, and an RRDB's first block also reads the RRDB output's gradient,
    left three blocks earlier."""
    B, H, Wd, bufs = saved["B"], saved["H"], saved["W"], saved["bufs"]
    first, nblk = 3 * saved["first"], 3 * saved["num_block"]
    # conv_body: its input is channels 0..63 of the last buffer (stride 192)
    strided_wgrad(ctx, bufs[nblk - first], STRIDE, d_feat, FEAT, 0, B, H, Wd, FEAT, FEAT, G["conv_body.weight"],
                  G["conv_body.bias"])
    dt = ctx.alloc((B, H, Wd, FEAT))
    conv(ctx, d_feat, W.packed("conv_body", 2), B, H, Wd, FEAT, FEAT, y=dt)
    Ds = [ctx.alloc((B, H, Wd, STRIDE)) for _ in range(min(4, nblk - first))]

    def grad_of(n):   # (holder, pixel stride) of the gradient of block n's input (n = nblk: the body's output)
        return (dt, FEAT) if n == nblk else (Ds[(n - first) % 4], STRIDE)
    for n in range(nblk - 1, first - 1, -1):
        i, j = divmod(n, 3)
        g, gs = grad_of(n + 1)
        gr, grs = grad_of(n + 3) if j == 0 else (None, 0)
        dense_block_backward(ctx, W, G, f"body.{i}.rdb{j + 1}.", bufs[n - first], grad_of(n)[0], g, gs, j == 2, gr, grs,
                             B, H, Wd)
    return grad_of(first)[0]


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

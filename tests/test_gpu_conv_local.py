"""Local parity of the persistent conv kernels (conv3x3.hip: k_conv3x3_g ping-pong, k_conv3x3_p
one-group, k_conv3x3_v DMA-fed wide) with every block walking several tiles.

The other per-kernel conv tests give a persistent block one tile, two at most: group B of the
ping-pong kernel never computes, no halo is fetched under a running epilogue, no partial waits
for the next phase, no store drains behind the next tile's MFMAs.  Here the shapes come from the
device's CU count (parity.conv_shape; at 256 CUs 3 x 152 x 160, 1 x 520 x 536 and 1 x 424 x 440):
every block of k_conv3x3_g / _p sees 4 or 5 tiles, every block of k_conv3x3_v 2 or 3, and one
image edge is ragged, so a block mixes full and ragged tiles.  The premises are asserted from
parity.tiles_per_block, which restates fen_detail::persistent_grid and the kernels' `nmine`.

Every 16-bit output is measured against the float64 conv + epilogue of the same rounded
operands per (image, row), (image, column), (image, channel) band, per element, per 16 x 16 conv
tile and per visit index (the tiles a block computes first, second, ...), each bounded by the
1.5 / 1.5 / 4 factors of the fp32 yardstick with the kernels' rounding points
(parity.conv_case).  The per-tile channel partials are held to their worst-case fp32 bound.
Outputs sit between sentinel guards that must come back bit-unchanged, start as NaN and must be
finite wherever the kernel has to write, and two launches into separate buffers must agree bit
for bit (a halo consumed before it landed does not repeat).  tests/test_parity_cpu.py plants the
faults these bounds are for.  fp32 runs the streamed kernel, one tile per block: not here.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 3
_DEVICE = {}
RATIOS = {}          # (test, prec) -> worst got / yard ratio per metric over the cases run


def _num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV, dtype)


def _nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2)


def _operands(c, name, mode):
    """x and the packed filter of a case on the device, once per (dtype, case, pack mode)."""
    from src.hip.program import Ctx, ptr
    key = (c.prec, name, mode)
    if key not in _DEVICE:
        ctx = Ctx(c.dtype, DEV)
        Cout, Cin = c.w.shape[:2]
        wp = torch.empty(ctx.lib.fen_packed_elems(mode, Cout, Cin), dtype=c.dtype, device=DEV)
        wd = c.w.to(DEV).contiguous()
        ctx.emit("pack", ctx.lib.fen_pack_conv_w, ctx.code, mode, Cout, Cin, ptr(wd), ptr(wp))
        torch.cuda.synchronize()
        _DEVICE[key] = (ctx, _nhwc(c.x, c.dtype), wp)
    return _DEVICE[key]


class Guarded:
    """An output carved out of a larger allocation: `guard` elements of a sentinel bit pattern
    before and after, the output itself NaN."""

    def __init__(self, shape, dtype, guard):
        n = 1
        for s in shape:
            n *= s
        self.itype, self.sent = (torch.int16, 0x5A5A) if dtype != torch.float32 else (torch.int32, 0x5A5A5A5A)
        self.buf = torch.empty(n + 2 * guard, dtype=dtype, device=DEV)
        self.buf.view(self.itype).fill_(self.sent)
        self.n, self.guard = n, guard
        self.t = self.buf[guard:guard + n].view(shape)
        self.t.fill_(float("nan"))

    def guards_intact(self):
        raw = self.buf.view(self.itype)
        return bool((raw[:self.guard] == self.sent).all()) and bool((raw[self.guard + self.n:] == self.sent).all())

    def bits(self):
        return self.t.contiguous().view(self.itype)


def _launch(c, name, *, dot=False, pre_elide=0, nan_pre=False):
    """One fen_conv3x3 call of the case into fresh guarded buffers -> {output name: Guarded}."""
    from src.hip import lib as L, net
    ctx, xd, wp = _operands(c, name, 1 if c.shuffle else 0)
    B, Cin, H, W = c.x.shape
    Cout = c.w.shape[0]
    s = 2 if c.shuffle else 1
    oshape = (B, s * H, s * W, Cout // (s * s))
    row = 16 * W * Cout                                       # one row of conv tiles of the output
    out = {"y": Guarded(oshape, c.dtype, row)}
    kw = {}
    epi = {"none": 0, "prelu": L.EPI_PRELU, "pool": L.EPI_POOL, "prelu_bwd": L.EPI_PRELU_BWD,
           "relu_bwd": L.EPI_RELU_BWD}[c.mode] | (L.EPI_SHUFFLE if c.shuffle else 0) | (L.EPI_DOT if dot else 0)
    if c.want_pre:
        out["y_pre"] = Guarded(oshape, c.dtype, row)
        kw["y_pre"] = out["y_pre"].t
    if c.pool2:
        out["y_pool"] = Guarded((B, H // 2, W // 2, Cout), c.dtype, row // 4)
        kw["y_pool"] = out["y_pool"].t
    if c.mode in ("pool", "prelu_bwd") or dot:
        ntiles = B * net.tiles(H, W)
        out["part"] = Guarded((ntiles, Cout), torch.float32, -(-W // 16) * Cout)
        kw["part"] = out["part"].t
    if c.bias is not None:
        kw["bias"] = c.bias.to(DEV)
    if c.alpha is not None:
        kw["alpha"] = c.alpha.to(DEV)
    if dot:
        kw["pre_in"] = _nhwc(c.dot_in, c.dtype)
    elif c.pre_in is not None:
        pre = c.pre_in.clone()
        if nan_pre:                                           # NaN wherever the kernel must read post_in instead
            pre[:, c.rec] = float("nan")
        kw["pre_in"] = _nhwc(pre, c.dtype)
    if c.post_in is not None:
        kw["post_in"] = _nhwc(c.post_in, c.dtype)
    net.conv(ctx, xd, wp, B, H, W, Cin, Cout, epi=epi, y=out["y"].t, res=[_nhwc(r, c.dtype) for r in c.res],
             pre_elide=pre_elide, **kw)
    return out


def _check(test, name, c, *, dot=False, pre_elide=0, elided=False, nan_pre=False):
    what = f"{test} {c.prec}"
    B, _, H, W = c.x.shape
    tpb, ok = parity.conv_premises(name, B, H, W, _num_cus())
    print(f"{what}: {B}x{H}x{W}, {tpb.k.numel()} tiles on {tpb.nslot} slots: {tpb.lo}..{tpb.hi} tiles per block")
    assert ok, (name, B, H, W, _num_cus(), tpb.lo, tpb.hi)
    one, two = (_launch(c, name, dot=dot, pre_elide=pre_elide, nan_pre=nan_pre) for _ in range(2))
    torch.cuda.synchronize()
    for k in one:
        assert one[k].guards_intact() and two[k].guards_intact(), f"{what}: write outside {k}"
        assert torch.equal(one[k].bits(), two[k].bits()), f"{what}: {k} differs between two launches"
    worst = RATIOS.setdefault((test.split("[")[0], c.prec), {})
    for k in ("y_pre", "y", "y_pool"):
        if k not in one:
            continue
        if k == "y_pre" and elided:                           # every slope of the block > 0: not written
            assert bool(torch.isnan(one[k].t).all()), f"{what}: y_pre written despite pre_elide"
            continue
        got = _nchw(one[k].t)
        assert bool(torch.isfinite(got).all()), f"{what}: {k} has unwritten or non-finite elements"
        ts = {"y_pool": 8}.get(k, 32 if c.shuffle else 16)
        r = parity.assert_local(got, c.ref[k], c.yard[k], f"{what} {k}")
        r.update(parity.assert_tiles(got, c.ref[k], c.yard[k], ts, ts, tpb, f"{what} {k}"))
        for m, v in r.items():
            worst[m] = max(worst.get(m, 0.0), v)
    if "part" in one:
        if dot:
            ref, bound = parity.dot_part(_nchw(one["y"].t), c.dot_in)
        else:
            ref, bound = c.ref["part"], c.part_bound()
        f = parity.assert_part(one["part"].t, ref, bound, tpb, what)
        worst["part"] = max(worst.get("part", 0.0), f)
    print(f"{what}: worst so far " + " ".join(f"{m} {v:.3f}" if m != "part" else f"{m} {v:.2e}" for m, v in worst.items()))


def _case(prec, name, **kw):
    return parity.conv_case(prec, *parity.conv_shape(name, _num_cus()), seed=SEED, **kw)


PRECS = ["bf16", "fp16"]
UP = dict(mode="prelu", bias=True, shuffle=True)
G_UP = {"y_pre": dict(UP, want_pre=True), "no_y_pre": dict(UP),
        "elide_all_positive": dict(UP, want_pre=True, alpha="pos"), "elide_mixed": dict(UP, want_pre=True)}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", sorted(G_UP))
def test_conv_g_upsampler(prec, case):
    """k_conv3x3_g, BIAS | PRELU | SHUFFLE (64 -> 256): with and without y_pre, and with pre_elide.
    A 64-row co-block of the packed filter holds one shuffle phase of all 64 output channels, so
    every block sees every slope: all slopes > 0 elides y_pre in all four co-blocks (it stays
    NaN), one slope <= 0 in none (y_pre written everywhere)."""
    elide = case.startswith("elide")
    _check(f"test_conv_g_upsampler[{case}]", "up", _case(prec, "up", **G_UP[case]), pre_elide=int(elide),
           elided=case == "elide_all_positive")


G_C64 = {"prelu_y_pre": dict(mode="prelu", bias=True, want_pre=True), "prelu": dict(mode="prelu", bias=True),
         "prelu_maxpool": dict(mode="prelu", bias=True, pool2=True, alpha="relu"), "bias_res1": dict(bias=True, nres=1),
         "relu_bwd": dict(mode="relu_bwd"), "res0": dict(), "res1": dict(nres=1), "res2": dict(nres=2),
         "res3": dict(nres=3), "dot": dict(), "dot_res1": dict(nres=1)}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", sorted(G_C64))
def test_conv_g_c64(prec, case):
    """k_conv3x3_g's 64 -> 64 instantiations (conv_dispatch's switch on the epilogue key)."""
    c = _case(prec, "c64", **G_C64[case])
    dot = case.startswith("dot")
    if dot:
        c.dot_in = torch.randn(c.ref["y"].shape, generator=torch.Generator().manual_seed(77)).to(c.dtype).float()
    _check(f"test_conv_g_c64[{case}]", "c64", c, dot=dot)


P_C64 = {"pool": dict(mode="pool", bias=True), "prelu_bwd": dict(mode="prelu_bwd"),
         "prelu_bwd_post_in": dict(mode="prelu_bwd", post_in=True),
         "runtime_prelu_res1": dict(mode="prelu", bias=True, nres=1, want_pre=True)}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", sorted(P_C64))
def test_conv_p_c64(prec, case):
    """k_conv3x3_p: BIAS | POOL, PRELU_BWD (with post_in: pre_in is NaN wherever the kernel must
    read post_in instead) and the runtime-mode epilogue (a key without an instantiation)."""
    _check(f"test_conv_p_c64[{case}]", "c64", _case(prec, "c64", **P_C64[case]), nan_pre=case == "prelu_bwd_post_in")


V_WIDE = {"prelu_y_pre": dict(mode="prelu", bias=True, want_pre=True), "bias": dict(bias=True),
          "prelu_bwd": dict(mode="prelu_bwd"), "relu_bwd": dict(mode="relu_bwd"), "none": dict(),
          "prelu_maxpool": dict(mode="prelu", bias=True, pool2=True, alpha="relu")}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", sorted(V_WIDE))
def test_conv_v_wide(prec, case):
    """k_conv3x3_v (128 -> 128): its five epilogue instantiations and the fused max pool."""
    _check(f"test_conv_v_wide[{case}]", "wide", _case(prec, "wide", **V_WIDE[case]))

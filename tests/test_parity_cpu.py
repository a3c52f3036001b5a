"""The detector behind the strip kernels' local bounds (tests/parity.py), proved on the CPU.

1. The yardstick is the oracle: rounded_group / rounded_group_grads with no rounding equal the
   oracle's residual_group and its autograd in float64.
2. Flatness: under 16-bit rounding alone every (image, row), (image, column) and (image, channel)
   band of rounded_group is within 1.25x of the whole-tensor rel-L2 -- what assert_local's 1.5
   margin relies on.
3. Planted faults: a second realisation of the same rounding (the group run on the mirrored
   image with mirrored filters and mirrored back: same values, other fp32 summation order) passes
   assert_local; with one local fault planted in it -- a counted number of corrupted elements --
   assert_local raises, by at least 5x its factor in at least one metric.  The whole-tensor
   bound of test_gpu_group_strip.py (5e-3 bf16 / 1e-3 fp16 per RCAB + 1), with the fault's
   energy scaled to the bench's batch of 32, accepts the faults listed in OLD_BOUND_ACCEPTS;
   the larger ones (eight rows, a whole image) it does reject at 64 rows -- printed, not
   asserted.
"""
import os
import sys

import pytest
import torch

from oracle import fen_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity  # noqa: E402
from test_gpu_group_strip import _params  # noqa: E402

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
_CACHE = {}


def _case(prec, B, H, n):
    """-> (x, qr, oracle64, yardstick), computed once per case and left unchanged."""
    key = (prec, B, H, n)
    if key not in _CACHE:
        dtype = DT[prec]
        q = _params(n, seed=31 + n)
        x = torch.randn(B, 64, H, 64, generator=torch.Generator().manual_seed(7)).to(dtype).float()
        qr = {k: (v.to(dtype).float() if v.dim() == 4 else v) for k, v in q.items()}
        ref = parity.rounded_group(x.double(), qr, n, None)
        yard = parity.rounded_group(x, qr, n, dtype)
        _CACHE[key] = (x, qr, ref, yard)
    return _CACHE[key]


def _mirrored_copy(x, qr, n, dtype):
    """rounded_group on the left-right mirrored image with mirrored filters, mirrored back."""
    qm = {k: (v.flip(3) if v.dim() == 4 else v) for k, v in qr.items()}
    return parity.rounded_group(x.flip(3), qm, n, dtype).flip(3).contiguous()


def test_unrounded_yardstick_is_the_oracle():
    n = 3
    q = _params(n, seed=3)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 64, 16, 64, generator=g).double()
    dy = torch.randn(2, 64, 16, 64, generator=g).double()
    dres = torch.randn(2, 64, 16, 64, generator=g).double()
    q64 = {k: v.double() for k, v in q.items()}
    rec, attn = {}, {}
    y = parity.rounded_group(x, q, n, None, record=rec)
    ref = O.residual_group(x, q64, "rg.", n, 0.2, attn=attn)
    assert float((y - ref).abs().max()) <= 1e-12
    for j in range(n):
        assert float((rec[f"s{j}"] - attn[f"group0_rcab{j}"]).abs().max()) <= 1e-13
    leaves = {k: v.clone().requires_grad_(True) for k, v in q64.items()}
    xl = x.clone().requires_grad_(True)
    (O.residual_group(xl, leaves, "rg.", n, 0.2) * dy).sum().backward()
    dx, grads = parity.rounded_group_grads(x, q, n, None, dy, dres)
    assert float((dx - (xl.grad + dres)).abs().max()) <= 1e-12
    for k, v in leaves.items():
        assert float((grads[k] - v.grad).abs().max()) <= 1e-10 * max(1.0, float(v.grad.abs().max())), k


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_round_both_rounds_value_and_gradient(prec):
    dtype = DT[prec]
    x = torch.randn(1000, generator=torch.Generator().manual_seed(0)).requires_grad_(True)
    g = torch.randn(1000, generator=torch.Generator().manual_seed(1))
    y = parity.RoundBoth.apply(x, dtype)
    assert torch.equal(y.detach(), x.detach().to(dtype).float())
    (y * g).sum().backward()
    assert torch.equal(x.grad, g.to(dtype).float())


def test_local_errors_counts_what_it_says():
    ref = torch.ones(2, 4, 3, 5)
    got = ref.clone()
    got[1, 2, 1, 3] = 3.0                                   # one element off by 2
    e = parity.local_errors(got, ref)
    assert e["global"] == pytest.approx((4.0 / 120) ** 0.5)
    assert e["row"] == pytest.approx((4.0 / 20) ** 0.5)     # a row band: 4 channels x 5 columns
    assert e["col"] == pytest.approx((4.0 / 12) ** 0.5)     # a column band: 4 channels x 3 rows
    assert e["chan"] == pytest.approx((4.0 / 15) ** 0.5)    # a channel band: 3 rows x 5 columns
    assert e["elem"] == pytest.approx(2.0)
    z = torch.zeros(1, 1, 2, 2)
    assert parity.local_errors(z, z) == dict.fromkeys(parity.METRICS, 0.0)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,n", [(2, 16, 3), (2, 64, 10)])
def test_rounding_error_is_flat_over_bands(prec, B, H, n):
    _, _, ref, yard = _case(prec, B, H, n)
    e = parity.local_errors(yard, ref)
    print(f"{prec} B={B} H={H} n={n}: " + " ".join(f"{k} {e[k]:.3e}" for k in parity.METRICS))
    assert 0 < e["global"] <= (5e-3 if prec == "bf16" else 1e-3) * (n + 1)
    for k in ("row", "col", "chan"):
        assert e[k] <= 1.25 * e["global"], (k, e[k], e["global"])


def _row_seam(t):
    t[0, :, 7, :] = t[0, :, 8, :].clone()
    return 64 * 64


def _chan_row(t):
    t[0, 5, 20, :] = 0
    return 64


def _corner_pixel(t):
    t[-1, :, -1, -1] = 0
    return 64


def _strip_shift(t):
    t[-1, :, 24:32, :] = t[-1, :, 23:31, :].clone()
    return 8 * 64 * 64


def _image_swap(t):
    t[[0, 1]] = t[[1, 0]].clone()
    return 2 * t[0].numel()


FAULTS = {"row_seam": _row_seam, "chan_row": _chan_row, "corner_pixel": _corner_pixel, "strip_shift": _strip_shift,
          "image_swap": _image_swap}
# (dtype, fault) the old whole-tensor bound accepts at n = 10, H = 64 once scaled to B = 32
OLD_BOUND_ACCEPTS = {("bf16", "row_seam"), ("bf16", "chan_row"), ("bf16", "corner_pixel"), ("fp16", "chan_row"),
                     ("fp16", "corner_pixel")}


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_second_realisation_passes(prec):
    B, H, n = 2, 64, 10
    x, qr, ref, yard = _case(prec, B, H, n)
    got = _mirrored_copy(x, qr, n, DT[prec])
    assert not torch.equal(got, yard)                       # another summation order, other roundings
    ratio = parity.assert_local(got, ref, yard, f"{prec} mirrored copy")
    assert all(ratio[k] <= 1.1 for k in ("global", "row", "col", "chan")) and ratio["elem"] <= 1.5, ratio


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_fault_is_flagged(prec, fault):
    B, H, n = 2, 64, 10
    x, qr, ref, yard = _case(prec, B, H, n)
    clean = _mirrored_copy(x, qr, n, DT[prec])
    got = clean.clone()
    count = FAULTS[fault](got)
    changed = int((got != clean).sum())
    assert 0.99 * count <= changed <= count, (changed, count)
    with pytest.raises(AssertionError):
        parity.assert_local(got, ref, yard, f"{prec} {fault}")
    eg, ey = parity.local_errors(got, ref), parity.local_errors(yard, ref)
    margin = max(eg[k] / ey[k] / parity.FACTOR[k] for k in parity.METRICS)
    # the same fault in a batch of 32: its energy diluted by B / 32, the rounding error as it is
    ec = parity.local_errors(clean, ref)["global"]
    at32 = (ec ** 2 + max(eg["global"] ** 2 - ec ** 2, 0.0) * B / 32) ** 0.5
    old = (5e-3 if prec == "bf16" else 1e-3) * (n + 1)
    print(f"{prec} {fault}: {changed} elements, flagged by {margin:.1f}x the factor; whole-tensor rel-L2 "
          f"{eg['global']:.2e} at B={B}, {at32:.2e} at B=32 (old bound {old:.2e}: "
          f"{'accepts' if at32 <= old else 'rejects'})")
    assert margin >= 5.0, margin
    if (prec, fault) in OLD_BOUND_ACCEPTS:
        assert at32 <= old, (at32, old)


# ---------------------------------------------------------------------------------------
# the conv kernels' detector (parity.conv_case, assert_local + assert_tiles, assert_part)
# ---------------------------------------------------------------------------------------
# 4. tiles_per_block restates persistent_grid / nmine: the counts of the 256-CU shapes.
# 5. Flatness at the three conv shapes: row, column, channel, tile and visit-index bands of the
#    yardstick within 1.25x of its whole-tensor rel-L2.
# 6. Planted faults on the yardstick of the upsampler stage conv (64 -> 256, bias + PixelShuffle +
#    PReLU, 3 x 152 x 160) and on the pool partials of the 64 -> 64 conv (1 x 520 x 536): each
#    exceeds a factor (the partial bound) at least five-fold, by the measured excess listed in
#    CONV_FAULT_EXCESS / PART_FAULT_EXCESS (the weakest: the bias of median magnitude dropped from
#    one channel in bf16, 10.8x, and a tile sum short of its median pixel, 5.3x); the old
#    whole-tensor max-abs bound of test_gpu_kernels.py (_tol) accepts the dropped bias and the
#    wrong slope.
NUM_CUS = 256
SEED = 3


def _up_case(prec):
    return parity.conv_case(prec, *parity.conv_shape("up", NUM_CUS), seed=SEED, mode="prelu", bias=True, shuffle=True,
                            want_pre=True)


def _pool_case(prec):
    return parity.conv_case(prec, *parity.conv_shape("c64", NUM_CUS), seed=SEED, mode="pool", bias=True)


def test_tiles_per_block_at_256_cus():
    assert parity.conv_shape("up", 256) == (3, 152, 160, 64, 256)
    assert parity.conv_shape("c64", 256) == (1, 520, 536, 64, 64)
    assert parity.conv_shape("wide", 256) == (1, 424, 440, 128, 128)
    for name, ntiles, nslot, lo, n_hi in (("up", 300, 64, 4, 44), ("c64", 1122, 256, 4, 98), ("wide", 756, 256, 2, 244)):
        B, H, W, _, _ = parity.conv_shape(name, 256)
        tpb, ok = parity.conv_premises(name, B, H, W, 256)
        assert ok and tpb.k.numel() == ntiles and tpb.nslot == nslot and (tpb.lo, tpb.hi) == (lo, lo + 1)
        per_slot = torch.bincount(torch.arange(ntiles) % nslot, minlength=nslot)
        assert int((per_slot == lo + 1).sum()) == n_hi and int((per_slot == lo).sum()) == nslot - n_hi
        assert int(tpb.k.max()) == lo and bool((torch.bincount(tpb.k)[:lo] == nslot).all())
    # fewer tiles than CUs: one tile per block; the wide kernel's floor; ncot rounds the grid down
    assert parity.tiles_per_block(16, 4, 256)[:2] == (1, 1) and parity.tiles_per_block(16, 4, 256).nslot == 16
    assert parity.tiles_per_block(512, 1, 256)[:2] == (2, 2)
    assert parity.tiles_per_block(100, 3, 256).nslot == 85 and parity.tiles_per_block(100, 3, 256)[:2] == (1, 2)
    assert parity.tiles_per_block(10, 4, 2, floor=4).nslot == 1
    # another part: the premises hold at the shape conv_shape picks
    for cus in (304, 120, 64):
        for name in parity.CONV_CASES:
            B, H, W, _, _ = parity.conv_shape(name, cus)
            assert parity.conv_premises(name, B, H, W, cus)[1], (cus, name)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["up", "c64", "wide"])
def test_conv_rounding_error_is_flat(prec, name):
    shape = parity.conv_shape(name, NUM_CUS)
    up = name == "up"
    c = parity.conv_case(prec, *shape, seed=SEED, mode="prelu", bias=True, shuffle=up, want_pre=True)
    tpb, _ = parity.conv_premises(name, *shape[:3], NUM_CUS)
    ts = 32 if up else 16
    for o in ("y_pre", "y"):
        e = parity.local_errors(c.yard[o], c.ref[o])
        e.update(parity.tile_errors(c.yard[o], c.ref[o], ts, ts, tpb.k))
        print(f"{prec} {name} {o}: " + " ".join(f"{k} {e[k]:.3e}" for k in parity.METRICS + ("tile", "visit")))
        assert 0 < e["global"] <= (2.5e-3 if prec == "bf16" else 3.2e-4)      # 2^-9 / 2^-12 relative: about 0.29 ulp rms
        for k in ("row", "col", "chan", "tile", "visit"):
            assert e[k] <= 1.25 * e["global"], (k, e[k], e["global"])


def _tile_box(c, t, ts):
    """tile t of the case's conv -> (b, row slice, column slice) in an output space with ts x ts tiles."""
    B, _, H, W = c.x.shape
    nth, ntw = -(-H // 16), -(-W // 16)
    b, r = divmod(t, nth * ntw)
    ty, tx = divmod(r, ntw)
    return b, slice(ty * ts, (ty + 1) * ts), slice(tx * ts, (tx + 1) * ts)


def _full_tile_with_full_predecessor(c, nslot):
    B, _, H, W = c.x.shape
    nth, ntw = -(-H // 16), -(-W // 16)

    def full(t):
        ty, tx = divmod(t % (nth * ntw), ntw)
        return 16 * ty + 16 <= H and 16 * tx + 16 <= W
    return next(t for t in range(2 * nslot, B * nth * ntw) if full(t) and full(t - nslot))


def _median_bias_channel(c):
    return int(c.bias.abs().argsort()[c.bias.numel() // 2])


def _f_dropped_bias(c, tpb):
    b = c.bias.clone()
    b[_median_bias_channel(c)] = 0
    return c.epilogue(c.base["z32"], c.dtype, bias=b)


def _f_wrong_slope(c, tpb):
    a = c.alpha.clone()
    a[17] *= 1.1
    return c.epilogue(c.base["z32"], c.dtype, alpha=a)


def _f_stale_tile(c, tpb):
    """one tile holds what its slot computed one visit earlier"""
    out = {k: v.clone() for k, v in c.yard.items()}
    t = _full_tile_with_full_predecessor(c, tpb.nslot)
    b, rs, cs = _tile_box(c, t, 32)
    b0, rs0, cs0 = _tile_box(c, t - tpb.nslot, 32)
    for k in ("y", "y_pre"):
        out[k][b, :, rs, cs] = c.yard[k][b0, :, rs0, cs0]
    return out


def _f_stale_halo_row(c, tpb):
    """one tile's MFMAs read its top halo row (18 pixels) before it landed: the row still holds
    the halo row of the tile the slot had before.  Changes the tile's first output row."""
    t = _full_tile_with_full_predecessor(c, tpb.nslot)
    b, rs, cs = _tile_box(c, t, 16)
    b0, rs0, cs0 = _tile_box(c, t - tpb.nslot, 16)
    h0, w0, hp, wp = rs.start, cs.start, rs0.start, cs0.start
    xp = torch.nn.functional.pad(c.x, (1, 1, 1, 1))                      # padded: halo row h0 - 1 is row h0
    halo = xp[b, :, h0:h0 + 3, w0:w0 + 18].clone()
    halo[:, 0] = xp[b0, :, hp, wp:wp + 18]
    z = c.base["z32"].clone()
    z[b, :, h0, w0:w0 + 16] = torch.nn.functional.conv2d(halo[None], c.w)[0, :, 0]
    return c.epilogue(z, c.dtype)


def _f_dropped_tap(c, tpb):
    """one output channel of the conv misses one of its nine taps"""
    co = 4 * 21 + 2
    w1 = torch.zeros(1, *c.w.shape[1:])
    w1[0, :, 0, 2] = c.w[co, :, 0, 2]
    z = c.base["z32"].clone()
    z[:, co] -= torch.nn.functional.conv2d(c.x, w1, None, padding=1)[:, 0]
    return c.epilogue(z, c.dtype)


def _f_unwritten_ragged_tile(c, tpb):
    """a ragged tile (8 of its 16 rows inside the image) never stored: the buffer's old zeros"""
    B, _, H, W = c.x.shape
    nth, ntw = -(-H // 16), -(-W // 16)
    assert H % 16 == 8
    t = (1 * nth + nth - 1) * ntw + 3
    b, rs, cs = _tile_box(c, t, 32)
    out = {k: v.clone() for k, v in c.yard.items()}
    for k in ("y", "y_pre"):
        out[k][b, :, rs, cs] = 0
    return out


CONV_FAULTS = {"dropped_bias": _f_dropped_bias, "wrong_slope": _f_wrong_slope, "stale_tile": _f_stale_tile,
               "stale_halo_row": _f_stale_halo_row, "dropped_tap": _f_dropped_tap,
               "unwritten_ragged_tile": _f_unwritten_ragged_tile}
# measured: the fault's worst metric / (factor x the yardstick's metric), and the metric it is in
CONV_FAULT_EXCESS = {
    ("bf16", "dropped_bias"): (10.8, "y_pre chan"), ("fp16", "dropped_bias"): (86.1, "y_pre chan"),
    ("bf16", "wrong_slope"): (8.7, "y chan"), ("fp16", "wrong_slope"): (69.5, "y chan"),
    ("bf16", "stale_tile"): (556.4, "y_pre tile"), ("fp16", "stale_tile"): (4447.2, "y_pre tile"),
    ("bf16", "stale_halo_row"): (103.2, "y_pre row"), ("fp16", "stale_halo_row"): (829.7, "y_pre row"),
    ("bf16", "dropped_tap"): (65.6, "y_pre chan"), ("fp16", "dropped_tap"): (524.1, "y_pre chan"),
    ("bf16", "unwritten_ragged_tile"): (396.8, "y_pre tile"), ("fp16", "unwritten_ragged_tile"): (3171.8, "y_pre tile"),
}
# measured: worst |partial - float64 tile sum| / bound (a plain fp32 realisation: 1.8e-4)
PART_FAULT_EXCESS = {("bf16", "late"): 2636.0, ("fp16", "late"): 2638.9, ("bf16", "last_missing"): 643.8,
                     ("fp16", "last_missing"): 644.4, ("bf16", "dropped_pixel"): 5.3, ("fp16", "dropped_pixel"): 5.3}


def _conv_margin(c, got, tpb):
    """-> (worst metric / (factor x yardstick's) over both outputs, its name)"""
    best = (0.0, "")
    for o in ("y_pre", "y"):
        eg, ey = parity.local_errors(got[o], c.ref[o]), parity.local_errors(c.yard[o], c.ref[o])
        tg, ty = (parity.tile_errors(t[o], c.ref[o], 32, 32, tpb.k) for t in (got, c.yard))
        for k in parity.METRICS:
            best = max(best, (eg[k] / ey[k] / parity.FACTOR[k], f"{o} {k}"))
        for k in ("tile", "visit"):
            best = max(best, (tg[k] / ty[k] / parity.BAND, f"{o} {k}"))
    return best


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("fault", sorted(CONV_FAULTS))
def test_conv_planted_fault_is_flagged(prec, fault):
    c = _up_case(prec)
    tpb, _ = parity.conv_premises("up", *c.x.shape[0:1], *c.x.shape[2:], NUM_CUS)
    got = CONV_FAULTS[fault](c, tpb)
    assert not torch.equal(got["y"], c.yard["y"])
    with pytest.raises(AssertionError):
        for o in ("y_pre", "y"):
            parity.assert_local(got[o], c.ref[o], c.yard[o], f"{prec} {fault} {o}")
            parity.assert_tiles(got[o], c.ref[o], c.yard[o], 32, 32, tpb, f"{prec} {fault} {o}")
    margin, where = _conv_margin(c, got, tpb)
    print(f"{prec} {fault}: flagged by {margin:.1f}x the factor in {where}")
    assert margin >= 5.0, (margin, where)
    assert margin >= 0.9 * CONV_FAULT_EXCESS[prec, fault][0], (margin, CONV_FAULT_EXCESS[prec, fault])


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_old_conv_bound_accepts_bias_and_slope_faults(prec):
    """test_gpu_kernels.py: max|got - ref| <= 3e-2 max(1, |ref|max) against the fp32 conv of the
    unrounded operands."""
    c = _up_case(prec)
    with torch.no_grad():
        v = parity.pixel_shuffle2(torch.nn.functional.conv2d(c.base["x_raw"], c.base["w_raw"], c.bias, padding=1))
    old_ref = {"y_pre": v, "y": parity._prelu(v, c.alpha)}
    for fault in ("dropped_bias", "wrong_slope"):
        got = CONV_FAULTS[fault](c, None)
        for o in ("y_pre", "y"):
            err = float((got[o] - old_ref[o]).abs().max())
            tol = 3e-2 * max(1.0, float(old_ref[o].abs().max()))
            print(f"{prec} {fault} {o}: max|d| {err:.3f}, old bound {tol:.3f}, "
                  f"fault alone {float((got[o] - c.yard[o]).abs().max()):.3f}")
            assert err <= tol, (fault, o, err, tol)


def _p_late(c, tpb, part):
    """every partial folded into the row of its slot's next tile (the first visit's rows correct)"""
    out = part.clone()
    out[tpb.nslot:] = part[:-tpb.nslot]
    return out


def _p_last_missing(c, tpb, part):
    """the block's last tile never folded: the row keeps what the buffer held (zeros)"""
    out = part.clone()
    out[-1] = 0
    return out


def _p_dropped_pixel(c, tpb, part):
    """one tile sum of one channel misses the pixel of median magnitude"""
    t, ch = 700, 11
    b, rs, cs = _tile_box(c, t, 16)
    v = (c.base["z32"][b, ch, rs, cs] + c.bias[ch]).flatten()
    out = part.clone()
    out[t, ch] -= v[v.abs().argsort()[v.numel() // 2]]
    return out


PART_FAULTS = {"late": _p_late, "last_missing": _p_last_missing, "dropped_pixel": _p_dropped_pixel}


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_conv_partials_bound_and_faults(prec):
    c = _pool_case(prec)
    tpb, _ = parity.conv_premises("c64", c.x.shape[0], *c.x.shape[2:], NUM_CUS)
    ref, bound, part = c.ref["part"], c.part_bound(), c.yard["part"]
    assert part.dtype == torch.float32
    clean = parity.assert_part(part, ref, bound, tpb, f"{prec} fp32 tile sums")
    assert clean <= 1e-2, clean                              # a plain fp32 realisation: far inside
    unwritten = part.clone()
    unwritten[-1] = float("nan")
    with pytest.raises(AssertionError, match="not written"):
        parity.assert_part(unwritten, ref, bound, tpb, f"{prec} unwritten row")
    for fault in sorted(PART_FAULTS):
        got = PART_FAULTS[fault](c, tpb, part)
        with pytest.raises(AssertionError):
            parity.assert_part(got, ref, bound, tpb, f"{prec} {fault}")
        excess = float(((got.double() - ref).abs() / bound).max())
        print(f"{prec} partials {fault}: {excess:.1f}x the bound")
        assert excess >= 5.0, (fault, excess)
        assert excess >= 0.9 * PART_FAULT_EXCESS[prec, fault], (excess, PART_FAULT_EXCESS[prec, fault])

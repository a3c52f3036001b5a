"""Local parity metrics for the strip-resident kernels (fen_group_strip, fen_group_strip_chain,
fen_group_strip_bwd) and the persistent conv kernels, and the CPU yardsticks their bounds are
derived from.

A whole-tensor rel-L2 sees a fault that repeats in every image.  A fault confined to one row,
one channel or one strip of one image (a wrong halo row, a missed hand-off, a late ticket) is
diluted in it by sqrt(faulty elements / all elements) and passes a bound that leaves room for
the 16-bit rounding of n RCABs.  `local_errors` therefore also measures the worst (image, row),
(image, column) and (image, channel) band and the worst single element; under rounding alone
these are flat (a band's rel-L2 is within a few percent of the global one), under a local fault
they jump by 25x and more (tests/test_parity_cpu.py plants such faults and asserts the jump).

The bound is not a constant.  `rounded_group` restates the oracle's residual_group with the
tensors the kernels' headers say they round (a1, t_j, every RCAB's output, the group output)
rounded to the 16-bit format, everything else in the caller's float type: an independent
realisation of the same rounding.  `assert_local(got, ref, yard, what)` measures the kernel
and the yardstick against the same high-precision reference and bounds every kernel metric by
a fixed factor of the yardstick's: BAND = 1.5 for the three band metrics, GLOBAL = 1.5 for the
whole-tensor rel-L2, ELEM = 4 for max|d| / rms(ref) (an extreme-value statistic).  The factors
are never derived from the kernel's output; a planted fault exceeds them at least five-fold
(asserted in test_parity_cpu.py).

Measured kernel / yardstick ratios on the MI355X (worst over the cases of each test; the five
metrics in the order global, row, column, channel, element) are listed in MEASURED below.

The persistent conv kernels (k_conv3x3_g, k_conv3x3_p, k_conv3x3_v; tests/test_gpu_conv_local.py)
are held to the same factors, one conv at a time.  `tiles_per_block` restates the launch grid
and a block's tile walk, so a test can assert that its shape gives every block several tiles;
`conv_case` builds the rounded operands, the float64 reference and the fp32 yardstick of one conv
with one of the kernels' epilogues (its docstring lists the rounding points); `tile_errors` /
`assert_tiles` add two bands to the five metrics: the worst (image, 16 x 16 conv tile) and the
worst visit index (all tiles their blocks compute k-th), which tells "first tile fine, steady
state wrong" from "one channel wrong everywhere"; `assert_part` holds the per-tile channel
partials to the worst-case error of an fp32 sum (ConvCase.part_bound, dot_part).  Their measured
ratios are in MEASURED_CONV.
"""
import collections
import math

import torch

BAND, GLOBAL, ELEM = 1.5, 1.5, 4.0
METRICS = ("global", "row", "col", "chan", "elem")
FACTOR = dict(zip(METRICS, (GLOBAL, BAND, BAND, BAND, ELEM)))

# worst kernel / yardstick ratio per test and dtype (global, row, col, chan, elem), MI355X.
# Nothing exceeds 1.09, so the factors stand as first set (1.5 / 1.5 / 4); the weakest planted
# fault (bf16, one pixel's 64 channels zeroed) reaches 24x in the row and column bands and 90x
# per element.  The backward's whole-tensor ratio sits below 1 in bf16: the yardstick rounds the
# gradient of a1 and of t's direct path, the kernels dz1 and the whole dt.
MEASURED = {
    ("test_forward_local", "bf16"): (1.001, 1.001, 1.011, 1.010, 1.000),
    ("test_forward_local", "fp16"): (1.001, 1.001, 1.016, 1.020, 1.000),
    ("test_forward_late_tickets", "bf16"): (0.999, 1.001, 1.000, 1.005, 1.000),
    ("test_forward_late_tickets", "fp16"): (1.000, 0.995, 0.999, 1.010, 1.000),
    ("test_backward_dx_local strip", "bf16"): (0.970, 0.977, 1.021, 0.976, 1.084),
    ("test_backward_dx_local per-RCAB", "bf16"): (0.970, 0.973, 1.021, 0.984, 1.084),
    ("test_backward_dx_local strip", "fp16"): (0.996, 0.998, 0.999, 0.998, 1.000),
    ("test_backward_spotlight", "bf16"): (0.938, 1.003, 1.018, 0.941, 1.000),
    ("test_backward_spotlight", "fp16"): (0.995, 1.064, 1.004, 1.001, 1.000),
    ("test_training_forward_saves_local", "bf16"): (1.002, 1.006, 1.006, 1.000, 1.089),
    ("test_training_forward_saves_local", "fp16"): (1.000, 1.002, 1.014, 1.009, 1.062),
    ("test_group_strip_vs_oracle", "bf16"): (1.002, 1.004, 1.026, 1.019, 1.004),
    ("test_group_strip_vs_oracle", "fp16"): (1.001, 1.006, 1.015, 1.012, 1.020),
    ("test_group_chain_vs_oracle", "bf16"): (1.002, 0.991, 1.002, 0.997, 1.000),
    ("test_group_chain_vs_oracle", "fp16"): (1.000, 0.995, 1.022, 1.021, 1.000),
    ("test_group_strip_bwd_vs_oracle", "bf16"): (0.999, 0.988, 1.052, 0.989, 1.031),
    ("test_group_strip_bwd_fp16_vs_oracle", "fp16"): (0.991, 1.041, 0.999, 0.998, 1.000),
}

# the conv kernels, worst over the cases and outputs of each test in tests/test_gpu_conv_local.py
# (global, row, column, channel, element, tile, visit index; then the largest fraction of the
# partials' fp32 bound, None where the test has no partials), MI355X, 256 CUs.  A single conv's
# fp32 summation order disappears under the 16-bit rounding of its output: every ratio is 1.000
# to three digits but the wide kernel's fp16 element metric.  The DOT partials of k_conv3x3_g use
# more of their (n - 1)-term-only bound than the pool / PReLU-backward partials of theirs.
MEASURED_CONV = {
    ("test_conv_g_upsampler", "bf16"): (1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 1.000, None),
    ("test_conv_g_upsampler", "fp16"): (1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 1.000, None),
    ("test_conv_g_c64", "bf16"): (1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 2.35e-3),
    ("test_conv_g_c64", "fp16"): (1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 3.79e-3),
    ("test_conv_p_c64", "bf16"): (1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 2.29e-4),
    ("test_conv_p_c64", "fp16"): (1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 2.09e-4),
    ("test_conv_v_wide", "bf16"): (1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 1.00e-4),
    ("test_conv_v_wide", "fp16"): (1.000, 1.000, 1.000, 1.000, 1.001, 1.000, 1.000, 1.01e-4),
}


def _rel(num, den):
    """sqrt(num / den) elementwise; a band whose reference is exactly zero counts 0 if the
    result is zero there too, inf otherwise."""
    safe = torch.where(den > 0, den, torch.ones_like(den))
    r = torch.sqrt(num / safe)
    return torch.where(den > 0, r, torch.where(num > 0, torch.full_like(r, math.inf), torch.zeros_like(r)))


def local_errors(got, ref):
    """got, ref NCHW -> dict of five floats (float64 arithmetic): the whole-tensor rel-L2, the
    worst rel-L2 over (image, row), (image, column) and (image, channel) bands, and
    max|got - ref| / rms(ref)."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    assert g.shape == r.shape and g.dim() == 4, (g.shape, r.shape)
    d2, r2 = (g - r) ** 2, r ** 2
    out = {"global": float(_rel(d2.sum(), r2.sum()))}
    for name, dims in (("row", (1, 3)), ("col", (1, 2)), ("chan", (2, 3))):
        out[name] = float(_rel(d2.sum(dims), r2.sum(dims)).max())
    out["elem"] = float(_rel(d2.max(), r2.mean()))
    return out


def _fmt(e):
    return " ".join(f"{k} {e[k]:.3e}" for k in METRICS)


def assert_local(got, ref, yard, what, factor=None):
    """Every metric of `got` against `ref` is at most FACTOR x the same metric of the yardstick
    `yard` against `ref`.  Prints the ten numbers; -> the five got / yard ratios."""
    factor = factor or FACTOR
    eg, ey = local_errors(got, ref), local_errors(yard, ref)
    ratio = {k: (eg[k] / ey[k] if ey[k] > 0 else (0.0 if eg[k] == 0 else math.inf)) for k in METRICS}
    print(f"{what}: got  {_fmt(eg)}")
    print(f"{what}: yard {_fmt(ey)}")
    print(f"{what}: got/yard " + " ".join(f"{k} {ratio[k]:.3f}" for k in METRICS))
    bad = {k: (eg[k], ey[k], ratio[k]) for k in METRICS if not eg[k] <= factor[k] * ey[k]}
    assert not bad, f"{what}: (got, yardstick, ratio) over the factor {factor}: {bad}"
    return ratio


# ---------------------------------------------------------------------------------------
# the yardstick: residual_group with the kernels' rounding points
# ---------------------------------------------------------------------------------------
class RoundBoth(torch.autograd.Function):
    """Identity that rounds to `dtype` and back: the value in the forward, the gradient in the
    backward."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.dtype = dtype
        return x.to(dtype).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).to(g.dtype), None


def _rnd(t, dtype):
    return t if dtype is None else RoundBoth.apply(t, dtype)


def _prelu(x, a):
    return torch.where(x > 0, x, a.view(1, -1, 1, 1) * x)


def _conv(x, w, b):
    return torch.nn.functional.conv2d(x, w, b, padding=1)


def _group(x, p, n, dtype, pre, res_scale, record, chain_in=None):
    out = x if chain_in is None else chain_in
    for j in range(n):
        b = f"{pre}blocks.{j}."
        xj = out
        z1 = _conv(xj, p[b + "conv1.weight"], p[b + "conv1.bias"])
        a1 = _rnd(_prelu(z1, p[b + "prelu.weight"]), dtype)
        t = _conv(a1, p[b + "conv2.weight"], p[b + "conv2.bias"])
        # the gate from the unrounded t (the kernels pool their fp32 sums, not the stored t)
        h = torch.relu(t.mean(dim=(2, 3)) @ p[b + "channel_attention.fc.0.weight"].t())
        s = torch.sigmoid(h @ p[b + "channel_attention.fc.2.weight"].t())
        tr = _rnd(t, dtype)
        out = _rnd(tr * s[:, :, None, None] * res_scale + xj, dtype)
        if record is not None:
            record[f"x{j}"], record[f"z1{j}"], record[f"a1{j}"] = xj.detach(), z1.detach(), a1.detach()
            record[f"t{j}"], record[f"s{j}"] = tr.detach(), s.detach()
    if record is not None:
        record["x_last"] = out.detach()
    return _conv(out, p[pre + "conv.weight"], p[pre + "conv.bias"]) + x


def rounded_group(x, p, n, dtype, pre="rg.", res_scale=0.2, record=None):
    """The oracle's residual_group (RCABs, group conv, skip) on NCHW `x` with a1, t_j and every
    RCAB's output rounded to `dtype` (the SE gate from the unrounded t), the group output
    rounded; arithmetic in x's float type (the parameters are cast to it).  dtype=None rounds
    nothing: the oracle itself, in float64 when x is.  record: filled with RCAB j's input x{j},
    z1{j}, a1{j}, t{j} (as stored: rounded), s{j} and the chain's output x_last."""
    p = {k: v.to(x.dtype) for k, v in p.items()}
    with torch.no_grad():
        y = _group(x, p, n, dtype, pre, res_scale, record)
        return y if dtype is None else y.to(dtype).to(x.dtype)


def rounded_group_grads(x, p, n, dtype, dy, dres=None, pre="rg.", res_scale=0.2):
    """dx (and the parameter gradients) of the group by autograd of `rounded_group`'s chain
    with RoundBoth at a1, t_j, every RCAB's output and the chain's input: its backward rounds
    the gradients there, standing in for the kernels' rounding of dz1, dt and every RCAB's
    input gradient.  dx = the chain's gradient + dy (the skip) + dres, rounded as stored.
    dtype=None: the oracle's plain autograd.  -> (dx, {name: gradient})."""
    leaves = {k: v.detach().to(x.dtype).clone().requires_grad_(True) for k, v in p.items()}
    xl = x.detach().clone().requires_grad_(True)
    y = _group(xl, leaves, n, dtype, pre, res_scale, None, chain_in=_rnd(xl, dtype))
    (y * dy.to(x.dtype)).sum().backward()
    dx = xl.grad if dres is None else xl.grad + dres.to(x.dtype)
    if dtype is not None:
        dx = dx.to(dtype).to(x.dtype)
    return dx, {k: v.grad for k, v in leaves.items()}


# ---------------------------------------------------------------------------------------
# the conv kernels (k_conv3x3_g / _p / _v): tiles per block, operands, reference, yardstick
# ---------------------------------------------------------------------------------------
TilesPerBlock = collections.namedtuple("TilesPerBlock", "lo hi k nslot")


def tiles_per_block(ntiles, ncot, num_cus, floor=0):
    """fen_detail::persistent_grid and the persistent kernels' `nmine`, restated: the grid is
    one block per CU rounded down to whole sets of the `ncot` blocks that share a tile, at least
    `floor`, at most ntiles * ncot; nslot = grid / ncot blocks walk the tiles, block `slot`
    takes t = slot, slot + nslot, ... -- (ntiles - slot + nslot - 1) / nslot of them, one more
    for slot < ntiles % nslot.  -> (fewest, most tiles of a block with any, the visit index
    k = t // nslot of every tile, nslot)."""
    grid = num_cus - num_cus % ncot
    grid = min(max(grid, floor), ntiles * ncot)
    nslot = grid // ncot
    nmine = [(ntiles - s + nslot - 1) // nslot for s in range(min(nslot, ntiles))]
    return TilesPerBlock(min(nmine), max(nmine), torch.arange(ntiles) // nslot, nslot)


# the per-kernel conv cases: name -> (Cin, Cout, ncot, grid floor, B, fewest tiles a block must
# see, (H, W) at 256 CUs).  "up": k_conv3x3_g on the upsampler stage conv; "c64": k_conv3x3_g /
# k_conv3x3_p on the 64-channel convs; "wide": k_conv3x3_v (Cout / 128 channel tiles, grid floor).
CONV_CASES = {"up": (64, 256, 4, 0, 3, 4, (152, 160)), "c64": (64, 64, 1, 0, 1, 4, (520, 536)),
              "wide": (128, 128, 1, 1, 1, 2, (424, 440))}


def conv_premises(name, B, H, W, num_cus):
    """-> (TilesPerBlock, whether the shape makes the case's point): every block sees at least
    the case's fewest tiles, both counts occur (for "wide": most blocks the larger), and an
    image edge is ragged (so one block mixes full and ragged tiles)."""
    _, _, ncot, floor, _, least, _ = CONV_CASES[name]
    ntiles = B * -(-H // 16) * -(-W // 16)
    tpb = tiles_per_block(ntiles, ncot, num_cus, floor)
    ok = tpb.lo >= least and tpb.hi == tpb.lo + 1 and (H % 16 == 8 or W % 16 == 8) and H % 8 == 0 and W % 8 == 0
    if name == "wide":
        ok = ok and 2 * (ntiles % tpb.nslot) > tpb.nslot
    return tpb, ok


def conv_shape(name, num_cus):
    """(B, H, W, Cin, Cout) of a case for a part with `num_cus` CUs: the 256-CU shape where its
    premises hold, else the smallest H = 16 th - 8, W = 16 tw - 8 (tw = th or th + 1) at which
    they do."""
    Cin, Cout, _, _, B, _, hw = CONV_CASES[name]
    if not conv_premises(name, B, *hw, num_cus)[1]:
        hw = next((16 * th - 8, 16 * tw - 8) for th in range(1, 200) for tw in (th, th + 1)
                  if conv_premises(name, B, 16 * th - 8, 16 * tw - 8, num_cus)[1])
    return (B, *hw, Cin, Cout)


def _tiled(t, th, tw):
    """NCHW -> [B, C, nth, th, ntw, tw], zero-padded to whole tiles."""
    B, C, H, W = t.shape
    nth, ntw = -(-H // th), -(-W // tw)
    p = torch.zeros(B, C, nth * th, ntw * tw, dtype=t.dtype)
    p[:, :, :H, :W] = t
    return p.view(B, C, nth, th, ntw, tw)


def tile_sums(t, th=16, tw=16):
    """NCHW -> [tile][channel] sums over th x tw tiles, tile = (b * nth + ty) * ntw + tx: the
    layout of fen_conv_desc.part."""
    s = _tiled(t, th, tw).sum((3, 5))                     # [B, C, nth, ntw]
    return s.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def tile_errors(got, ref, th, tw, k=None):
    """The worst rel-L2 over (image, th x tw tile) with the tile's index, and the worst rel-L2
    over the tiles grouped by visit index k[tile] with that k (float64 arithmetic).  The tile
    index is (b * nth + ty) * ntw + tx, the conv kernels' own when th x tw is the image of a
    16 x 16 conv tile in the output's space (32 x 32 after PixelShuffle, 8 x 8 after the pool)."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    assert g.shape == r.shape and g.dim() == 4, (g.shape, r.shape)
    d2 = _tiled((g - r) ** 2, th, tw).sum((1, 3, 5)).reshape(-1)
    r2 = _tiled(r ** 2, th, tw).sum((1, 3, 5)).reshape(-1)
    e = _rel(d2, r2)
    out = {"tile": float(e.max()), "tile_at": int(e.argmax())}
    if k is not None:
        assert k.numel() == e.numel(), (k.numel(), e.numel())
        nk = int(k.max()) + 1
        ev = _rel(torch.zeros(nk, dtype=d2.dtype).index_add_(0, k, d2),
                  torch.zeros(nk, dtype=d2.dtype).index_add_(0, k, r2))
        out["visit"], out["visit_at"] = float(ev.max()), int(ev.argmax())
    return out


def assert_tiles(got, ref, yard, th, tw, tpb, what):
    """tile_errors of `got` at most BAND x the yardstick's, per tile and per visit index.  The
    message names the worst tile, its slot and its visit index.  -> the two got / yard ratios."""
    eg, ey = tile_errors(got, ref, th, tw, tpb.k), tile_errors(yard, ref, th, tw, tpb.k)
    t = eg["tile_at"]
    where = f"tile {t} (slot {t % tpb.nslot}, visit k={t // tpb.nslot} of {tpb.lo}..{tpb.hi}), worst visit k={eg['visit_at']}"
    ratio = {m: (eg[m] / ey[m] if ey[m] > 0 else (0.0 if eg[m] == 0 else math.inf)) for m in ("tile", "visit")}
    print(f"{what}: got  tile {eg['tile']:.3e} visit {eg['visit']:.3e} at {where}")
    print(f"{what}: yard tile {ey['tile']:.3e} visit {ey['visit']:.3e}")
    print(f"{what}: got/yard tile {ratio['tile']:.3f} visit {ratio['visit']:.3f}")
    bad = {m: (eg[m], ey[m], ratio[m]) for m in ("tile", "visit") if not eg[m] <= BAND * ey[m]}
    assert not bad, f"{what}: (got, yardstick, ratio) over the factor {BAND} at {where}: {bad}"
    return ratio


def assert_part(got, ref, bound, tpb, what):
    """Every (tile, channel) partial finite and within `bound` of the float64 tile sum `ref`.
    Prints and returns the achieved fraction of the bound."""
    g = got.detach().double().cpu()
    assert g.shape == ref.shape == bound.shape, (g.shape, ref.shape, bound.shape)
    nonfin = (~torch.isfinite(g)).any(1).nonzero().flatten().tolist()
    assert not nonfin, (f"{what}: partial rows not written: tiles {nonfin[:8]} "
                        f"(slot, k) {[(t % tpb.nslot, t // tpb.nslot) for t in nonfin[:8]]}")
    frac = (g - ref).abs() / bound
    worst = int(frac.argmax())
    t, c = divmod(worst, g.shape[1])
    f = float(frac.flatten()[worst])
    print(f"{what}: partials at {f:.3e} of the fp32 bound (tile {t}, slot {t % tpb.nslot}, visit k={t // tpb.nslot}, "
          f"channel {c})")
    assert f <= 1.0, f"{what}: partial of tile {t} (slot {t % tpb.nslot}, visit k={t // tpb.nslot}) channel {c} at {f:.3g}x its bound"
    return f


def dot_part(y_stored, pre_in):
    """DOT partials from the kernel's own stored y (NCHW): the float64 tile sums of y * pre_in and
    their bound.  A product of two 16-bit values is exact in fp32, so only the summation of the
    n = 256 terms rounds: 2^-24 (n - 1) sum |t_i|."""
    t = y_stored.double() * pre_in.double()
    return tile_sums(t), 2.0 ** -24 * 255 * tile_sums(t.abs())


DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
_CONV_CACHE = {}


def _conv_base(prec, B, H, W, Cin, Cout, seed):
    """x, w (generated in fp32, rounded to the compute dtype) and their bias-free convs in
    float64 and fp32, once per (seed, shape, dtype)."""
    key = (prec, B, H, W, Cin, Cout, seed)
    if key not in _CONV_CACHE:
        dtype = DT[prec]
        g = torch.Generator().manual_seed(seed)
        x_raw = torch.randn(B, Cin, H, W, generator=g)
        w_raw = torch.randn(Cout, Cin, 3, 3, generator=g) * (1.2 / (3 * Cin ** 0.5))
        x, w = x_raw.to(dtype).float(), w_raw.to(dtype).float()
        with torch.no_grad():
            z64 = torch.nn.functional.conv2d(x.double(), w.double(), None, padding=1)
            z32 = torch.nn.functional.conv2d(x, w, None, padding=1)
        _CONV_CACHE[key] = {"x": x, "w": w, "x_raw": x_raw, "w_raw": w_raw, "z64": z64, "z32": z32}
    return _CONV_CACHE[key]


def _conv_abs(base):
    """sum_k |x_k w_k| per output element (float64), once per base."""
    if "abs" not in base:
        with torch.no_grad():
            base["abs"] = torch.nn.functional.conv2d(base["x"].double().abs(), base["w"].double().abs(), None, padding=1)
    return base["abs"]



def pixel_shuffle2(t):
    """[B, 4C, H, W] -> [B, C, 2H, 2W], channel 4c + 2i + j to pixel (2h + i, 2w + j)."""
    return torch.nn.functional.pixel_shuffle(t, 2)


class ConvCase:
    """Operands, float64 reference and fp32 yardstick of one fen_conv3x3 call (see conv_case)."""

    def __init__(self, prec, base, **kw):
        self.prec, self.dtype, self.base = prec, DT[prec], base
        self.x, self.w = base["x"], base["w"]
        self.__dict__.update(kw)

    def epilogue(self, z, rdt, bias=None, alpha=None):
        """The kernels' epilogue on a bias-free conv result `z` (NCHW, float64 or fp32), in z's
        float type, rounding to `rdt` (None: nowhere) where a 16-bit tensor is stored.
        -> {"y", "y_pre", "y_pool", "part"} (those the case has)."""
        f = z.dtype
        bias = self.bias if bias is None else bias
        alpha = self.alpha if alpha is None else alpha
        rnd = (lambda t: t) if rdt is None else (lambda t: t.to(rdt).to(f))
        v = z if bias is None else z + bias.to(f).view(1, -1, 1, 1)
        for r in self.res:
            v = v + r.to(f)
        out = {}
        if self.mode == "prelu_bwd":
            # the sign source per channel: post_in where the channel's group of 4 has all slopes
            # > 0 (the kernel then divides the slope partial by the slope), pre_in elsewhere
            a = alpha.to(f).view(1, -1, 1, 1)
            src = self.pre_in.to(f)
            scale = torch.ones_like(a)
            if self.post_in is not None:
                rec = self.rec.view(1, -1, 1, 1)
                src = torch.where(rec, self.post_in.to(f), src)
                scale = torch.where(rec, 1.0 / a, scale)
            neg = ~(src > 0)
            out["part"] = tile_sums(torch.where(neg, v * src, torch.zeros_like(v))) * scale.view(1, -1)
            out["y"] = rnd(torch.where(neg, v * a, v))
            return out
        if self.mode == "relu_bwd":
            out["y"] = rnd(torch.where(self.pre_in.to(f) > 0, v, torch.zeros_like(v)))
            return out
        if self.mode == "pool":
            out["part"] = tile_sums(v)                         # of the fp32 sums, not the stored y
        if self.shuffle:
            v = pixel_shuffle2(v)
        if self.mode == "prelu":
            if self.want_pre:
                out["y_pre"] = rnd(v)
            # PReLU of the fp32 accumulator (final_v / prelu_f(v[r], ..)), not of the stored y_pre
            v = _prelu(v, alpha.to(f))
        out["y"] = rnd(v)
        if self.pool2:
            out["y_pool"] = torch.nn.functional.max_pool2d(out["y"], 2)   # max commutes with the rounding
        return out

    def part_bound(self):
        """2^-24 ((n - 1) sum |t_i| + ops sum_i |f_i| A_i) per (tile, channel): the worst case of
        an fp32 sum of n = 256 terms t_i = f_i z_i, each z_i itself an fp32 sum of K = 9 Cin
        products plus the bias and residual adds (ops = K + 1 + residuals, one more for the
        product with f_i and three for the division by the slope where there is one), A_i =
        sum_k |x_k w_k| + |b| + sum |res|; f_i = 1 for POOL, the PReLU-backward's pre-activation
        where it is <= 0."""
        u, K = 2.0 ** -24, 9 * self.x.shape[1]
        A = _conv_abs(self.base)
        if self.bias is not None:
            A = A + self.bias.double().abs().view(1, -1, 1, 1)
        for r in self.res:
            A = A + r.double().abs()
        ops = K + 1 + len(self.res)
        ref = self.ref_terms
        if self.mode == "prelu_bwd":
            ops += 4
            A = A * self.ref_factor.abs()
        return u * (255 * tile_sums(ref.abs()) + ops * tile_sums(A)) * self.ref_scale.view(1, -1)


def conv_case(prec, B, H, W, Cin, Cout, *, seed=0, mode="none", bias=False, nres=0, shuffle=False, want_pre=False,
              pool2=False, alpha="mixed", post_in=False):
    """Operands, reference and yardstick of one 3x3 conv with one of the kernels' epilogues.

    mode: "none", "prelu", "pool", "prelu_bwd", "relu_bwd" (DOT's partials come from the kernel's
    own y: dot_part).  x, w, the residuals, pre_in and post_in are generated in fp32 and rounded
    to the compute dtype; bias and slopes stay fp32, as the kernels take them.  `.ref` is the
    epilogue in float64 on the float64 conv of those operands, `.yard` the same in fp32 (torch
    CPU) rounded to the 16-bit format exactly where the kernels store a 16-bit tensor:
      * y_pre = round(v), v = conv + bias + residuals in fp32 (conv_epilogue final_v(.., k = 0);
        k_conv3x3_g pass 2 `v[r]`);
      * y = round(PReLU(v)) with PReLU applied to the fp32 v, not to the stored y_pre (final_v
        k = 1; k_conv3x3_g `o[r] = prelu_f(v[r], ..)`); without PReLU y = round(v);
      * PixelShuffle only moves elements (the slope of a shuffled channel c = cp % Cq);
      * y_pool = the 2x2 max of the stored y, no further rounding (pool2_store);
      * PRELU_BWD: y = round(v * (pre > 0 ? 1 : slope)) from the fp32 v; RELU_BWD: y = round(pre > 0 ? v : 0);
      * the POOL / PRELU_BWD partials are sums of the fp32 v, never of a rounded value.
    Nothing else is rounded.  The bias-free convs are cached per (seed, shape, dtype): every
    epilogue of one shape shares one float64 conv.  alpha: "mixed" (some slopes <= 0), "pos", "relu"
    (zeros)."""
    base = _conv_base(prec, B, H, W, Cin, Cout, seed)
    dtype = DT[prec]
    g = torch.Generator().manual_seed(1000 + seed)
    Ca = Cout // 4 if shuffle else Cout                       # channels after the shuffle
    c = ConvCase(prec, base, mode=mode, shuffle=shuffle, want_pre=want_pre, pool2=pool2, bias=None, alpha=None,
                 res=[], pre_in=None, post_in=None, rec=None)
    b_all = torch.randn(Cout, generator=g) * 0.1
    a_all = torch.rand(Ca, generator=g) * 0.45 + 0.05
    if bias:
        c.bias = b_all
    if mode in ("prelu", "prelu_bwd"):
        if alpha == "mixed":
            a_all[5], a_all[9], a_all[Ca - 24] = -0.2, 0.0, -0.05
        c.alpha = torch.zeros(Ca) if alpha == "relu" else a_all
    c.res = [torch.randn(B, Cout, H, W, generator=g).to(dtype).float() for _ in range(nres)]
    if mode in ("prelu_bwd", "relu_bwd"):
        c.pre_in = torch.randn(B, Cout, H, W, generator=g).to(dtype).float()
        c.pre_in[0, :, 0, :4] = 0                             # pre == 0 counts as not positive
    if post_in:
        # the forward's stored activation of pre_in; the kernel reads it instead of pre_in for the
        # channel groups of 4 whose slopes are all > 0
        c.post_in = _prelu(c.pre_in, c.alpha).to(dtype).float()
        c.rec = (c.alpha.view(-1, 4) > 0).all(1).repeat_interleave(4)
    z64, z32 = base["z64"], base["z32"]
    c.ref = c.epilogue(z64, None)
    c.yard = c.epilogue(z32, dtype)
    if "part" in c.ref:
        v = z64 if c.bias is None else z64 + c.bias.double().view(1, -1, 1, 1)
        for r in c.res:
            v = v + r.double()
        c.ref_scale = torch.ones(Cout, dtype=torch.float64)
        if mode == "prelu_bwd":
            src = c.pre_in.double()
            if post_in:
                src = torch.where(c.rec.view(1, -1, 1, 1), c.post_in.double(), src)
                c.ref_scale = torch.where(c.rec, 1.0 / c.alpha.double().abs().clamp_min(1e-30), c.ref_scale)
            c.ref_factor = torch.where(src > 0, torch.zeros_like(src), src)
            c.ref_terms = v * c.ref_factor
        else:
            c.ref_terms = v
    return c

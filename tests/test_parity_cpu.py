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

"""Local parity of the strip-resident kernels (fen_group_strip, fen_group_strip_bwd): errors
confined to one row, one image or one strip.

The whole-tensor rel-L2 of test_gpu_group_strip.py / test_gpu_group_strip_bwd.py dilutes a
fault that sits in one row of one image by sqrt(1 / (B * H)).  Here every result is measured
per (image, row), (image, column) and (image, channel) band and per element against the float64
oracle, and bounded by a fixed factor of the same metric of the CPU yardstick (the oracle with
the kernels' documented rounding points, tests/parity.py: 1.5x per band and whole-tensor, 4x
per element) -- bounds derived at run time from the yardstick, never from the kernel's output.
tests/test_parity_cpu.py shows that a single wrong row, channel row, pixel or strip exceeds
them at least five-fold.

Shapes (W = C = 64): one strip per image (H=8, no seam), one seam (H=16), an interior strip
with both halos (H=24), eight strips (H=64); B=40 x 8 strips = 320 blocks, more than CUs, so
the last tickets wait for a CU -- built from two images tiled 20 times, every replica
bit-identical to the first pair (the pool partials are summed in strip order per image,
group_strip.hip "summed in strip order", and nothing else depends on the ticket).  Backward
spotlight: dy is zero outside one strip of one image, so every other image's dx is exactly
zero and each parameter gradient comes from that strip alone -- a lost or doubled strip
contribution is O(1) instead of 1/320 of the sum.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity  # noqa: E402
from test_gpu_group_strip import _params, _run, _run_save, _work_error  # noqa: E402
from test_gpu_group_strip_bwd import _fwd_bwd, _rel  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _rounded_weights(q, dtype):
    return {k: (v.to(dtype).float() if v.dim() == 4 else v) for k, v in q.items()}


def _nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV, dtype)


def _nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,n", [(3, 8, 2), (2, 16, 3), (2, 24, 2), (2, 64, 3)])
def test_forward_local(prec, B, H, n):
    dtype = DT[prec]
    q = _params(n, seed=51 + n)
    qr = _rounded_weights(q, dtype)
    x = torch.randn(B, 64, H, 64, generator=torch.Generator().manual_seed(B + H)).to(dtype).float()
    ref = parity.rounded_group(x.double(), qr, n, None)
    yard = parity.rounded_group(x, qr, n, dtype)
    y, _, ctx, used = _run(q, n, _nhwc(x, dtype), dtype)
    assert used and _work_error(ctx) == [(0, 0, 0)]
    parity.assert_local(_nchw(y), ref, yard, f"fwd {prec} B={B} H={H} n={n}")


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_forward_late_tickets(prec):
    """B=40 (320 blocks): every replica of the two tiled images bit-identical to the first
    pair, and that pair within the local bounds."""
    dtype = DT[prec]
    B, H, n = 40, 64, 2
    q = _params(n, seed=57)
    qr = _rounded_weights(q, dtype)
    x2 = torch.randn(2, 64, H, 64, generator=torch.Generator().manual_seed(17)).to(dtype).float()
    ref = parity.rounded_group(x2.double(), qr, n, None)
    yard = parity.rounded_group(x2, qr, n, dtype)
    y, _, ctx, used = _run(q, n, _nhwc(x2.repeat(B // 2, 1, 1, 1), dtype), dtype)
    assert used and _work_error(ctx) == [(0, 0, 0)]
    differ = [b for b in range(B) if not torch.equal(y[b], y[b % 2])]
    assert not differ, differ
    parity.assert_local(_nchw(y[:2]), ref, yard, f"fwd late tickets {prec}")


def _bwd_inputs(B, H, dtype, seed, dres):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 64, H, 64, generator=g).to(dtype).float()
    dy = (torch.randn(B, 64, H, 64, generator=g) * 1e-2).to(dtype).float()
    r = (torch.randn(B, 64, H, 64, generator=g) * 1e-2).to(dtype).float() if dres else None
    return x, dy, r


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,n,dres", [(3, 8, 2, False), (2, 24, 3, True), (2, 64, 3, False)])
def test_backward_dx_local(prec, B, H, n, dres):
    """dx of the strip backward (both dtypes) and, in bf16, of the per-RCAB backward, each
    within the local bounds of the oracle's."""
    dtype = DT[prec]
    q = _params(n, seed=61 + n)
    qr = _rounded_weights(q, dtype)
    x, dy, r = _bwd_inputs(B, H, dtype, seed=B + H, dres=dres)
    dx_ref, _ = parity.rounded_group_grads(x.double(), qr, n, None, dy, r)
    dx_yard, _ = parity.rounded_group_grads(x, qr, n, dtype, dy, r)
    xd, dyd, rd = _nhwc(x, dtype), _nhwc(dy, dtype), (_nhwc(r, dtype) if dres else None)
    bf16 = prec == "bf16"
    dx_s, _, _, used = _fwd_bwd(q, n, xd, dyd, dtype, True, dres=rd, wgrads=bf16)
    assert used
    parity.assert_local(_nchw(dx_s), dx_ref, dx_yard, f"dx strip {prec} B={B} H={H} n={n}")
    if bf16:
        dx_p, _, _, used_p = _fwd_bwd(q, n, xd, dyd, dtype, False, dres=rd)
        assert not used_p
        parity.assert_local(_nchw(dx_p), dx_ref, dx_yard, f"dx per-RCAB {prec} B={B} H={H} n={n}")


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,n,img,strip,dres", [(3, 24, 2, 0, 0, False), (3, 24, 2, 1, 1, True),
                                                  (40, 64, 2, 39, 7, False)])
def test_backward_spotlight(prec, B, H, n, img, strip, dres):
    """dy (and dres) zero outside one 8-row strip of one image."""
    dtype = DT[prec]
    q = _params(n, seed=71 + n)
    qr = _rounded_weights(q, dtype)
    x, dy, r = _bwd_inputs(B, H, dtype, seed=B + H + strip, dres=dres)
    mask = torch.zeros(B, 1, H, 1)
    mask[img, :, 8 * strip:8 * strip + 8] = 1
    dy = dy * mask
    r = r * mask if dres else None
    lit = slice(img, img + 1)
    rl = r[lit] if dres else None
    dx_ref, g_ref = parity.rounded_group_grads(x[lit].double(), qr, n, None, dy[lit], rl)
    dx_yard, _ = parity.rounded_group_grads(x[lit], qr, n, dtype, dy[lit], rl)
    xd, dyd, rd = _nhwc(x, dtype), _nhwc(dy, dtype), (_nhwc(r, dtype) if dres else None)
    bf16 = prec == "bf16"
    dx_s, g_s, _, used = _fwd_bwd(q, n, xd, dyd, dtype, True, dres=rd, wgrads=bf16)
    assert used
    dark = [b for b in range(B) if b != img and int(torch.count_nonzero(dx_s[b])) != 0]
    assert not dark, dark
    parity.assert_local(_nchw(dx_s[lit]), dx_ref, dx_yard, f"spotlight {prec} B={B} H={H} image {img} strip {strip}")
    if bf16:
        _, g_p, _, used_p = _fwd_bwd(q, n, xd, dyd, dtype, False, dres=rd)
        assert not used_p
        worst = (0.0, "")
        for k in g_ref:
            es, ep = _rel(g_s[k], g_ref[k]), _rel(g_p[k], g_ref[k])
            worst = max(worst, (es, k))
            assert es <= 1.25 * ep + 1e-2, (k, es, ep)
        print(f"  worst parameter gradient: {worst[1]} rel {worst[0]:.2e}")


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_training_forward_saves_local(prec):
    """The training forward's saved a1, t_j and x_j of the last RCAB (what the backward reads)
    against the same intermediates of the oracle and of the yardstick."""
    dtype = DT[prec]
    B, H, n = 2, 16, 3
    q = _params(n, seed=81)
    qr = _rounded_weights(q, dtype)
    x = torch.randn(B, 64, H, 64, generator=torch.Generator().manual_seed(23)).to(dtype).float()
    rec_ref, rec_yard = {}, {}
    ref = parity.rounded_group(x.double(), qr, n, None, record=rec_ref)
    yard = parity.rounded_group(x, qr, n, dtype, record=rec_yard)
    y, sv, used = _run_save(q, n, _nhwc(x, dtype), dtype, True)
    assert used
    parity.assert_local(_nchw(y), ref, yard, f"train fwd {prec} y")
    blk = sv["blocks"][n - 1]
    for k in ("a1", "t", "x"):
        name = f"{k}{n - 1}"
        parity.assert_local(_nchw(blk[k]), rec_ref[name], rec_yard[name], f"train fwd {prec} saved {name}")

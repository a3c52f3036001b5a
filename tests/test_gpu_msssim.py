"""MS-SSIM on the HIP path (csrc/msssim.hip via src/losses/ssim.py) against the reference's own
value (tests/golden/g7_ssim.npz) and the CPU oracle's restatement with autograd (fp32); the
engine's L1 + w (1 - MS-SSIM) step against oracle autograd, then inside a captured graph."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import fen_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 3, 32, 32),       # the minimum: the last level is 2 x 2
          (1, 1, 33, 47),       # odd at several levels (floor cropping), one channel
          (2, 3, 100, 70),      # ragged 32-tiles at levels 0 and 1
          (3, 3, 64, 96)]       # the batch-global mean over B > 1
# the value and every level mean: the project's SSIM bound is 2e-6 on one mean, the exponents of
# the product sum to 1.87
VAL_TOL = 4e-6
# the gradient, relative to max |grad|: the per-scale SSIM bound is 1e-4; the fp32 oracle itself
# sits <= 1.4e-5 from a float64 replay on these shapes
GRAD_TOL = 2e-4


def _inputs(B, C, H, W):
    torch.manual_seed(B * 1000 + H)
    p = torch.rand(B, C, H, W)
    t = (0.6 * p + 0.4 * torch.rand(B, C, H, W)).clamp(0, 1)
    return p, t


@functools.lru_cache(maxsize=None)
def _oracle(B, C, H, W, weights=None):
    """(pred, target, MS-SSIM, per-level means, d(MS-SSIM)/dpred) of the fp32 CPU oracle."""
    p, t = _inputs(B, C, H, W)
    w = None if weights is None else torch.tensor(weights)
    pr = p.clone().requires_grad_(True)
    val = O.ms_ssim(pr, t, weights=w)
    val.backward()
    levels = 5 if weights is None else len(weights)
    means, a, b = [], p, t
    with torch.no_grad():
        for i in range(levels):
            lum, cs = O._ssim_terms(a, b, 11, 1.5, 1.0)
            means.append(float((lum * cs).mean() if i == levels - 1 else cs.mean()))
            a, b = F.avg_pool2d(a, 2, 2), F.avg_pool2d(b, 2, 2)
    return p, t, float(val.detach()), means, pr.grad.detach()


def _check_vs_oracle(shape, weights=None):
    from src.losses import MSSSIMLoss, ms_ssim
    from src.losses.ssim import _ms_run
    p, t, val, means, gref = _oracle(*shape, weights=weights)
    w = None if weights is None else torch.tensor(weights)
    td = t.to(DEV)
    out, _ = _ms_run(p.to(DEV), td, 11, 1.5, 1.0, w)
    out = out.cpu()
    for i, m in enumerate(means):           # per level first: a failure names its level
        print(f"{shape} level {i}: mean {float(out[1 + i]):.7f} oracle {m:.7f} diff {abs(float(out[1 + i]) - m):.2e}")
        assert abs(float(out[1 + i]) - m) <= VAL_TOL, f"level {i}"
    print(f"{shape} value {float(out[0]):.7f} oracle {val:.7f} diff {abs(float(out[0]) - val):.2e}")
    assert abs(float(out[0]) - val) <= VAL_TOL
    kw = {} if w is None else {"weights": w}
    assert abs(float(ms_ssim(p.to(DEV), td, **kw)) - val) <= VAL_TOL
    pd = p.clone().to(DEV).requires_grad_(True)
    loss = MSSSIMLoss(**kw)(pd, td)
    loss.backward()
    assert abs(float(loss.detach()) - (1 - val)) <= VAL_TOL
    e = float((pd.grad.cpu() + gref).abs().max() / gref.abs().max())       # d(1 - ms) = -d(ms)
    print(f"{shape} gradient: max err / max |grad| = {e:.3e}")
    assert e <= GRAD_TOL, e


def test_msssim_matches_reference_golden(golden):
    from src.losses import ms_ssim
    g = golden("g7_ssim.npz")
    p, t = torch.from_numpy(g["pred64"]).to(DEV), torch.from_numpy(g["target64"]).to(DEV)
    got = float(ms_ssim(p, t))
    print(f"golden: {got:.7f} reference {float(g['msssim']):.7f}")
    assert abs(got - float(g["msssim"])) <= VAL_TOL
    assert abs(float(ms_ssim(p, p)) - 1.0) <= 1e-6


@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_msssim_vs_oracle(B, C, H, W):
    _check_vs_oracle((B, C, H, W))


def test_msssim_custom_weights():
    """Three scales: `levels` is the length of the weights, not 5."""
    _check_vs_oracle((2, 3, 40, 36), weights=(0.2, 0.3, 0.5))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_msssim_grad_accumulates_into_nhwc16(dtype):
    """grad_mode 2: grad_scale * d(MS-SSIM)/dpred ADDED to channels 0..C-1 of an NHWC [B,H,W,16]
    buffer (the generator's dL/dsr), padding channels untouched.  The correlated inputs of the
    shape tests (every level mean positive: no NaN path)."""
    from src.hip import lib as L
    from src.hip.program import ptr
    from src.losses.ssim import MS_SSIM_WEIGHTS, _window1d
    B, C, H, W = 2, 3, 40, 36
    p, t, _, _, gref = _oracle(B, C, H, W)
    scale = -0.3
    expect = scale * gref
    lib = L.load()
    base = 2e-4          # the order of the L1 gradient the buffer holds in the engine (w / N)
    buf = torch.full((B, H, W, 16), base, device=DEV, dtype=dtype)
    win = _window1d(11, 1.5).to(DEV)
    wts = torch.tensor(MS_SSIM_WEIGHTS, device=DEV)
    work = torch.empty(lib.fen_msssim_work_floats(B, C, H, W, 5), device=DEV)
    out = torch.empty(6, device=DEV)
    pd, td = p.to(DEV), t.to(DEV)
    L.check(lib.fen_msssim(L.dtype_code(dtype), B, C, H, W, ptr(pd), ptr(td), ptr(win), 11, 1e-4, 9e-4, ptr(wts), 5,
                           ptr(work), ptr(out), ptr(buf), scale, 2, torch.cuda.current_stream().cuda_stream), "msssim")
    torch.cuda.synchronize()
    base_q = torch.tensor(base, dtype=dtype).float()
    got = buf[..., :C].float().cpu().permute(0, 3, 1, 2) - base_q
    tol = 2e-4 if dtype == torch.float32 else 1e-2      # relative to max |expect| + base (bf16 storage)
    e = float((got - expect).abs().max() / (expect.abs().max() + base))
    print(f"{dtype} accumulate: max err / (max |expect| + base) = {e:.3e}")
    assert e <= tol
    assert bool((buf[..., C:].float().cpu() == base_q).all())


def test_msssim_deterministic():
    from src.losses.ssim import _ms_run
    p, t = _inputs(2, 3, 100, 70)
    pd, td = p.to(DEV), t.to(DEV)
    o1, g1 = _ms_run(pd, td, 11, 1.5, 1.0, None, grad_scale=-1.0)
    o2, g2 = _ms_run(pd, td, 11, 1.5, 1.0, None, grad_scale=-1.0)
    assert torch.equal(o1, o2) and torch.equal(g1, g2)


def test_msssim_refusals():
    from src.losses import MSSSIMLoss, ms_ssim
    small = torch.rand(1, 3, 16, 16, device=DEV)
    with pytest.raises(ValueError):
        ms_ssim(small, small)
    with pytest.raises(ValueError):
        MSSSIMLoss()(small, small)
    cpu = torch.rand(1, 3, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ms_ssim(cpu, cpu)
    with pytest.raises(NotImplementedError):
        ms_ssim(cpu.to(DEV), cpu.to(DEV), window_size=7)


def test_engine_step_with_msssim_fp32(golden):
    """FENEngine(ms_ssim_weight=0.2) fp32: generator grads of L1 + 0.2 (1 - MS-SSIM) vs oracle
    autograd; then the same program once more inside a captured graph (no host synchronisation
    in the launch sequence) with the loss unchanged."""
    from src.hip.engine import FENEngine
    from src.models import FaceEnhanceNet
    g1 = golden("g1_config1.npz")
    sd = {k[2:]: torch.from_numpy(v) for k, v in g1.items() if k.startswith("p/")}
    m = FaceEnhanceNet(num_channels=64, num_groups=1, blocks_per_group=2, reduction_ratio=4, scale_factor=4,
                       res_scale=0.2, precision="fp32")
    m.load_state_dict(sd)
    hr = torch.from_numpy(g1["hr"])
    eng = FENEngine(m, batch=2, lr_hw=(32, 32), dtype=torch.float32, train=True, ms_ssim_weight=0.2)
    eng.hr.copy_(hr.to(DEV))
    eng.ctx.run()
    torch.cuda.synchronize()
    shape = O.NetShape(64, 1, 2, 4, 4, 0.2)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    out = O.forward(leaves, O.lr_from_hr(hr), shape, training=True)
    loss = (out - hr).abs().mean() + 0.2 * (1 - O.ms_ssim(out, hr))
    loss.backward()
    got = float(eng.total_loss())
    print(f"engine loss {got:.7f} oracle {float(loss.detach()):.7f}")
    assert abs(got - float(loss.detach())) <= 1e-5 * float(loss.detach())
    bad = {}
    for k, gg in eng.grads.items():
        ref = leaves[k].grad.double()
        e = float((gg.cpu().double() - ref).norm() / max(ref.norm(), 1e-30))
        if not e <= 1e-4:
            bad[k] = e
    assert not bad, bad
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        eng.ctx.run()
    eng.ms_ssim_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert float(eng.total_loss()) == got

"""src.evaluation on the HIP path: fen_image_metrics (csrc/metrics.hip) against a CPU
restatement -- psnr_batch in float64 on the same fp32 inputs and the fp32 oracle's per-image
SSIM -- its dataset table / cursor contract, determinism, graph capture and refusals; then
MetricCalculator.evaluate_dataset / compute_metrics against the module path measured on the host.

Measured on an MI355X over the twelve kernel cases: mse relative error <= 1.34e-7, PSNR <= 2.4e-6
dB, per-image SSIM <= 3.0e-7; evaluate_dataset per image <= 9.0e-7 dB and <= 3.0e-8 SSIM."""
import functools

import numpy as np
import pytest
import torch

from oracle import fen_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 3, 32, 32),       # one tile
          (3, 3, 40, 72),       # ragged tiles in both dimensions, B > 1
          (2, 1, 11, 13),       # smaller than a tile, barely window-sized, one channel
          (5, 3, 64, 64)]
# mse against float64, relative: a fixed-order tree over at most 12,288 fp32 terms (a linear sum's
# worst case would be 12288 * 2^-24 = 7e-4)
MSE_RTOL = 1e-5
# PSNR in dB: d(10 log10 x) = 4.343 dx / x, so the mse bound gives 4.4e-5 dB; the fp32 log10, the
# product and the stored value add a few ulp of at most 100 dB (7.6e-6 each)
PSNR_TOL = 1e-4
SENTINEL = -777.0


def _ssim_close(got, ref):
    """The per-image SSIM bound of tests/test_gpu_ssim.py:43 (values against the oracle)."""
    return torch.allclose(got, ref, atol=2e-6)


def _inputs(B, C, H, W):
    """As tests/test_gpu_msssim.py::_inputs."""
    torch.manual_seed(B * 1000 + H)
    p = torch.rand(B, C, H, W)
    t = (0.6 * p + 0.4 * torch.rand(B, C, H, W)).clamp(0, 1)
    return p, t


def _transform(p, flags):
    """flags on pred, restated in numpy float32."""
    a = p.numpy().astype(np.float32)
    if flags & 1:
        a = np.clip(a, np.float32(0), np.float32(1))
    if flags & 2:
        a = np.floor(a * np.float32(255)) / np.float32(255)
    assert a.dtype == np.float32
    return torch.from_numpy(a)


def _psnr64(p, t):
    """(mse, psnr_batch) in float64 on fp32 inputs."""
    mse = ((p.double() - t.double()) ** 2).mean(dim=[1, 2, 3])
    return mse, 10 * torch.log10(1.0 / (mse + 1e-10))


@functools.lru_cache(maxsize=None)
def _case(B, C, H, W, flags):
    """(pred, target, mse64, psnr64, oracle per-image SSIM): computed once, shared, left unchanged."""
    p, t = _inputs(B, C, H, W)
    if flags:
        p = p * 1.6 - 0.3               # [-0.3, 1.3]: the clamp bites
    q = _transform(p, flags)
    mse, ps = _psnr64(q, t)
    return p, t, mse, ps, O.ssim(q, t, size_average=False)


def _run(p, t, flags=0, **kw):
    from src.evaluation.metrics import image_metrics
    return image_metrics(p.to(DEV), t.to(DEV), 1.0, flags, **kw)


@pytest.mark.parametrize("flags", [0, 1, 3])
@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_kernel_vs_cpu_restatement(B, C, H, W, flags):
    p, t, mse, ps, ss = _case(B, C, H, W, flags)
    out = _run(p, t, flags).cpu()
    e_mse = float(((out[0].double() - mse).abs() / mse).max())
    e_ps = float((out[1].double() - ps).abs().max())
    e_ss = float((out[2] - ss).abs().max())
    print(f"{(B, C, H, W)} flags {flags}: mse rel {e_mse:.3e}  psnr {e_ps:.3e} dB  ssim {e_ss:.3e}")
    assert e_mse <= MSE_RTOL
    assert e_ps <= PSNR_TOL
    assert _ssim_close(out[2], ss), e_ss
    if flags == 0:
        from src.evaluation import psnr, psnr_batch
        assert torch.equal(psnr_batch(p.to(DEV), t.to(DEV)).cpu(), out[1])
        glob = 10 * np.log10(1.0 / float(mse.mean()))
        assert abs(float(psnr(p.to(DEV), t.to(DEV))) - glob) <= PSNR_TOL


@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_quantised_codes_equal_numpy(B, C, H, W):
    """Flag 3 on a tensor against its own numpy-quantised copy: every 8-bit code equal means
    mse = 0 exactly, PSNR = 10 log10(1 / 1e-10) = 100 dB."""
    p = _case(B, C, H, W, 3)[0]
    out = _run(p, _transform(p, 3), 3).cpu()
    assert bool((out[0] == 0).all()), out[0]
    assert float((out[1] - 100.0).abs().max()) <= PSNR_TOL
    assert float((out[2] - 1.0).abs().max()) <= 2e-6


def _table(cap, guard=16):
    """A [2, cap] table inside a larger sentinel-filled buffer."""
    big = torch.full((2 * cap + 2 * guard,), SENTINEL, device=DEV)
    return big, big[guard:guard + 2 * cap].view(2, cap)


def test_table_contract():
    B, cap = 3, 8
    big, table = _table(cap)
    state = torch.zeros(2, dtype=torch.int32, device=DEV)
    cursor, nvalid = state[0:1], state[1:2]
    outs = []
    for call, n in enumerate([3, 3, 1]):
        p, t = _inputs(B, 3, 40 + call, 36)
        nvalid.fill_(n)
        outs.append((_run(p, t, 1, table=table, cursor=cursor, nvalid=nvalid).cpu(), n))
    assert int(cursor) == 7
    tab = table.cpu()
    exp = torch.cat([o[1:, :n] for o, n in outs], dim=1)
    assert torch.equal(tab[:, :7], exp)
    assert bool((tab[:, 7] == SENTINEL).all())
    p, t = _inputs(B, 3, 44, 36)
    nvalid.fill_(3)
    o4 = _run(p, t, 1, table=table, cursor=cursor, nvalid=nvalid).cpu()
    assert int(cursor) == 10
    tab = table.cpu()
    assert torch.equal(tab[:, :7], exp) and torch.equal(tab[:, 7], o4[1:, 0])
    g = big.cpu()
    assert bool((g[:16] == SENTINEL).all()) and bool((g[-16:] == SENTINEL).all())
    # nvalid NULL: all B images
    big2, table2 = _table(cap)
    c2 = torch.zeros(1, dtype=torch.int32, device=DEV)
    o = _run(p, t, 1, table=table2, cursor=c2).cpu()
    assert int(c2) == B and torch.equal(table2.cpu()[:, :B], o[1:])


def test_deterministic():
    p, t = _case(3, 3, 40, 72, 1)[:2]
    res = []
    for _ in range(2):
        _, table = _table(4)
        cur = torch.zeros(1, dtype=torch.int32, device=DEV)
        o = _run(p, t, 1, table=table, cursor=cur)
        res.append((o.cpu(), table.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_captured_replay_with_device_nvalid():
    """One captured call serves batches of different valid counts: nvalid and the cursor are read
    on the device at replay time."""
    from src.evaluation.metrics import image_metrics
    from src.hip import lib as L
    B, C, H, W = 3, 3, 40, 72
    p, t = _case(B, C, H, W, 1)[:2]
    pd, td = p.to(DEV), t.to(DEV)
    _, table = _table(8)
    state = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = torch.empty(3, B, device=DEV)
    work = torch.empty(L.load().fen_image_metrics_work_floats(B, C, H, W), device=DEV)
    kw = dict(table=table, cursor=state[0:1], nvalid=state[1:2], out=out, work=work)
    image_metrics(pd, td, 1.0, 1, **kw)          # warm-up: the window reaches the device
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        image_metrics(pd, td, 1.0, 1, **kw)
    table.fill_(SENTINEL)
    state[0] = 0
    state[1] = 3
    graph.replay()
    state[1:2].fill_(1)
    graph.replay()
    torch.cuda.synchronize()
    o, tab = out.cpu(), table.cpu()
    assert int(state[0]) == 4
    assert torch.equal(tab[:, :3], o[1:]) and torch.equal(tab[:, 3], o[1:, 0])
    assert bool((tab[:, 4:] == SENTINEL).all())


def test_refusals():
    from src.hip import lib as L
    from src.hip.program import ptr
    lib = L.load()
    B, C, H, W = 1, 3, 32, 32
    f = torch.zeros(B, C, H, W, device=DEV)
    win = torch.full((11,), 1 / 11, device=DEV)
    work = torch.empty(lib.fen_image_metrics_work_floats(B, C, H, W), device=DEV)
    out = torch.empty(3, B, device=DEV)
    table = torch.empty(2, 4, device=DEV)

    def call(ws=11, dr=1.0, flags=0, tab=None, cur=None):
        return lib.fen_image_metrics(B, C, H, W, ptr(f), ptr(f), ptr(win), ws, 1e-4, 9e-4, dr, flags, ptr(work),
                                     ptr(out), ptr(tab), 0 if tab is None else 4, cur, None, None)
    assert call(ws=7) == -2
    assert call(flags=2) == -1
    assert call(flags=3, dr=255.0) == -1
    assert call(flags=1, tab=table, cur=None) == -1
    assert lib.fen_image_metrics_work_floats(B, C, 0, W) == 0
    from src.evaluation import SSIM
    with pytest.raises(NotImplementedError):
        SSIM(window_size=7)(f, f)


# ---------------------------------------------------------------------- MetricCalculator
def _model():
    from src.models import FaceEnhanceNet
    torch.manual_seed(0)
    m = FaceEnhanceNet(num_channels=64, num_groups=1, blocks_per_group=1, precision="fp32")
    with torch.no_grad():
        m.conv_last.weight.normal_(0, 1e-3)
    return m.to(DEV).eval()


def _host_expectation(model, hrs):
    """Per image through the module path: SR on the host, clamped; mse / PSNR in float64, the
    oracle's SSIM, and sum |d SSIM / d SR| (how far an SR perturbation can move the SSIM)."""
    from src.training.trainer import bicubic_down4
    ps, ss, rmse, sens = [], [], [], []
    for hr in hrs:
        hr = hr[None]
        with torch.no_grad():
            sr = model(bicubic_down4(hr.to(DEV))).cpu().clamp(0, 1)
        mse, p = _psnr64(sr, hr)
        srg = sr.clone().requires_grad_(True)
        s = O.ssim(srg, hr, size_average=False)
        s.sum().backward()
        ps.append(float(p)), ss.append(float(s.detach())), rmse.append(float(mse.sqrt()))
        sens.append(float(srg.grad.abs().sum()))
    return np.array(ps), np.array(ss), np.array(rmse), np.array(sens)


def test_evaluate_dataset_and_compute_metrics():
    from torch.utils.data import DataLoader
    from src.data import SyntheticHRDataset
    from src.evaluation import MetricCalculator
    from src.training.trainer import bicubic_down4
    model = _model()
    ds = SyntheticHRDataset(5, 64, seed=3)
    hrs = [ds[i]["hr"] for i in range(5)]
    loader = DataLoader(ds, batch_size=2, shuffle=False, num_workers=0)      # 2 + 2 + 1: a partial last batch
    calc = MetricCalculator(device=DEV)
    res = calc.evaluate_dataset(model, loader)
    assert {"psnr_mean", "psnr_std", "ssim_mean", "ssim_std", "per_image", "num_images"} <= set(res)
    assert res["num_images"] == 5
    ps, ss = res["per_image"]["psnr"], res["per_image"]["ssim"]
    assert ps.shape == (5,) and ss.shape == (5,) and ps.dtype == np.float64
    eps_, essim, rmse, sens = _host_expectation(model, hrs)
    # The engine's SR is within EPS = 1e-3 (max abs, the project's fp32 module-vs-engine bound) of
    # the module's.  |d| moves by at most EPS per pixel, so rmse' <= rmse + EPS and the PSNR moves
    # by at most 20 log10(1 + EPS / rmse) <= 8.686 EPS / rmse dB: with rmse >= 0.1 on these images
    # (asserted) at most 0.087 dB, plus the kernel's PSNR_TOL.  The SSIM moves by at most
    # EPS * sum |d SSIM / d SR| to first order (x 1.1 for the rest), plus the kernel bound.
    EPS = 1e-3
    assert rmse.min() >= 0.1, rmse
    ps_tol = 20 * np.log10(1 + EPS / rmse) + PSNR_TOL
    ss_tol = 1.1 * EPS * sens + 2e-6 + 1e-5 * np.abs(essim)
    print("psnr", ps, "expected", eps_, "max diff", np.abs(ps - eps_).max(), "allowed", ps_tol.min())
    print("ssim", ss, "expected", essim, "max diff", np.abs(ss - essim).max(), "allowed", ss_tol.min())
    assert (np.abs(ps - eps_) <= ps_tol).all()
    assert (np.abs(ss - essim) <= ss_tol).all()
    assert res["psnr_mean"] == float(np.mean(ps)) and res["psnr_std"] == float(np.std(ps))
    bm = np.array([ss[0:2].mean(), ss[2:4].mean(), ss[4:5].mean()])
    assert res["ssim_mean"] == float(np.mean(bm)) and res["ssim_std"] == float(np.std(bm))
    # batches that carry 'lr' (here the same LR the kernel synthesises): the same numbers, from
    # the engine cached for this shape
    batches = [{"hr": b["hr"], "lr": bicubic_down4(b["hr"].to(DEV))} for b in loader]
    res2 = calc.evaluate_dataset(model, batches)
    assert len(calc._engines) == 1
    assert np.array_equal(res2["per_image"]["psnr"], ps) and np.array_equal(res2["per_image"]["ssim"], ss)
    assert res2["ssim_mean"] == res["ssim_mean"] and res2["num_images"] == 5
    # 8-bit quantised SR: each pixel moves by less than 1/255, and the numbers change
    res3 = calc.evaluate_dataset(model, loader, quantize=True)
    q_tol = 20 * np.log10(1 + (EPS + 1 / 255) / rmse) + PSNR_TOL
    assert (np.abs(res3["per_image"]["psnr"] - eps_) <= q_tol).all()
    assert not np.array_equal(res3["per_image"]["psnr"], ps)
    # compute_metrics on one batch: the batch-global PSNR and the batch-mean SSIM
    p, t = _case(3, 3, 40, 72, 0)[:2]
    mse, _, ssr = _case(3, 3, 40, 72, 0)[2:]
    m = calc.compute_metrics(p, t)
    assert set(m) == {"psnr", "ssim"} and all(isinstance(v, float) for v in m.values())
    assert abs(m["psnr"] - 10 * np.log10(1.0 / float(mse.mean()))) <= PSNR_TOL
    assert abs(m["ssim"] - float(ssr.double().mean())) <= 2e-6 + 1e-5 * abs(float(ssr.mean()))

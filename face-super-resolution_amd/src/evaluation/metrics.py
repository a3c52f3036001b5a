"""Evaluation metrics (reference src/evaluation/metrics.py:17-270) on the HIP path.

`psnr`, `psnr_batch`, `PSNR`, `SSIM`, `LPIPS`, `MetricCalculator` and `compute_fid` keep the
reference's names and signatures.  For GPU tensors the per-image numbers come from one
fen_image_metrics call (csrc/metrics.hip): SR and HR are read once, each 32x32 tile leaves its
SSIM-map sum and its squared-error sum, a one-block finish reduces them per image in a fixed
order to mse / PSNR / SSIM on the device.  CPU tensors take the torch formulas for PSNR; SSIM
has no CPU path (src.losses.ssim).

`MetricCalculator.evaluate_dataset` runs the model as a captured inference FENEngine and lets
the kernel append every batch's per-image PSNR / SSIM to a dataset-long device table through a
cursor and a valid count kept in device memory: nothing comes back to the host inside the
loop, the table is copied once at the end, and a partial last batch is padded to the engine's
batch with the valid count set, so it is weighted by its images.

`LPIPS(weights=PATH)` is LPIPS v0.1 with the AlexNet backbone on the HIP path (src/hip/lpips.py,
csrc/lpips.hip): per-image values on the device, the input range decided on the device, no host
wait; `MetricCalculator(lpips_weights=PATH)` records them next to PSNR / SSIM and reads them with
the same single copy.  Without `weights` LPIPS is the reference's wrapper of the `lpips` package
(`available` False and 0 when that is not installed).  FID is not built here: without
`pytorch_fid`, `compute_fid` returns -1.0.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn

from ..hip import lib as L
from ..hip.program import ptr
from ..losses.ssim import _window1d
from ..losses.ssim import ssim as compute_ssim

FLAG_CLAMP, FLAG_QUANTIZE = 1, 2      # fen_image_metrics flags (include/fen.h)

_windows: Dict[torch.device, torch.Tensor] = {}


def _window(device) -> torch.Tensor:
    w = _windows.get(device)
    if w is None:
        w = _windows[device] = _window1d(11, 1.5).to(device)
    return w


def image_metrics(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0, flags: int = 0,
                  table: Optional[torch.Tensor] = None, cursor: Optional[torch.Tensor] = None,
                  nvalid: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                  work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One fen_image_metrics call on GPU tensors [B,C,H,W] -> out fp32 [3,B] on the device:
    per-image mse, PSNR (dB, the psnr_batch formula) and mean SSIM (window 11, sigma 1.5, K =
    (0.01, 0.03)).  flags: FLAG_CLAMP clamps pred to [0, data_range], FLAG_QUANTIZE (with it,
    data_range 1) then quantises pred to 8 bits.  table fp32 [2,cap] with cursor / nvalid
    (int32 device scalars; nvalid None: all B): the dataset record described in include/fen.h.
    Nothing is synchronised or read back."""
    if not (pred.is_cuda and target.is_cuda):
        raise RuntimeError("the HIP image metrics run on ROCm GPU tensors (got CPU); there is no CPU path")
    if pred.shape != target.shape or pred.dim() != 4:
        raise ValueError(f"pred / target must be [B,C,H,W] of one shape (got {tuple(pred.shape)}, "
                         f"{tuple(target.shape)})")
    lib = L.load()
    B, C, H, W = pred.shape
    p = pred.detach().float().contiguous()
    t = target.detach().float().contiguous()
    nwork = int(lib.fen_image_metrics_work_floats(B, C, H, W))
    if work is None or work.numel() < nwork:
        work = torch.empty(max(nwork, 1), device=p.device)
    if out is None:
        out = torch.empty(3, B, device=p.device)
    cap = 0 if table is None else int(table.shape[1])
    L.check(lib.fen_image_metrics(B, C, H, W, ptr(p), ptr(t), ptr(_window(p.device)), 11,
                                  (0.01 * data_range) ** 2, (0.03 * data_range) ** 2, float(data_range), int(flags),
                                  ptr(work), ptr(out), ptr(table), cap, ptr(cursor), ptr(nvalid),
                                  torch.cuda.current_stream().cuda_stream), "image_metrics")
    return out


def _as4d(x: torch.Tensor) -> torch.Tensor:
    if x.dim() == 3:
        return x.unsqueeze(0)
    if x.dim() != 4:
        raise ValueError(f"the HIP PSNR takes [B,C,H,W] or [C,H,W] tensors (got {tuple(x.shape)})")
    return x


def psnr(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """metrics.py:17-34: the batch-global PSNR in dB, inf at zero MSE.  GPU tensors: the mean of
    the kernel's per-image mse (images of one size: the global mean), no host read."""
    if pred.is_cuda:
        mse = image_metrics(_as4d(pred), _as4d(target), data_range)[0].mean()
        return 10 * torch.log10(data_range ** 2 / mse)          # mse 0 -> inf
    mse = torch.mean((pred - target) ** 2)
    if mse == 0:
        return torch.tensor(float('inf'))
    return 10 * torch.log10(data_range ** 2 / mse)


def psnr_batch(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """metrics.py:37-52: PSNR per image [B], 10 log10(range^2 / (mse + 1e-10))."""
    if pred.is_cuda:
        return image_metrics(pred, target, data_range)[1].clone()
    mse = torch.mean((pred - target) ** 2, dim=[1, 2, 3])
    return 10 * torch.log10(data_range ** 2 / (mse + 1e-10))


class PSNR(nn.Module):
    """PSNR metric module (metrics.py:55-64)."""

    def __init__(self, data_range: float = 1.0):
        super().__init__()
        self.data_range = data_range

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return psnr(pred, target, self.data_range)


class SSIM(nn.Module):
    """SSIM metric module (metrics.py:67-78) on src.losses.ssim.ssim: GPU tensors, window 11."""

    def __init__(self, data_range: float = 1.0, window_size: int = 11):
        super().__init__()
        self.data_range = data_range
        self.window_size = window_size

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return compute_ssim(pred, target, window_size=self.window_size, data_range=self.data_range)


class LPIPS(nn.Module):
    """Learned Perceptual Image Patch Similarity (metrics.py:81-126).

    weights=None: the `lpips` package when it is installed; otherwise `available` is False and
    forward returns 0, as in the reference.  That path decides the input range with a host read
    of pred.min() per call.

    weights=PATH (a .pth state dict, src.hip.lpips.load_lpips_weights): LPIPS v0.1 on the AlexNet
    backbone through the HIP kernels, `available` True.  The range rule (pred.min() >= 0: both
    inputs become 2x - 1) is decided on the device; nothing waits for the host.  AlexNet is the
    only backbone built."""

    def __init__(self, net: str = 'alex', verbose: bool = False, weights=None):
        super().__init__()
        self.net = net
        self._hip = None
        if weights is not None:
            if net != 'alex':
                raise NotImplementedError(f"LPIPS(net={net!r}, weights=...): AlexNet (net='alex') is the only "
                                          "backbone built on the HIP path")
            from ..hip.lpips import AlexLpips, load_lpips_weights
            self._hip = AlexLpips(load_lpips_weights(weights))
            self.loss_fn = None
            self.available = True
            return
        try:
            import lpips
            self.loss_fn = lpips.LPIPS(net=net, verbose=verbose)
            self.available = True
        except ImportError:
            print("Warning: lpips not installed. LPIPS metric unavailable.")
            self.available = False
            self.loss_fn = None

    def per_image(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """LPIPS per image, [B] on pred's device (zeros when unavailable)."""
        if self._hip is not None:
            return self._hip.per_image(pred, target)
        if not self.available:
            return torch.zeros(pred.shape[0], device=pred.device)
        if pred.min() >= 0:             # [0, 1] -> [-1, 1]; a host wait
            pred = pred * 2 - 1
            target = target * 2 - 1
        return self.loss_fn(pred, target).reshape(-1)

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if self._hip is not None:
            return self._hip.per_image(pred, target).mean()
        if not self.available:
            return torch.tensor(0.0, device=pred.device)
        if pred.min() >= 0:             # [0, 1] -> [-1, 1]
            pred = pred * 2 - 1
            target = target * 2 - 1
        return self.loss_fn(pred, target).mean()


def metric_pred(sr: torch.Tensor, quantize: bool = False) -> torch.Tensor:
    """SR as fen_image_metrics sees it under FLAG_CLAMP (| FLAG_QUANTIZE): clamped to [0, 1], then
    floor(x * 255) / 255 in fp32 -- the tensor LPIPS is computed on, so all three metrics measure
    the same image."""
    sr = sr.float().clamp(0, 1)
    return torch.floor(sr * 255) / 255 if quantize else sr


class MetricCalculator:
    """Metric calculator for evaluation (metrics.py:129-224)."""

    def __init__(self, device: str = 'cuda', lpips_weights=None):
        self.device = torch.device(device if torch.cuda.is_available() else 'cpu')
        self.psnr = PSNR().to(self.device)
        self.ssim = SSIM().to(self.device)
        self.lpips = LPIPS(weights=lpips_weights).to(self.device)
        self._engines: Dict[tuple, tuple] = {}

    @torch.no_grad()
    def compute_metrics(self, pred: torch.Tensor, target: torch.Tensor) -> Dict[str, float]:
        """{'psnr': the batch-global PSNR, 'ssim': the batch-mean SSIM} (+ 'lpips' when
        available) as floats: one metrics call, one host read."""
        pred = pred.to(self.device)
        target = target.to(self.device)
        if self.device.type == 'cuda':
            o = image_metrics(_as4d(pred), _as4d(target)).cpu().double()
            mse = float(o[0].mean())
            metrics = {'psnr': float('inf') if mse == 0 else 10 * float(np.log10(1.0 / mse)),
                       'ssim': float(o[2].mean())}
        else:
            metrics = {'psnr': self.psnr(pred, target).item(), 'ssim': self.ssim(pred, target).item()}
        if self.lpips.available:
            metrics['lpips'] = self.lpips(pred, target).item()
        return metrics

    def _engine(self, model: nn.Module, B: int, H: int, W: int):
        """The captured inference engine for HR batches [B,3,H,W], built once per shape (and
        model) in the model's compute dtype; its packed weights are refreshed on every use."""
        from ..hip.engine import FENEngine
        key = (B, H, W)
        ent = self._engines.get(key)
        if ent is None or ent[0] is not model:
            s = model.scale_factor
            if H % s or W % s:
                raise ValueError(f"HR {H} x {W} is not a multiple of the scale factor {s}")
            eng = FENEngine(model, batch=B, lr_hw=(H // s, W // s), dtype=model.compute_dtype, train=False,
                            device=self.device)
            eng.capture()
            ent = self._engines[key] = (model, eng)
        else:
            ent[1].pack()
        return ent[1]

    @torch.no_grad()
    def evaluate_dataset(self, model: nn.Module, dataloader, desc: str = 'Evaluating',
                         quantize: bool = False) -> Dict[str, object]:
        """Evaluate `model` over `dataloader` (batches {'hr': [b,3,H,W]} with an optional
        'lr'; without it LR is synthesised from HR by fen_bicubic_down4, as in training).

        Per batch: a copy into the engine's input, a graph replay, one fen_image_metrics call on
        the clamped (quantize: and 8-bit quantised) SR that appends to a device table; no host
        synchronisation until the single copy of the table after the last batch.  Returns the
        reference's psnr_mean / psnr_std (over images) and ssim_mean / ssim_std (over per-batch
        means, a batch mean covering its valid images), float64 on the host, plus per_image =
        {'psnr', 'ssim'} arrays and num_images.

        With LPIPS available: lpips_mean / lpips_std over images and per_image['lpips'], computed
        on the same clamped (quantize: 8-bit) SR.  On the HIP path (lpips_weights) the per-image
        values go into the same device buffer as the PSNR / SSIM table and come back with that
        one copy: no extra host wait.  The `lpips`-package path still waits once per batch (its
        range test reads pred.min() on the host)."""
        if self.device.type != 'cuda':
            raise RuntimeError("evaluate_dataset runs the HIP inference engine: it needs a ROCm GPU")
        try:
            from tqdm import tqdm
            batches = tqdm(dataloader, desc=desc)
        except ImportError:
            batches = dataloader
        model = model.to(self.device)
        model.eval()
        lib = L.load()
        flags = FLAG_CLAMP | (FLAG_QUANTIZE if quantize else 0)
        eng = hr_buf = state = table = lp_table = out = work = None
        counts: List[int] = []
        seen = 0
        for batch in batches:
            hr = batch['hr']
            lr = batch.get('lr')
            n = int(hr.shape[0])
            if eng is None:
                B, C, H, W = (int(v) for v in hr.shape)
                eng = self._engine(model, B, H, W)
                cap = len(dataloader) * B
                hr_buf = torch.zeros(B, C, H, W, device=self.device)
                # one buffer, one copy at the end: int32 [cursor, nvalid], then the table's
                # 2 x cap floats, then cap floats of per-image LPIPS
                state = torch.zeros(2 + 3 * cap, dtype=torch.int32, device=self.device)
                table = state[2:2 + 2 * cap].view(torch.float32).view(2, cap)
                lp_table = state[2 + 2 * cap:].view(torch.float32)
                out = torch.empty(3, B, device=self.device)
                work = torch.empty(max(int(lib.fen_image_metrics_work_floats(B, C, H, W)), 1), device=self.device)
                state[1] = B
                filled = B
            if n > B or tuple(hr.shape[1:]) != (C, H, W):
                raise ValueError(f"batch {tuple(hr.shape)} does not fit the first batch's [{B},{C},{H},{W}]")
            if n < B:                       # a partial batch: zero-padded, counted by its images
                hr_buf.zero_()
                eng.x.zero_()
            hr_buf[:n].copy_(hr, non_blocking=True)
            if n != filled:
                state[1:2].fill_(n)
                filled = n
            if lr is not None:
                eng.x[:n].copy_(lr, non_blocking=True)
            else:
                L.check(lib.fen_bicubic_down4(B, C, H, W, ptr(hr_buf), ptr(eng.x),
                                              torch.cuda.current_stream().cuda_stream), "bicubic_down4")
            eng.replay()
            image_metrics(eng.out, hr_buf, 1.0, flags, table=table, cursor=state[0:1], nvalid=state[1:2], out=out,
                          work=work)
            if self.lpips.available and seen + n <= cap:
                # the host knows every batch's size, so the offset needs no device cursor
                lp_table[seen:seen + n].copy_(self.lpips.per_image(metric_pred(eng.out, quantize), hr_buf)[:n])
            seen += n
            counts.append(n)
        if eng is None:
            raise ValueError("evaluate_dataset: the dataloader yielded no batch")
        host = state.cpu()                  # the one read: waits for the stream
        eng.check_status()
        total = int(host[0])
        if total > cap:
            raise RuntimeError(f"evaluate_dataset: {total} images for a table of {cap} (len(dataloader) x the first "
                               "batch's size): the per-image record overflowed")
        tab = host[2:2 + 2 * cap].view(torch.float32).view(2, cap).numpy().astype(np.float64)
        ps, ss = tab[0, :total], tab[1, :total]
        ends = np.cumsum(counts)
        batch_ssim = np.array([ss[e - c:e].mean() for c, e in zip(counts, ends)])
        results: Dict[str, object] = {
            'psnr_mean': float(np.mean(ps)), 'psnr_std': float(np.std(ps)),
            'ssim_mean': float(np.mean(batch_ssim)), 'ssim_std': float(np.std(batch_ssim)),
            'per_image': {'psnr': ps, 'ssim': ss}, 'num_images': total,
        }
        if self.lpips.available:
            lp = host[2 + 2 * cap:].view(torch.float32).numpy().astype(np.float64)[:total]
            results['lpips_mean'] = float(np.mean(lp))
            results['lpips_std'] = float(np.std(lp))
            results['per_image']['lpips'] = lp
        return results


def compute_fid(real_images: List[np.ndarray], fake_images: List[np.ndarray], device: str = 'cuda') -> float:
    """Frechet Inception Distance (metrics.py:227-270) through the `pytorch_fid` package when it
    is installed; otherwise -1.0 with the reference's warning."""
    try:
        from pytorch_fid import fid_score
    except ImportError:
        print("Warning: pytorch_fid not installed. FID computation unavailable.")
        return -1.0
    import os
    import tempfile

    from PIL import Image
    with tempfile.TemporaryDirectory() as real_dir, tempfile.TemporaryDirectory() as fake_dir:
        for d, images in ((real_dir, real_images), (fake_dir, fake_images)):
            for i, img in enumerate(images):
                Image.fromarray(np.asarray(img, dtype=np.uint8)).save(os.path.join(d, f'{i:05d}.png'))
        return float(fid_score.calculate_fid_given_paths([real_dir, fake_dir], batch_size=50, device=device,
                                                         dims=2048))


__all__ = ["psnr", "psnr_batch", "PSNR", "SSIM", "LPIPS", "MetricCalculator", "compute_fid", "image_metrics",
           "metric_pred", "FLAG_CLAMP", "FLAG_QUANTIZE"]

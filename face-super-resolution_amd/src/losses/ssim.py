"""SSIM loss / metric (reference src/losses/ssim_loss.py:14-226) on the HIP path.

`ssim`, `create_gaussian_window` and `SSIMLoss` keep the reference's signatures.  The
computation is one fen_ssim launch (csrc/ssim.hip: separable 11-tap Gaussian passes in LDS,
the SSIM map and its per-tile sums; with a gradient, d(SSIM)/d(pred) in closed form in the
same launch) plus fixed-order column sums -- no CPU path.  Window 11 only on the kernel (the
reference's default and the configs' ssim_window_size).

`ms_ssim` and `MSSSIMLoss` keep the reference's signatures too: one fen_msssim call
(csrc/msssim.hip: the 2x2 pooling pyramid, per scale the same tiled passes with the
contrast-structure map and its gradient coefficients, a one-block finish, the pull-back of the
per-scale gradients to full resolution).  MS-SSIM is built as this module and as an engine term
(FENEngine(ms_ssim_weight=)); it is not yet selectable through CombinedLoss, which still
refuses ms_ssim_weight (0 in every stage config).
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn as nn

from ..hip import lib as L
from ..hip.program import ptr


def create_gaussian_window(window_size: int, sigma: float, channels: int) -> torch.Tensor:
    """ssim_loss.py:14-41 (the [channels,1,ws,ws] depthwise window)."""
    g = _window1d(window_size, sigma)
    w2 = g[:, None] @ g[None, :]
    return w2.expand(channels, 1, window_size, window_size).contiguous()


def _window1d(window_size: int, sigma: float) -> torch.Tensor:
    coords = torch.arange(window_size, dtype=torch.float32)
    coords -= window_size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def _check(pred, target, window_size):
    if not (pred.is_cuda and target.is_cuda):
        raise RuntimeError("the HIP SSIM runs on ROCm GPU tensors (got CPU); there is no CPU path")
    if pred.shape != target.shape or pred.dim() != 4:
        raise ValueError(f"pred / target must be [B,C,H,W] of one shape (got {tuple(pred.shape)}, "
                         f"{tuple(target.shape)})")
    if window_size != 11:
        raise NotImplementedError("the HIP SSIM kernel implements window_size=11 (the reference default)")


def _run(pred, target, window_size, sigma, data_range, K, grad_scale=None):
    """-> (per-image SSIM [B] fp32 on the device, NCHW fp32 grad_scale * d(sum S)/dpred or None)."""
    lib = L.load()
    B, C, H, W = pred.shape
    p = pred.detach().float().contiguous()
    t = target.detach().float().contiguous()
    win = _window1d(window_size, sigma).to(p.device)
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    rows = lib.fen_ssim_parts(B, C, H, W)
    part = torch.empty(rows * B, device=p.device)
    grad = torch.empty_like(p) if grad_scale is not None else None
    s = torch.cuda.current_stream().cuda_stream
    L.check(lib.fen_ssim(L.F32, B, C, H, W, ptr(p), ptr(t), ptr(win), window_size, C1, C2, ptr(part),
                         ptr(grad), 0.0 if grad_scale is None else float(grad_scale), 0 if grad is None else 1, s),
            "ssim")
    per_img = torch.empty(B, device=p.device)
    L.check(lib.fen_colsum(rows, B, ptr(part), 1.0 / (C * H * W), ptr(per_img), 0, s), "ssim colsum")
    return per_img, grad


def ssim(pred: torch.Tensor, target: torch.Tensor, window_size: int = 11, sigma: float = 1.5,
         data_range: float = 1.0, size_average: bool = True, K: Tuple[float, float] = (0.01, 0.03)) -> torch.Tensor:
    """ssim_loss.py:44-98 (a metric: no gradient flows through this function)."""
    _check(pred, target, window_size)
    per_img, _ = _run(pred, target, window_size, sigma, data_range, K)
    return per_img.mean() if size_average else per_img


class _SSIMFn(torch.autograd.Function):
    @staticmethod
    def forward(fctx, pred, target, window_size, sigma, data_range, size_average):
        B, C, H, W = pred.shape
        n = (B * C * H * W) if size_average else (C * H * W)
        per_img, grad = _run(pred, target, window_size, sigma, data_range, (0.01, 0.03),
                             grad_scale=-1.0 / n if pred.requires_grad else None)
        fctx.grad = grad
        fctx.size_average = size_average
        return 1 - (per_img.mean() if size_average else per_img)

    @staticmethod
    def backward(fctx, g):
        d = fctx.grad
        if fctx.size_average:
            d = d * g
        else:
            d = d * g.view(-1, 1, 1, 1)
        return d, None, None, None, None, None


class SSIMLoss(nn.Module):
    """1 - SSIM (ssim_loss.py:174-226); gradient w.r.t. pred in closed form on the GPU."""

    def __init__(self, window_size: int = 11, sigma: float = 1.5, data_range: float = 1.0,
                 size_average: bool = True, channel: int = 3):
        super().__init__()
        self.window_size = window_size
        self.sigma = sigma
        self.data_range = data_range
        self.size_average = size_average
        self.channel = channel
        self.register_buffer('window', create_gaussian_window(window_size, sigma, channel))

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        _check(pred, target, self.window_size)
        return _SSIMFn.apply(pred, target, self.window_size, self.sigma, self.data_range, self.size_average)


MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _ms_weights(weights, device) -> torch.Tensor:
    if weights is None:
        weights = MS_SSIM_WEIGHTS
    w = torch.as_tensor(weights, dtype=torch.float32).detach().reshape(-1).to(device).contiguous()
    if not 1 <= w.numel() <= 8:
        raise NotImplementedError(f"the HIP MS-SSIM runs 1 to 8 scales (got {w.numel()} weights)")
    return w


def _ms_run(pred, target, window_size, sigma, data_range, weights, grad_scale=None):
    """-> (out fp32 [1 + levels] on the device: MS-SSIM, then each level's batch mean (the
    contrast-structure mean M_i, the SSIM mean at the last level); NCHW fp32 grad_scale *
    d(MS-SSIM)/dpred or None).  One fen_msssim call (csrc/msssim.hip): nothing comes back to
    the host."""
    _check(pred, target, window_size)
    lib = L.load()
    B, C, H, W = pred.shape
    w = _ms_weights(weights, pred.device)
    levels = w.numel()
    if min(H, W) < 2 ** levels:
        raise ValueError(f"MS-SSIM over {levels} scales needs min(H, W) >= {2 ** levels} (got {H} x {W}): the "
                         f"reference pools once after every scale")
    p = pred.detach().float().contiguous()
    t = target.detach().float().contiguous()
    win = _window1d(window_size, sigma).to(p.device)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    work = torch.empty(lib.fen_msssim_work_floats(B, C, H, W, levels), device=p.device)
    out = torch.empty(1 + levels, device=p.device)
    grad = torch.empty_like(p) if grad_scale is not None else None
    L.check(lib.fen_msssim(L.F32, B, C, H, W, ptr(p), ptr(t), ptr(win), window_size, C1, C2, ptr(w), levels, ptr(work),
                           ptr(out), ptr(grad), 0.0 if grad_scale is None else float(grad_scale),
                           0 if grad is None else 1, torch.cuda.current_stream().cuda_stream), "msssim")
    return out, grad


def ms_ssim(pred: torch.Tensor, target: torch.Tensor, window_size: int = 11, sigma: float = 1.5,
            data_range: float = 1.0, weights=None) -> torch.Tensor:
    """ssim_loss.py:101-171 (a metric: no gradient flows through this function).  One scalar
    for the batch; len(weights) scales, the last weight unused, as in the reference."""
    out, _ = _ms_run(pred, target, window_size, sigma, data_range, weights)
    return out[0].clone()


class _MSSSIMFn(torch.autograd.Function):
    @staticmethod
    def forward(fctx, pred, target, window_size, sigma, data_range, weights):
        out, grad = _ms_run(pred, target, window_size, sigma, data_range, weights,
                            grad_scale=-1.0 if pred.requires_grad else None)
        fctx.grad = grad
        return 1 - out[0]

    @staticmethod
    def backward(fctx, g):
        return fctx.grad * g, None, None, None, None, None


class MSSSIMLoss(nn.Module):
    """1 - MS-SSIM (ssim_loss.py:229-270); gradient w.r.t. pred in closed form on the GPU, in
    the same call as the value."""

    def __init__(self, window_size: int = 11, sigma: float = 1.5, data_range: float = 1.0, weights=None):
        super().__init__()
        self.window_size = window_size
        self.sigma = sigma
        self.data_range = data_range
        if weights is None:
            weights = torch.tensor(MS_SSIM_WEIGHTS)
        self.register_buffer('weights', torch.as_tensor(weights, dtype=torch.float32))

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return _MSSSIMFn.apply(pred, target, self.window_size, self.sigma, self.data_range, self.weights)


__all__ = ["create_gaussian_window", "ssim", "ms_ssim", "SSIMLoss", "MSSSIMLoss"]

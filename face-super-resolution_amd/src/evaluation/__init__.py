"""Evaluation metrics of the reference's src/evaluation package (metrics.py) on the HIP path.
The visualisation and explainability modules are not built here."""
from .metrics import LPIPS, PSNR, SSIM, MetricCalculator, compute_fid, psnr, psnr_batch

__all__ = ["psnr", "psnr_batch", "PSNR", "SSIM", "LPIPS", "MetricCalculator", "compute_fid"]

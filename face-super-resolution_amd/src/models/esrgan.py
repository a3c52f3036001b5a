"""The ESRGAN baseline (reference src/models/esrgan.py) on the HIP path: `RRDBNet`, `RRDB`,
`ResidualDenseBlock`, `ESRGANBaseline`, `create_esrgan_baseline`.

Same constructor signatures, attribute names and state_dict (keys and OIHW fp32 shapes) as the
reference, plus a `precision=` keyword ('fp32' | 'bf16' | 'fp16') as FaceEnhanceNet has.  The
forward runs csrc/rrdb.hip through src/hip/rrdb.py: GPU tensors only, NCHW fp32 out.

Inference only.  The reference freezes every parameter of this model (esrgan.py:161-163), so no
backward is built: a backward through any of these modules raises NotImplementedError.  The
kernels are written for the published network, num_feat = 64 and num_grow_ch = 32; other widths
are refused with NotImplementedError.

Weights are never downloaded: `ESRGANBaseline` loads `weights_dir/<model_name>.pth` only.
"""
from __future__ import annotations

import warnings
from pathlib import Path
from typing import Optional, Union

import numpy as np
import torch
import torch.nn as nn

from ..hip import rrdb as R
from ..hip.autograd import Runtime
from .blocks import compute_dtype

_NO_BACKWARD = ("the ESRGAN baseline is inference-only on the HIP backend (the reference freezes its parameters): "
                "no backward is built; run it under torch.no_grad() or with frozen parameters")


class _InferenceFn(torch.autograd.Function):
    """Ties the output to the inputs that require a gradient, so a backward raises instead of
    silently treating the network as a constant."""

    @staticmethod
    def forward(ctx, run, x, *params):
        return run(x)

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError(_NO_BACKWARD)


def _check_widths(num_feat: int, num_grow_ch: int) -> None:
    if num_feat != R.FEAT or num_grow_ch != R.GROW:
        raise NotImplementedError(f"the HIP RRDB kernels implement num_feat = {R.FEAT}, num_grow_ch = {R.GROW} "
                                  f"(got {num_feat}, {num_grow_ch})")


def _check_input(x: torch.Tensor, channels: int) -> None:
    if not x.is_cuda:
        raise RuntimeError("the HIP backend runs on a ROCm GPU tensor (got a CPU tensor); there is no CPU path")
    if x.dim() != 4 or x.shape[1] != channels:
        raise ValueError(f"expected [B,{channels},H,W] (got {tuple(x.shape)})")


class _HipModule(nn.Module):
    """Shared plumbing: live packed weights (re-packed when a parameter changes, as
    FaceEnhanceNet's) and the inference-only autograd tie."""

    def _init_runtime(self, precision: str) -> None:
        self.precision = precision
        self._rt = Runtime(self, None, compute_dtype(precision))

    @property
    def compute_dtype(self) -> torch.dtype:
        return self._rt.dtype

    def _apply_inference(self, run, x: torch.Tensor) -> torch.Tensor:
        if torch.is_grad_enabled():
            params = [p for p in self.parameters() if p.requires_grad]
            if x.requires_grad or params:
                return _InferenceFn.apply(run, x, *params)
        return run(x)

    def _blocks(self, x: torch.Tensor, prefixes, outer: bool) -> torch.Tensor:
        """x [B,64,H,W] through the dense blocks `prefixes` (outer: they form one RRDB)."""
        rt = self._rt
        B, _, H, Wd = (int(v) for v in x.shape)
        W, c = rt.wt(x.device), rt.ctx(x.device)
        bufs = [c.alloc((B, H, Wd, R.STRIDE)) for _ in range(min(4, len(prefixes) + 1))]
        bufs[0][..., :R.FEAT].copy_(x.permute(0, 2, 3, 1))     # module boundary: NCHW in
        for n, pre in enumerate(prefixes):
            last = outer and n == len(prefixes) - 1
            R.dense_block(c, W, pre, bufs[n % 4], bufs[(n + 1) % 4], bufs[0] if last else None, B, H, Wd)
        return bufs[len(prefixes) % 4][..., :R.FEAT].permute(0, 3, 1, 2).float()


class ResidualDenseBlock(_HipModule):
    """Five 3x3 convs over cat(x, x1, ..), LeakyReLU(0.2) after the first four, `x5 * 0.2 + x`
    (reference esrgan.py:85-103)."""

    def __init__(self, num_feat: int = 64, num_grow_ch: int = 32, precision: str = "fp32"):
        super().__init__()
        self.num_feat, self.num_grow_ch = num_feat, num_grow_ch
        self.conv1 = nn.Conv2d(num_feat, num_grow_ch, 3, 1, 1)
        self.conv2 = nn.Conv2d(num_feat + num_grow_ch, num_grow_ch, 3, 1, 1)
        self.conv3 = nn.Conv2d(num_feat + 2 * num_grow_ch, num_grow_ch, 3, 1, 1)
        self.conv4 = nn.Conv2d(num_feat + 3 * num_grow_ch, num_grow_ch, 3, 1, 1)
        self.conv5 = nn.Conv2d(num_feat + 4 * num_grow_ch, num_feat, 3, 1, 1)
        self.lrelu = nn.LeakyReLU(negative_slope=0.2, inplace=True)
        self._init_runtime(precision)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _check_input(x, self.num_feat)
        _check_widths(self.num_feat, self.num_grow_ch)
        return self._apply_inference(lambda t: self._blocks(t, [""], outer=False), x)


class RRDB(_HipModule):
    """Three dense blocks and `out * 0.2 + x` (reference esrgan.py:69-82)."""

    def __init__(self, num_feat: int, num_grow_ch: int = 32, precision: str = "fp32"):
        super().__init__()
        self.num_feat, self.num_grow_ch = num_feat, num_grow_ch
        self.rdb1 = ResidualDenseBlock(num_feat, num_grow_ch, precision)
        self.rdb2 = ResidualDenseBlock(num_feat, num_grow_ch, precision)
        self.rdb3 = ResidualDenseBlock(num_feat, num_grow_ch, precision)
        self._init_runtime(precision)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _check_input(x, self.num_feat)
        _check_widths(self.num_feat, self.num_grow_ch)
        return self._apply_inference(lambda t: self._blocks(t, ["rdb1.", "rdb2.", "rdb3."], outer=True), x)


class RRDBNet(_HipModule):
    """conv_first -> num_block RRDBs -> conv_body (+ skip) -> 2 x (nearest x2, conv, LeakyReLU)
    -> conv_hr -> LeakyReLU -> conv_last (reference esrgan.py:17-66)."""

    def __init__(self, num_in_ch: int = 3, num_out_ch: int = 3, num_feat: int = 64, num_block: int = 23,
                 num_grow_ch: int = 32, scale: int = 4, precision: str = "fp32"):
        super().__init__()
        _check_widths(num_feat, num_grow_ch)
        if not 1 <= num_in_ch <= 8 or not 1 <= num_out_ch <= 16:
            raise NotImplementedError(f"the HIP RRDB kernels take 1..8 input and 1..16 output channels "
                                      f"(got {num_in_ch}, {num_out_ch})")
        self.scale = scale
        self.num_in_ch, self.num_out_ch, self.num_block = num_in_ch, num_out_ch, num_block
        self.conv_first = nn.Conv2d(num_in_ch, num_feat, 3, 1, 1)
        self.body = nn.Sequential(*[RRDB(num_feat, num_grow_ch, precision) for _ in range(num_block)])
        self.conv_body = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up1 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_hr = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_last = nn.Conv2d(num_feat, num_out_ch, 3, 1, 1)
        self.lrelu = nn.LeakyReLU(negative_slope=0.2, inplace=True)
        self._init_runtime(precision)

    def _run(self, x: torch.Tensor) -> torch.Tensor:
        rt = self._rt
        xc = x.detach().contiguous().float()
        return R.forward(rt.ctx(x.device), rt.wt(x.device), xc, self.num_block, self.num_out_ch)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: [B,num_in_ch,H,W] on the GPU, any H, W >= 1 -> [B,num_out_ch,4H,4W] fp32."""
        _check_input(x, self.num_in_ch)
        return self._apply_inference(self._run, x)


class ESRGANBaseline(nn.Module):
    """The comparison baseline's wrapper (reference esrgan.py:106-274): a frozen 23-block RRDBNet
    with `forward`, `inference`, `inference_batch` and `get_model_info`."""

    KNOWN_WEIGHTS = ("RealESRGAN_x4plus", "ESRGAN_x4")

    def __init__(self, model_name: str = "RealESRGAN_x4plus", scale: int = 4, device: Optional[str] = None,
                 weights_dir: str = "checkpoints/pretrained", precision: str = "fp32"):
        super().__init__()
        self.scale = scale
        self.model_name = model_name
        self.weights_dir = Path(weights_dir)
        if device is None:
            self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        else:
            self.device = torch.device(device)
        self._check_weights_present()
        self.model = RRDBNet(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=23, num_grow_ch=32, scale=scale,
                             precision=precision)
        self._load_weights()
        self.model = self.model.to(self.device)
        self.model.eval()
        for p in self.model.parameters():
            p.requires_grad = False

    @property
    def weights_path(self) -> Path:
        return self.weights_dir / f"{self.model_name}.pth"

    def _check_weights_present(self) -> None:
        """The reference downloads a known model's weights when the file is missing; this build
        never fetches anything, so that case is an error naming the expected file."""
        if not self.weights_path.exists() and self.model_name in self.KNOWN_WEIGHTS:
            raise FileNotFoundError(f"pre-trained weights for {self.model_name!r} not found at {self.weights_path}; "
                                    "no download is attempted: place the .pth file there")

    def _load_weights(self) -> None:
        path = self.weights_path
        if not path.exists():
            warnings.warn(f"no pre-trained weights found for {self.model_name!r} at {path}: using randomly "
                          "initialised weights (for testing only)")
            return
        state = torch.load(path, map_location="cpu", weights_only=True)
        for key in ("params_ema", "params"):
            if isinstance(state, dict) and key in state:
                state = state[key]
                break
        self.model.load_state_dict(state, strict=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: [B,3,H,W] in [0,1] -> [B,3,H*scale,W*scale]."""
        return self.model(x)

    @torch.no_grad()
    def inference(self, lr_image: Union[np.ndarray, torch.Tensor], return_numpy: bool = True):
        """One image: (H,W,3) uint8 / float array, or a (3,H,W) / (1,3,H,W) tensor (uint8 tensors
        in either HWC or CHW layout are scaled by 1/255) -> clamped SR, (4H,4W,3) uint8 numpy
        `(x * 255).astype(uint8)` or, return_numpy=False, a (3,4H,4W) tensor."""
        if isinstance(lr_image, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(lr_image))
            hwc = True
        else:
            t = lr_image
            hwc = t.dim() == 3 and t.shape[-1] == 3 and t.shape[0] != 3
        if t.dtype == torch.uint8:
            t = t.float() / 255.0
        if hwc:
            t = t.permute(2, 0, 1)
        if t.dim() == 3:
            t = t.unsqueeze(0)
        sr = torch.clamp(self.forward(t.to(self.device).float()), 0, 1)
        if not return_numpy:
            return sr.squeeze(0)
        img = sr.squeeze(0).cpu().numpy().transpose(1, 2, 0)
        return (img * 255).astype(np.uint8)

    @torch.no_grad()
    def inference_batch(self, lr_batch: torch.Tensor) -> torch.Tensor:
        """[B,3,H,W] in [0,1] -> clamped [B,3,H*scale,W*scale]."""
        return torch.clamp(self.forward(lr_batch.to(self.device)), 0, 1)

    def get_model_info(self) -> dict:
        total = sum(p.numel() for p in self.model.parameters())
        trainable = sum(p.numel() for p in self.model.parameters() if p.requires_grad)
        return {
            "name": self.model_name,
            "scale": self.scale,
            "total_params": total,
            "trainable_params": trainable,
            "size_mb": total * 4 / (1024 ** 2),
            "device": str(self.device),
        }


def create_esrgan_baseline(device: Optional[str] = None, weights_dir: str = "checkpoints/pretrained",
                           precision: str = "fp32") -> ESRGANBaseline:
    """Factory (reference esrgan.py:277-294): the RealESRGAN_x4plus baseline."""
    return ESRGANBaseline(model_name="RealESRGAN_x4plus", scale=4, device=device, weights_dir=weights_dir,
                          precision=precision)

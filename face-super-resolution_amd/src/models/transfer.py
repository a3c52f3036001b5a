"""The transfer model (reference src/models/transfer.py) on the HIP path: `TrainingStage`,
`TransferModelConfig`, `FaceSpecificHead`, `TransferSRModel`, `create_transfer_model`.

A 16-block RRDB backbone (ESRGAN's feature extractor: conv_first, the RRDBs, conv_body + skip)
followed by a face-specific head: 4 RCABs, conv_after + skip, the PixelShuffle upsampler and
conv_last (no bicubic skip, no clamp).  Same constructor signatures, attribute names, construction
order and state_dict (keys and OIHW fp32 shapes) as the reference, so a seeded model is
bit-identical to it -- the upsampler keeps its ICNR init here, nothing re-initialises it -- plus a
`precision=` keyword ('fp32' | 'bf16' | 'fp16') as the other models have.

The forward runs src/hip/transfer.py: GPU tensors only, NCHW fp32 out.  Training: stage 1 (head
only) trains through autograd -- the backbone runs its inference kernels and saves nothing, the
head's backward fills every `face_head.*` gradient.  Stages 2 and 3 unfreeze backbone blocks.  A model
built with `train_backbone=True` trains them: the forward keeps one 192-channel buffer per dense
block from the first trainable RRDB on (rrdb.trunk(save_from=...)) and the backward runs the dense
blocks' data and weight gradients (rrdb.trunk_backward).  It is opt-in: without the keyword the
flags, parameter groups and forward of stages 2 and 3 work as before and a backward that reaches a
backbone parameter raises NotImplementedError.  fp16 is inference-only.

The kernels are written for the published widths (64 features, 32 growth channels) and power-of-
two scales; anything else is refused.  Pre-trained weights are read from a local path only.
"""
from __future__ import annotations

from dataclasses import dataclass
from enum import Enum
from typing import Any, Dict, List, Optional

import torch
import torch.nn as nn

from ..hip import lib as L
from ..hip import rrdb as R
from ..hip import transfer as T
from ..hip.autograd import LiveWeights, Runtime, _check_grad, as_nchw, to_nhwc
from .blocks import RCAB, UpsampleModule, compute_dtype
from .esrgan import RRDB, _check_input

_NO_RRDB_BACKWARD = ("the RRDB backward (data and weight gradients of the dense blocks) is not implemented on the "
                     "HIP backend: stage 1 (STAGE1_HEAD_ONLY) trains; stages 2 and 3 need that backward for the "
                     "unfrozen backbone parameters, and the LR input takes no gradient either")


class TrainingStage(Enum):
    """Progressive unfreezing (reference transfer.py:17-21)."""
    STAGE1_HEAD_ONLY = 1
    STAGE2_PARTIAL_FINETUNE = 2
    STAGE3_FULL_FINETUNE = 3


@dataclass
class TransferModelConfig:
    """Reference transfer.py:24-42, field for field."""
    backbone_blocks: int = 16
    freeze_blocks: int = 16
    head_blocks: int = 4
    head_channels: int = 64
    scale_factor: int = 4
    stage1_lr: float = 2e-4
    stage2_lr: float = 2e-5
    stage3_lr: float = 1e-5


def _check_config(channels: int, scale: int) -> None:
    if channels != R.FEAT:
        raise NotImplementedError(f"the HIP RRDB kernels and the head's strip kernels implement {R.FEAT} channels "
                                  f"(got {channels})")
    if scale < 1 or scale & (scale - 1):
        raise NotImplementedError(f"the upsampler is built from x2 stages: scale_factor must be a power of two "
                                  f"(got {scale})")


class _BackboneTie(torch.autograd.Function):
    """Ties the backbone's output to whatever of its inputs requires a gradient, so that a backward
    reaching them raises instead of silently treating the backbone as a constant."""

    @staticmethod
    def forward(ctx, run, x, *params):
        return run(x)

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError(_NO_RRDB_BACKWARD)


class _BackboneFn(torch.autograd.Function):
    """The backbone with RRDBs `first`.. and conv_body trainable (train_backbone=True): x NCHW fp32
    -> feat [B,64,H,W] (a view of the NHWC buffer); backward fills the gradients of `names`, the
    backbone parameters that require one, in order."""

    @staticmethod
    def forward(ctx, x, rt: Runtime, num_block: int, first: int, names, *params):
        L.check_strip_status()
        xc = x.detach().contiguous().float()
        feat, saved = R.trunk(rt.ctx(x.device), rt.wt(x.device), xc, num_block, save_from=first)
        ctx.rt, ctx.saved, ctx.names = rt, saved, names
        return as_nchw(feat)

    @staticmethod
    def backward(ctx, dfeat):
        _check_grad(ctx.rt)
        rt, saved = ctx.rt, ctx.saved
        if saved is None:
            raise RuntimeError("the backbone's saved buffers were released by an earlier backward")
        params = dict(rt.module.named_parameters())
        keys = ["conv_body.weight", "conv_body.bias"]
        for i in range(saved["first"], saved["num_block"]):
            keys += [f"body.{i}.rdb{j}.conv{k}.{t}" for j in (1, 2, 3) for k in (1, 2, 3, 4, 5) for t in ("weight", "bias")]
        G = {k: torch.empty_like(params[k], dtype=torch.float32) for k in keys}
        R.trunk_backward(rt.ctx(dfeat.device), rt.wt(dfeat.device), G, saved, to_nhwc(dfeat, rt.dtype))
        ctx.saved = None
        return (None, None, None, None, None) + tuple(G[k] for k in ctx.names)


class _HeadFn(torch.autograd.Function):
    """FaceSpecificHead over its own parameters: feat [B,C,H,W] (channels_last storage is free)
    -> NCHW fp32 [B,3,sH,sW]."""

    @staticmethod
    def forward(ctx, feat, rt: Runtime, *params):
        L.check_strip_status()
        fh = to_nhwc(feat, rt.dtype)
        out, sv = T.head(rt.spec, rt.ctx(feat.device), rt.wt(feat.device), fh, save=rt.grad_mode)
        ctx.rt, ctx.sv = rt, sv
        return out

    @staticmethod
    def backward(ctx, dout):
        _check_grad(ctx.rt)
        L.check_strip_status()
        rt, sv = ctx.rt, ctx.sv
        named = list(rt.module.named_parameters())
        G = {T.head_key(k): torch.empty_like(p) for k, p in named}
        dx = T.head_backward(rt.spec, rt.ctx(dout.device), rt.wt(dout.device), G, sv, dout)
        ctx.sv = None
        return (as_nchw(dx) if ctx.needs_input_grad[0] else None, None) + tuple(G[T.head_key(k)] for k, _ in named)


class _HeadRuntime(Runtime):
    """Runtime exposing a FaceSpecificHead's parameters under the group / tail builders' keys."""

    def wt(self, device):
        if self.weights is None or self.weights.device != device:
            self.weights = LiveWeights({T.head_key(k): v for k, v in self.module.named_parameters()},
                                       self.dtype, device)
        self.weights.refresh()
        return self.weights


class FaceSpecificHead(nn.Module):
    """num_blocks RCABs -> conv_after (+ the head's input) -> UpsampleModule -> conv_last
    (reference transfer.py:45-91)."""

    def __init__(self, in_channels: int = 64, num_blocks: int = 4, scale_factor: int = 4, precision: str = "fp32"):
        super().__init__()
        _check_config(in_channels, scale_factor)
        self.rcab_blocks = nn.ModuleList([RCAB(num_channels=in_channels, reduction_ratio=4, precision=precision)
                                          for _ in range(num_blocks)])
        self.conv_after = nn.Conv2d(in_channels, in_channels, 3, 1, 1)
        self.upsample = UpsampleModule(in_channels, scale_factor, precision=precision)
        self.conv_last = nn.Conv2d(in_channels, 3, 3, 1, 1)
        self._rt = _HeadRuntime(self, T.head_spec(in_channels, num_blocks, scale_factor), compute_dtype(precision))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _check_input(x, self.conv_after.in_channels)
        params = [p for _, p in self.named_parameters()]
        self._rt.grad_mode = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        return _HeadFn.apply(x, self._rt, *params)


class TransferSRModel(nn.Module):
    """The frozen-then-unfrozen RRDB backbone and the trainable face head (reference
    transfer.py:94-320)."""

    def __init__(self, config: Optional[TransferModelConfig] = None, pretrained_path: Optional[str] = None,
                 precision: str = "fp32", train_backbone: bool = False):
        super().__init__()
        self.config = TransferModelConfig() if config is None else config
        self.precision = precision
        # opt-in: stages 2 and 3 train through the RRDB backward; off, they refuse (_BackboneTie)
        self.train_backbone = bool(train_backbone)
        _check_config(self.config.head_channels, self.config.scale_factor)
        self.backbone = self._create_backbone()
        self.face_head = FaceSpecificHead(in_channels=self.config.head_channels, num_blocks=self.config.head_blocks,
                                          scale_factor=self.config.scale_factor, precision=precision)
        self._rt = Runtime(self.backbone, None, compute_dtype(precision))
        if pretrained_path:
            self._load_pretrained(pretrained_path)
        self.current_stage = TrainingStage.STAGE1_HEAD_ONLY
        self._update_frozen_layers()

    @property
    def compute_dtype(self) -> torch.dtype:
        return self._rt.dtype

    def _create_backbone(self) -> nn.Module:
        """conv_first, the RRDBs and conv_body, created in this order (the RNG order of the reference)."""
        ch = self.config.head_channels
        first = nn.Conv2d(3, ch, 3, 1, 1)
        body = nn.ModuleList([RRDB(ch, num_grow_ch=R.GROW, precision=self.precision)
                              for _ in range(self.config.backbone_blocks)])
        after = nn.Conv2d(ch, ch, 3, 1, 1)
        return nn.ModuleDict({"conv_first": first, "body": body, "conv_body": after})

    def _load_pretrained(self, path: str) -> None:
        """An RRDBNet state dict (plain, or under 'params_ema' / 'params') -> the backbone: conv_first,
        conv_body and the first backbone_blocks body blocks; the rest (conv_up*, conv_hr, conv_last,
        later blocks) is dropped.  A local file, tensors only (weights_only=True)."""
        state = torch.load(path, map_location="cpu", weights_only=True)
        for wrap in ("params_ema", "params"):
            if isinstance(state, dict) and wrap in state:
                state = state[wrap]
                break
        picked = {}
        for key, value in state.items():
            if key.startswith("conv_first"):
                picked["conv_first." + key.rsplit(".", 1)[-1]] = value
            elif key.startswith("conv_body"):
                picked["conv_body." + key.rsplit(".", 1)[-1]] = value
            elif key.startswith("body."):
                if int(key.split(".")[1]) < self.config.backbone_blocks:
                    picked[key] = value
        self.backbone.load_state_dict(picked, strict=False)
        print(f"Loaded pre-trained weights from {path}")

    # ---- stages -------------------------------------------------------------------------------
    def set_training_stage(self, stage: TrainingStage) -> None:
        self.current_stage = stage
        self._update_frozen_layers()
        print(f"Training stage set to: {stage.name}")

    def _update_frozen_layers(self) -> None:
        n = self.config.backbone_blocks
        if self.current_stage == TrainingStage.STAGE1_HEAD_ONLY:
            self._freeze_backbone(0, n)
        elif self.current_stage == TrainingStage.STAGE2_PARTIAL_FINETUNE:
            self._freeze_backbone(0, n - 4)
            self._unfreeze_backbone(n - 4, n)
        elif self.current_stage == TrainingStage.STAGE3_FULL_FINETUNE:
            self._unfreeze_backbone(0, n)
        self._unfreeze_head()

    def _set_blocks(self, start: int, end: int, flag: bool) -> None:
        body = self.backbone["body"]
        for i in range(start, min(end, len(body))):
            body[i].requires_grad_(flag)
        # conv_body follows the last blocks
        if end >= self.config.backbone_blocks:
            self.backbone["conv_body"].requires_grad_(flag)

    def _freeze_backbone(self, start: int, end: int) -> None:
        # the reference's quirk, kept: every freeze also freezes conv_first, and no unfreeze ever
        # touches it, so conv_first stays frozen from stage 1 on
        self.backbone["conv_first"].requires_grad_(False)
        self._set_blocks(start, end, False)

    def _unfreeze_backbone(self, start: int, end: int) -> None:
        self._set_blocks(start, end, True)

    def _unfreeze_head(self) -> None:
        self.face_head.requires_grad_(True)

    # ---- forward ------------------------------------------------------------------------------
    def _run_backbone(self, x: torch.Tensor) -> torch.Tensor:
        rt = self._rt
        xc = x.detach().contiguous().float()
        feat = T.backbone(rt.ctx(x.device), rt.wt(x.device), xc, self.config.backbone_blocks)
        return as_nchw(feat)              # a view: the head reads the NHWC buffer as it is

    def _run_backbone_saving(self, x: torch.Tensor) -> torch.Tensor:
        """The training forward of stages 2 and 3 (train_backbone=True): the saved range starts at the
        first RRDB with a trainable parameter, read from the flags at every forward."""
        if x.requires_grad:
            raise NotImplementedError("gradient w.r.t. the LR input image is not provided by the HIP backend")
        if any(p.requires_grad for p in self.backbone["conv_first"].parameters()):
            raise NotImplementedError("conv_first is frozen in every training stage (reference transfer.py); its "
                                      "weight gradient is not built on the HIP backend")
        named = [(k, p) for k, p in self.backbone.named_parameters() if p.requires_grad]
        n = self.config.backbone_blocks
        first = min([int(k.split(".")[1]) for k, _ in named if k.startswith("body.")], default=n)
        return _BackboneFn.apply(x, self._rt, n, first, tuple(k for k, _ in named), *(p for _, p in named))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: LR [B,3,H,W] on the GPU, any H, W >= 1 -> SR [B,3,H*scale,W*scale] fp32."""
        _check_input(x, 3)
        if not torch.is_grad_enabled():           # inference: backbone and head over one Ctx
            head = self.face_head._rt
            xc = x.detach().contiguous().float()
            return T.forward(head.spec, head.ctx(x.device), self._rt.wt(x.device), head.wt(x.device), xc,
                             self.config.backbone_blocks)
        tied = [p for p in self.backbone.parameters() if p.requires_grad]
        if self.train_backbone and tied:
            feat = self._run_backbone_saving(x)
        elif x.requires_grad or tied:
            feat = _BackboneTie.apply(self._run_backbone, x, *tied)
        else:
            feat = self._run_backbone(x)
        return self.face_head(feat)

    # ---- optimizer groups / info ----------------------------------------------------------------
    def get_trainable_params(self) -> List[Dict[str, Any]]:
        """Parameter groups with the stage's learning rates (reference transfer.py:271-304):
        head / backbone = stage1_lr / -, stage2_lr / 0.1 stage2_lr, stage3_lr / stage3_lr."""
        groups: Dict[bool, list] = {False: [], True: []}
        for name, p in self.named_parameters():
            if p.requires_grad:
                groups["face_head" in name].append(p)
        cfg = self.config
        head_lr, backbone_lr = {
            TrainingStage.STAGE1_HEAD_ONLY: (cfg.stage1_lr, 0),
            TrainingStage.STAGE2_PARTIAL_FINETUNE: (cfg.stage2_lr, cfg.stage2_lr * 0.1),
            TrainingStage.STAGE3_FULL_FINETUNE: (cfg.stage3_lr, cfg.stage3_lr),
        }[self.current_stage]
        out = []
        if groups[False]:
            out.append({"params": groups[False], "lr": backbone_lr})
        if groups[True]:
            out.append({"params": groups[True], "lr": head_lr})
        return out

    def get_model_info(self) -> Dict[str, Any]:
        total = sum(p.numel() for p in self.parameters())
        trainable = sum(p.numel() for p in self.parameters() if p.requires_grad)
        return {
            "name": "TransferSRModel",
            "total_params": total,
            "trainable_params": trainable,
            "size_mb": total * 4 / (1024 ** 2),
            "backbone_blocks": self.config.backbone_blocks,
            "head_blocks": self.config.head_blocks,
            "current_stage": self.current_stage.name,
            "frozen_params": total - trainable,
        }


def create_transfer_model(pretrained_path: Optional[str] = None, precision: str = "fp32", train_backbone: bool = False,
                          **kwargs) -> TransferSRModel:
    """Factory (reference transfer.py:323-338): kwargs override TransferModelConfig fields."""
    return TransferSRModel(TransferModelConfig(**kwargs), pretrained_path, precision=precision,
                           train_backbone=train_backbone)

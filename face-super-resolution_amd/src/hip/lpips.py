"""LPIPS v0.1 with the AlexNet backbone on the HIP path (csrc/lpips.hip): forward only, fp32, one
value per image, no host synchronisation.

`load_lpips_weights` reads one .pth state dict (weights_only, nothing is ever downloaded) into
the canonical names conv{0..4}.weight / conv{0..4}.bias / lin{0..4}.  `AlexLpips` owns the packed
filters and, per (B, H, W), the recorded launch sequence with its activations and workspace:
prep (range flag + scaling layer, SR and HR stacked into one NHWC-4 batch of 2B so every filter
read serves both), 5 convs, 2 pools, 5 heads, finish.  `per_image(pred, target)` replays it on
the current stream and returns a [B] device tensor.  The first call for a device packs the filters
and the first call for a shape allocates its buffers; the pack stream is synchronised once, so
later calls may run on any stream.  After one eager call of the same shape `per_image` is
capturable in a hipGraph; a first call inside a capture raises instead of capturing the set-up.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Tuple

import torch

from . import lib as L
from .program import current_stream_handle, ptr

# AlexNet `features` (torchvision geometry): (index in features, Cin, Cout, kernel, stride, pad)
ALEX_CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1),
              (10, 256, 256, 3, 1, 1))
MIN_SIZE = 31       # the smallest H, W for which every feature map is non-empty


def _conv_out(n: int, k: int, s: int, p: int) -> int:
    return (n + 2 * p - k) // s + 1


def tap_sizes(H: int, W: int) -> List[Tuple[int, int]]:
    """(h, w) of the five taps (the ReLU outputs) for an H x W input; floor division throughout."""
    h1, w1 = _conv_out(H, 11, 4, 2), _conv_out(W, 11, 4, 2)
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    h3, w3 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    return [(h1, w1), (h2, w2), (h3, w3), (h3, w3), (h3, w3)]


def load_lpips_weights(source) -> Dict[str, torch.Tensor]:
    """A .pth path (loaded with weights_only=True) or a state dict -> {conv{k}.weight [Cout,Cin,
    kh,kw], conv{k}.bias [Cout], lin{k} [C]} as fp32 CPU tensors, k = 0..4.

    Accepted spellings for the convs: torchvision's `features.{0,3,6,8,10}.{weight,bias}`, and the
    `lpips` module's `net.slice1.0.*`, `net.slice2.3.*`, `net.slice3.6.*`, `net.slice4.8.*`,
    `net.slice5.10.*`.  The linear layers are `lin{0..4}.model.1.weight` of shape [1,C,1,1].
    `scaling_layer.*` buffers and any other key are ignored.  The `lpips` spellings are written
    from memory: that package was not available when this loader was written, so nobody has
    checked them against a real lpips checkpoint yet.

    A missing key is a KeyError, a wrong shape a ValueError; both name the key."""
    if isinstance(source, dict):
        sd = source
    else:
        sd = torch.load(source, map_location="cpu", weights_only=True)
        if not isinstance(sd, dict):
            raise ValueError(f"LPIPS weights {source}: expected a state dict, got {type(sd).__name__}")
    out: Dict[str, torch.Tensor] = {}
    for k, (idx, cin, cout, ks, _, _) in enumerate(ALEX_CONVS):
        for part, shape in (("weight", (cout, cin, ks, ks)), ("bias", (cout,))):
            names = (f"features.{idx}.{part}", f"net.slice{k + 1}.{idx}.{part}")
            found = [n for n in names if n in sd]
            if not found:
                raise KeyError(f"LPIPS weights: neither '{names[0]}' nor '{names[1]}' in the state dict")
            t = sd[found[0]]
            if tuple(t.shape) != shape:
                raise ValueError(f"LPIPS weights: '{found[0]}' has shape {tuple(t.shape)}, expected {shape}")
            out[f"conv{k}.{part}"] = t.detach().float().cpu().contiguous()
        name = f"lin{k}.model.1.weight"
        if name not in sd:
            raise KeyError(f"LPIPS weights: '{name}' not in the state dict")
        t = sd[name]
        if tuple(t.shape) != (1, cout, 1, 1):
            raise ValueError(f"LPIPS weights: '{name}' has shape {tuple(t.shape)}, expected {(1, cout, 1, 1)}")
        out[f"lin{k}"] = t.detach().float().cpu().reshape(cout).contiguous()
    return out


class _Plan:
    """The recorded sequence of one (B, H, W): launches as (name, fn, args) with the stream
    appended at run time, and every buffer they touch."""

    def __init__(self):
        self.ops: List[Tuple[str, Callable, tuple]] = []
        self.hold: List[torch.Tensor] = []
        self.pred = self.target = self.out = None


class AlexLpips:
    def __init__(self, weights: Dict[str, torch.Tensor]):
        self.weights = weights
        self.lib = L.load()
        self._packed: Dict[torch.device, dict] = {}
        self._plans: Dict[tuple, _Plan] = {}

    def _pack(self, device) -> dict:
        """The filters packed to [K][Cout] (conv1 with Cin 3 -> 4), biases and lin vectors on
        `device`, once.  The stream the pack kernels ran on is synchronised before the entry is
        cached: a later call on another stream finds them finished, and the unpacked device
        copies can go."""
        ent = self._packed.get(device)
        if ent is None:
            self._no_capture("pack its filters")
            ent, srcs = {}, []
            s = current_stream_handle()
            for k, (_, cin, cout, ks, _, _) in enumerate(ALEX_CONVS):
                cpad = (cin + 3) // 4 * 4
                w = self.weights[f"conv{k}.weight"].to(device)
                wp = torch.empty(ks * ks * cpad, cout, device=device)
                L.check(self.lib.fen_conv2d_f32_pack(cout, cin, ks, ks, cpad, ptr(w), ptr(wp), s), "conv2d_f32_pack")
                ent[f"w{k}"], ent[f"b{k}"] = wp, self.weights[f"conv{k}.bias"].to(device)
                ent[f"lin{k}"] = self.weights[f"lin{k}"].to(device)
                srcs.append(w)              # alive until the pack kernels have run
            torch.cuda.current_stream().synchronize()       # once per device, never per call
            del srcs
            self._packed[device] = ent
        return ent

    @staticmethod
    def _no_capture(what: str) -> None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"AlexLpips: the first call has to {what}; call per_image once eagerly with this "
                               "shape before capturing it in a graph")

    def _plan(self, B: int, H: int, W: int, device) -> _Plan:
        key = (B, H, W, device)
        plan = self._plans.get(key)
        if plan is not None:
            return plan
        self._no_capture("allocate the buffers of this shape")
        lib = self.lib
        nwork = int(lib.fen_lpips_work_floats(B, H, W))
        if nwork == 0:
            raise L.FenError(f"LPIPS (AlexNet) takes images of at least {MIN_SIZE} x {MIN_SIZE} (got B={B}, {H} x {W})")
        pk = self._pack(device)
        plan = _Plan()
        N = 2 * B

        def buf(*shape):
            t = torch.empty(shape, device=device)
            plan.hold.append(t)
            return t
        plan.pred, plan.target = buf(B, 3, H, W), buf(B, 3, H, W)
        work, plan.out = buf(nwork), buf(B)
        x = buf(N, H, W, 4)
        plan.ops.append(("lpips_prep", lib.fen_lpips_prep,
                         (B, H, W, ptr(plan.pred), ptr(plan.target), ptr(work), nwork, ptr(x))))
        h, w, c = H, W, 4
        for k, (_, _, cout, ks, stride, pad) in enumerate(ALEX_CONVS):
            if k in (1, 2):         # the pools sit before conv 2 and conv 3
                ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
                y = buf(N, ho, wo, c)
                plan.ops.append(("maxpool3s2_f32", lib.fen_maxpool3s2_f32, (N, h, w, c, ptr(x), ptr(y))))
                x, h, w = y, ho, wo
            ho, wo = _conv_out(h, ks, stride, pad), _conv_out(w, ks, stride, pad)
            y = buf(N, ho, wo, cout)
            plan.ops.append(("conv2d_f32", lib.fen_conv2d_f32,
                             (N, h, w, c, cout, ks, ks, stride, pad, ptr(x), ptr(pk[f"w{k}"]), ptr(pk[f"b{k}"]), 1,
                              ptr(y))))
            plan.ops.append(("lpips_head", lib.fen_lpips_head, (B, H, W, k, ptr(y), ptr(pk[f"lin{k}"]), ptr(work), nwork)))
            x, h, w, c = y, ho, wo, cout
        plan.ops.append(("lpips_finish", lib.fen_lpips_finish, (B, H, W, ptr(work), nwork, ptr(plan.out))))
        self._plans[key] = plan
        return plan

    @torch.no_grad()
    def per_image(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """pred, target [B,3,H,W] GPU tensors -> LPIPS per image, a new fp32 [B] device tensor.
        Nothing is synchronised or read back."""
        if not (pred.is_cuda and target.is_cuda):
            raise RuntimeError("the HIP LPIPS runs on ROCm GPU tensors (got CPU); there is no CPU path")
        if pred.shape != target.shape or pred.dim() != 4 or pred.shape[1] != 3:
            raise ValueError(f"pred / target must be [B,3,H,W] of one shape (got {tuple(pred.shape)}, "
                             f"{tuple(target.shape)})")
        B, _, H, W = (int(v) for v in pred.shape)
        plan = self._plan(B, H, W, pred.device)
        plan.pred.copy_(pred)
        plan.target.copy_(target)
        s = current_stream_handle()
        for name, fn, args in plan.ops:
            L.check(fn(*args, s), name)
        return plan.out.clone()

"""Plain-torch restatement of the transfer model (TransferSRModel), the checker of the HIP path at
the shapes the golden vectors (tests/golden/g13_*.npz) do not cover.  Test infrastructure only: it
runs on the CPU and the package never imports it.

The network: the RRDB backbone of rrdb_ref (conv_first 3->64, num_block RRDBs, conv_body and
`feat + body`), then the head: num_head RCABs -- conv 3x3, PReLU(64), conv 3x3, a squeeze-and-
excitation gate (mean over pixels, Linear 64->16 without bias, ReLU, Linear 16->64 without bias,
sigmoid), `gated * 0.2 + x` --, conv_after and `+ head input`, log2(scale) stages of conv 64->256,
PixelShuffle(2), PReLU(64), and conv_last 64->3.  No global skip, no clamp.

`store` is applied to every tensor the HIP path writes to memory in its compute dtype (the
backbone's as in rrdb_ref; in the head PReLU(conv1), conv2's output, each RCAB's output, the
group output and each upsampler stage), which makes forward() the 16-bit path's CPU replay:
`replay(net, x, dtype)` rounds the 3x3 conv weights to dtype (not conv_first's, no bias, no PReLU
slope, no gate weight: the HIP path keeps those in fp32), runs in float64 and rounds every stored
activation.  `replay_grads` does the same for the stage-1 gradients of mean|out - hr|: the
rounding points also round the gradient that flows back through them, as the HIP backward stores
its activation gradients in the compute dtype.
"""
import copy
import glob
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rrdb_ref  # noqa: E402

RES_SCALE = 0.2


def _same(t):
    return t


class RefRCAB(nn.Module):
    def __init__(self, ch=64, reduction=4):
        super().__init__()
        self.conv1 = nn.Conv2d(ch, ch, 3, 1, 1)
        self.prelu = nn.PReLU(ch)
        self.conv2 = nn.Conv2d(ch, ch, 3, 1, 1)
        cr = max(ch // reduction, 8)
        self.channel_attention = nn.Module()
        self.channel_attention.fc = nn.Sequential(nn.Linear(ch, cr, bias=False), nn.ReLU(), nn.Linear(cr, ch, bias=False),
                                                  nn.Sigmoid())

    def forward(self, x, store=_same):
        t = store(self.conv2(store(self.prelu(self.conv1(x)))))
        gate = self.channel_attention.fc(t.mean(dim=(2, 3)))
        return store(t * gate[:, :, None, None] * RES_SCALE + x)


class RefStage(nn.Module):
    def __init__(self, ch=64):
        super().__init__()
        self.conv = nn.Conv2d(ch, 4 * ch, 3, 1, 1)
        self.prelu = nn.PReLU(ch)

    def forward(self, x, store=_same):
        return store(self.prelu(F.pixel_shuffle(self.conv(x), 2)))


class RefHead(nn.Module):
    def __init__(self, ch=64, num_blocks=4, scale=4):
        super().__init__()
        self.rcab_blocks = nn.ModuleList([RefRCAB(ch) for _ in range(num_blocks)])
        self.conv_after = nn.Conv2d(ch, ch, 3, 1, 1)
        self.upsample = nn.Module()
        self.upsample.stages = nn.Sequential(*[RefStage(ch) for _ in range(scale.bit_length() - 1)])
        self.conv_last = nn.Conv2d(ch, 3, 3, 1, 1)

    def forward(self, x, store=_same):
        t = x
        for blk in self.rcab_blocks:
            t = blk(t, store)
        t = store(self.conv_after(t) + x)
        for st in self.upsample.stages:
            t = st(t, store)
        return self.conv_last(t)


class RefTransfer(nn.Module):
    def __init__(self, backbone_blocks=16, head_blocks=4, scale=4):
        super().__init__()
        self.backbone = nn.ModuleDict({
            "conv_first": nn.Conv2d(3, 64, 3, 1, 1),
            "body": nn.ModuleList([rrdb_ref.RefRRDB() for _ in range(backbone_blocks)]),
            "conv_body": nn.Conv2d(64, 64, 3, 1, 1),
        })
        self.face_head = RefHead(64, head_blocks, scale)

    def features(self, x, store=_same):
        feat = store(self.backbone["conv_first"](x))
        t = feat
        for blk in self.backbone["body"]:
            t = blk(t, store)
        return store(feat + self.backbone["conv_body"](t))

    def forward(self, x, store=_same):
        return self.face_head(self.features(x, store), store)


def from_state_dict(sd, backbone_blocks, head_blocks, scale=4):
    net = RefTransfer(backbone_blocks, head_blocks, scale).eval()
    net.load_state_dict({k: torch.as_tensor(v).float() for k, v in sd.items()})
    return net


def load_g13(golden):
    """Every array of tests/golden/g13_transfer_*.npz in one dict (golden: conftest's loader)."""
    g = {}
    here = os.path.dirname(os.path.abspath(__file__))
    for path in sorted(glob.glob(os.path.join(here, "golden", "g13_transfer_*.npz"))):
        g.update(golden(os.path.basename(path)))
    return g


def golden_state_dict(g):
    """The fp16 parameters of the g13 files as an fp32 state_dict."""
    return {k[2:]: torch.from_numpy(v.astype("float32")) for k, v in g.items() if k.startswith("w/")}


def _is_conv3x3_weight(key, p):
    return key.endswith(".weight") and p.dim() == 4 and not key.startswith("backbone.conv_first.")


def _rounded_double(net, dtype):
    n = copy.deepcopy(net).double()
    with torch.no_grad():
        for k, p in n.named_parameters():
            if _is_conv3x3_weight(k, p):
                p.copy_(p.float().to(dtype).double())
    return n


@torch.no_grad()
def replay(net, x, dtype, features=False):
    """The 16-bit HIP path on the CPU (module docstring) -> fp32 output (or the head's input)."""
    n = _rounded_double(net, dtype)

    def store(t):
        return t.float().to(dtype).double()
    return (n.features(x.double(), store) if features else n(x.double(), store)).float()


class _RoundBoth(torch.autograd.Function):
    """Rounds the value going forward and the gradient going back (rnd: forward too or not)."""

    @staticmethod
    def forward(ctx, t, dtype, fwd):
        ctx.dtype = dtype
        return t.float().to(dtype).double() if fwd else t

    @staticmethod
    def backward(ctx, g):
        return g.float().to(ctx.dtype).double(), None, None


def l1_grads(net, x, hr):
    """fp32 stage-1 gradients of mean|out - hr| -> {face_head key: grad}."""
    n = copy.deepcopy(net)
    for p in n.parameters():
        p.requires_grad_(False)
    for p in n.face_head.parameters():
        p.requires_grad_(True)
    with torch.no_grad():
        feat = n.features(x)
    (n.face_head(feat) - hr).abs().mean().backward()
    return {"face_head." + k: p.grad.detach() for k, p in n.face_head.named_parameters()}


def replay_grads(net, x, hr, dtype):
    """The 16-bit stage-1 step on the CPU -> {face_head key: grad (fp32)}."""
    n = _rounded_double(net, dtype)
    for p in n.parameters():
        p.requires_grad_(False)
    for p in n.face_head.parameters():
        p.requires_grad_(True)

    def store(t):
        return _RoundBoth.apply(t, dtype, True)
    with torch.no_grad():
        feat = n.features(x.double(), lambda t: t.float().to(dtype).double())
    out = _RoundBoth.apply(n.face_head(feat, store), dtype, False)    # dL/dsr is stored in dtype
    (out - hr.double()).abs().mean().backward()
    return {"face_head." + k: p.grad.detach().float() for k, p in n.face_head.named_parameters()}

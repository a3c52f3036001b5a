"""Plain-torch restatement of the ESRGAN baseline network (RRDBNet), the checker of the HIP path
at the shapes the golden vectors (tests/golden/g11_rrdb*.npz) do not cover.  Test infrastructure
only: it runs on the CPU and the package never imports it.

The network: conv_first 3->64; num_block RRDBs, each three dense blocks and `out * 0.2 + x`; a
dense block is five 3x3 convs over cat(x, x1, ..) -- Cin 64, 96, 128, 160, 192, Cout 32 x 4 then
64 -- LeakyReLU(0.2) after the first four, returning `x5 * 0.2 + x`; conv_body and `feat +
body`; two stages of nearest x2 -> conv 64->64 -> LeakyReLU; conv_hr -> LeakyReLU -> conv_last.

`store`: applied to every tensor the HIP path writes to memory in its compute dtype -- conv_first's
output, x1..x4, each dense block's output (after the fused residuals: the RRDB's outer residual
is applied before the one store), conv_body + feat, the two upsampler stages and conv_hr --
which makes forward() the 16-bit path's CPU replay: `replay(net, x, dtype)` rounds the 3x3 conv
weights to dtype (not conv_first's and no bias: the HIP path keeps those in fp32), runs the
convs in float64 and rounds every stored activation.
"""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

SLOPE = 0.2


def _act(t):
    return F.leaky_relu(t, SLOPE)


def _same(t):
    return t


class RefDenseBlock(nn.Module):
    def __init__(self, num_feat=64, num_grow_ch=32):
        super().__init__()
        for k in range(5):
            cout = num_feat if k == 4 else num_grow_ch
            setattr(self, f"conv{k + 1}", nn.Conv2d(num_feat + k * num_grow_ch, cout, 3, 1, 1))

    def forward(self, x, store=_same, outer=None):
        cat = [x]
        for k in range(4):
            cat.append(store(_act(getattr(self, f"conv{k + 1}")(torch.cat(cat, 1)))))
        y = self.conv5(torch.cat(cat, 1)) * SLOPE + x
        if outer is not None:
            y = y * SLOPE + outer
        return store(y)


class RefRRDB(nn.Module):
    def __init__(self, num_feat=64, num_grow_ch=32):
        super().__init__()
        self.rdb1 = RefDenseBlock(num_feat, num_grow_ch)
        self.rdb2 = RefDenseBlock(num_feat, num_grow_ch)
        self.rdb3 = RefDenseBlock(num_feat, num_grow_ch)

    def forward(self, x, store=_same):
        return self.rdb3(self.rdb2(self.rdb1(x, store), store), store, outer=x)


class RefRRDBNet(nn.Module):
    def __init__(self, num_in_ch=3, num_out_ch=3, num_feat=64, num_block=23, num_grow_ch=32):
        super().__init__()
        self.conv_first = nn.Conv2d(num_in_ch, num_feat, 3, 1, 1)
        self.body = nn.Sequential(*[RefRRDB(num_feat, num_grow_ch) for _ in range(num_block)])
        for name in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
            setattr(self, name, nn.Conv2d(num_feat, num_feat, 3, 1, 1))
        self.conv_last = nn.Conv2d(num_feat, num_out_ch, 3, 1, 1)

    def forward(self, x, store=_same):
        feat = store(self.conv_first(x))
        t = feat
        for blk in self.body:
            t = blk(t, store)
        t = store(feat + self.conv_body(t))
        for conv in (self.conv_up1, self.conv_up2):
            t = store(_act(conv(F.interpolate(t, scale_factor=2, mode="nearest"))))
        return self.conv_last(store(_act(self.conv_hr(t))))


def from_state_dict(sd, num_block):
    net = RefRRDBNet(num_block=num_block).eval()
    net.load_state_dict({k: torch.as_tensor(v).float() for k, v in sd.items()})
    return net


@torch.no_grad()
def replay(net, x, dtype):
    """The 16-bit HIP path on the CPU (module docstring) -> fp32 output."""
    n = copy.deepcopy(net).double()
    for k, p in n.named_parameters():
        if k.endswith(".weight") and not k.startswith("conv_first."):
            p.copy_(p.float().to(dtype).double())

    def store(t):
        return t.float().to(dtype).double()
    return n(x.double(), store).float()


def golden_state_dict(golden):
    """The fp16 parameters of g11_rrdb.npz + g11_rrdb_body.npz as an fp32 state_dict."""
    sd = {}
    for name in ("g11_rrdb.npz", "g11_rrdb_body.npz"):
        for k, v in golden(name).items():
            if k.startswith("w/"):
                sd[k[2:]] = torch.from_numpy(v.astype("float32"))
    return sd

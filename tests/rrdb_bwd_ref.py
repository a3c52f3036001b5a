"""CPU yardsticks of the dense blocks' backward (stages 2 and 3 of the transfer model).  Test
infrastructure only: it runs on the CPU and the package never imports it.

Built on transfer_ref.RefTransfer / rrdb_ref (validated against the g11 / g13 goldens):
  stage_grads      autograd of the restatement with RRDBs `first`.., conv_body and the head trainable
  dgrad_launch     one fen_rrdb_dgrad launch restated in float64
  wgrad_launch     one fen_rrdb_wgrad launch restated in float64
  manual_grads     the HIP path's own algorithm on the CPU in float64 -- the gradient buffer D of each
                   block, filled by the five launches in the kernel's order -- with every tensor
                   the HIP path stores (conv weights, activations, each read-modify-write of D, the
                   head's stored gradients) rounded to `dtype`: the 16-bit replay.  With dtype =
                   None nothing is rounded and it must equal autograd (the algorithm's own check).
"""
import copy
import glob
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transfer_ref  # noqa: E402

SLOPE = 0.2
S32 = float(torch.tensor(0.2, dtype=torch.float32))               # the kernels' fp32 constants
S32SQ = float(torch.tensor(0.2, dtype=torch.float32) * torch.tensor(0.2, dtype=torch.float32))


def load_g14(golden):
    g = {}
    here = os.path.dirname(os.path.abspath(__file__))
    for path in sorted(glob.glob(os.path.join(here, "golden", "g14_transfer_bwd_*.npz"))):
        g.update(golden(os.path.basename(path)))
    return g


def set_stage(n, first):
    """requires_grad as the model's stage with RRDBs first.. unfrozen (conv_first always frozen)."""
    for p in n.parameters():
        p.requires_grad_(False)
    for i, blk in enumerate(n.backbone["body"]):
        blk.requires_grad_(i >= first)
    n.backbone["conv_body"].requires_grad_(True)
    n.face_head.requires_grad_(True)
    return n


def stage_grads(net, x, hr, first, double=True):
    """Autograd of mean|out - hr| -> {state-dict key: grad} for every trainable parameter."""
    n = set_stage(copy.deepcopy(net).double() if double else copy.deepcopy(net), first)
    if double:
        x, hr = x.double(), hr.double()
    (n(x) - hr).abs().mean().backward()
    return {k: p.grad.detach() for k, p in n.named_parameters() if p.grad is not None}


def lrelu_d(act):
    return torch.where(act > 0, torch.ones_like(act), torch.full_like(act, SLOPE))


def dgrad(dy, w):
    """Gradient w.r.t. the input of conv2d(., w, padding=1) given the output's gradient dy."""
    return F.conv_transpose2d(dy, w, padding=1)


def dgrad_launch(dx, dy, w, cout, accumulate, s, r1=None, s1=0.0, r2=None, s2=0.0, act=None):
    """fen_rrdb_dgrad on NCHW float64 tensors -> the new dx (channels >= cout unchanged)."""
    v = s * dgrad(dy, w)
    assert v.shape[1] == cout
    if accumulate:
        v = v + dx[:, :cout]
    if r1 is not None:
        v[:, :64] += s1 * r1
    if r2 is not None:
        v[:, :64] += s2 * r2
    if act is not None:
        v[:, cout - 32:] *= lrelu_d(act[:, cout - 32:cout])
    out = dx.clone()
    out[:, :cout] = v
    return out


def wgrad_launch(x, dy, scale):
    """fen_rrdb_wgrad: x [B,Cin,H,W], dy [B,Cout,H,W] -> (dw OIHW, db)."""
    dw = torch.nn.grad.conv2d_weight(x, (dy.shape[1], x.shape[1], 3, 3), dy, padding=1)
    return scale * dw, scale * dy.sum(dim=(0, 2, 3))


def block_backward(blk, buf, g, third, g_rrdb, rnd):
    """fen_rrdb_block_bwd on the CPU: blk a RefDenseBlock (float64), buf its 192-channel forward
    buffer, g the output's gradient -> (D, {convK.weight / .bias: grad})."""
    gs = S32 if third else 1.0
    ws = [getattr(blk, f"conv{k}").weight.detach() for k in range(1, 6)]
    D = torch.zeros_like(buf)
    D = rnd(dgrad_launch(D, g, ws[4], 192, False, (S32SQ if third else S32), r1=g, s1=gs, act=buf))
    for k in (4, 3, 2, 1):
        cout = 64 + 32 * (k - 1)
        new = dgrad_launch(D, D[:, cout:cout + 32], ws[k - 1], cout, True, 1.0,
                           r2=g_rrdb if k == 1 else None, s2=1.0, act=buf if k > 1 else None)
        D = torch.cat([rnd(new[:, :cout]), D[:, cout:]], 1)
    G = {}
    for k in range(1, 6):
        cin = 64 + 32 * (k - 1)
        dy, sc = (D[:, cin:cin + 32], 1.0) if k < 5 else (g, (S32SQ if third else S32))
        G[f"conv{k}.weight"], G[f"conv{k}.bias"] = wgrad_launch(buf[:, :cin], dy, sc)
    return D, G


def backbone_forward(bb, x, rnd):
    """-> (feat + conv_body(t), the 192-channel buffer of every dense block, t)."""
    feat = rnd(bb["conv_first"](x))
    t, bufs = feat, []
    for rrdb in bb["body"]:
        x_rrdb = t
        for j, blk in enumerate((rrdb.rdb1, rrdb.rdb2, rrdb.rdb3)):
            cat = [t]
            for k in range(1, 5):
                cat.append(rnd(F.leaky_relu(getattr(blk, f"conv{k}")(torch.cat(cat, 1)), SLOPE)))
            buf = torch.cat(cat, 1)
            y = blk.conv5(buf) * SLOPE + t
            if j == 2:
                y = y * SLOPE + x_rrdb
            t = rnd(y)
            bufs.append(buf)
    return rnd(feat + bb["conv_body"](t)), bufs, t


def manual_grads(net, x, hr, first, dtype=None):
    """The HIP path's stage step on the CPU (module docstring) -> {state-dict key: float64 grad}."""
    if dtype is None:
        n, rnd, store = copy.deepcopy(net).double(), (lambda t: t), (lambda t: t)
    else:
        n = transfer_ref._rounded_double(net, dtype)

        def rnd(t):
            return t.float().to(dtype).double()

        def store(t):
            return transfer_ref._RoundBoth.apply(t, dtype, True)
    set_stage(n, first)
    bb = n.backbone
    with torch.no_grad():
        body, bufs, t = backbone_forward(bb, x.double(), rnd)
    feat_in = body.clone().requires_grad_(True)
    h_in = feat_in if dtype is None else transfer_ref._RoundBoth.apply(feat_in, dtype, False)
    out = n.face_head(h_in, store)
    if dtype is not None:
        out = transfer_ref._RoundBoth.apply(out, dtype, False)
    (out - hr.double()).abs().mean().backward()
    G = {"face_head." + k: p.grad.detach() for k, p in n.face_head.named_parameters()}
    d_feat = feat_in.grad.detach()
    with torch.no_grad():
        G["backbone.conv_body.weight"], G["backbone.conv_body.bias"] = wgrad_launch(t, d_feat, 1.0)
        grads = {3 * len(bb["body"]): rnd(dgrad(d_feat, bb["conv_body"].weight))}
        for nb in range(3 * len(bb["body"]) - 1, 3 * first - 1, -1):
            i, j = divmod(nb, 3)
            blk = getattr(bb["body"][i], f"rdb{j + 1}")
            D, Gb = block_backward(blk, bufs[nb], grads[nb + 1], j == 2, grads[nb + 3] if j == 0 else None, rnd)
            grads[nb] = D[:, :64]
            for k, v in Gb.items():
                G[f"backbone.body.{i}.rdb{j + 1}.{k}"] = v
    return G

"""Bit-exact pin of the strip kernels (test infrastructure; runs on the GPU, once, at the commit
whose arithmetic is to be pinned -- BEFORE a kernel edit that claims to keep the bits).

The existing "chain vs per-group, bit-exact" tests compare two instantiations of the same
source, so a change that moves both passes them.  This records what k_group_strip computes, on
one small case that runs every path of the kernel:
  B = 2, H = 24, W = 64, 64 channels, ng = 2 groups of NB = 2 RCABs + conv_after_body.
  S = 3 strips: a first strip, an interior one with two neighbours, a last one (both edge
  corrections of the pool slice); NB = 2: the j > 0 combine and both hand-off parities;
  ng = 2 + the tail: the group conv epilogue, the kind-2 hand-off and conv_after_body; B = 2:
  the image indexing.
Inputs and parameters are drawn on the CPU from seeded generators (case()); PReLU slopes of
mixed sign around 0.25; about half of conv1's outputs negative (asserted here on the CPU).

g12_strip_chain.npz holds, per dtype (fp16, bf16), as raw 16-bit words / fp32:
  <p>/fb          the inference chain's output (conv_after_body's), in full  [2,24,64,64] u16
  <p>/s           its gates s_out, [ng * NB, B, 64] f32
  <p>/h_sha       SHA-256 of the body output (the last group's)
  <p>/train/...   the training instantiation (pre_elide off): SHA-256 of every saved tensor
                  (x, z1, a1, t, mean, hid, s per RCAB; x_last per group) and of its output
  <p>/g0_sha, <p>/g0_s   the single-group entry fen_group_strip on group 0: its output's
                  SHA-256 and its gates
tests/test_gpu_strip_golden.py runs the same calls and compares.

Usage:  python tests/golden/make_golden_strip.py        (needs the built library and a GPU)
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "face-super-resolution_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

B, H, W, C, CR, G, NB = 2, 24, 64, 64, 16, 2, 2
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
FILE = "g12_strip_chain.npz"
DEV = "cuda"


def case():
    """-> (parameters by state_dict key, x [B,H,W,C] fp32), all from seeded CPU generators."""
    g = torch.Generator().manual_seed(1207)
    q = {}
    for gi in range(G):
        pre = f"residual_groups.{gi}."
        for j in range(NB):
            b = f"{pre}blocks.{j}."
            q[b + "conv1.weight"] = torch.randn(C, C, 3, 3, generator=g) * 0.06
            q[b + "conv1.bias"] = torch.randn(C, generator=g) * 0.1
            q[b + "prelu.weight"] = 0.25 + torch.randn(C, generator=g) * 0.3      # mixed sign
            q[b + "conv2.weight"] = torch.randn(C, C, 3, 3, generator=g) * 0.06
            q[b + "conv2.bias"] = torch.randn(C, generator=g) * 0.1
            q[b + "channel_attention.fc.0.weight"] = torch.randn(CR, C, generator=g) * 0.3
            q[b + "channel_attention.fc.2.weight"] = torch.randn(C, CR, generator=g) * 0.3
        q[pre + "conv.weight"] = torch.randn(C, C, 3, 3, generator=g) * 0.05
        q[pre + "conv.bias"] = torch.randn(C, generator=g) * 0.1
    q["conv_after_body.weight"] = torch.randn(C, C, 3, 3, generator=g) * 0.05
    q["conv_after_body.bias"] = torch.randn(C, generator=g) * 0.1
    x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(1208))
    return q, x


def words(t):
    """A tensor's raw storage words (u16 for the 16-bit formats, else its own dtype), on the CPU."""
    t = t.detach().contiguous().cpu()
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def sha(t):
    return hashlib.sha256(words(t).tobytes()).hexdigest()


def _forward(q, dtype, g_count, save, attn):
    from src.hip.net import Forward, NetSpec, Weights
    from src.hip.program import Ctx
    ctx = Ctx(dtype, DEV)
    Wt = Weights({k: v.to(DEV) for k, v in q.items()}, dtype, DEV)
    ctx.keep(Wt)
    return Forward(NetSpec(C=C, G=g_count, NB=NB, Cr=CR), ctx, Wt, save=save, attn=attn), ctx


def run_case(prec):
    """Every pinned quantity of one dtype -> {key: np array / str}, by the product's own calls."""
    from src.hip import lib as L, net
    dtype = DT[prec]
    q, x32 = case()
    x = x32.to(DEV, dtype)
    out = {}
    # inference: the chained launch, conv_after_body inside it
    attn = {}
    fw, ctx = _forward(q, dtype, G, False, attn)
    assert fw._chain_ok(x), "outside fen_group_strip_chain's envelope"
    outs = [torch.empty_like(x), torch.empty_like(x)]
    fb = torch.empty_like(x)
    ctx.keep([outs, fb])
    h, _ = fw.body(x, [outs[g & 1] for g in range(G)], fb=fb)
    torch.cuda.synchronize()
    L.check_strip_status()
    assert fw.fb_done
    out["fb"] = words(fb)
    out["s"] = np.stack([words(attn[f"group{g}_rcab{j}"]) for g in range(G) for j in range(NB)])
    out["h_sha"] = sha(h)
    # training: the chained launch with every saved tensor, z1 always written
    old = net.PRE_ELIDE
    net.PRE_ELIDE = False
    try:
        fw, ctx = _forward(q, dtype, G, True, None)
        assert fw._chain_ok(x)
        outs = [torch.empty_like(x) for _ in range(G)]
        ctx.keep(outs)
        h, saved = fw.body(x, outs)
        torch.cuda.synchronize()
    finally:
        net.PRE_ELIDE = old
    L.check_strip_status()
    out["train/h_sha"] = sha(h)
    for g in range(G):
        assert not saved[g]["z1_elided"]
        out[f"train/g{g}/x_last"] = sha(saved[g]["x_last"])
        for j, blk in enumerate(saved[g]["blocks"]):
            for k in ("x", "z1", "a1", "t", "mean", "hid", "s"):
                out[f"train/g{g}/b{j}/{k}"] = sha(blk[k])
    # the single-group entry on group 0
    attn = {}
    fw, ctx = _forward(q, dtype, 1, False, attn)
    assert not fw._chain_ok(x) and fw._strip_ok(x)
    y0 = torch.empty_like(x)
    ctx.keep(y0)
    h, _ = fw.body(x, [y0])
    torch.cuda.synchronize()
    L.check_strip_status()
    out["g0_sha"] = sha(h)
    out["g0_s"] = np.stack([words(attn[f"group0_rcab{j}"]) for j in range(NB)])
    return out


def _conv1_negative_fraction(q, x32, dtype):
    """CPU: the share of negative values in conv1 + b1 of group 0's first RCAB (its input is x):
    PReLU's negative branch must be well exercised."""
    import torch.nn.functional as F
    xr = x32.to(dtype).float().permute(0, 3, 1, 2)
    w = q["residual_groups.0.blocks.0.conv1.weight"].to(dtype).float()
    z = F.conv2d(xr, w, q["residual_groups.0.blocks.0.conv1.bias"], padding=1)
    return float((z < 0).float().mean())


if __name__ == "__main__":
    q, x32 = case()
    store = {}
    for prec in DT:
        neg = _conv1_negative_fraction(q, x32, DT[prec])
        assert 0.4 <= neg <= 0.6, neg
        al = torch.cat([v for k, v in q.items() if k.endswith("prelu.weight")])
        assert bool((al < 0).any()) and bool((al > 0.25).any()) and abs(float(al.mean()) - 0.25) < 0.1
        r = run_case(prec)
        again = run_case(prec)                       # the pin must at least repeat itself
        for k, v in r.items():
            same = np.array_equal(v, again[k]) if isinstance(v, np.ndarray) else v == again[k]
            assert same, f"{prec}/{k} differs between two runs"
            store[f"{prec}/{k}"] = v if isinstance(v, np.ndarray) else np.array(v)
        print(f"{prec}: conv1 negative share {neg:.3f}, fb sha {hashlib.sha256(r['fb'].tobytes()).hexdigest()[:16]}")
    path = os.path.join(HERE, FILE)
    np.savez_compressed(path, **store)
    print(FILE, os.path.getsize(path), "bytes,", len(store), "entries")

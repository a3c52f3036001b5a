"""Transfer model (TransferSRModel) golden vectors (test infrastructure; runs ONLY where the
reference is present, on the CPU).

Imports the reference package from FEN_REFERENCE, builds TransferSRModel(TransferModelConfig(
backbone_blocks=1, head_blocks=2)) under a fixed seed, rounds every parameter to fp16 BEFORE the
reference runs (so the parameters can be stored as fp16), moves conv_last and the PReLU slopes away
from anything degenerate and records
  x              the input [2,3,12,20] in [0,1] (ragged tiles: even, but no multiple of 16)
  feat           the head's input [2,64,12,20] (a failure names backbone or head)
  out            the reference's fp32 output [2,3,48,80]
  feat_f64_err, out_f64_err      max |fp32 run - float64 run| of the reference itself
  hr             a target [2,3,48,80]
  g/<key>        the stage-1 gradient of mean|out - hr| for every face_head.* parameter (fp32)
  gerr/<key>     |fp32 gradient - float64 gradient| / |float64 gradient| (2-norms) of the reference
  w/<key>        the state_dict as fp16
  default/...    the default config (16 / 4): total_params, and trainable_params, the number of
                 trainable tensors and the conv_first / conv_body / first / last block flags in each
                 of the three stages, and the parameter groups' sizes and learning rates
  seed/names, seed/sum, seed/abs   per parameter of TransferSRModel() under torch.manual_seed(42):
                 float64 sum and sum of magnitudes (the construction-parity test)
No committed file may exceed 1 MiB, so the arrays are spread over g13_transfer_NN.npz files.
Nothing from the reference travels except these numbers.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_transfer.py
"""
import contextlib
import copy
import glob
import io
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = os.environ.get("FEN_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
from src.models.transfer import TrainingStage, TransferModelConfig, TransferSRModel  # noqa: E402

LIMIT = 900_000     # raw bytes per file (random fp16 / fp32 data does not compress)

quiet = contextlib.redirect_stdout(io.StringIO())
torch.manual_seed(1311)
with quiet:
    net = TransferSRModel(TransferModelConfig(backbone_blocks=1, head_blocks=2)).eval()
gen = torch.Generator().manual_seed(13)
with torch.no_grad():
    head = net.face_head
    head.conv_last.weight.add_(0.02 * torch.randn(head.conv_last.weight.shape, generator=gen))
    head.conv_last.bias.copy_(torch.tensor([0.05, -0.03, 0.11]))
    for m in net.modules():
        if isinstance(m, torch.nn.PReLU):          # slopes in [0.1, 0.4], every 7th one -0.1: 4-channel
            m.weight.copy_(0.1 + 0.3 * torch.rand(m.weight.shape, generator=gen))     # groups of both kinds
            m.weight[::7] = -0.1
    for p in net.parameters():
        p.copy_(p.half().float())
    x = torch.rand(2, 3, 12, 20, generator=gen)
    hr = torch.rand(2, 3, 48, 80, generator=gen)


def features(m, t):
    f = m.backbone["conv_first"](t)
    b = f
    for blk in m.backbone["body"]:
        b = blk(b)
    return f + m.backbone["conv_body"](b)


def grads(m, t, target):
    m.zero_grad()
    (m(t) - target).abs().mean().backward()
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


with torch.no_grad():
    feat, out = features(net, x), net(x)
    net64 = copy.deepcopy(net).double()
    feat64, out64 = features(net64, x.double()), net64(x.double())
g32 = grads(net, x, hr)
g64 = grads(net64, x.double(), hr.double())
assert all(k.startswith("face_head.") for k in g32) and len(g32) == len(list(net.face_head.parameters()))

arrays = {"x": x.numpy(), "hr": hr.numpy(), "feat": feat.numpy(), "out": out.numpy(),
          "feat_f64_err": np.float64((feat.double() - feat64).abs().max()),
          "out_f64_err": np.float64((out.double() - out64).abs().max())}
for k, v in g32.items():
    arrays["g/" + k] = v.numpy()
    arrays["gerr/" + k] = np.float64((v.double() - g64[k]).norm() / g64[k].norm())
for k, v in net.state_dict().items():
    h = v.numpy().astype(np.float16)
    assert np.array_equal(h.astype(np.float32), v.numpy()), k
    arrays["w/" + k] = h

# the default configuration: counts, flags and parameter groups per stage
torch.manual_seed(42)
with quiet:
    big = TransferSRModel()
names = [k for k, _ in big.named_parameters()]
arrays["seed/names"] = np.array(names)
arrays["seed/sum"] = np.array([float(p.detach().double().sum()) for p in big.parameters()])
arrays["seed/abs"] = np.array([float(p.detach().double().abs().sum()) for p in big.parameters()])
arrays["default/total_params"] = np.int64(big.get_model_info()["total_params"])
for stage in TrainingStage:
    with quiet:
        big.set_training_stage(stage)
    info = big.get_model_info()
    pre = f"default/stage{stage.value}/"
    arrays[pre + "trainable_params"] = np.int64(info["trainable_params"])
    arrays[pre + "trainable_names"] = np.array([k for k, p in big.named_parameters() if p.requires_grad])
    groups = big.get_trainable_params()
    arrays[pre + "group_sizes"] = np.array([sum(p.numel() for p in g["params"]) for g in groups], dtype=np.int64)
    arrays[pre + "group_lrs"] = np.array([g["lr"] for g in groups], dtype=np.float64)

for old in glob.glob(os.path.join(OUT, "g13_transfer_*.npz")):
    os.remove(old)
files, cur, size = [], {}, 0
for k in sorted(arrays, key=lambda k: (k.startswith(("w/", "g/")), k)):
    n = np.asarray(arrays[k]).nbytes
    if cur and size + n > LIMIT:
        files.append(cur)
        cur, size = {}, 0
    cur[k] = arrays[k]
    size += n
files.append(cur)
for i, f in enumerate(files):
    path = os.path.join(OUT, f"g13_transfer_{i:02d}.npz")
    np.savez_compressed(path, **f)
    print(os.path.basename(path), len(f), "arrays", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)
print("params", sum(v.numel() for v in net.state_dict().values()), "max|out|", float(out.abs().max()),
      "f32 vs f64", float(arrays["out_f64_err"]), "worst gerr", max(float(arrays[k]) for k in arrays if k.startswith("gerr/")))

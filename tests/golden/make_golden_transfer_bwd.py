"""Transfer model stage-3 gradient golden vectors (test infrastructure; runs ONLY where the
reference is present, on the CPU).

Imports the reference package from FEN_REFERENCE, builds TransferSRModel(TransferModelConfig(
backbone_blocks=1, head_blocks=2)), loads the fp16-exact parameters, the input x and the target hr
already recorded in tests/golden/g13_transfer_*.npz, sets STAGE3_FULL_FINETUNE and records
  g/<key>        the gradient of mean|out - hr| for every backbone.* parameter that has one (fp32;
                 conv_first is frozen in every stage and has none)
  gerr/<key>     |fp32 gradient - float64 gradient| / |float64 gradient| (2-norms) of the reference
  frozen         the names of the backbone parameters without a gradient
About 0.76 M floats: no committed file may exceed 1 MiB, so the arrays are spread over
g14_transfer_bwd_NN.npz files.  Nothing from the reference travels except these numbers.

Usage:  FEN_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_transfer_bwd.py
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
REF = os.environ["FEN_REFERENCE"]      # the reference checkout
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
from src.models.transfer import TrainingStage, TransferModelConfig, TransferSRModel  # noqa: E402

LIMIT = 900_000     # raw bytes per file (random fp32 data does not compress)

g13 = {}
for path in sorted(glob.glob(os.path.join(OUT, "g13_transfer_*.npz"))):
    with np.load(path) as f:
        g13.update({k: f[k] for k in f.files})
sd = {k[2:]: torch.from_numpy(v.astype(np.float32)) for k, v in g13.items() if k.startswith("w/")}
x, hr = torch.from_numpy(g13["x"]), torch.from_numpy(g13["hr"])

quiet = contextlib.redirect_stdout(io.StringIO())
with quiet:
    net = TransferSRModel(TransferModelConfig(backbone_blocks=1, head_blocks=2))
    net.load_state_dict(sd)
    net.set_training_stage(TrainingStage.STAGE3_FULL_FINETUNE)
net.train()


def grads(m, t, target):
    m.zero_grad()
    (m(t) - target).abs().mean().backward()
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


g32 = grads(net, x, hr)
g64 = grads(copy.deepcopy(net).double(), x.double(), hr.double())
# the head's gradients of this run are the stage-1 ones g13 holds: the two files describe one step
for k, v in g32.items():
    if k.startswith("face_head."):
        assert np.array_equal(v.numpy(), g13["g/" + k]), k

arrays = {"frozen": np.array([k for k, v in g32.items() if k.startswith("backbone.") and v is None])}
for k, v in g32.items():
    if k.startswith("backbone.") and v is not None:
        arrays["g/" + k] = v.numpy()
        arrays["gerr/" + k] = np.float64((v.double() - g64[k]).norm() / g64[k].norm())

for old in glob.glob(os.path.join(OUT, "g14_transfer_bwd_*.npz")):
    os.remove(old)
files, cur, size = [], {}, 0
for k in sorted(arrays, key=lambda k: (k.startswith("g/"), k)):
    n = np.asarray(arrays[k]).nbytes
    if cur and size + n > LIMIT:
        files.append(cur)
        cur, size = {}, 0
    cur[k] = arrays[k]
    size += n
files.append(cur)
for i, f in enumerate(files):
    path = os.path.join(OUT, f"g14_transfer_bwd_{i:02d}.npz")
    np.savez_compressed(path, **f)
    print(os.path.basename(path), len(f), "arrays", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)
print("frozen", list(arrays["frozen"]), "gradients", sum(1 for k in arrays if k.startswith("g/")),
      "worst gerr", max(float(arrays[k]) for k in arrays if k.startswith("gerr/")))

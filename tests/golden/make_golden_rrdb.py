"""RRDBNet (ESRGAN baseline) golden vectors (test infrastructure; runs ONLY in the survey
container, on the CPU).

Loads the reference's src/models/esrgan.py by file path (the module imports only torch and
numpy), builds RRDBNet(num_block=1) under a fixed seed, rounds every parameter to fp16 BEFORE
the reference runs (so the parameters can be stored as fp16: 870,659 of them) and records
  x            the input [2,3,12,20] in [0,1]
  out          the reference's fp32 output [2,3,48,80]
  rrdb0        body[0] (the first RRDB) applied to conv_first(x), [2,64,12,20]: a failure can
               name the block
  out_f64_err  max |fp32 run - float64 run| of the reference itself (the fixture's own error)
  w/<key>      the state_dict as fp16
No committed file may exceed 1 MiB, so the parameters are split over two files:
g11_rrdb.npz (everything but body.0.rdb1 / rdb2) and g11_rrdb_body.npz (those two blocks).
Nothing from the reference travels except these numbers.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rrdb.py
"""
import copy
import importlib.util
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = os.environ.get("FEN_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))

spec = importlib.util.spec_from_file_location("ref_esrgan", os.path.join(REF, "src", "models", "esrgan.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

torch.manual_seed(1123)
net = ref.RRDBNet(num_block=1).eval()
with torch.no_grad():
    for p in net.parameters():
        p.copy_(p.half().float())
    x = torch.rand(2, 3, 12, 20, generator=torch.Generator().manual_seed(11))
    out = net(x)
    feat = net.conv_first(x)
    rrdb0 = net.body[0](feat)
    out64 = copy.deepcopy(net).double()(x.double())
err64 = float((out.double() - out64).abs().max())

sd = {k: v.numpy().astype(np.float16) for k, v in net.state_dict().items()}
assert all(np.array_equal(v.astype(np.float32), net.state_dict()[k].numpy()) for k, v in sd.items())
body = {"w/" + k: v for k, v in sd.items() if k.startswith(("body.0.rdb1.", "body.0.rdb2."))}
rest = {"w/" + k: v for k, v in sd.items() if "w/" + k not in body}
np.savez_compressed(os.path.join(OUT, "g11_rrdb.npz"), x=x.numpy(), out=out.numpy(),
                    rrdb0=rrdb0.numpy(), out_f64_err=np.float64(err64), **rest)
np.savez_compressed(os.path.join(OUT, "g11_rrdb_body.npz"), **body)
print("params", sum(v.size for v in sd.values()), "max|out|", float(out.abs().max()), "f32 vs f64", err64)
for f in ("g11_rrdb.npz", "g11_rrdb_body.npz"):
    print(f, os.path.getsize(os.path.join(OUT, f)))

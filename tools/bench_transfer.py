"""Transfer model timings: the no-skip conv_last (FEN_EPI_LAST | FEN_EPI_NOSKIP)
against fen_rrdb_conv(nchw_out=1) on the same input at B=32 256x256, the inference forward at
64x64 -> 256x256 B=32 fp16, the stage-1, stage-2 and stage-3 eager steps at B=32 bf16 (the last two
with train_backbone=True) and one dense block's backward (fen_rrdb_block_bwd: its five data-gradient
launches, and with its five weight gradients) at B=32 64x64 bf16.

    python tools/bench_transfer.py [--reps 5]

Device time per launch from a captured graph of n launches (no host gaps; 300 of a conv_last
route, 17-28 ms per timed replay), the median of --reps
replays; the two conv_last routes alternate within one process."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'face-super-resolution_amd'))
import torch  # noqa: E402

from src.hip import lib as L, net  # noqa: E402
from src.hip.program import Ctx, ptr  # noqa: E402
from src.hip.rrdb import rrdb_conv  # noqa: E402
from src.hip import rrdb as R  # noqa: E402
from src.models import TrainingStage, create_transfer_model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
B = 32


def graph_us(f, n, reps):
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            f()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1000 / n)
    return out


for dtype in (torch.float16, torch.bfloat16):
    ctx = Ctx(dtype, 'cuda')
    x = torch.randn(B, 256, 256, 64, device='cuda', dtype=dtype)
    wl = torch.randn(3, 64, 3, 3, device='cuda') * 0.01
    bl = torch.zeros(3, device='cuda')
    wp = torch.empty(ctx.lib.fen_packed_elems(0, 3, 64), device='cuda', dtype=dtype)
    ctx.emit('p', ctx.lib.fen_pack_conv_w, ctx.code, 0, 3, 64, ptr(wl), ptr(wp))
    o1 = torch.empty(B, 3, 256, 256, device='cuda')
    o2 = torch.empty(B, 3, 256, 256, device='cuda')

    def fast():
        net.conv(ctx, x, wp, B, 256, 256, 64, 3, bias=bl, epi=L.EPI_LAST | L.EPI_NOSKIP, y=o1)

    def mfma16():
        rrdb_conv(ctx, x, 64, wp, bl, o2, 0, 0, B, 256, 256, 64, 3, nchw_out=1)
    a, b = [], []
    for _ in range(2):                      # alternate the two routes
        a += graph_us(fast, 300, args.reps)
        b += graph_us(mfma16, 300, args.reps)
    print(json.dumps({"dtype": str(dtype), "noskip_us": round(statistics.median(a), 2), "noskip_all": [round(v, 1) for v in a],
                      "rrdb_conv_us": round(statistics.median(b), 2), "rrdb_conv_all": [round(v, 1) for v in b],
                      "GBs_noskip": round(x.numel() * 2 / statistics.median(a) / 1e3, 1),
                      "max_abs_diff": float((o1 - o2).abs().max())}))
    del x, o1, o2

torch.manual_seed(0)
lr = torch.rand(B, 3, 64, 64, device='cuda')
hr = torch.rand(B, 3, 256, 256, device='cuda')
m = create_transfer_model(precision="fp16").cuda().eval()
with torch.no_grad():
    ts = graph_us(lambda: m(lr), 3, args.reps)
print(json.dumps({"inference_fp16_B32_ms": round(statistics.median(ts) / 1e3, 3), "all_ms": [round(v / 1e3, 3) for v in ts]}))
del m
def eager_step_ms(stage):
    m = create_transfer_model(precision="bf16", train_backbone=stage > 1).cuda().train()
    m.set_training_stage(TrainingStage(stage))
    opt = torch.optim.AdamW(m.get_trainable_params())

    def step():
        opt.zero_grad(set_to_none=True)
        (m(lr) - hr).abs().mean().backward()
        opt.step()
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            step()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 5)
    return ts


for stage in (1, 2, 3):
    ts = eager_step_ms(stage)
    print(json.dumps({f"stage{stage}_step_bf16_B32_ms_eager": round(statistics.median(ts), 3),
                      "all_ms": [round(v, 3) for v in ts]}))
    torch.cuda.empty_cache()

# one dense block's backward at B = 32, 64 x 64, bf16: data gradients alone, then with the weight gradients
ctx = Ctx(torch.bfloat16, 'cuda')
torch.manual_seed(1)
params = {}
for k in range(5):
    params[f"conv{k + 1}.weight"] = torch.randn(32 if k < 4 else 64, 64 + 32 * k, 3, 3, device='cuda') * 0.02
    params[f"conv{k + 1}.bias"] = torch.zeros(32 if k < 4 else 64, device='cuda')
Wt = net.Weights(params, torch.bfloat16, 'cuda')
G = {k: torch.empty_like(v) for k, v in params.items()}
buf = torch.randn(B, 64, 64, 192, device='cuda').bfloat16()
D = torch.empty_like(buf)
g = (torch.randn(B, 64, 64, 64, device='cuda') * 1e-3).bfloat16()
# MFMA work: 2 * 9 * pixels * sum(Cin * Cout) per pass
flop = 2 * 9 * B * 64 * 64 * sum((64 + 32 * k) * (32 if k < 4 else 64) for k in range(5))
PEAK = 2.5168e15   # dense bf16 MFMA peak of the part (spec), FLOP/s
for name, weights in (("dgrad", False), ("dgrad_wgrad", True)):
    ts = graph_us(lambda: R.dense_block_backward(ctx, Wt, G, "", buf, D, g, 64, False, None, 0, B, 64, 64,
                                                  weights=weights), 20, args.reps)
    us = statistics.median(ts)
    n = 2 if weights else 1
    print(json.dumps({f"block_bwd_{name}_us": round(us, 1), "all_us": [round(v, 1) for v in ts],
                      "frac_mfma_peak": round(n * flop / (us * 1e-6) / PEAK, 4)}))

#!/usr/bin/env python
"""Time LPIPS (AlexNet, HIP path) per batch: AlexLpips.per_image at B x 3 x S x S replayed from a
hipGraph, and the five fen_conv2d_f32 launches of the same plan captured alone, both with HIP
events over `--iters` replays per round, `--rounds` rounds alternated (the median round is
reported).  Prints one JSON line: times in ms, the convs' share, and the convs' rate against the
157.3 TFLOP/s fp32 matrix peak (FLOPs counted from the shapes: 2 M N K per conv with the real
Cin, both images of every pair).

    python tools/bench_lpips.py [--batch 32] [--size 256] [--iters 50] [--rounds 7]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "face-super-resolution_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_F32_MATRIX = 157.3e12


def conv_flops(B, H, W):
    """FLOPs of the five convs for B image pairs (2B images)."""
    from src.hip.lpips import ALEX_CONVS, tap_sizes
    total = 0
    for (h, w), (_, cin, cout, ks, _, _) in zip(tap_sizes(H, W), ALEX_CONVS):
        total += 2 * (2 * B * h * w) * cout * (cin * ks * ks)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    import lpips_ref as R
    from src.hip import lib as L
    from src.hip.lpips import AlexLpips, load_lpips_weights
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips.py: needs a ROCm GPU")
    B, S = args.batch, args.size
    m = AlexLpips(load_lpips_weights(R.make_weights(0)))
    pred = R.make_images(B, S, S, seed=1).cuda()
    target = R.make_images(B, S, S, seed=2).cuda()
    out = m.per_image(pred, target)                    # warm-up: plan, packed weights, code objects
    torch.cuda.synchronize()
    plan = m._plan(B, S, S, pred.device)
    convs = [op for op in plan.ops if op[0] == "conv2d_f32"]

    def run_convs():
        s = torch.cuda.current_stream().cuda_stream
        for name, fn, a in convs:
            L.check(fn(*a, s), name)
    graphs = {}
    for name, body in (("per_image", lambda: m.per_image(pred, target)), ("convs", run_convs)):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            body()
        g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                g.replay()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.iters)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    fl = conv_flops(B, S, S)
    print(json.dumps({
        "batch": B, "size": S, "per_image_ms": round(med["per_image"], 4), "convs_ms": round(med["convs"], 4),
        "per_image_ms_min_max": [round(min(times["per_image"]), 4), round(max(times["per_image"]), 4)],
        "convs_share": round(med["convs"] / med["per_image"], 3), "conv_gflop_per_pair": round(fl / B / 1e9, 3),
        "convs_tflops": round(fl / (med["convs"] * 1e-3) / 1e12, 2),
        "convs_fraction_of_f32_matrix_peak": round(fl / (med["convs"] * 1e-3) / PEAK_F32_MATRIX, 4),
        "lpips_mean": float(out.mean()),
    }))


if __name__ == "__main__":
    main()

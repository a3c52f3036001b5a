"""The ESRGAN baseline (23-block RRDBNet, csrc/rrdb.hip) at LR 64x64 -> 256x256: B = 1 (the
reference's own latency set-up) and B = 32, one process.  The forward is captured as a graph
(random weights: the time does not depend on them); after a warm-up, REPLAYS back-to-back
replays are timed by device events, ROUNDS times: ms per forward (median, min, max over the
rounds), img/s and the fraction of the MFMA peak (2500 TFLOP/s fp16 / bf16 dense, bench.py's
figure; fp32 is reported against the same number for scale only) from the network's conv FLOPs.

    python tools/bench_rrdb.py [--precision fp16|bf16|fp32] [--batches 1,32] [--blocks 23]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "face-super-resolution_amd"))
import torch  # noqa: E402
from src.models import RRDBNet  # noqa: E402

PEAK_TFLOPS = 2500.0
LR = 64


def conv_flops(num_block: int, h: int, w: int) -> float:
    """2 * 9 * Cin * Cout per output pixel, summed over the network, for one image."""
    dense = sum((64 + 32 * k) * 32 for k in range(4)) + 192 * 64
    lr_px = 3 * 64 + 3 * num_block * dense + 64 * 64             # conv_first, the RRDBs, conv_body
    return 18.0 * h * w * (lr_px + 4 * 64 * 64 + 16 * 64 * 64 + 16 * 64 * 64 + 16 * 64 * 3)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp16", choices=["fp16", "bf16", "fp32"])
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--blocks", type=int, default=23)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    torch.manual_seed(0)
    net = RRDBNet(num_block=a.blocks, precision=a.precision).to("cuda").eval()
    flops = conv_flops(a.blocks, LR, LR)
    for B in (int(v) for v in a.batches.split(",")):
        x = torch.rand(B, 3, LR, LR, device="cuda")
        with torch.no_grad():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    net(x)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                y = net(x)
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.replays):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / a.replays)
        med = statistics.median(ms)
        print(json.dumps({
            "model": f"RRDBNet x{a.blocks}", "precision": a.precision, "B": B, "lr": [LR, LR], "out": list(y.shape),
            "ms": {"median": round(med, 3), "min": round(min(ms), 3), "max": round(max(ms), 3)},
            "img_per_s": round(B / med * 1e3, 1), "gflop_per_img": round(flops / 1e9, 2),
            "frac_mfma_peak": round(B * flops / (med * 1e-3) / 1e12 / PEAK_TFLOPS, 4),
            "finite": bool(torch.isfinite(y).all()),
        }), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

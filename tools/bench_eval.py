"""fen_image_metrics (flags 1: SR clamped in registers, per-image mse / PSNR / SSIM in one tile
launch + a one-block finish) against the launches that give the same numbers without it -- a
clamped copy, ssim(size_average=False) (fen_ssim + fen_colsum) and the torch psnr_batch ops -- in
one process at B=32, 3x256x256 fp32.  Each side is captured as a graph of CALLS back-to-back
calls; the graphs are replayed alternately over ROUNDS rounds (warm-up first), timed by device
events: us per call (median, min, max over the rounds) and the ratio of the medians.

Then MetricCalculator.evaluate_dataset's loop with the bench's 6x10 fp16 model at B=32: NB
batches already on the device (no loader in the timing), host clock around the whole call, which
ends in its one device-to-host copy: ms per batch, next to the engine's replay alone."""
import json
import os
import statistics
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "face-super-resolution_amd"))
import torch  # noqa: E402
from src.evaluation.metrics import FLAG_CLAMP, MetricCalculator, image_metrics  # noqa: E402
from src.hip import lib as L  # noqa: E402
from src.hip.program import ptr  # noqa: E402
from src.losses.ssim import _window1d  # noqa: E402

B, C, H, W = int(os.environ.get("B", "32")), 3, 256, 256
CALLS, REPLAYS, ROUNDS = 20, int(os.environ.get("REPLAYS", "50")), int(os.environ.get("ROUNDS", "7"))
NB = int(os.environ.get("NB", "20"))
lib = L.load()
t = torch.rand(B, C, H, W, device="cuda")
p = 0.6 * t + 0.5 * torch.rand(B, C, H, W, device="cuda") - 0.05        # leaves [0, 1]: the clamp works
out = torch.empty(3, B, device="cuda")
work = torch.empty(lib.fen_image_metrics_work_floats(B, C, H, W), device="cuda")


def fused():
    return image_metrics(p, t, 1.0, FLAG_CLAMP, out=out, work=work)


win = _window1d(11, 1.5).cuda()
rows = lib.fen_ssim_parts(B, C, H, W)
part = torch.empty(rows * B, device="cuda")
per_img = torch.empty(B, device="cuda")


def pair():
    """What src.losses.ssim.ssim(size_average=False) launches (its window already on the device:
    a capture admits no host copy), on a clamped copy, and psnr_batch's torch ops."""
    c = p.clamp(0, 1)
    s = torch.cuda.current_stream().cuda_stream
    L.check(lib.fen_ssim(L.F32, B, C, H, W, ptr(c), ptr(t), ptr(win), 11, 1e-4, 9e-4, ptr(part), None, 0.0, 0, s), "ssim")
    L.check(lib.fen_colsum(rows, B, ptr(part), 1.0 / (C * H * W), ptr(per_img), 0, s), "ssim colsum")
    mse = torch.mean((c - t) ** 2, dim=[1, 2, 3])
    return per_img, 10 * torch.log10(1.0 / (mse + 1e-10))


def capture(f):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            f()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for _ in range(CALLS):
            f()
    return g


def time_graph(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (REPLAYS * CALLS)


s_ref, ps_ref = pair()
o = fused().clone()
res = {"B": B, "shape": [C, H, W],
       "max_abs_psnr_diff_dB": float((o[1] - ps_ref).abs().max()), "max_abs_ssim_diff": float((o[2] - s_ref).abs().max())}
graphs = {"fused": capture(fused), "pair": capture(pair)}
for g in graphs.values():          # warm-up of both graphs
    for _ in range(10):
        g.replay()
torch.cuda.synchronize()
times = {k: [] for k in graphs}
for _ in range(ROUNDS):             # alternating
    for k, g in graphs.items():
        times[k].append(time_graph(g))
for k, v in times.items():
    res[f"{k}_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
res["fused_over_pair"] = round(res["fused_us"]["median"] / res["pair_us"]["median"], 3)
print(json.dumps(res), flush=True)

if os.environ.get("NO_DATASET") != "1":
    import bench  # noqa: E402
    hr, _ = bench.bench_batch(B, 0)
    model = bench.build_model("fp16")
    calc = MetricCalculator("cuda")
    batches = [{"hr": hr} for _ in range(NB)]
    calc.evaluate_dataset(model, batches[:2])                   # builds and captures the engine
    torch.cuda.synchronize()
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        r = calc.evaluate_dataset(model, batches)
        walls.append((time.perf_counter() - t0) * 1e3 / NB)
    eng = calc._engines[(B, H, W)][1]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(NB):
        eng.replay()
    torch.cuda.synchronize()
    rep = (time.perf_counter() - t0) * 1e3 / NB
    print(json.dumps({"evaluate_dataset_ms_per_batch": {"median": round(statistics.median(walls), 4),
                                                        "min": round(min(walls), 4), "max": round(max(walls), 4)},
                      "engine_replay_ms": round(rep, 4), "batches": NB, "B": B, "precision": "fp16",
                      "psnr_mean": round(r["psnr_mean"], 4), "ssim_mean": round(r["ssim_mean"], 6)}), flush=True)

"""fen_msssim (value + gradient accumulated into an NHWC16 bf16 buffer, grad_mode 2) against the
fen_ssim_ex pair of the stage-2 SSIM term, same process, at B=32, 3x256x256: us per call by HIP
events and their ratio.  MS-SSIM filters 1.33x the pixels of level 0 (the pyramid) and adds the
pooling, finish and combine launches."""
import json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'face-super-resolution_amd'))
import torch
from src.hip import lib as L
from src.hip.program import ptr
from src.losses.ssim import MS_SSIM_WEIGHTS, _window1d
B, C, H, W = int(os.environ.get("B", "32")), 3, 256, 256
LEVELS = len(MS_SSIM_WEIGHTS)
lib = L.load()
p = torch.rand(B, C, H, W, device="cuda")
t = (0.6 * p + 0.4 * torch.rand(B, C, H, W, device="cuda")).clamp(0, 1)
buf = torch.zeros(B, H, W, 16, device="cuda", dtype=torch.bfloat16)
win = _window1d(11, 1.5).cuda()
wts = torch.tensor(MS_SSIM_WEIGHTS, device="cuda")
s = torch.cuda.current_stream().cuda_stream
part = torch.empty(lib.fen_ssim_parts(B, C, H, W) * B, device="cuda")
work = torch.empty(lib.fen_ssim_work_floats(B, C, H, W), device="cuda")
ms_work = torch.empty(lib.fen_msssim_work_floats(B, C, H, W, LEVELS), device="cuda")
ms_out = torch.empty(1 + LEVELS, device="cuda")
runs = {
    "ssim_ex": lambda: L.check(lib.fen_ssim_ex(L.BF16, B, C, H, W, ptr(p), ptr(t), ptr(win), 11, 1e-4, 9e-4, ptr(part),
                                               ptr(buf), -1e-6, 2, ptr(work), s), "ssim_ex"),
    "msssim": lambda: L.check(lib.fen_msssim(L.BF16, B, C, H, W, ptr(p), ptr(t), ptr(win), 11, 1e-4, 9e-4, ptr(wts),
                                             LEVELS, ptr(ms_work), ptr(ms_out), ptr(buf), -1e-6, 2, s), "msssim"),
    "msssim_value": lambda: L.check(lib.fen_msssim(L.BF16, B, C, H, W, ptr(p), ptr(t), ptr(win), 11, 1e-4, 9e-4,
                                                   ptr(wts), LEVELS, ptr(ms_work), ptr(ms_out), None, 0.0, 0, s),
                                    "msssim"),
}
res = {"B": B, "work_MB": round(ms_work.numel() * 4 / 2 ** 20, 1)}
for name, f in runs.items():
    for _ in range(5): f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50): f()
    e1.record(); torch.cuda.synchronize()
    res[f"{name}_us"] = round(e0.elapsed_time(e1) * 1e3 / 50, 2)
res["msssim_over_ssim_ex"] = round(res["msssim_us"] / res["ssim_ex_us"], 3)
res["ms_ssim"] = round(float(ms_out[0]), 6)
print(json.dumps(res))

#!/usr/bin/env python
"""Evaluate a checkpoint: per-image PSNR / SSIM over a validation set on the HIP path.

    python scripts/evaluate.py --checkpoint X.pth [--data-root DIR | --synthetic N] \\
        [--batch-size 32] [--precision fp16|bf16|fp32] [--quantize] [--json OUT] [--model custom|esrgan|transfer] \\
        [--lpips-weights FILE]

The checkpoint is loaded weights-only (FaceEnhanceNet.from_pretrained); the images come from
get_dataloader(mode='val') -- the full images, in order, the last batch partial -- and LR is
synthesised from HR on the GPU as in training.  MetricCalculator.evaluate_dataset runs the
captured inference engine and one fused metrics call per batch, with one host read at the end.
--quantize rounds SR to 8 bits first, as the reference's scripts/test_model.py does before it
measures.  --model esrgan evaluates the ESRGAN comparison baseline instead (a 23-block RRDBNet;
--checkpoint is its state dict -- plain, or under 'params_ema' / 'params' -- or absent for random
weights with a warning): the same loader, LR synthesis and fused fen_image_metrics call per batch,
the forward run eagerly at whatever size the images have.  --model transfer evaluates a
TransferSRModel the same way: --checkpoint is its state dict, plain or under 'model_state_dict' /
'state_dict', with an optional 'model_config' (the Trainer's checkpoints) or 'config' dict; its
TransferModelConfig fields are used, other keys ignored.  Prints psnr_mean / psnr_std /
ssim_mean / ssim_std / num_images; --json OUT writes them with the per-image arrays.
--lpips-weights FILE (every --model) adds LPIPS v0.1 on the AlexNet backbone through the HIP kernels
(src.evaluation.LPIPS(weights=FILE): a .pth state dict of AlexNet's convs and the five linear
layers, never downloaded): lpips_mean / lpips_std and the per-image values, on the same clamped
(--quantize: 8-bit) SR as PSNR and SSIM, still with one host read at the end.
"""
import argparse
import json
import sys
from pathlib import Path

PKG = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(PKG))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="PSNR / SSIM of a FaceEnhanceNet checkpoint over a validation set")
    ap.add_argument("--model", choices=["custom", "esrgan", "transfer"], default="custom",
                    help="custom: FaceEnhanceNet (default); esrgan: the RRDBNet baseline; transfer: TransferSRModel")
    ap.add_argument("--checkpoint", default=None,
                    help="a reference-format .pth checkpoint (required for --model custom; esrgan: a RRDBNet "
                         "state dict, or none for random weights)")
    src = ap.add_mutually_exclusive_group()
    src.add_argument("--data-root", default=None, help="a directory of HxWx3 .npy images (or DIR/val)")
    src.add_argument("--synthetic", type=int, default=0, metavar="N", help="N seeded synthetic HR images instead")
    ap.add_argument("--hr-size", type=int, default=256, help="the side of the --synthetic images")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--num-workers", type=int, default=0, help="host loader workers (0: load in this process)")
    ap.add_argument("--precision", choices=["fp16", "bf16", "fp32"], default=None,
                    help="the compute precision (default: the checkpoint's config, else fp32)")
    ap.add_argument("--quantize", action="store_true", help="quantise SR to 8 bits before measuring")
    ap.add_argument("--json", default=None, metavar="OUT", help="write the results and per-image arrays here")
    ap.add_argument("--lpips-weights", default=None, metavar="FILE",
                    help="a .pth state dict of AlexNet + the LPIPS linear layers: also report LPIPS (HIP path)")
    args = ap.parse_args(argv)
    if args.model in ("custom", "transfer") and not args.checkpoint:
        ap.error("the following arguments are required: --checkpoint")
    return args


def evaluate_esrgan(args, loader):
    """The baseline over `loader`: per batch LR = fen_bicubic_down4(HR) (or the batch's 'lr'), one
    RRDBNet forward, one fen_image_metrics call on the clamped (--quantize: 8-bit) SR; the
    per-image numbers stay on the device until one read at the end.  The statistics are
    MetricCalculator.evaluate_dataset's: PSNR over images, SSIM over per-batch means."""
    import warnings

    import torch

    from src.models import RRDBNet
    model = RRDBNet(precision=args.precision or "fp32")
    if args.checkpoint:
        state = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
        for key in ("params_ema", "params"):
            if isinstance(state, dict) and key in state:
                state = state[key]
                break
        model.load_state_dict(state, strict=False)
    else:
        warnings.warn("--model esrgan without --checkpoint: randomly initialised weights (for testing only)")
    return eager_metrics(model, args, loader)


def evaluate_transfer(args, loader):
    """A TransferSRModel checkpoint over `loader`, measured as the baseline is (eager_metrics)."""
    from dataclasses import fields

    import torch

    from src.models import TransferModelConfig, TransferSRModel
    ckpt = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
    known = {f.name for f in fields(TransferModelConfig)}
    cfg = (ckpt.get("model_config") or ckpt.get("config")) if isinstance(ckpt, dict) else None
    cfg = TransferModelConfig(**{k: v for k, v in cfg.items() if k in known}) if isinstance(cfg, dict) else None
    for key in ("model_state_dict", "state_dict"):
        if isinstance(ckpt, dict) and key in ckpt:
            ckpt = ckpt[key]
            break
    model = TransferSRModel(cfg, precision=args.precision or "fp32")
    model.load_state_dict(ckpt)
    return eager_metrics(model, args, loader)


def eager_metrics(model, args, loader):
    """model's eager forward over `loader` -> the statistics of evaluate_esrgan's docstring."""
    import numpy as np
    import torch

    from src.evaluation.metrics import FLAG_CLAMP, FLAG_QUANTIZE, LPIPS, image_metrics, metric_pred
    from src.hip import lib as L
    model = model.to("cuda").eval()
    lpips = LPIPS(weights=args.lpips_weights) if getattr(args, "lpips_weights", None) else None
    lps = []
    flags = FLAG_CLAMP | (FLAG_QUANTIZE if args.quantize else 0)
    lib = L.load()
    outs = []
    with torch.no_grad():
        for batch in loader:
            hr = batch["hr"].to("cuda").float().contiguous()
            lr = batch.get("lr")
            B, C, H, W = (int(v) for v in hr.shape)
            if lr is None:
                if H % 4 or W % 4:
                    raise ValueError(f"HR {H} x {W} is not a multiple of the scale factor 4")
                lr = torch.empty(B, C, H // 4, W // 4, device="cuda")
                L.check(lib.fen_bicubic_down4(B, C, H, W, hr.data_ptr(), lr.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "bicubic_down4")
            sr = model(lr.to("cuda"))
            outs.append(image_metrics(sr, hr, 1.0, flags).clone())
            if lpips is not None:               # per image, on the SR the other two metrics saw; stays on the device
                lps.append(lpips.per_image(metric_pred(sr, args.quantize), hr))
    if not outs:
        raise ValueError("evaluate.py: the dataloader yielded no batch")
    if lps:                                                  # the LPIPS values ride behind each batch's metrics
        outs = [torch.cat([o.reshape(-1), l]) for o, l in zip(outs, lps)]
    host = [o.cpu().double().numpy() for o in outs]          # the one wait for the stream
    if lps:
        lp = np.concatenate([o[-l.numel():] for o, l in zip(host, lps)])
        host = [o[:-l.numel()].reshape(3, -1) for o, l in zip(host, lps)]
    ps = np.concatenate([o[1] for o in host])
    ss = np.concatenate([o[2] for o in host])
    batch_ssim = np.array([o[2].mean() for o in host])
    res = {"psnr_mean": float(ps.mean()), "psnr_std": float(ps.std()), "ssim_mean": float(batch_ssim.mean()),
           "ssim_std": float(batch_ssim.std()), "per_image": {"psnr": ps, "ssim": ss}, "num_images": int(ps.size)}
    if lps:
        res.update(lpips_mean=float(lp.mean()), lpips_std=float(lp.std()))
        res["per_image"]["lpips"] = lp
    return res


def main(argv=None) -> int:
    args = parse_args(argv)
    import torch

    from src.data import get_dataloader
    from src.evaluation import MetricCalculator
    from src.models import FaceEnhanceNet

    if not args.synthetic and not args.data_root:
        raise SystemExit("evaluate.py: give --data-root DIR or --synthetic N")
    if not torch.cuda.is_available():
        raise SystemExit("evaluate.py: the HIP path needs a ROCm GPU")
    if args.model in ("esrgan", "transfer"):
        loader = get_dataloader(args.data_root, mode="val", batch_size=args.batch_size, num_workers=args.num_workers,
                                hr_patch_size=args.hr_size, synthetic=args.synthetic, device="cpu")
        res = evaluate_esrgan(args, loader) if args.model == "esrgan" else evaluate_transfer(args, loader)
        per = res.pop("per_image")
        res.update(model=args.model, checkpoint=str(args.checkpoint), precision=args.precision or "fp32",
                   quantize=bool(args.quantize))
        print(json.dumps(res))
        if args.json:
            with open(args.json, "w") as f:
                json.dump(dict(res, per_image={k: [float(v) for v in a] for k, a in per.items()}), f)
        return 0
    model = FaceEnhanceNet.from_pretrained(args.checkpoint)
    if args.precision is not None and args.precision != model.config.precision:
        cfg = model.config
        cfg.precision = args.precision
        sd = model.state_dict()
        model = FaceEnhanceNet(cfg)
        model.load_state_dict(sd)
    # the host loader: full images in order and an exact partial last batch (the device loader
    # fills its last batch up with images from the start, which would be counted twice)
    loader = get_dataloader(args.data_root, mode="val", batch_size=args.batch_size, num_workers=args.num_workers,
                            hr_patch_size=args.hr_size, synthetic=args.synthetic, device="cpu")
    res = MetricCalculator(device="cuda", lpips_weights=args.lpips_weights).evaluate_dataset(
        model, loader, quantize=args.quantize)
    per = res.pop("per_image")
    res.update(checkpoint=str(args.checkpoint), precision=model.config.precision, quantize=bool(args.quantize))
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(res, per_image={k: [float(v) for v in a] for k, a in per.items()}), f)
    return 0


if __name__ == "__main__":
    sys.exit(main())

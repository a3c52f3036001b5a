#!/usr/bin/env python
"""Evaluate a checkpoint: per-image PSNR / SSIM over a validation set on the HIP path.

    python scripts/evaluate.py --checkpoint X.pth [--data-root DIR | --synthetic N] \\
        [--batch-size 32] [--precision fp16|bf16|fp32] [--quantize] [--json OUT]

The checkpoint is loaded weights-only (FaceEnhanceNet.from_pretrained); the images come from
get_dataloader(mode='val') -- the full images, in order, the last batch partial -- and LR is
synthesised from HR on the GPU as in training.  MetricCalculator.evaluate_dataset runs the
captured inference engine and one fused metrics call per batch, with one host read at the end.
--quantize rounds SR to 8 bits first, as the reference's scripts/test_model.py does before it
measures.  Prints psnr_mean / psnr_std / ssim_mean / ssim_std / num_images; --json OUT writes
them with the per-image arrays.
"""
import argparse
import json
import sys
from pathlib import Path

PKG = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(PKG))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="PSNR / SSIM of a FaceEnhanceNet checkpoint over a validation set")
    ap.add_argument("--checkpoint", required=True, help="a reference-format .pth checkpoint")
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
    return ap.parse_args(argv)


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
    res = MetricCalculator(device="cuda").evaluate_dataset(model, loader, quantize=args.quantize)
    per = res.pop("per_image")
    res.update(checkpoint=str(args.checkpoint), precision=model.config.precision, quantize=bool(args.quantize))
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(res, per_image={k: [float(v) for v in a] for k, a in per.items()}), f)
    return 0


if __name__ == "__main__":
    sys.exit(main())

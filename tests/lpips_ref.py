"""LPIPS v0.1 on the AlexNet backbone, restated in plain torch ops from its definition --
independent of csrc/lpips.hip and src/hip/lpips.py -- and parameterised by dtype: float64 is the
reference, float32 (torch CPU) the yardstick the kernels' error is measured against.

    input range   pred.min() >= 0: pred and target both become 2x - 1 (pred alone decides)
    scaling       (x - shift) / scale per channel
    backbone      AlexNet features: conv 11/4/2 3->64, ReLU, pool 3/2, conv 5/1/2 64->192, ReLU,
                  pool 3/2, conv 3/1/1 192->384, ReLU, 384->256, ReLU, 256->256, ReLU; the five
                  ReLU outputs are the taps
    per tap       f / (sqrt(sum_c f^2) + 1e-10) for both images, squared difference, weighted by
                  lin[c], summed over channels, averaged over the tap's pixels
    result        the sum over the taps, per image

`fault` plants one deviation from the definition (tests/test_lpips_cpu.py shows that each moves
the result by far more than the GPU test's tolerance).
"""
import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# (index in torchvision's features, Cin, Cout, kernel, stride, pad)
CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1),
         (10, 256, 256, 3, 1, 1))
FAULTS = ("pad1", "ceil", "noeps", "norm_after", "skip_tap")

# The end-to-end tolerance of tests/test_gpu_lpips.py: per image, relative,
#     |got - ref64| <= E2E_MARGIN * yard * ref64,
# yard = the worst relative error of the float32 restatement against the float64 one over the
# images of the same kind of case (all shapes).  One image's LPIPS is a sum of ~10^4 rounded
# terms, so its fp32 error is one random draw that can cancel to almost nothing; the worst of the
# kind's draws estimates the scale of the fp32 error, which the kernels share (same formats, other
# summation order).  The margin is parity.GLOBAL; measured ratios (at most 1.000) are in
# tests/test_gpu_lpips.py MEASURED_E2E.
E2E_MARGIN = 1.5


def make_weights(seed=0, conv3_bias=None):
    """A state dict in torchvision's spelling plus lin{k}.model.1.weight: Kaiming-scaled conv
    weights (std sqrt(2 / fan_in)), small biases, non-negative lin = rand * (2 / C).
    conv3_bias: a constant for features.6.bias (-1e3 zeroes every feature from tap 3 on)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, (idx, cin, cout, ks, _, _) in enumerate(CONVS):
        sd[f"features.{idx}.weight"] = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
        sd[f"features.{idx}.bias"] = torch.randn(cout, generator=g) * 0.05
        sd[f"lin{k}.model.1.weight"] = (torch.rand(cout, generator=g) * (2.0 / cout)).view(1, cout, 1, 1)
    if conv3_bias is not None:
        sd["features.6.bias"] = torch.full((384,), float(conv3_bias))
    return sd


def to_lpips_spelling(sd):
    """The same tensors under the `lpips` module's names (net.slice{k+1}.{idx}.*), with its
    scaling_layer buffers added."""
    out = {}
    for k, (idx, *_rest) in enumerate(CONVS):
        for part in ("weight", "bias"):
            out[f"net.slice{k + 1}.{idx}.{part}"] = sd[f"features.{idx}.{part}"]
        out[f"lin{k}.model.1.weight"] = sd[f"lin{k}.model.1.weight"]
    out["scaling_layer.shift"] = torch.tensor(SHIFT).view(1, 3, 1, 1)
    out["scaling_layer.scale"] = torch.tensor(SCALE).view(1, 3, 1, 1)
    return out


def make_images(B, H, W, seed=0, noise=0.1):
    """[B,3,H,W] in [0,1]: a smooth field (an 8x-upsampled coarse random grid) plus noise."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(B, 3, -(-H // 8) + 1, -(-W // 8) + 1, generator=g)
    smooth = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    return (smooth + noise * torch.randn(B, 3, H, W, generator=g)).clamp(0, 1)


def prepare(pred, target, dtype):
    """The range rule and the scaling layer -> (pred, target) in `dtype`."""
    p, t = pred.to(dtype), target.to(dtype)
    if bool(pred.min() >= 0):
        p, t = p * 2 - 1, t * 2 - 1
    shift = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    return (p - shift) / scale, (t - shift) / scale


def features(x, sd, fault=None, inputs=None):
    """The five taps of x (already scaled, NCHW) in x's dtype.  inputs: a list that receives
    each conv's input."""
    taps = []
    for k, (idx, _, _, _, stride, pad) in enumerate(CONVS):
        if k in (1, 2):
            x = F.max_pool2d(x, 3, 2, ceil_mode=(fault == "ceil"))
        w, b = sd[f"features.{idx}.weight"].to(x.dtype), sd[f"features.{idx}.bias"].to(x.dtype)
        if fault == "pad1" and k == 0:
            pad = 1
        if fault == "skip_tap" and k == 1:
            w = w.clone()
            w[:, :, 2, 3] = 0
        if inputs is not None:
            inputs.append(x)
        x = torch.relu(F.conv2d(x, w, b, stride=stride, padding=pad))
        taps.append(x)
    return taps


def tap_distance(a, b, lin, fault=None):
    """One tap: [B,C,h,w] x 2 -> [B]."""
    eps = 0.0 if fault == "noeps" else 1e-10
    lin = lin.to(a.dtype).view(1, -1, 1, 1)
    if fault == "norm_after":
        d = a - b
        d = d / (torch.sqrt((d * d).sum(1, keepdim=True)) + eps)
    else:
        na = torch.sqrt((a * a).sum(1, keepdim=True)) + eps
        nb = torch.sqrt((b * b).sum(1, keepdim=True)) + eps
        d = a / na - b / nb
    return (lin * d * d).sum(1).mean(dim=(1, 2))


@torch.no_grad()
def lpips(pred, target, sd, dtype=torch.float64, fault=None):
    """LPIPS per image, [B] in `dtype`."""
    p, t = prepare(pred, target, dtype)
    fp, ft = features(p, sd, fault), features(t, sd, fault)
    total = 0
    for k in range(5):
        total = total + tap_distance(fp[k], ft[k], sd[f"lin{k}.model.1.weight"], fault)
    return total


def tap_shapes(H, W):
    """(h, w) of the five taps by the floor-division formulas."""
    h1, w1 = (H + 4 - 11) // 4 + 1, (W + 4 - 11) // 4 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    h3, w3 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    return [(h1, w1), (h2, w2), (h3, w3), (h3, w3), (h3, w3)]


# ------------------------------------------------------------------ the end-to-end cases
E2E_SHAPES = ((3, 64, 64), (2, 48, 80), (1, 67, 61), (1, 32, 32))
E2E_KINDS = ("far", "near", "signed", "mixed", "zero_vec")
_CASES = {}


def e2e_inputs(kind, B, H, W):
    """(pred, target, weight seed / conv3 bias) of one case.
    far: SR unrelated to HR.  near: SR = HR + 1e-3 noise.  signed: inputs already in [-1, 1]
    (pred has negatives: no rescale).  mixed: pred >= 0, target with negatives: both rescaled.
    zero_vec: conv3 bias -1e3, every feature vector from tap 3 on is all zero."""
    hr = make_images(B, H, W, seed=100 + H)
    g = torch.Generator().manual_seed(7 + H)
    if kind == "near":
        sr = hr + 1e-3 * torch.randn(B, 3, H, W, generator=g)
        sr = sr - sr.min().clamp(max=0)                  # keep pred >= 0: the usual [0, 1] route
    else:
        sr = make_images(B, H, W, seed=200 + H)
    if kind == "signed":
        sr, hr = sr * 2 - 1, hr * 2 - 1
        assert float(sr.min()) < 0
    if kind == "mixed":
        hr = hr - 0.25
        assert float(sr.min()) >= 0 and float(hr.min()) < 0
    return sr, hr, make_weights(3, conv3_bias=-1e3 if kind == "zero_vec" else None)


def e2e_case(kind, B, H, W):
    """-> dict(pred, target, sd, ref64 [B], yard32 [B]); computed once, shared, left unchanged."""
    key = (kind, B, H, W)
    if key not in _CASES:
        sr, hr, sd = e2e_inputs(kind, B, H, W)
        _CASES[key] = dict(pred=sr, target=hr, sd=sd, ref=lpips(sr, hr, sd, torch.float64),
                           yard=lpips(sr, hr, sd, torch.float32).double())
    return _CASES[key]


def e2e_yard_error(kind):
    """The worst relative error of the float32 restatement over the kind's images (all shapes)."""
    worst = 0.0
    for B, H, W in E2E_SHAPES:
        c = e2e_case(kind, B, H, W)
        worst = max(worst, float(((c["yard"] - c["ref"]).abs() / c["ref"]).max()))
    return worst

"""LPIPS (AlexNet) without a GPU: the public surface, the weight loader, the properties of the
restated definition (tests/lpips_ref.py), and the teeth of the GPU test's tolerance: every
planted fault moves the float64 result by many times what tests/test_gpu_lpips.py allows."""
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_ref as R  # noqa: E402


def test_signature_defaults():
    from src.evaluation import LPIPS, MetricCalculator
    p = inspect.signature(LPIPS.__init__).parameters
    assert p["weights"].default is None and p["net"].default == "alex"
    assert inspect.signature(MetricCalculator.__init__).parameters["lpips_weights"].default is None
    assert callable(LPIPS.per_image)


def test_weights_with_another_backbone_raises():
    from src.evaluation import LPIPS
    for net in ("vgg", "squeeze"):
        with pytest.raises(NotImplementedError, match="AlexNet"):
            LPIPS(net=net, weights=R.make_weights(0))


def test_hip_path_is_available_and_refuses_cpu_tensors():
    from src.evaluation import LPIPS
    m = LPIPS(weights=R.make_weights(0))
    assert m.available is True
    x = torch.rand(1, 3, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.per_image(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x, x)


def test_loader_spellings_and_errors(tmp_path):
    from src.hip.lpips import load_lpips_weights
    sd = R.make_weights(1)
    a = load_lpips_weights(sd)
    b = load_lpips_weights(R.to_lpips_spelling(sd))           # scaling_layer.* ignored
    path = tmp_path / "w.pth"
    torch.save(sd, path)
    c = load_lpips_weights(str(path))
    assert set(a) == {f"conv{k}.{p}" for k in range(5) for p in ("weight", "bias")} | {f"lin{k}" for k in range(5)}
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    assert a["conv0.weight"].shape == (64, 3, 11, 11) and a["lin2"].shape == (384,)
    assert torch.equal(a["lin1"], sd["lin1.model.1.weight"].view(-1))
    for missing in ("features.6.bias", "lin3.model.1.weight"):
        bad = {k: v for k, v in sd.items() if k != missing}
        with pytest.raises(KeyError, match=missing.replace(".", r"\.")):
            load_lpips_weights(bad)
    bad = dict(sd)
    bad["features.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r"features\.3\.weight"):
        load_lpips_weights(bad)
    bad = dict(sd)
    bad["lin4.model.1.weight"] = torch.zeros(256)
    with pytest.raises(ValueError, match=r"lin4\.model\.1\.weight"):
        load_lpips_weights(bad)


def test_c_abi_host_refusals():
    """Every refusal returns before any launch, so the loaded library answers on the CPU."""
    from src.hip import lib as L
    lib = L.load()
    P = 0x10000
    assert lib.fen_lpips_work_floats(2, 64, 64) == 320 + 2 * (4 + 1 + 1 + 1 + 1)   # 225, 49, 9, 9, 9 pixels / 64
    assert lib.fen_lpips_work_floats(2, 30, 64) == 0 and lib.fen_lpips_work_floats(2, 64, 30) == 0
    assert lib.fen_lpips_work_floats(0, 64, 64) == 0
    assert lib.fen_lpips_work_floats(1, 31, 31) > 0
    n = lib.fen_lpips_work_floats(2, 64, 64)
    assert lib.fen_lpips_prep(2, 30, 64, P, P, P, n, P, None) == -2
    assert lib.fen_lpips_prep(2, 64, 64, None, P, P, n, P, None) == -1
    assert lib.fen_lpips_prep(2, 64, 64, P, P, P, n - 1, P, None) == -1           # a short workspace
    assert lib.fen_lpips_head(2, 64, 64, 5, P, P, P, n, None) == -1
    assert lib.fen_lpips_head(2, 64, 64, 0, P, None, P, n, None) == -1
    assert lib.fen_lpips_head(2, 64, 64, 0, P, P, P, n - 1, None) == -1
    assert lib.fen_lpips_finish(2, 64, 64, P, n, None, None) == -1
    assert lib.fen_lpips_finish(2, 64, 30, P, n, P, None) == -2

    def conv(N=2, H=15, W=15, Cin=64, Cout=192, k=5, s=1, p=2, x=P, w=P, y=P):
        return lib.fen_conv2d_f32(N, H, W, Cin, Cout, k, k, s, p, x, w, P, 1, y, None)
    assert conv(x=None) == -1 and conv(w=None) == -1 and conv(y=None) == -1
    assert conv(x=P + 4) == -1                                # not 16-B aligned
    assert conv(Cout=96) == -2
    assert conv(Cin=3) == -2                                  # K = 75: not a multiple of 4
    assert conv(H=2, k=11, p=2) == -2                         # an empty output
    assert conv(s=0) == -1
    assert lib.fen_maxpool3s2_f32(2, 15, 15, 64, None, P, None) == -1
    assert lib.fen_maxpool3s2_f32(2, 15, 15, 63, P, P, None) == -2
    assert lib.fen_maxpool3s2_f32(2, 2, 15, 64, P, P, None) == -2
    assert lib.fen_conv2d_f32_pack(64, 3, 11, 11, 2, P, P, None) == -1            # Cin_pad < Cin


# ------------------------------------------------------------------ the restatement
def test_restatement_properties():
    sd = R.make_weights(0)
    a, b = R.make_images(2, 64, 64, seed=1), R.make_images(2, 64, 64, seed=2)
    d = R.lpips(a, b, sd)
    assert d.shape == (2,) and bool((d > 0).all())
    assert bool((R.lpips(a, a, sd) == 0).all())                               # identity
    assert torch.allclose(d, R.lpips(b, a, sd), rtol=1e-12, atol=0)           # symmetric
    # the range rule is pred's alone: pred >= 0 with a target that has negatives rescales both
    t = b - 0.25
    assert float(a.min()) >= 0 and float(t.min()) < 0
    assert torch.allclose(R.lpips(a, t, sd), R.lpips(a.double() * 2 - 1, t.double() * 2 - 1, sd), rtol=1e-12, atol=0)
    assert not torch.allclose(R.lpips(a, t, sd), R.lpips(t, a, sd), rtol=1e-3, atol=0)   # pred < 0: no rescale
    # a pixel whose whole feature vector is 0 after ReLU: 0 / (0 + eps), finite
    z = R.make_weights(0, conv3_bias=-1e3)
    p, _ = R.prepare(a, b, torch.float64)
    assert float(R.features(p, z)[2].abs().max()) == 0
    for dt in (torch.float64, torch.float32):
        assert bool(torch.isfinite(R.lpips(a, b, z, dt)).all())


@pytest.mark.parametrize("H,W", [(31, 31), (32, 32), (64, 64), (48, 80), (67, 61)])
def test_output_sizes(H, W):
    sd = R.make_weights(0)
    p, _ = R.prepare(torch.rand(1, 3, H, W), torch.rand(1, 3, H, W), torch.float32)
    taps = R.features(p, sd)
    from src.hip.lpips import tap_sizes
    assert [tuple(t.shape[2:]) for t in taps] == R.tap_shapes(H, W) == tap_sizes(H, W)
    assert [t.shape[1] for t in taps] == [64, 192, 384, 256, 256]
    assert all(h >= 1 and w >= 1 for h, w in R.tap_shapes(H, W))
    if (H, W) == (31, 31):
        assert R.tap_shapes(31, 31)[2] == (1, 1)
        with pytest.raises(RuntimeError):                     # 30: the second pool has nothing to take
            R.features(R.prepare(torch.rand(1, 3, 30, 30), torch.rand(1, 3, 30, 30), torch.float32)[0], sd)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_exceed_the_gpu_tolerance(fault):
    """Each fault in the float64 restatement moves LPIPS, relative to its value, by at least 5x what
    the GPU end-to-end test allows for its 'far' cases (E2E_MARGIN x the fp32 yardstick's error):
    every image of at least one of that test's shapes.  (ceil and floor pooling agree wherever
    (h - 3) is even -- 64 x 64, 48 x 80 and 32 x 32 -- which is why 67 x 61 is among the shapes.)"""
    allowed = R.E2E_MARGIN * R.e2e_yard_error("far")
    worst = None
    for B, H, W in R.E2E_SHAPES:
        c = R.e2e_case("far", B, H, W)
        if fault == "pad1" and (H, W) == (32, 32):
            continue                                          # pad 1 leaves the second pool nothing to take here
        moved = (R.lpips(c["pred"], c["target"], c["sd"], torch.float64, fault=fault) - c["ref"]).abs() / c["ref"]
        # eps matters only where a feature vector is (nearly) zero: the zero-vector weights below
        if fault != "noeps":
            worst = float(moved.min()) if worst is None else max(worst, float(moved.min()))
    if fault == "noeps":
        c = R.e2e_case("zero_vec", 3, 64, 64)
        broken = R.lpips(c["pred"], c["target"], c["sd"], torch.float64, fault=fault)
        assert not bool(torch.isfinite(broken).any())         # 0 / 0 in taps 3..5: caught as non-finite
        return
    print(f"{fault}: moves LPIPS by >= {worst:.3e} relative; allowed {allowed:.3e}; ratio {worst / allowed:.1f}")
    assert worst >= 5 * allowed, (fault, worst, allowed)

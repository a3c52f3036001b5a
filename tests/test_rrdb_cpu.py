"""ESRGAN baseline (RRDBNet), everything that runs without a GPU: the plain-torch restatement
against the reference's recorded numbers, the module surface (state_dict keys and shapes), the
weight-file policy, the inference-only contract and the refusals."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rrdb_ref  # noqa: E402


@pytest.fixture(scope="module")
def ref_net(golden):
    return rrdb_ref.from_state_dict(rrdb_ref.golden_state_dict(golden), num_block=1)


def test_restatement_reproduces_golden(golden, ref_net):
    """rrdb_ref on the recorded fp16-exact weights equals the reference's fp32 run to 1e-6 of the
    output's range (the reference is itself ~4e-8 absolute from its float64 run), for the first
    RRDB alone and for the whole network."""
    g = golden("g11_rrdb.npz")
    x = torch.from_numpy(g["x"])
    with torch.no_grad():
        r0 = ref_net.body[0](ref_net.conv_first(x))
        out = ref_net(x)
    for name, got, want in (("rrdb0", r0, g["rrdb0"]), ("out", out, g["out"])):
        want = torch.from_numpy(want)
        assert got.shape == want.shape
        rel = float((got - want).abs().max() / want.abs().max())
        print(f"{name}: rel {rel:.2e} (max|ref| {float(want.abs().max()):.4f})")
        assert rel <= 1e-6, (name, rel)
    assert float(g["out_f64_err"]) < 1e-6 * float(abs(g["out"]).max())


def test_state_dict_matches_restatement():
    from src.models import RRDBNet
    sd = RRDBNet(num_block=2).state_dict()
    ref = rrdb_ref.RefRRDBNet(num_block=2).state_dict()
    assert set(sd) == set(ref), set(sd) ^ set(ref)
    for k, v in ref.items():
        assert sd[k].shape == v.shape and sd[k].dtype == torch.float32, k
    assert "body.1.rdb3.conv5.weight" in sd and sd["body.1.rdb3.conv5.weight"].shape == (64, 192, 3, 3)
    assert sum(v.numel() for v in RRDBNet(num_block=1).state_dict().values()) == 870659


def test_known_weights_missing_is_file_not_found(tmp_path, monkeypatch):
    """A known model name without its file: FileNotFoundError naming the path, and nothing is
    fetched (urlretrieve / urlopen would fail the test)."""
    import urllib.request

    from src.models import ESRGANBaseline, create_esrgan_baseline

    def no_network(*a, **k):
        raise AssertionError("the ESRGAN baseline tried to reach the network")
    monkeypatch.setattr(urllib.request, "urlretrieve", no_network)
    monkeypatch.setattr(urllib.request, "urlopen", no_network)
    for name in ("RealESRGAN_x4plus", "ESRGAN_x4"):
        with pytest.raises(FileNotFoundError) as e:
            ESRGANBaseline(model_name=name, device="cpu", weights_dir=str(tmp_path))
        assert str(tmp_path / f"{name}.pth") in str(e.value)
    with pytest.raises(FileNotFoundError):
        create_esrgan_baseline(device="cpu", weights_dir=str(tmp_path))


def test_backward_raises_not_implemented():
    """The autograd tie every forward goes through when something requires a gradient: its
    backward refuses, so the frozen network is never silently treated as a constant."""
    from src.models import esrgan
    x = torch.ones(3, requires_grad=True)
    y = esrgan._InferenceFn.apply(lambda t: t * 2.0, x)
    assert y.requires_grad
    with pytest.raises(NotImplementedError, match="inference-only"):
        y.sum().backward()


def test_refusals_without_gpu():
    from src.hip import lib as L
    from src.models import RRDBNet, ResidualDenseBlock
    with pytest.raises(NotImplementedError):
        RRDBNet(num_feat=32, num_block=1)
    with pytest.raises(NotImplementedError):
        RRDBNet(num_grow_ch=16, num_block=1)
    with pytest.raises(ValueError):
        RRDBNet(num_block=1, precision="fp8")
    net = RRDBNet(num_block=1)
    with pytest.raises(RuntimeError, match="GPU"):
        net(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="GPU"):
        ResidualDenseBlock()(torch.zeros(1, 64, 8, 8))
    # the C-ABI validates before any launch
    lib = L.load()
    assert lib.fen_rrdb_conv(None, None) == -1
    d = L.RrdbConvDesc()
    d.dtype, d.B, d.H, d.W, d.Cin, d.Cout = L.F16, 1, 8, 8, 64, 32
    d.x = d.w = d.bias = d.y = 0x1000
    d.x_stride = d.y_stride = 192
    d.y_off = 32                                   # in place, the written slice inside the read range
    assert lib.fen_rrdb_conv(d, None) == -1
    d.y = 0x100000
    d.Cin = 80                                     # not 64 + 32 j
    assert lib.fen_rrdb_conv(d, None) == -2
    d.Cin, d.Cout = 64, 48
    assert lib.fen_rrdb_conv(d, None) == -2
    d.Cout, d.B, d.H, d.W = 32, 1 << 11, 1 << 10, 1 << 10     # 2^31 pixels
    assert lib.fen_rrdb_conv(d, None) == -2
    d.B, d.H, d.W, d.up2 = 1, 7, 8, 1              # odd H under the fused upsample
    assert lib.fen_rrdb_conv(d, None) == -1
    d.up2, d.x = 0, None
    assert lib.fen_rrdb_conv(d, None) == -1
    b = L.RrdbBlockDesc()
    b.dtype, b.B, b.H, b.W, b.num_feat, b.num_grow_ch = L.F32, 1, 8, 8, 64, 16
    b.buf, b.next = 0x1000, 0x100000
    for k in range(5):
        b.w[k] = b.bias[k] = 0x1000
    assert lib.fen_rrdb_block(b, None) == -2       # num_grow_ch
    b.num_feat, b.num_grow_ch = 32, 32
    assert lib.fen_rrdb_block(b, None) == -2       # num_feat
    b.num_feat, b.next = 64, 0x1000
    assert lib.fen_rrdb_block(b, None) == -1       # next == buf
    b.next, b.w[3] = 0x100000, None
    assert lib.fen_rrdb_block(b, None) == -1
    assert lib.fen_rrdb_block(None, None) == -1
    assert lib.fen_rrdb_first(L.F32, 1, 3, 8, 8, None, None, None, None, 192, None, None) == -1
    assert lib.fen_rrdb_first(L.F32, 1, 3, 0, 8, 16, 16, 16, 16, 192, None, None) == -1
    assert lib.fen_rrdb_first(L.F32, 1, 9, 8, 8, 16, 16, 16, 16, 192, None, None) == -2

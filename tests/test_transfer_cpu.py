"""Transfer model (TransferSRModel), everything that runs without a GPU: the plain-torch
restatement against the reference's recorded numbers (forward, the head's input, the stage-1
gradients), seeded construction, the stages' flags / counts / parameter groups, the pre-trained
weight mapping and the refusals."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transfer_ref  # noqa: E402

golden_state_dict = transfer_ref.golden_state_dict


@pytest.fixture(scope="module")
def g13(golden):
    return transfer_ref.load_g13(golden)


@pytest.fixture(scope="module")
def ref_net(g13):
    return transfer_ref.from_state_dict(golden_state_dict(g13), 1, 2)


def test_restatement_reproduces_golden(g13, ref_net):
    """transfer_ref on the recorded fp16-exact weights against the reference's fp32 run.  Both are
    fp32 evaluations of the same function in different operation orders, each about the recorded
    fp32-vs-float64 error away from the exact value, so they may differ by twice that; 4x leaves
    room for the error not being the same in both."""
    x = torch.from_numpy(g13["x"])
    with torch.no_grad():
        feat, out = ref_net.features(x), ref_net(x)
    for name, got in (("feat", feat), ("out", out)):
        want = torch.from_numpy(g13[name])
        assert got.shape == want.shape
        err, bound = float((got - want).abs().max()), 4 * float(g13[name + "_f64_err"])
        print(f"{name}: max|d| {err:.2e} (bound {bound:.2e}, max|ref| {float(want.abs().max()):.4f})")
        assert err <= bound, (name, err, bound)
    assert float(g13["out_f64_err"]) < 1e-5 * float(np.abs(g13["out"]).max())


def test_restatement_gradients_reproduce_golden(g13, ref_net):
    """The stage-1 gradients of mean|out - hr|, per face_head parameter, relative 2-norm error at
    most 4x the reference's own fp32-vs-float64 figure for that parameter (+ 1e-6: fp32 epsilon
    times a few, for the parameters whose recorded figure happens to be tiny)."""
    grads = transfer_ref.l1_grads(ref_net, torch.from_numpy(g13["x"]), torch.from_numpy(g13["hr"]))
    keys = [k[2:] for k in g13 if k.startswith("g/")]
    assert sorted(keys) == sorted(grads) and len(keys) == 2 * 7 + 2 + 2 * 3 + 2
    for k in keys:
        want = torch.from_numpy(g13["g/" + k])
        rel = float((grads[k] - want).norm() / want.norm())
        assert rel <= 4 * float(g13["gerr/" + k]) + 1e-6, (k, rel, float(g13["gerr/" + k]))


def test_state_dict_matches_restatement(g13):
    from src.models import TransferModelConfig, TransferSRModel
    m = TransferSRModel(TransferModelConfig(backbone_blocks=1, head_blocks=2))
    sd, ref = m.state_dict(), golden_state_dict(g13)
    assert list(sd) == list(transfer_ref.RefTransfer(1, 2).state_dict()) and set(sd) == set(ref)
    for k, v in ref.items():
        assert sd[k].shape == v.shape and sd[k].dtype == torch.float32, k
    for k in ("backbone.conv_first.weight", "backbone.body.0.rdb3.conv5.bias", "backbone.conv_body.bias",
              "face_head.rcab_blocks.1.channel_attention.fc.2.weight", "face_head.conv_after.weight",
              "face_head.upsample.stages.1.prelu.weight", "face_head.conv_last.bias"):
        assert k in sd, k
    m.load_state_dict(ref)


def test_seeded_construction_matches_reference(g13):
    """torch.manual_seed(42) + TransferSRModel(): every parameter's sum and sum of magnitudes equal
    the reference's (same construction order, same initialisers; the upsampler keeps ICNR)."""
    from src.models import TransferSRModel
    torch.manual_seed(42)
    m = TransferSRModel()
    names = [k for k, _ in m.named_parameters()]
    assert names == [str(n) for n in g13["seed/names"]]
    s = np.array([float(p.detach().double().sum()) for p in m.parameters()])
    a = np.array([float(p.detach().double().abs().sum()) for p in m.parameters()])
    assert np.array_equal(s, g13["seed/sum"]) and np.array_equal(a, g13["seed/abs"])
    w = m.face_head.upsample.stages[0].conv.weight
    assert torch.equal(w[0], w[3]) and not torch.equal(w[0], w[4])          # ICNR survived


def test_stages_flags_counts_and_groups(g13, capsys):
    from src.models import TrainingStage, TransferSRModel, create_transfer_model
    m = create_transfer_model()
    assert isinstance(m, TransferSRModel) and m.current_stage is TrainingStage.STAGE1_HEAD_ONLY
    total = int(g13["default/total_params"])
    for stage in (TrainingStage.STAGE1_HEAD_ONLY, TrainingStage.STAGE2_PARTIAL_FINETUNE,
                  TrainingStage.STAGE3_FULL_FINETUNE, TrainingStage.STAGE2_PARTIAL_FINETUNE):
        m.set_training_stage(stage)
        assert stage.name in capsys.readouterr().out
        pre = f"default/stage{stage.value}/"
        info = m.get_model_info()
        assert info["name"] == "TransferSRModel" and info["current_stage"] == stage.name
        assert info["total_params"] == total and info["trainable_params"] == int(g13[pre + "trainable_params"])
        assert info["frozen_params"] == total - info["trainable_params"]
        assert info["backbone_blocks"] == 16 and info["head_blocks"] == 4
        assert abs(info["size_mb"] - total * 4 / 2 ** 20) < 1e-9
        assert [k for k, p in m.named_parameters() if p.requires_grad] == [str(n) for n in g13[pre + "trainable_names"]]
        groups = m.get_trainable_params()
        assert [sum(p.numel() for p in g["params"]) for g in groups] == list(g13[pre + "group_sizes"])
        assert [float(g["lr"]) for g in groups] == list(g13[pre + "group_lrs"])
        # the quirks: conv_first never trains again; conv_body is frozen exactly while every block is
        assert not m.backbone["conv_first"].weight.requires_grad
        assert m.backbone["conv_body"].weight.requires_grad == (stage is not TrainingStage.STAGE1_HEAD_ONLY)
    m.set_training_stage(TrainingStage.STAGE1_HEAD_ONLY)
    groups = m.get_trainable_params()
    assert len(groups) == 1 and groups[0]["lr"] == 2e-4
    assert all(p.requires_grad for p in m.face_head.parameters())
    assert not any(p.requires_grad for p in m.backbone.parameters())


def test_load_pretrained_maps_rrdbnet(tmp_path, capsys):
    """An RRDBNet state dict wrapped in 'params_ema' -> the backbone: conv_first, conv_body and the
    blocks below backbone_blocks; the file's other entries are dropped and the head is untouched."""
    import rrdb_ref
    from src.models import TransferModelConfig, TransferSRModel, create_transfer_model
    torch.manual_seed(3)
    src = rrdb_ref.RefRRDBNet(num_block=3).state_dict()
    path = tmp_path / "rrdb.pth"
    torch.save({"params_ema": src, "params": {"conv_first.weight": torch.zeros(64, 3, 3, 3)}}, path)
    torch.manual_seed(4)
    plain = TransferSRModel(TransferModelConfig(backbone_blocks=2, head_blocks=1))
    torch.manual_seed(4)
    m = TransferSRModel(TransferModelConfig(backbone_blocks=2, head_blocks=1), str(path))
    assert str(path) in capsys.readouterr().out
    sd = m.state_dict()
    for k, v in sd.items():
        if k.startswith("backbone."):
            assert torch.equal(v, src[k[len("backbone."):]]), k
        else:
            assert torch.equal(v, plain.state_dict()[k]), k
    assert not any(p.requires_grad for p in m.backbone.parameters())
    torch.save({"params": src}, path)
    m2 = create_transfer_model(str(path), backbone_blocks=2, head_blocks=1, precision="bf16")
    assert torch.equal(m2.backbone["body"][1].rdb2.conv3.weight, src["body.1.rdb2.conv3.weight"])
    assert m2.compute_dtype == torch.bfloat16
    torch.save({"params": src, "hook": print}, path)
    with pytest.raises(Exception, match="(?i)weights.only|unsupported global"):   # refused, not unpickled
        TransferSRModel(TransferModelConfig(backbone_blocks=2, head_blocks=1), str(path))


def test_refusals_and_backbone_tie_without_gpu():
    from src.hip import lib as L
    from src.models import FaceSpecificHead, TransferModelConfig, TransferSRModel
    from src.models import transfer as TM
    with pytest.raises(NotImplementedError):
        TransferSRModel(TransferModelConfig(backbone_blocks=1, head_channels=32))
    with pytest.raises(NotImplementedError):
        TransferSRModel(TransferModelConfig(backbone_blocks=1, scale_factor=3))
    with pytest.raises(NotImplementedError):
        FaceSpecificHead(in_channels=128)
    with pytest.raises(ValueError):
        TransferSRModel(TransferModelConfig(backbone_blocks=1), precision="fp8")
    m = TransferSRModel(TransferModelConfig(backbone_blocks=1, head_blocks=1))
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(1, 3, 8, 8))
    # the tie every forward with a trainable backbone parameter goes through
    x = torch.ones(3, requires_grad=True)
    y = TM._BackboneTie.apply(lambda t: t * 2.0, x)
    with pytest.raises(NotImplementedError, match="RRDB backward"):
        y.sum().backward()
    # FEN_EPI_NOSKIP: validated before any launch
    lib = L.load()
    d = L.ConvDesc()
    d.dtype, d.B, d.H, d.W, d.Cin, d.Cout = L.BF16, 1, 16, 16, 64, 3
    d.x = d.w = d.y = d.bias = 0x1000
    d.epi = L.EPI_NOSKIP | L.EPI_BIAS
    assert lib.fen_conv3x3(d, None) == -1                    # not without FEN_EPI_LAST
    d.epi = L.EPI_LAST | L.EPI_NOSKIP | L.EPI_BIAS
    d.clamp = 1
    assert lib.fen_conv3x3(d, None) == -1                    # never clamps
    d.clamp, d.scale = 0, 4
    assert lib.fen_conv3x3(d, None) == -1                    # takes no skip geometry
    d.scale, d.lr = 0, 0x1000
    assert lib.fen_conv3x3(d, None) == -1
    d.lr, d.Cout = None, 5
    assert lib.fen_conv3x3(d, None) == -1
    d.Cout, d.epi = 3, L.EPI_LAST | L.EPI_NOSKIP | L.EPI_BIAS | L.EPI_POOL
    d.part = 0x1000
    assert lib.fen_conv3x3(d, None) == -2
    d.epi, d.H, d.hr, d.dout, d.loss_part = L.EPI_LAST | L.EPI_NOSKIP | L.EPI_BIAS, 20, 0x1000, 0x1000, 0x1000
    assert lib.fen_conv3x3(d, None) == -2                    # the L1 epilogue on ragged tiles
    d.hr, d.epi = None, L.EPI_LAST | L.EPI_NOSKIP
    assert lib.fen_conv3x3(d, None) == -2                    # the fallback conv needs a bias

"""Transfer model (TransferSRModel) on the HIP path: the reference's recorded numbers (the head's
input, the output, the stage-1 gradients), ragged / multi-tile shapes and the buffer rotation
against the plain-torch restatement, the 16-bit precisions against their CPU replay, head-only
training (gradients, frozen backbone, weight refresh, the stage-2 refusal), the no-skip conv_last
kernel through the C-ABI, graph capture and evaluate.py --model transfer."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transfer_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FP32_BOUND = 1e-3          # the project's fp32 bound, relative to the output's range
# fp32 module gradients, per parameter, relative 2-norm: the bound test_gpu_module.py (lines 68-69,
# 213) and test_gpu_train64.py (docstring line 11, line 102) apply to conv weights and biases,
# PReLU slopes and the gate's linear layers alike
GRAD_BOUND = 1e-4
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def g13(golden):
    return transfer_ref.load_g13(golden)


@pytest.fixture(scope="module")
def gsd(g13):
    return transfer_ref.golden_state_dict(g13)


@pytest.fixture(scope="module")
def ref_net(gsd):
    return transfer_ref.from_state_dict(gsd, 1, 2)


def _hip_net(sd, backbone_blocks, head_blocks, precision):
    from src.models import TransferModelConfig, TransferSRModel
    net = TransferSRModel(TransferModelConfig(backbone_blocks=backbone_blocks, head_blocks=head_blocks),
                          precision=precision)
    net.load_state_dict(sd)
    return net.to(DEV)


def _random_sd(backbone_blocks, head_blocks, seed):
    torch.manual_seed(seed)
    ref = transfer_ref.RefTransfer(backbone_blocks, head_blocks)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, torch.nn.PReLU):
                m.weight.copy_(0.1 + 0.3 * torch.rand(m.weight.shape, generator=gen))
                m.weight[::5] = -0.1
    return {k: v.clone() for k, v in ref.state_dict().items()}


def _rel(got, want):
    return float((got.detach().cpu().float() - want).abs().max() / want.abs().max())


def test_golden_fp32(g13, gsd):
    """max|d| <= 1e-3 max|ref| against the reference's recorded fp32 run: the head's input first
    (a failure names backbone or head), then the output."""
    net = _hip_net(gsd, 1, 2, "fp32").eval()
    x = torch.from_numpy(g13["x"]).to(DEV)
    with torch.no_grad():
        e0 = _rel(net._run_backbone(x), torch.from_numpy(g13["feat"]))
        print(f"fp32 golden: feat rel err {e0:.3e}")
        assert e0 <= FP32_BOUND, f"the backbone is off: {e0}"
        out = net(x)
    assert out.shape == (2, 3, 48, 80) and out.dtype == torch.float32
    e1 = _rel(out, torch.from_numpy(g13["out"]))
    print(f"fp32 golden: out rel err {e1:.3e}")
    assert e1 <= FP32_BOUND, f"the head is off: {e1}"


@pytest.fixture(scope="module")
def nets_small():
    sd = _random_sd(1, 2, 5)
    return _hip_net(sd, 1, 2, "fp32").eval(), transfer_ref.from_state_dict(sd, 1, 2)


@pytest.mark.parametrize("shape", [(1, 3, 16, 16), (1, 3, 7, 10), (3, 3, 20, 36)])
def test_shapes_fp32(nets_small, shape):
    """One full tile; smaller than a tile and odd both ways; several tiles and the batch stride."""
    net, ref = nets_small
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(sum(shape)))
    with torch.no_grad():
        want = ref(x)
        got = net(x.to(DEV))
    assert got.shape == want.shape
    e = _rel(got, want)
    print(f"fp32 {shape}: rel err {e:.3e}")
    assert e <= FP32_BOUND, e


def test_two_backbone_blocks_fp32():
    """backbone_blocks = 2: the rotation of the dense-block buffers across RRDBs."""
    sd = _random_sd(2, 1, 7)
    x = torch.rand(1, 3, 12, 20, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        e = _rel(_hip_net(sd, 2, 1, "fp32").eval()(x.to(DEV)), transfer_ref.from_state_dict(sd, 2, 1)(x))
    print(f"fp32 backbone_blocks=2: rel err {e:.3e}")
    assert e <= FP32_BOUND, e


@pytest.mark.parametrize("shape", ["golden", (1, 3, 16, 64)])
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_16bit_against_replay(g13, gsd, ref_net, precision, shape):
    """The rule test_gpu_rrdb.py states: the HIP output may be as far from the CPU replay (weights
    and every stored activation rounded to the 16-bit type, float64 sums) as twice the replay's own
    distance from the fp32 reference.  On the golden input (ragged: the per-op kernels and the
    fallback conv_last) and on a 16 x 64 input (the strip-resident head and the streaming no-skip
    conv_last)."""
    dtype = DTYPES[precision]
    if shape == "golden":
        x, ref = torch.from_numpy(g13["x"]), torch.from_numpy(g13["out"])
    else:
        x = torch.rand(*shape, generator=torch.Generator().manual_seed(9))
        with torch.no_grad():
            ref = ref_net(x)
    rep = transfer_ref.replay(ref_net, x, dtype)
    with torch.no_grad():
        out = _hip_net(gsd, 1, 2, precision).eval()(x.to(DEV)).cpu()
    assert out.dtype == torch.float32 and out.shape == ref.shape
    e_replay = float((rep - ref).abs().max())
    e_hip = float((out - rep).abs().max())
    print(f"{precision} {shape}: max|hip - replay| {e_hip:.3e}, max|replay - fp32 ref| {e_replay:.3e}, "
          f"max|ref| {float(ref.abs().max()):.4f}")
    assert e_hip <= 2 * e_replay, (e_hip, e_replay)


def _stage1_grads(net, x, hr):
    net.train()
    net.zero_grad()
    out = net(x.to(DEV))
    loss = (out - hr.to(DEV)).abs().mean()
    loss.backward()
    torch.cuda.synchronize()
    return out.detach(), {k: p.grad for k, p in net.named_parameters()}


def test_stage1_gradients_fp32(g13, gsd):
    """loss.backward() in STAGE1_HEAD_ONLY: every face_head.* gradient against the reference's
    recorded one, per parameter, at GRAD_BOUND; every backbone gradient stays None."""
    net = _hip_net(gsd, 1, 2, "fp32")
    out, grads = _stage1_grads(net, torch.from_numpy(g13["x"]), torch.from_numpy(g13["hr"]))
    assert _rel(out, torch.from_numpy(g13["out"])) <= FP32_BOUND
    worst = 0.0
    for k, g in grads.items():
        if k.startswith("backbone."):
            assert g is None, k
            continue
        want = torch.from_numpy(g13["g/" + k]).double()
        assert g is not None and g.shape == want.shape, k
        rel = float((g.cpu().double() - want).norm() / want.norm())
        worst = max(worst, rel)
        print(f"fp32 grad {k}: rel {rel:.2e}")
        assert rel <= GRAD_BOUND, (k, rel)
    print(f"fp32 stage-1 gradients: worst rel {worst:.2e}")


def test_stage1_gradients_bf16(g13, gsd, ref_net):
    """bf16 against the 16-bit replay of the step (transfer_ref.replay_grads), per parameter, by
    the 2x rule: |hip - replay| <= 2 |replay - fp32 reference| in the 2-norm."""
    x, hr = torch.from_numpy(g13["x"]), torch.from_numpy(g13["hr"])
    rep = transfer_ref.replay_grads(ref_net, x, hr, torch.bfloat16)
    _, grads = _stage1_grads(_hip_net(gsd, 1, 2, "bf16"), x, hr)
    bad = {}
    for k, r in rep.items():
        ref = torch.from_numpy(g13["g/" + k])
        e_replay = float((r - ref).norm())
        e_hip = float((grads[k].cpu().float() - r).norm())
        print(f"bf16 grad {k}: |hip - replay| {e_hip:.3e}, |replay - ref| {e_replay:.3e}, |ref| {float(ref.norm()):.3e}")
        if not e_hip <= 2 * e_replay:
            bad[k] = (e_hip, e_replay)
    assert not bad, bad
    assert all(g is None for k, g in grads.items() if k.startswith("backbone."))


def test_fp16_trains_nowhere_and_weight_refresh(gsd, g13):
    """fp16 is inference-only; one AdamW step over get_trainable_params() changes the output (the
    packed weights are refreshed) and leaves the backbone's parameters as they were."""
    x, hr = torch.from_numpy(g13["x"]), torch.from_numpy(g13["hr"])
    net16 = _hip_net(gsd, 1, 2, "fp16").train()
    with pytest.raises(NotImplementedError, match="inference-only"):
        net16(x.to(DEV)).sum().backward()
    net = _hip_net(gsd, 1, 2, "bf16")
    opt = torch.optim.AdamW(net.get_trainable_params())
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["lr"] == 2e-4
    before, _ = _stage1_grads(net, x, hr)
    back = {k: v.clone() for k, v in net.backbone.state_dict().items()}
    opt.step()
    with torch.no_grad():
        after = net(x.to(DEV))
    assert float((after - before).abs().max()) > 1e-4
    assert all(torch.equal(v, back[k]) for k, v in net.backbone.state_dict().items())


def test_stage2_backward_refuses():
    """Stage 2 unfreezes the last 4 blocks (so 4 of them here) and conv_body: flags, parameter
    groups and the forward work; the backward names what is missing."""
    from src.models import TrainingStage
    sd = _random_sd(4, 1, 11)
    net = _hip_net(sd, 4, 1, "fp32").train()
    net.set_training_stage(TrainingStage.STAGE2_PARTIAL_FINETUNE)
    assert net.backbone["conv_body"].weight.requires_grad and len(net.get_trainable_params()) == 2
    x = torch.rand(1, 3, 8, 8, generator=torch.Generator().manual_seed(6))
    out = net(x.to(DEV))
    with torch.no_grad():
        assert _rel(out, transfer_ref.from_state_dict(sd, 4, 1)(x)) <= FP32_BOUND
    with pytest.raises(NotImplementedError, match="RRDB backward"):
        out.mean().backward()


# ---------------------------------------------------------------- the no-skip conv_last kernel
def _conv_last_noskip(dtype, feat, w, b, hr=None, l1_scale=0.0, clamp=0):
    """One fen_conv3x3(FEN_EPI_LAST | FEN_EPI_NOSKIP) launch on sentinel-filled outputs."""
    from src.hip import lib as L
    lib = L.load()
    code = L.dtype_code(dtype)
    B, C, H, W = feat.shape
    stream = torch.cuda.current_stream().cuda_stream
    x = feat.permute(0, 2, 3, 1).contiguous().to(DEV).to(dtype)
    wd, bd = w.to(DEV).contiguous(), b.to(DEV).contiguous()
    wpk = torch.empty(lib.fen_packed_elems(0, 3, C), dtype=dtype, device=DEV)
    L.check(lib.fen_pack_conv_w(code, 0, 3, C, wd.data_ptr(), wpk.data_ptr(), stream), "pack")
    out = torch.full((B, 3, H, W), float("nan"), device=DEV)
    d = L.ConvDesc()
    d.dtype, d.B, d.H, d.W, d.Cin, d.Cout = code, B, H, W, C, 3
    d.x, d.w, d.bias, d.y = x.data_ptr(), wpk.data_ptr(), bd.data_ptr(), out.data_ptr()
    d.epi, d.clamp = L.EPI_LAST | L.EPI_NOSKIP | L.EPI_BIAS, clamp
    dout = part = hrd = None
    if hr is not None:
        hrd = hr.to(DEV).contiguous()
        dout = torch.full((B, H, W, 16), float("nan"), dtype=dtype, device=DEV)
        part = torch.full((B * (H // 16) * (W // 16),), float("nan"), device=DEV)
        d.hr, d.dout, d.loss_part, d.l1_scale = hrd.data_ptr(), dout.data_ptr(), part.data_ptr(), l1_scale
    rc = lib.fen_conv3x3(ctypes.byref(d), stream)
    torch.cuda.synchronize()
    return rc, out, dout, part


@pytest.fixture(scope="module")
def cl_case():
    g = torch.Generator().manual_seed(17)
    w = torch.randn(3, 64, 3, 3, generator=g) * 0.05
    b = torch.tensor([0.3, -0.2, 0.1])
    feats = {s: torch.randn(2, 64, *s, generator=g) for s in ((32, 48), (20, 36))}
    return w, b, feats


@pytest.mark.parametrize("hw", [(32, 48), (20, 36)])
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_conv_last_noskip_abi(cl_case, precision, hw):
    """B=2 at 32x48 (whole tiles: 16-bit runs the streaming kernel) and at the ragged 20x36 (the
    fen_rrdb_conv fallback), every dtype, outputs pre-filled with NaN.  fp32: conv2d at the fp32
    bound.  16-bit: against the same conv on the rounded operands in float64, where only the
    accumulation is left: 64 * 9 fp32 products summed in another order, bounded by
    sqrt(576) * 2^-24 * sum|w x| <= 1e-5 max|ref| here; checked at 1e-4.  Two runs give the same
    bits."""
    dtype = DTYPES[precision]
    w, b, feats = cl_case
    feat = feats[hw]
    rc, out, _, _ = _conv_last_noskip(dtype, feat, w, b)
    assert rc == 0
    assert bool(torch.isfinite(out).all()), "an output element was not written"
    if precision == "fp32":
        want = torch.nn.functional.conv2d(feat, w, b, padding=1)
        tol = FP32_BOUND
    else:
        want = torch.nn.functional.conv2d(feat.to(dtype).double(), w.to(dtype).double(), b.double(), padding=1).float()
        tol = 1e-4
    e = _rel(out, want)
    print(f"conv_last no-skip {precision} {hw}: rel err {e:.3e}")
    assert e <= tol, e
    rc2, out2, _, _ = _conv_last_noskip(dtype, feat, w, b)
    assert rc2 == 0 and torch.equal(out, out2)
    # no clamp in any mode: values outside [0, 1] survive
    assert float(out.min()) < 0.0 and float(out.max()) > 1.0


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_conv_last_noskip_l1_epilogue(cl_case, precision):
    """With hr given (training): dout = sign(out - hr) * l1_scale exactly wherever |out - hr|
    exceeds the output's error bound (1e-4 max|out|, as above), channels 3..15 of dout are zero
    (the zero-padded NHWC16 layout of fen_conv_desc.dout), the tile sums add up to the L1 computed
    from `out`, and a second run gives the same bits."""
    dtype = DTYPES[precision]
    w, b, feats = cl_case
    feat = feats[(32, 48)]
    hr = torch.rand(2, 3, 32, 48, generator=torch.Generator().manual_seed(23))
    scale = 2.0 ** -10                                   # exact in both 16-bit formats
    rc, out, dout, part = _conv_last_noskip(dtype, feat, w, b, hr=hr, l1_scale=scale)
    assert rc == 0 and bool(torch.isfinite(out).all())
    plain = _conv_last_noskip(dtype, feat, w, b)[1]
    assert torch.equal(out, plain)                      # the epilogue does not change the output
    diff = out.cpu() - hr
    d = dout.float().cpu()
    assert bool(torch.isfinite(d).all()) and float(d[..., 3:].abs().max()) == 0.0
    got = d[..., :3].permute(0, 3, 1, 2)
    sure = diff.abs() > 1e-4 * float(out.abs().max())
    want = torch.sign(diff) * torch.tensor(scale).to(dtype).float()
    assert torch.equal(got[sure], want[sure])
    assert bool(((got == 0) | (got.abs() == want.abs().max())).all())
    l1 = float(diff.double().abs().sum())
    assert part.shape == (2 * 2 * 3,) and bool(torch.isfinite(part).all())
    assert abs(float(part.double().sum()) - l1) <= 1e-5 * l1
    per_tile = diff.abs().double().reshape(2, 3, 2, 16, 3, 16).sum(dim=(1, 3, 5)).reshape(-1)
    assert float((part.cpu().double() - per_tile).abs().max()) <= 1e-5 * float(per_tile.max())
    again = _conv_last_noskip(dtype, feat, w, b, hr=hr, l1_scale=scale)
    assert torch.equal(again[2].view(torch.int16), dout.view(torch.int16)) and torch.equal(again[3], part)


def test_conv_last_noskip_refusals_launch_nothing(cl_case):
    """A refused descriptor leaves the NaN-filled outputs untouched: a clamp request, and the L1
    epilogue on a shape the streaming kernel does not take."""
    w, b, feats = cl_case
    rc, out, _, _ = _conv_last_noskip(torch.bfloat16, feats[(32, 48)], w, b, clamp=1)
    assert rc == -1 and bool(torch.isnan(out).all())
    hr = torch.rand(2, 3, 20, 36)
    rc, out, dout, part = _conv_last_noskip(torch.bfloat16, feats[(20, 36)], w, b, hr=hr, l1_scale=1.0)
    assert rc == -2 and bool(torch.isnan(out).all()) and bool(torch.isnan(dout.float()).all())
    assert bool(torch.isnan(part).all())


def test_deterministic_and_capturable(gsd):
    """Eager, captured and replayed twice: the same bits (16 x 64: the strip-resident head and the
    streaming conv_last are in the graph)."""
    net = _hip_net(gsd, 1, 2, "fp16").eval()
    x = torch.rand(2, 3, 16, 64, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        a = net(x).clone()
        assert torch.equal(a, net(x))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            net(x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = net(x)
        for _ in range(2):
            y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, a)


def test_evaluate_cli_transfer(tmp_path, capsys, gsd):
    """scripts/evaluate.py --model transfer, in process, on a checkpoint saved here."""
    import importlib.util
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "fen_evaluate_cli", os.path.join(root, "face-super-resolution_amd", "scripts", "evaluate.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    ckpt = tmp_path / "transfer.pth"
    torch.save({"model_state_dict": gsd, "config": {"backbone_blocks": 1, "head_blocks": 2}}, ckpt)
    out = tmp_path / "res.json"
    assert cli.main(["--model", "transfer", "--checkpoint", str(ckpt), "--synthetic", "3", "--hr-size", "32",
                     "--batch-size", "2", "--precision", "fp16", "--json", str(out)]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["model"] == "transfer" and res["num_images"] == 3 and np.isfinite(res["psnr_mean"])
    per = json.load(open(out))["per_image"]
    assert len(per["psnr"]) == 3 and len(per["ssim"]) == 3
    assert abs(np.mean(per["psnr"]) - res["psnr_mean"]) < 1e-9
    with pytest.raises(SystemExit):
        cli.parse_args(["--model", "transfer", "--synthetic", "2"])       # needs --checkpoint


def test_train_cli_transfer(tmp_path, capsys):
    """scripts/train.py --model transfer, in process: the reference's model.transfer.* keys, one
    epoch of stage 1 on --synthetic images with CombinedLoss (L1 + perceptual) on the unfused
    Trainer path.  The optimizer holds the model's one parameter group (the head, 2e-4), the head
    moves, the backbone does not and has no gradient, and the checkpoint evaluates."""
    import importlib.util
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "fen_train_cli", os.path.join(root, "face-super-resolution_amd", "scripts", "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cfg = {"project": {"seed": 3}, "data": {"batch_size": 2, "num_workers": 0, "hr_size": 64},
           "model": {"type": "transfer", "transfer": {"backbone_blocks": 1, "freeze_blocks": 1, "head_blocks": 1,
                                                       "head_channels": 64}},
           "loss": {"l1_weight": 1.0, "perceptual_weight": 0.5, "ssim_weight": 0.0},
           "augmentation": {"random_crop": {"hr_patch_size": 64}},
           "training": {"epochs": 1, "mixed_precision": False, "scheduler": {"type": "cosine"}},
           "checkpoint": {"save_dir": str(tmp_path / "ck"), "save_every": 1}}
    path = tmp_path / "transfer.yaml"
    path.write_text(yaml.safe_dump(cfg))
    made = {}
    real = cli.Trainer

    def spy(model, *a, **k):
        made["before"] = {n: p.detach().clone() for n, p in model.named_parameters()}
        made["trainer"] = real(model, *a, **k)
        return made["trainer"]
    cli.Trainer = spy
    cli.main(["--config", str(path), "--synthetic", "4", "--precision", "bf16", "--no-wandb"])
    tr = made["trainer"]
    assert type(tr.model).__name__ == "TransferSRModel" and tr.fused_l1 is None and tr.global_step == 2
    assert len(tr.optimizer.param_groups) == 1 and tr.optimizer.defaults["lr"] != 2e-4
    n_head = sum(1 for _ in tr.model.face_head.parameters())
    assert len(tr.optimizer.param_groups[0]["params"]) == n_head
    assert abs(tr.optimizer.param_groups[0]["initial_lr"] - 2e-4) < 1e-12
    moved = 0
    for n, p in tr.model.named_parameters():
        same = torch.equal(p.detach().cpu(), made["before"][n].cpu())
        if n.startswith("backbone."):
            assert same and p.grad is None, n
        else:
            moved += not same
    assert moved >= n_head - 2, moved           # (a parameter whose gradient is exactly zero may stay)
    assert np.isfinite(tr.training_history["train_loss"][0]) and np.isfinite(tr.training_history["val_psnr"][0])
    ck = torch.load(tmp_path / "ck" / "final_model.pth", map_location="cpu", weights_only=True)
    assert ck["model_config"]["backbone_blocks"] == 1 and ck["optimizer_state_dict"]["state"]
    spec2 = importlib.util.spec_from_file_location(
        "fen_evaluate_cli2", os.path.join(root, "face-super-resolution_amd", "scripts", "evaluate.py"))
    ev = importlib.util.module_from_spec(spec2)
    spec2.loader.exec_module(ev)
    capsys.readouterr()
    assert ev.main(["--model", "transfer", "--checkpoint", str(tmp_path / "ck" / "final_model.pth"), "--synthetic",
                    "2", "--hr-size", "32", "--batch-size", "2", "--precision", "bf16"]) == 0

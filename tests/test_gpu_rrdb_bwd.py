"""The dense blocks' backward on the GPU (stages 2 and 3 of the transfer model, train_backbone=True):
fen_rrdb_dgrad / fen_rrdb_wgrad / fen_rrdb_block_bwd alone against their float64 restatements
(tests/rrdb_bwd_ref.py), the module's stage-3 gradients against the reference's recorded ones
(tests/golden/g14_*), stage 2 and the stage switch against the restatement's autograd, bf16 against
the 16-bit replay, the optimizer step with refreshed packs, determinism and graph capture, and
scripts/train.py --transfer-stage 2."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rrdb_bwd_ref  # noqa: E402
import transfer_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FP32_BOUND = 1e-3          # the project's fp32 bound, relative to the compared slice's range
GRAD_BOUND = 1e-4          # the project's fp32 gradient bound, per tensor, relative 2-norm
SENTINEL = 777.0


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _pack2(lib, L, w, dtype=torch.float32):
    """OIHW fp32 (CPU) -> the mode-2 pack on the GPU."""
    wd = w.float().contiguous().to(DEV)
    co, ci = int(w.shape[0]), int(w.shape[1])
    out = torch.empty(lib.fen_packed_elems(2, co, ci), dtype=dtype, device=DEV)
    L.check(lib.fen_pack_conv_w(L.dtype_code(dtype), 2, co, ci, wd.data_ptr(), out.data_ptr(),
                                torch.cuda.current_stream().cuda_stream), "pack")
    return out


# ------------------------------------------------------------------------ 1. fen_rrdb_dgrad
PAIRS = [(32, 64), (32, 96), (32, 128), (32, 160), (64, 192)]
SHAPES = [(1, 7, 10), (1, 20, 36), (3, 16, 16)]
#          accumulate, act, r1 (s1), r2 (s2), s
CONFIGS = {"acc_act_r1_r2": (1, True, 0.5, 1.0, 0.3),
           "plain_scaled": (0, False, None, None, 1.7),
           "store_act_r1": (0, True, 0.2, None, 0.04),
           "acc_r2": (1, False, None, 1.0, 1.0)}


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pair", PAIRS)
def test_dgrad_launch_fp32(pair, shape, cfg):
    """One launch against its float64 restatement, per output channel slice (x, x1, .., x4):
    max|d| <= 1e-3 of the slice's max|ref|.  dx has 208 channels per pixel: [Cout, 208) -- which
    holds the dy slice when the launch is in place -- is sentinel-filled and must keep its bits."""
    from src.hip import lib as L
    lib = L.load()
    cin, cout = pair
    B, H, W = shape
    accumulate, use_act, s1, s2, s = CONFIGS[cfg]
    gen = torch.Generator().manual_seed(cin + cout + sum(shape))
    STR = 208
    dx0 = torch.randn(B, H, W, STR, generator=gen, dtype=torch.float64)
    dx0[..., cout:] = SENTINEL
    inplace = cin == 32
    dy = torch.randn(B, H, W, cin, generator=gen, dtype=torch.float64).float().double()
    if inplace:
        dx0[..., cout:cout + cin] = dy
    dx0 = dx0.float().double()
    w = (torch.randn(cin, cout, 3, 3, generator=gen) * 0.1).double()
    r1 = torch.randn(B, H, W, 64, generator=gen).double() if s1 is not None else None
    r2 = torch.randn(B, H, W, 192, generator=gen).double() if s2 is not None else None
    act = torch.randn(B, H, W, 192, generator=gen).double() if use_act else None
    want = rrdb_bwd_ref.dgrad_launch(_nchw(dx0), _nchw(dy), w, cout, accumulate, s,
                                     r1=None if r1 is None else _nchw(r1), s1=s1 or 0.0,
                                     r2=None if r2 is None else _nchw(r2[..., :64]), s2=s2 or 0.0,
                                     act=None if act is None else _nchw(act))
    want = _nhwc(want)

    dxd = dx0.float().to(DEV)
    dyd = dxd if inplace else dy.float().to(DEV)
    hold = [t.float().to(DEV) if t is not None else None for t in (r1, r2, act)]
    wpk = _pack2(lib, L, w)
    d = L.RrdbDgradDesc()
    d.dtype, d.B, d.H, d.W, d.Cin, d.Cout = L.F32, B, H, W, cin, cout
    d.dy, d.dy_stride, d.dy_off, d.w = dyd.data_ptr(), (STR if inplace else cin), (cout if inplace else 0), wpk.data_ptr()
    d.dx, d.dx_stride, d.accumulate, d.s = dxd.data_ptr(), STR, accumulate, s
    if r1 is not None:
        d.r1, d.r1_stride, d.s1 = hold[0].data_ptr(), 64, s1
    if r2 is not None:
        d.r2, d.r2_stride, d.s2 = hold[1].data_ptr(), 192, s2
    if act is not None:
        d.act, d.act_stride = hold[2].data_ptr(), 192
    before = dxd.clone()
    L.check(lib.fen_rrdb_dgrad(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "rrdb_dgrad")
    torch.cuda.synchronize()
    got = dxd.cpu().double()
    assert torch.equal(dxd[..., cout:], before[..., cout:]), "channels past Cout (the dy slice, the sentinels) changed"
    worst_abs = worst_norm = 0.0
    for c0 in [0] + list(range(64, cout, 32)):
        c1 = 64 if c0 == 0 else c0 + 32
        ref = want[..., c0:c1]
        err = float((got[..., c0:c1] - ref).abs().max() / ref.abs().max())
        worst_abs = max(worst_abs, err)
        worst_norm = max(worst_norm, float((got[..., c0:c1] - ref).norm() / ref.norm()))
        assert err <= FP32_BOUND, (c0, err)
    print(f"dgrad {pair} {shape} {cfg}: worst slice max-rel {worst_abs:.2e}, worst 2-norm ratio {worst_norm:.2e}")


# ------------------------------------------------------------------------ 2. fen_rrdb_wgrad
@pytest.mark.parametrize("cin,cout", [(64, 32), (96, 32), (128, 32), (160, 32), (192, 64), (64, 64)])
def test_wgrad_launch_fp32(cin, cout):
    """Both operands at pixel stride 192, dy from a nonzero channel offset, scale 0.2, accumulated
    onto a prefilled dw / db; B = 2 at 20 x 36 (six tiles, ragged both ways).  Relative 2-norm
    <= GRAD_BOUND per tensor, and a second run gives the same bits."""
    from src.hip import lib as L
    lib = L.load()
    B, H, W = 2, 20, 36
    gen = torch.Generator().manual_seed(cin * 3 + cout)
    xb = torch.randn(B, H, W, 192, generator=gen)
    yb = torch.randn(B, H, W, 192, generator=gen)
    off = 96 if cout == 32 else 128
    dw0 = torch.randn(cout, cin, 3, 3, generator=gen)
    db0 = torch.randn(cout, generator=gen)
    dw, db = rrdb_bwd_ref.wgrad_launch(_nchw(xb[..., :cin]).double(), _nchw(yb[..., off:off + cout]).double(), 0.2)
    want_w, want_b = dw + dw0.double(), db + db0.double()
    xd, yd = xb.to(DEV), yb.to(DEV)
    outs = []
    for _ in range(2):
        dwd, dbd = dw0.to(DEV), db0.to(DEV)
        d = L.RrdbWgradDesc()
        d.dtype, d.B, d.H, d.W, d.Cin, d.Cout = L.F32, B, H, W, cin, cout
        d.x, d.x_stride, d.dy, d.dy_stride, d.dy_off = xd.data_ptr(), 192, yd.data_ptr(), 192, off
        d.scale, d.dw, d.db, d.accumulate = 0.2, dwd.data_ptr(), dbd.data_ptr(), 1
        work = torch.empty(lib.fen_rrdb_wgrad_work_floats(ctypes.byref(d)), device=DEV)
        d.work = work.data_ptr()
        L.check(lib.fen_rrdb_wgrad(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "rrdb_wgrad")
        torch.cuda.synchronize()
        outs.append((dwd.cpu(), dbd.cpu()))
    ew = float((outs[0][0].double() - want_w).norm() / want_w.norm())
    eb = float((outs[0][1].double() - want_b).norm() / want_b.norm())
    print(f"wgrad Cin {cin} Cout {cout}: dw rel {ew:.2e}, db rel {eb:.2e}")
    assert ew <= GRAD_BOUND and eb <= GRAD_BOUND, (ew, eb)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------ 3. fen_rrdb_block_bwd
@pytest.fixture(scope="module")
def block_case():
    import rrdb_ref
    torch.manual_seed(21)
    blk = rrdb_ref.RefDenseBlock().double()
    gen = torch.Generator().manual_seed(22)
    B, H, W = 2, 12, 20
    x = torch.randn(B, 64, H, W, generator=gen).float().double()
    outer = torch.randn(B, 64, H, W, generator=gen).float().double()
    g = torch.randn(B, 64, H, W, generator=gen).float().double()
    g_rrdb = torch.randn(B, 64, H, W, generator=gen).float().double()
    with torch.no_grad():
        cat = [x]
        for k in range(1, 5):
            cat.append(torch.nn.functional.leaky_relu(getattr(blk, f"conv{k}")(torch.cat(cat, 1)), 0.2))
        buf = torch.cat(cat, 1).float().double()      # what the fp32 forward stores
    return blk, x, outer, g, g_rrdb, buf


def _block_bwd(block_case, third, with_rrdb, weights):
    from src.hip import lib as L
    lib = L.load()
    blk, x, outer, g, g_rrdb, buf = block_case
    B, _, H, W = x.shape
    bufd, gd, grd = _nhwc(buf).float().to(DEV), _nhwc(g).float().to(DEV), _nhwc(g_rrdb).float().to(DEV)
    D = torch.full((B, H, W, 192), float("nan"), device=DEV)
    d = L.RrdbBlockBwdDesc()
    d.dtype, d.B, d.H, d.W, d.num_feat, d.num_grow_ch = L.F32, B, H, W, 64, 32
    d.buf, d.D, d.g, d.g_stride, d.third = bufd.data_ptr(), D.data_ptr(), gd.data_ptr(), 64, int(third)
    if with_rrdb:
        d.g_rrdb, d.g_rrdb_stride = grd.data_ptr(), 64
    packs, G = [], {}
    for k in range(5):
        conv = getattr(blk, f"conv{k + 1}")
        packs.append(_pack2(lib, L, conv.weight.detach()))
        d.wt[k] = packs[-1].data_ptr()
        if weights:
            G[f"conv{k + 1}.weight"] = torch.full(conv.weight.shape, float("nan"), device=DEV)
            G[f"conv{k + 1}.bias"] = torch.full(conv.bias.shape, float("nan"), device=DEV)
            d.dw[k], d.db[k] = G[f"conv{k + 1}.weight"].data_ptr(), G[f"conv{k + 1}.bias"].data_ptr()
    work = torch.empty(lib.fen_rrdb_block_bwd_work_floats(L.F32, B, H, W), device=DEV)
    if weights:
        d.work = work.data_ptr()
    L.check(lib.fen_rrdb_block_bwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "rrdb_block_bwd")
    torch.cuda.synchronize()
    return _nchw(D[..., :64]).cpu().double(), {k: v.cpu().double() for k, v in G.items()}


@pytest.mark.parametrize("kind", ["plain", "third", "first"])
def test_block_bwd_fp32(block_case, kind):
    """A whole dense block at (2, 12, 20) against autograd of the restated block: a plain block, an
    RRDB's third (outer residual: the incoming gradient is scaled) and an RRDB's first (+ g_rrdb).
    The five dw / db and the input gradient within GRAD_BOUND; dw = NULL computes the same input
    gradient, bit for bit."""
    blk, x, outer, g, g_rrdb, _ = block_case
    xin = x.clone().requires_grad_(True)
    blk.zero_grad()
    y = blk(xin, outer=outer if kind == "third" else None)
    y.backward(g)
    want_dx = xin.grad + (g_rrdb if kind == "first" else 0)
    dx, G = _block_bwd(block_case, kind == "third", kind == "first", True)
    e = float((dx - want_dx).norm() / want_dx.norm())
    print(f"block_bwd {kind}: dx rel {e:.2e}")
    assert e <= GRAD_BOUND, e
    for k, p in blk.named_parameters():
        rel = float((G[k] - p.grad).norm() / p.grad.norm())
        print(f"block_bwd {kind} {k}: rel {rel:.2e}")
        assert rel <= GRAD_BOUND, (k, rel)
    dx2, _ = _block_bwd(block_case, kind == "third", kind == "first", False)
    assert torch.equal(dx, dx2)


# ------------------------------------------------------------------------ the module
@pytest.fixture(scope="module")
def g13(golden):
    return transfer_ref.load_g13(golden)


@pytest.fixture(scope="module")
def g14(golden):
    return rrdb_bwd_ref.load_g14(golden)


@pytest.fixture(scope="module")
def gsd(g13):
    return transfer_ref.golden_state_dict(g13)


@pytest.fixture(scope="module")
def ref_net(gsd):
    return transfer_ref.from_state_dict(gsd, 1, 2)


def _hip_net(sd, backbone_blocks, head_blocks, precision, train_backbone=True):
    from src.models import TransferModelConfig, TransferSRModel
    net = TransferSRModel(TransferModelConfig(backbone_blocks=backbone_blocks, head_blocks=head_blocks),
                          precision=precision, train_backbone=train_backbone)
    net.load_state_dict(sd)
    return net.to(DEV)


def _grads(net, x, hr):
    net.train()
    net.zero_grad()
    out = net(x.to(DEV))
    (out - hr.to(DEV)).abs().mean().backward()
    torch.cuda.synchronize()
    return out.detach(), {k: p.grad for k, p in net.named_parameters()}


def _stage(net, n):
    from src.models import TrainingStage
    net.set_training_stage(TrainingStage(n))
    return net


def test_stage3_gradients_fp32_golden(g13, g14, gsd):
    """Stage 3 on the g13 model: every backbone.* gradient except conv_first's against the
    reference's recorded one (g14) and every face_head.* gradient against g13, relative 2-norm <=
    GRAD_BOUND; conv_first has none; the output is bit-identical to the no_grad forward."""
    net = _stage(_hip_net(gsd, 1, 2, "fp32"), 3)
    x, hr = torch.from_numpy(g13["x"]), torch.from_numpy(g13["hr"])
    out, grads = _grads(net, x, hr)
    with torch.no_grad():
        assert torch.equal(out, net(x.to(DEV)))
    assert grads["backbone.conv_first.weight"] is None and grads["backbone.conv_first.bias"] is None
    seen = 0
    for k, g in grads.items():
        if k.startswith("backbone.conv_first."):
            continue
        want = torch.from_numpy((g14 if k.startswith("backbone.") else g13)["g/" + k]).double()
        assert g is not None and g.shape == want.shape, k
        rel = float((g.cpu().double() - want).norm() / want.norm())
        print(f"fp32 stage-3 grad {k}: rel {rel:.2e}")
        assert rel <= GRAD_BOUND, (k, rel)
        seen += k.startswith("backbone.")
    assert seen == 32


@pytest.mark.parametrize("shape", [(1, 3, 8, 8), (2, 3, 20, 12)])
def test_stage2_then_stage3_fp32(shape):
    """5 backbone blocks, 1 head block: stage 2 gives blocks 1..4 and conv_body gradients within
    GRAD_BOUND of the restatement's autograd, block 0 and conv_first none, and the frozen prefix
    is not saved (3 x 4 block buffers + the body's output).  Then stage 3 on the same model: block
    0 has a gradient within the same bound."""
    from src.hip import rrdb as R
    torch.manual_seed(31)
    ref = transfer_ref.RefTransfer(5, 1).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.half().float())
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.rand(*shape, generator=gen)
    hr = torch.rand(shape[0], 3, 4 * shape[2], 4 * shape[3], generator=gen)
    net = _hip_net(sd, 5, 1, "fp32")
    seen = []
    real = R.trunk

    def spy(*a, **k):
        res = real(*a, **k)
        if k.get("save_from") is not None:
            seen.append((k["save_from"], len(res[1]["bufs"])))
        return res
    R.trunk = spy
    try:
        for stage, first in ((2, 1), (3, 0)):
            _stage(net, stage)
            _, grads = _grads(net, x, hr)
            want = rrdb_bwd_ref.stage_grads(ref, x, hr, first)
            assert seen[-1] == (first, 3 * (5 - first) + 1)
            for k, g in grads.items():
                if k not in want:
                    assert g is None, k
                    continue
                rel = float((g.cpu().double() - want[k]).norm() / want[k].norm())
                assert rel <= GRAD_BOUND, (stage, k, rel)
            assert grads["backbone.conv_first.weight"] is None
            assert (grads["backbone.body.0.rdb1.conv1.weight"] is None) == (stage == 2)
            assert grads["backbone.body.1.rdb1.conv1.weight"] is not None and grads["backbone.conv_body.bias"] is not None
    finally:
        R.trunk = real


def test_stage3_gradients_bf16_replay(g13, g14, gsd, ref_net):
    """bf16 against the 16-bit replay of the step (rrdb_bwd_ref.manual_grads: weights, every stored
    activation and every stored gradient slice -- each read-modify-write of D -- rounded to bf16,
    float64 sums), per parameter, by the 2x rule of test_stage1_gradients_bf16: |hip - replay| <= 2
    |replay - fp32 reference| in the 2-norm.  No parameter is excluded."""
    x, hr = torch.from_numpy(g13["x"]), torch.from_numpy(g13["hr"])
    rep = rrdb_bwd_ref.manual_grads(ref_net, x, hr, 0, torch.bfloat16)
    _, grads = _grads(_stage(_hip_net(gsd, 1, 2, "bf16"), 3), x, hr)
    bad = {}
    assert len(rep) == 32 + len([k for k in grads if k.startswith("face_head.")])
    for k, r in rep.items():
        ref = torch.from_numpy((g14 if k.startswith("backbone.") else g13)["g/" + k]).double()
        e_replay = float((r - ref).norm())
        e_hip = float((grads[k].cpu().double() - r).norm())
        print(f"bf16 grad {k}: |hip - replay| {e_hip:.3e}, |replay - ref| {e_replay:.3e}, |ref| {float(ref.norm()):.3e}")
        if not e_hip <= 2 * e_replay:
            bad[k] = (e_hip, e_replay)
    assert not bad, bad


def test_fp16_and_input_gradient_still_refused(gsd, g13):
    x = torch.from_numpy(g13["x"])
    net16 = _stage(_hip_net(gsd, 1, 2, "fp16"), 3).train()
    with pytest.raises(NotImplementedError, match="inference-only"):
        net16(x.to(DEV)).sum().backward()
    net = _stage(_hip_net(gsd, 1, 2, "fp32"), 3).train()
    with pytest.raises(NotImplementedError, match="LR input"):
        net(x.to(DEV).requires_grad_(True))


def test_adamw_step_stage2_refreshes_packs():
    """One HipAdamW step over get_trainable_params() in stage 2 of a 5-block model (block 0 and
    conv_first frozen): the unfrozen backbone weights and the output change, the frozen ones keep
    their bits, and the next forward and backward use refreshed mode-0 and mode-2 packs -- compared
    with a freshly built model loaded from the updated state dict."""
    from src.training.optim import HipAdamW
    torch.manual_seed(41)
    sd = {k: v.clone() for k, v in transfer_ref.RefTransfer(5, 1).state_dict().items()}
    gen = torch.Generator().manual_seed(42)
    x, hr = torch.rand(1, 3, 8, 12, generator=gen), torch.rand(1, 3, 32, 48, generator=gen)
    net = _stage(_hip_net(sd, 5, 1, "bf16"), 2)
    groups = net.get_trainable_params()
    assert [g["lr"] for g in groups] == [2e-5 * 0.1, 2e-5]      # backbone, head (transfer.py:271-304)
    for g in groups:
        g["lr"] = g["lr"] * 1e3          # a step large enough to show in bf16
    opt = HipAdamW(groups, weight_decay=0.0)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    out0, _ = _grads(net, x, hr)
    opt.step()
    torch.cuda.synchronize()
    after = net.state_dict()
    for k, v in after.items():
        frozen = k.startswith(("backbone.conv_first.", "backbone.body.0."))
        assert torch.equal(v, before[k]) == frozen, k
    out1, g1 = _grads(net, x, hr)
    assert float((out1 - out0).abs().max()) > 0
    fresh = _stage(_hip_net({k: v.cpu() for k, v in after.items()}, 5, 1, "bf16"), 2)
    out2, g2 = _grads(fresh, x, hr)
    assert torch.equal(out1, out2)
    for k, g in g1.items():
        assert (g is None and g2[k] is None) or torch.equal(g, g2[k]), k


def test_deterministic_and_capturable(gsd, g13):
    """Two stage-3 backward passes give the same bits; the builder-level forward and backward
    (rrdb.trunk(save_from=0) + rrdb.trunk_backward) recorded once run eagerly, then captured in a
    graph and replayed, to the same gradients."""
    from src.hip import rrdb as R
    from src.hip.net import Weights
    from src.hip.program import Ctx
    x, hr = torch.from_numpy(g13["x"]), torch.from_numpy(g13["hr"])
    net = _stage(_hip_net(gsd, 1, 2, "bf16"), 3)
    _, ga = _grads(net, x, hr)
    ga = {k: (None if g is None else g.clone()) for k, g in ga.items()}
    _, gb = _grads(net, x, hr)
    for k, g in ga.items():
        assert (g is None and gb[k] is None) or torch.equal(g, gb[k]), k

    params = {k: v.detach() for k, v in net.backbone.named_parameters()}
    ctx = Ctx(torch.bfloat16, torch.device(DEV), record=True)
    W = Weights(params, torch.bfloat16, torch.device(DEV))
    xd = x.to(DEV)
    d_feat = (torch.randn(2, 12, 20, 64, generator=torch.Generator().manual_seed(8)) * 1e-3).to(DEV).bfloat16()
    body, saved = R.trunk(ctx, W, xd, 1, save_from=0)
    G = {k: torch.zeros_like(v) for k, v in params.items() if not k.startswith("conv_first.")}
    R.trunk_backward(ctx, W, G, saved, d_feat)
    ctx.run()
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in G.items()}
    assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in eager.values())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ctx.run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ctx.run()
    for _ in range(2):
        for v in G.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, v in G.items():
            assert torch.equal(v, eager[k]), k


def test_train_cli_transfer_stage2(tmp_path):
    """scripts/train.py --model transfer --transfer-stage 2 --synthetic, in process, two iterations
    on a 4-block model: it finishes, the unfrozen backbone moves, and the checkpoint holds the two
    optimizer groups with the reference's stage-2 learning rates (backbone 2e-6, head 2e-5)."""
    import importlib.util
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "fen_train_cli_s2", os.path.join(root, "face-super-resolution_amd", "scripts", "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cfg = {"project": {"seed": 3}, "data": {"batch_size": 2, "num_workers": 0, "hr_size": 64},
           "model": {"type": "transfer", "transfer": {"backbone_blocks": 4, "freeze_blocks": 4, "head_blocks": 1,
                                                       "head_channels": 64}},
           "loss": {"l1_weight": 1.0, "perceptual_weight": 0.0, "ssim_weight": 0.0},
           "augmentation": {"random_crop": {"hr_patch_size": 64}},
           "training": {"epochs": 1, "mixed_precision": False, "scheduler": {"type": "cosine"}},
           "checkpoint": {"save_dir": str(tmp_path / "ck"), "save_every": 1}}
    path = tmp_path / "transfer2.yaml"
    path.write_text(yaml.safe_dump(cfg))
    made = {}
    real = cli.Trainer

    def spy(model, *a, **k):
        made["before"] = {n: p.detach().clone() for n, p in model.named_parameters()}
        made["trainer"] = real(model, *a, **k)
        return made["trainer"]
    cli.Trainer = spy
    cli.main(["--config", str(path), "--synthetic", "4", "--precision", "bf16", "--no-wandb", "--transfer-stage", "2"])
    tr = made["trainer"]
    assert tr.model.train_backbone and tr.model.current_stage.value == 2 and tr.global_step == 2
    groups = tr.optimizer.param_groups
    assert len(groups) == 2
    assert abs(groups[0]["initial_lr"] - 2e-6) < 1e-15 and abs(groups[1]["initial_lr"] - 2e-5) < 1e-14
    moved = sum(not torch.equal(p.detach().cpu(), made["before"][n].cpu())
                for n, p in tr.model.named_parameters() if n.startswith("backbone.body."))
    assert moved > 0
    assert torch.equal(tr.model.backbone["conv_first"].weight.detach().cpu(), made["before"]["backbone.conv_first.weight"].cpu())
    ck = torch.load(tmp_path / "ck" / "final_model.pth", map_location="cpu", weights_only=True)
    gs = ck["optimizer_state_dict"]["param_groups"]
    assert len(gs) == 2 and abs(gs[0]["initial_lr"] - 2e-6) < 1e-15 and abs(gs[1]["initial_lr"] - 2e-5) < 1e-14

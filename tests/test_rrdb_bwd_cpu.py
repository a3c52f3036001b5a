"""The dense blocks' backward without a GPU: the yardsticks themselves (the restatement against the
reference's recorded stage-3 gradients, the HIP algorithm restated on the CPU against autograd),
the opt-in `train_backbone` keyword, and the new entry points' refusals (validated before any
launch)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rrdb_bwd_ref  # noqa: E402
import transfer_ref  # noqa: E402


@pytest.fixture(scope="module")
def g13(golden):
    return transfer_ref.load_g13(golden)


@pytest.fixture(scope="module")
def g14(golden):
    return rrdb_bwd_ref.load_g14(golden)


@pytest.fixture(scope="module")
def ref_net(g13):
    return transfer_ref.from_state_dict(transfer_ref.golden_state_dict(g13), 1, 2)


def test_restatement_stage3_gradients_reproduce_golden(g13, g14, ref_net):
    """Stage-3 gradients of mean|out - hr| on the g13 model, per backbone parameter: relative 2-norm
    error at most 4x the reference's own fp32-vs-float64 figure (+ 1e-6), the rule of
    test_transfer_cpu.py::test_restatement_gradients_reproduce_golden."""
    grads = rrdb_bwd_ref.stage_grads(ref_net, torch.from_numpy(g13["x"]), torch.from_numpy(g13["hr"]), 0, double=False)
    keys = [k[2:] for k in g14 if k.startswith("g/")]
    assert len(keys) == 3 * 5 * 2 + 2 and "backbone.conv_body.weight" in keys
    assert sorted(str(k) for k in g14["frozen"]) == ["backbone.conv_first.bias", "backbone.conv_first.weight"]
    for k in keys:
        want = torch.from_numpy(g14["g/" + k])
        rel = float((grads[k] - want).norm() / want.norm())
        assert rel <= 4 * float(g14["gerr/" + k]) + 1e-6, (k, rel, float(g14["gerr/" + k]))
    assert not any(k.startswith("backbone.conv_first") for k in grads)


def test_manual_algorithm_equals_autograd():
    """The launch sequence of fen_rrdb_block_bwd / trunk_backward restated in float64 (gradient
    buffers, accumulation order, activation derivative from the stored output, the RRDB-level scale
    and residual) against autograd of the restatement: two RRDBs, the first frozen (stage 2's
    shape of the problem), then none frozen."""
    torch.manual_seed(2)
    net = transfer_ref.RefTransfer(2, 1).eval()
    x = torch.rand(1, 3, 6, 7)
    hr = torch.rand(1, 3, 24, 28)
    for first in (1, 0):
        want = rrdb_bwd_ref.stage_grads(net, x, hr, first)
        got = rrdb_bwd_ref.manual_grads(net, x, hr, first)
        assert sorted(got) == sorted(want)
        for k, w in want.items():
            rel = float((got[k] - w).norm() / w.norm())
            # float64 against float64 with fp32-rounded constants (0.2f, 0.2f * 0.2f): 2^-24 relative
            assert rel <= 1e-6, (first, k, rel)


def test_default_path_and_keyword_without_gpu():
    from src.models import TransferModelConfig, TransferSRModel, create_transfer_model
    from src.models import transfer as TM
    m = TransferSRModel(TransferModelConfig(backbone_blocks=1, head_blocks=1))
    assert m.train_backbone is False
    x = torch.ones(3, requires_grad=True)
    y = TM._BackboneTie.apply(lambda t: t * 2.0, x)
    with pytest.raises(NotImplementedError, match="RRDB backward"):
        y.sum().backward()
    assert "stage 1 (STAGE1_HEAD_ONLY) trains" in TM._NO_RRDB_BACKWARD
    # train_backbone=True constructs without a GPU; the refusals are the same
    t = TransferSRModel(TransferModelConfig(backbone_blocks=1, head_blocks=1), train_backbone=True)
    assert t.train_backbone is True and sorted(t.state_dict()) == sorted(m.state_dict())
    assert create_transfer_model(backbone_blocks=1, head_blocks=1, train_backbone=True).train_backbone is True
    assert create_transfer_model(backbone_blocks=1, head_blocks=1).train_backbone is False
    with pytest.raises(NotImplementedError):
        TransferSRModel(TransferModelConfig(backbone_blocks=1, head_channels=32), train_backbone=True)
    with pytest.raises(NotImplementedError):
        TransferSRModel(TransferModelConfig(backbone_blocks=1, scale_factor=3), train_backbone=True)
    with pytest.raises(ValueError):
        TransferSRModel(TransferModelConfig(backbone_blocks=1), precision="fp8", train_backbone=True)
    with pytest.raises(RuntimeError, match="GPU"):
        t(torch.zeros(1, 3, 8, 8))


def _dgrad_desc(L):
    d = L.RrdbDgradDesc()
    d.dtype, d.B, d.H, d.W, d.Cin, d.Cout = L.BF16, 1, 16, 16, 32, 160
    d.dy, d.dy_stride, d.dy_off, d.w = 0x1000, 192, 160, 0x1000
    d.dx, d.dx_stride, d.accumulate, d.s = 0x1000, 192, 1, 1.0
    return d


def test_dgrad_refusals_without_a_launch():
    from src.hip import lib as L
    lib = L.load()
    EINVAL, EUNSUP = -1, -2

    def rc(**kw):
        d = _dgrad_desc(L)
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.fen_rrdb_dgrad(d, None)
    assert lib.fen_rrdb_dgrad(None, None) == EINVAL
    for p in ("dy", "w", "dx"):
        assert rc(**{p: None}) == EINVAL
    for dim in ("B", "H", "W", "Cin", "Cout"):
        assert rc(**{dim: 0}) == EINVAL
    assert rc(dtype=7) == EINVAL
    assert rc(dtype=L.F16) == EUNSUP                         # fp16 is inference-only
    assert rc(dy=0x1008) == EINVAL and rc(act=0x1004) == EINVAL and rc(r1=0x1002, r1_stride=192) == EINVAL
    assert rc(dy_stride=196) == EINVAL                       # 392 B: no whole 16-B chunks
    assert rc(dy_off=164, dy_stride=200) == EINVAL
    assert rc(dx_stride=128) == EINVAL                       # narrower than Cout
    assert rc(dy_stride=176) == EINVAL                       # the slice does not fit
    assert rc(dy_off=128) == EINVAL                          # same buffer, read range inside the written one
    assert rc(r2=0x2000, r2_stride=32) == EINVAL
    assert rc(act=0x2000, act_stride=128) == EINVAL
    assert rc(Cin=48) == EUNSUP and rc(Cin=64, dy_off=0, dy=0x2000, Cout=200) == EUNSUP and rc(Cout=80) == EUNSUP
    assert rc(Cout=32) == EUNSUP
    assert rc(B=1 << 15, H=1 << 8, W=1 << 8) == EUNSUP       # 2^31 pixels


def test_wgrad_and_block_refusals_without_a_launch():
    from src.hip import lib as L
    lib = L.load()
    EINVAL, EUNSUP = -1, -2

    def wdesc(**kw):
        d = L.RrdbWgradDesc()
        d.dtype, d.B, d.H, d.W, d.Cin, d.Cout = L.F32, 1, 8, 8, 96, 32
        d.x, d.x_stride, d.dy, d.dy_stride, d.dy_off = 0x1000, 192, 0x2000, 192, 96
        d.scale, d.dw, d.db, d.work = 1.0, 0x3000, 0x4000, 0x5000
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert lib.fen_rrdb_wgrad_work_floats(wdesc()) >= 9 * 32 * 96 + 32
    assert lib.fen_rrdb_wgrad_work_floats(wdesc(Cin=80)) == 0 and lib.fen_rrdb_wgrad_work_floats(None) == 0
    assert lib.fen_rrdb_wgrad(None, None) == EINVAL
    for p in ("x", "dy", "dw", "work"):
        assert lib.fen_rrdb_wgrad(wdesc(**{p: None}), None) == EINVAL
    assert lib.fen_rrdb_wgrad(wdesc(H=0), None) == EINVAL
    assert lib.fen_rrdb_wgrad(wdesc(dtype=9), None) == EINVAL
    assert lib.fen_rrdb_wgrad(wdesc(dtype=L.F16), None) == EUNSUP
    assert lib.fen_rrdb_wgrad(wdesc(Cin=80), None) == EUNSUP
    assert lib.fen_rrdb_wgrad(wdesc(Cout=48), None) == EUNSUP
    assert lib.fen_rrdb_wgrad(wdesc(x=0x1004), None) == EINVAL
    assert lib.fen_rrdb_wgrad(wdesc(x_stride=64), None) == EINVAL
    assert lib.fen_rrdb_wgrad(wdesc(dy_off=98), None) == EINVAL
    assert lib.fen_rrdb_wgrad(wdesc(dy_stride=120), None) == EINVAL
    assert lib.fen_rrdb_wgrad(wdesc(B=1 << 15, H=1 << 8, W=1 << 8), None) == EUNSUP

    def bdesc(**kw):
        d = L.RrdbBlockBwdDesc()
        d.dtype, d.B, d.H, d.W, d.num_feat, d.num_grow_ch = L.BF16, 1, 8, 8, 64, 32
        d.buf, d.D, d.g, d.g_stride = 0x1000, 0x2000, 0x3000, 64
        for k in range(5):
            d.wt[k], d.dw[k], d.db[k] = 0x4000, 0x5000, 0x6000
        d.work = 0x7000
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert lib.fen_rrdb_block_bwd_work_floats(L.BF16, 1, 8, 8) >= 9 * 64 * 192 + 64
    assert lib.fen_rrdb_block_bwd(None, None) == EINVAL
    for p in ("buf", "D", "g"):
        assert lib.fen_rrdb_block_bwd(bdesc(**{p: None}), None) == EINVAL
    assert lib.fen_rrdb_block_bwd(bdesc(work=None), None) == EINVAL        # weight gradients need it
    assert lib.fen_rrdb_block_bwd(bdesc(D=0x1000), None) == EINVAL         # D is the forward buffer
    assert lib.fen_rrdb_block_bwd(bdesc(g=0x2000), None) == EINVAL         # g lives in D
    assert lib.fen_rrdb_block_bwd(bdesc(g_rrdb=0x2000), None) == EINVAL
    assert lib.fen_rrdb_block_bwd(bdesc(num_grow_ch=16), None) == EUNSUP
    assert lib.fen_rrdb_block_bwd(bdesc(dtype=L.F16), None) == EUNSUP
    d = bdesc()
    d.wt[2] = None
    assert lib.fen_rrdb_block_bwd(d, None) == EINVAL
    d = bdesc()
    d.dw[1] = None                                                         # a bias gradient without its weight's
    assert lib.fen_rrdb_block_bwd(d, None) == EINVAL

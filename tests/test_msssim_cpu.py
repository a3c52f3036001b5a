"""MS-SSIM without a GPU: the module constructs with the reference's default weights, and
fen_msssim's host checks refuse bad arguments before any launch."""
import torch

EINVAL, EUNSUPPORTED = -1, -2
REF_WEIGHTS = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]      # ssim_loss.py:122, 255


def test_msssim_loss_constructs_on_cpu():
    from src.losses import MSSSIMLoss
    m = MSSSIMLoss()
    assert (m.window_size, m.sigma, m.data_range) == (11, 1.5, 1.0)
    assert "weights" in dict(m.named_buffers())
    assert torch.equal(m.weights, torch.tensor(REF_WEIGHTS))
    m3 = MSSSIMLoss(weights=torch.tensor([0.2, 0.3, 0.5]))
    assert torch.equal(m3.weights, torch.tensor([0.2, 0.3, 0.5]))


def test_msssim_work_floats():
    from src.hip import lib as L
    lib = L.load()
    n = lib.fen_msssim_work_floats(2, 3, 64, 64, 5)
    planes = 2 * 3
    px = sum((64 >> i) ** 2 for i in range(5))
    # the pooled pred / target of levels 1..4 and the five gradient maps at the least
    assert n >= planes * (2 * (px - 64 * 64) + px)
    assert lib.fen_msssim_work_floats(2, 3, 16, 16, 5) == 0
    assert lib.fen_msssim_work_floats(2, 3, 64, 64, 9) == 0


def _call(lib, dtype=0, B=2, C=3, H=64, W=64, pred=16, target=16, win=16, ws=11, weights=16, levels=5, work=16,
          out=16, grad=None, grad_mode=0):
    return lib.fen_msssim(dtype, B, C, H, W, pred, target, win, ws, 1e-4, 9e-4, weights, levels, work, out, grad, 1.0,
                          grad_mode, None)


def test_msssim_refusals_without_gpu():
    """Every refusal of include/fen.h's table is a host check before the first launch (the
    pointers here are never dereferenced)."""
    from src.hip import lib as L
    lib = L.load()
    for name in ("pred", "target", "win", "weights", "work", "out"):
        assert _call(lib, **{name: None}) == EINVAL, name
    assert _call(lib, grad_mode=3) == EINVAL
    assert _call(lib, grad_mode=-1) == EINVAL
    assert _call(lib, grad_mode=1, grad=None) == EINVAL
    assert _call(lib, grad_mode=2, grad=None) == EINVAL
    assert _call(lib, dtype=L.BF16, C=4, grad_mode=2, grad=16) == EINVAL
    assert _call(lib, ws=7) == EUNSUPPORTED
    assert _call(lib, levels=9) == EUNSUPPORTED
    assert _call(lib, levels=0) == EUNSUPPORTED
    assert _call(lib, H=16, W=16) == EUNSUPPORTED
    assert _call(lib, H=64, W=31) == EUNSUPPORTED


def test_msssim_cpu_tensors_raise():
    import pytest
    from src.losses import MSSSIMLoss, ms_ssim
    p = torch.rand(1, 3, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ms_ssim(p, p)
    with pytest.raises(RuntimeError, match="no CPU path"):
        MSSSIMLoss()(p, p)

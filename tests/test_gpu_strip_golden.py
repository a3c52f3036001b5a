"""Bit-exact pin of the strip kernels against tests/golden/g12_strip_chain.npz, recorded by
tests/golden/make_golden_strip.py from the build before the RCAB loop's vector work was cut
(the fp16 combine on v_fma_mix_f32, packed bias adds and interleaved row-sum reductions in the
a1 epilogue).  The chain-vs-per-group tests compare two instantiations of one source and
cannot see a change that moves both; this compares with recorded words.

One small case on which every path of k_group_strip runs (B = 2, H = 24: a first, an interior
and a last strip; 2 groups of 2 RCABs + conv_after_body): the inference output in full and the
gates, word for word; the training instantiation's saved tensors (x, z1, a1, t, mean, hid, s,
x_last; pre_elide off) and the single-group entry fen_group_strip by SHA-256.  A mismatch of the
output names the first differing (image, row, pixel, channel)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_strip as M  # noqa: E402

pytestmark = pytest.mark.gpu


def _first_diff(got, want):
    idx = np.argwhere(got != want)
    if not len(idx):
        return None
    b, r, p, c = (int(v) for v in idx[0])
    return (f"{len(idx)} of {got.size} words differ; first at image {b}, row {r}, pixel {p}, channel {c}: "
            f"0x{int(got[b, r, p, c]):04x} != 0x{int(want[b, r, p, c]):04x}")


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_strip_chain_matches_recorded_bits(prec, golden):
    want = {k[len(prec) + 1:]: v for k, v in golden(M.FILE).items() if k.startswith(prec + "/")}
    got = M.run_case(prec)
    assert sorted(got) == sorted(want)
    assert got["fb"].dtype == np.uint16 and got["fb"].shape == (M.B, M.H, M.W, M.C) == want["fb"].shape
    d = _first_diff(got["fb"], want["fb"])
    assert d is None, f"{prec} inference output: {d}"
    for k in ("s", "g0_s"):                                  # the gates, as fp32 words
        g, w = got[k].view(np.uint32), want[k].view(np.uint32)
        assert np.array_equal(g, w), f"{prec} {k}: {int((g != w).sum())} words differ, first at {np.argwhere(g != w)[0]}"
    bad = [k for k, v in got.items() if isinstance(v, str) and v != str(want[k])]
    assert not bad, f"{prec}: SHA-256 differs for {bad}"

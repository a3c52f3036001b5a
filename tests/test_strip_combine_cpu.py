"""The fp16 combine of the strip kernels, x' = x + g * t (t, x fp16 as stored, the gate g fp32),
read as the mix form -- f16 sources widened exactly, ONE fp32 fused multiply-add, ONE
round-to-nearest-even conversion to f16 -- gives the 16 bits of convert -> fmaf -> convert done
with separate instructions.  The kernels use v_fma_mix_f32 (widen + FMA) and the packed
conversion on this argument.  (v_fma_mixlo/hi_f16, which also rounds, was tried and does NOT
follow this reading on gfx950: tests/test_gpu_strip_golden.py saw last-bit differences.)

  * the mix form is modelled from exact arithmetic: t * g is exact in float64 (11 x 24 bits),
    the sum with x is made exact by TwoSum and folded to round-to-odd, so the one rounding to
    fp32 is the correctly rounded FMA; then numpy's RNE conversion to f16;
  * convert -> fmaf -> convert uses the C library's fmaf on numpy-converted operands.

The round-to-odd model IS the test's vectorised fmaf: it runs over all 65,536 f16 values of t
against 64 x and 64 gate values (subnormals, +-0, +-inf, the largest finite values and NaN among
them), and it is validated against the C library's fmaf by sampling, not on the whole grid (268 M
scalar calls): on every special combination, on a fixed stride through the grid, and -- so that
every one of the 65,536 t values meets the C library -- gate i takes the 1,024 t values
1024 i .. 1024 i + 1023 against 8 x values each.  Where the float64 sum is itself exact the model
must also equal the plain float64 path on the whole grid (a second check of the model).  NaN results
compare as NaN (payloads are not part of the kernels' contract).  The GPU side -- that the
instructions really behave so -- is tests/test_gpu_strip_golden.py."""
import ctypes
import ctypes.util

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3

F16_SPECIAL = [0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x83ff, 0x0400, 0x8400, 0x7bff, 0xfbff, 0x7c00, 0xfc00, 0x7e00,
               0x3c00, 0xbc00, 0x3555]


def _x_values():
    rnd = np.random.default_rng(7).integers(0, 1 << 16, 64 - len(F16_SPECIAL), dtype=np.uint16)
    return np.concatenate([np.array(F16_SPECIAL, np.uint16), rnd]).view(np.float16)


def _g_values():
    sp = np.array([0.0, -0.0, 1.0, 0.2, 0.1, 1e-45, -1e-45, 1.1754942e-38, 3.4028235e38, -3.4028235e38, np.inf, -np.inf,
                   np.nan, 65504.0, 2.0 ** -24, 0.19999999], np.float32)
    r = np.random.default_rng(8)
    sig = (0.2 / (1.0 + np.exp(-r.normal(0, 2, 32)))).astype(np.float32)      # rs * sigmoid: the gates' range
    wide = r.integers(0, 1 << 32, 16, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return np.concatenate([sp, sig, wide])


def mix_model(t, g, x):
    """f16 t, f32 g, f16 x (arrays) -> f16: exact product and sum, one rounding to fp32, one to f16."""
    with np.errstate(all="ignore"):
        p = t.astype(np.float64) * g.astype(np.float64)                       # exact: 11 x 24 bits
        c = x.astype(np.float64)
        s = p + c
        bb = s - p                                                            # TwoSum: s + e = p + c exactly
        e = (p - (s - bb)) + (c - bb)
        inexact = np.isfinite(s) & (e != 0)
        even = (s.view(np.uint64) & np.uint64(1)) == 0
        # round to odd: an inexact sum whose last bit is even moves one ulp towards the lost part
        toward = np.where(e > 0, np.inf, -np.inf)
        s_odd = np.where(inexact & even, np.nextafter(s, toward), s)
        return s_odd.astype(np.float32).astype(np.float16), s.astype(np.float32).astype(np.float16), ~inexact


def three_step(t, g, x):
    """convert -> fmaf (C library) -> convert, element by element."""
    tf, xf = t.astype(np.float32), x.astype(np.float32)
    out = np.array([_libm.fmaf(float(a), float(b), float(c)) for a, b, c in zip(tf, g, xf)], np.float32)
    with np.errstate(all="ignore"):
        return out.astype(np.float16)


def _same(a, b):
    return (a.view(np.uint16) == b.view(np.uint16)) | (np.isnan(a) & np.isnan(b))


def test_mix_form_equals_convert_fmaf_convert_on_the_grid():
    t_all = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16).view(np.float16)
    xs, gs = _x_values(), _g_values()
    assert len(xs) == 64 and len(gs) == 64
    T, X = np.meshgrid(t_all, xs, indexing="ij")                               # [65536, 64]
    T, X = T.ravel(), X.ravel()
    stride = 4099                                                             # a prime: the sample drifts through t and x
    checked = 0
    t_met = np.zeros(1 << 16, bool)
    for gi, gv in enumerate(gs):
        G = np.full(T.shape, gv, np.float32)
        m, plain, exact = mix_model(T, G, X)
        ok = _same(m, plain) | ~exact
        assert ok.all(), f"model: gate {gv!r}, first at {int(np.argmin(ok))}"
        tb = np.arange(1024 * gi, 1024 * (gi + 1))[:, None]                   # this gate's block of t values ...
        blk = (tb * 64 + (tb + 8 * np.arange(8)[None, :]) % 64).ravel()       # ... against 8 x values each
        idx = np.union1d(np.arange((gi * 61) % stride, T.size, stride), blk)
        t_met[idx // 64] = True
        ref = three_step(T[idx], G[idx], X[idx])
        ok = _same(m[idx], ref)
        assert ok.all(), (f"gate {gv!r}: t=0x{int(T[idx][np.argmin(ok)].view(np.uint16)):04x} "
                          f"x=0x{int(X[idx][np.argmin(ok)].view(np.uint16)):04x}: mix 0x{int(m[idx][np.argmin(ok)].view(np.uint16)):04x} "
                          f"!= 0x{int(ref[np.argmin(ok)].view(np.uint16)):04x}")
        checked += len(idx)
    assert checked > 500000 and t_met.all()


def test_mix_form_on_every_special_combination():
    sp = np.array(F16_SPECIAL, np.uint16).view(np.float16)
    gs = _g_values()[:16]
    T, G, X = (a.ravel() for a in np.meshgrid(sp, gs, sp, indexing="ij"))
    m, _, _ = mix_model(T, G, X)
    ref = three_step(T, G, X)
    ok = _same(m, ref)
    assert ok.all(), int(np.argmin(ok))


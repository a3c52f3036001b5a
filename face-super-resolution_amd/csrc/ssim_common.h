// The SSIM kernels' shared geometry and inner loops (ssim.hip, msssim.hip): the 11-tap window,
// the 32 x 32 output tile and the packed-fp32 horizontal pass over the five filtered terms.
#pragma once
#include "fen_common.h"

namespace {

constexpr int SR = 5;       // window radius (window 11)
constexpr int ST = 32;      // output tile
struct SsimWin {
    float g[2 * SR + 1];
};

inline int nblk(size_t n, int t = 256) { return (int)((n + t - 1) / t); }

// Horizontal pass over NCH column chunks of CW outputs: thread keeps the CW + 10 inputs of
// its chunk in registers and reads each LDS element once.  Packed fp32 (v_pk_fma_f32): the
// (p, t) and (p^2, t^2) sums two at a time, p t alone -- 3 FMA instructions per tap, not 5.
__device__ __forceinline__ f32x2 pfma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// G*a + 2 p G*b + t G*c with the contraction spelled out: the fused kernel and k_ssim_g2 round
// it identically whatever the surrounding code lets the compiler fuse
__device__ __forceinline__ float ssim_dcomb(f32x2 mab, float mc, float p, float t) {
    return __builtin_fmaf(t, mc, __builtin_fmaf(2.f * p, mab.y, mab.x));
}

template <int CW>
__device__ __forceinline__ void hrow(const SsimWin& win, const float* p, const float* t, float (&o)[5][CW]) {
    f32x2 pt[CW + 2 * SR], sq[CW + 2 * SR];
    float cr[CW + 2 * SR];
#pragma unroll
    for (int i = 0; i < CW + 2 * SR; ++i) {
        pt[i] = f32x2{p[i], t[i]};
        sq[i] = pt[i] * pt[i];
        cr[i] = pt[i].x * pt[i].y;
    }
#pragma unroll
    for (int c = 0; c < CW; ++c) {
        f32x2 s01 = {0.f, 0.f}, s23 = {0.f, 0.f};
        float s4 = 0.f;
#pragma unroll
        for (int j = 0; j < 2 * SR + 1; ++j) {
            const f32x2 g2 = {win.g[j], win.g[j]};
            s01 = pfma(g2, pt[c + j], s01);
            s23 = pfma(g2, sq[c + j], s23);
            s4 = fmaf(win.g[j], cr[c + j], s4);
        }
        o[0][c] = s01.x; o[1][c] = s01.y; o[2][c] = s23.x; o[3][c] = s23.y; o[4][c] = s4;
    }
}

}  // namespace

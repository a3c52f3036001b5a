// LPIPS v0.1 on the AlexNet backbone (reference src/evaluation/metrics.py:81-126, which wraps
// lpips.LPIPS(net='alex')), forward only, fp32 throughout, one value per image, no host
// synchronisation.  The pieces the other sources do not have:
//
//   fen_conv2d_f32        a forward convolution over NHWC fp32 with runtime KH, KW, stride and
//                         pad as an implicit GEMM on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32):
//                         M = output pixels of the whole batch, N = Cout, K = KH KW Cin in
//                         (kh, kw, ci) order, the filter packed once into [K][Cout]
//                         (fen_conv2d_f32_pack), zero borders by a bounds test in the gather,
//                         bias + ReLU in the epilogue
//   fen_maxpool3s2_f32    NHWC fp32, kernel 3, stride 2, no padding, floor
//   fen_lpips_prep        pred / target NCHW -> one stacked NHWC-4 batch [2B,H,W,4] with the
//                         range rule (pred.min() >= 0: both become 2x - 1; decided on the device
//                         by a min reduction that leaves a flag) and the scaling layer
//   fen_lpips_head        one tap: per pixel the two channel norms and
//                         sum_c lin[c] (a_c / (|a| + eps) - b_c / (|b| + eps))^2, per-image
//                         partial sums in the caller's workspace
//   fen_lpips_finish      out[b] = sum over the five taps of the tap's spatial mean
//
// No atomics anywhere: every sum has a fixed order, so two runs give the same bits, and the two
// halves of the stacked batch go through the same fmaf chain per output element, so SR == HR
// gives exactly 0.
#include "fen_common.h"

#include <math.h>

namespace {

inline int nblk(size_t n, int t = 256) { return (int)((n + t - 1) / t); }

// ------------------------------------------------------------------------------------------
// the convolution
// ------------------------------------------------------------------------------------------
// One block = a 64 (pixels) x 64 (output channels) tile, 4 waves; wave w owns pixels 16 w ..
// 16 w + 15 and all 64 channels: four independent 16x16 accumulators (the 16x16x4 f32 MFMA's
// dependent latency is 40 cycles against a 32-cycle issue interval).  K runs in stages of 16:
// the next stage's operands are loaded into registers while the MFMAs of the current one read
// LDS.  Rows of both LDS tiles are 80 floats: the four k rows of one MFMA step start 16 banks
// apart, so an operand read (16 consecutive columns x 4 rows) is conflict-free.
// A MFMA accumulates its four k in order onto C (a k-ordered fmaf chain, MI355X matrix-core
// numerics).  One chain over all of K (up to 3456 here) lets the rounding error grow as a K-step
// random walk: measured, twice the error of the fp32 CPU convolution.  So the sum is blocked in
// three levels: a stage's 16 k accumulate from 0 (blk), 4 stages are added into l1, 8 of those
// (512 k) into l2, and those into acc -- at most 16 + 4 + 8 + K / 512 + 2 roundings on the way
// to an output element, plus the bias; a fixed order, the same for every pixel.  Stage padding
// past K contributes fma(0, 0, acc) = acc.
constexpr int CT = 64, CK = 16, CLD = 80;

__global__ __launch_bounds__(256) void k_conv2d_f32(int M, int H, int W, int Cin, int Ho, int Wo, int Cout, int KW,
                                                    int K, int stride, int pad, const float* __restrict__ x,
                                                    const float* __restrict__ wp, const float* __restrict__ bias,
                                                    int relu, float* __restrict__ y) {
    __shared__ __attribute__((aligned(16))) float As[CK][CLD];
    __shared__ __attribute__((aligned(16))) float Bs[CK][CLD];
    const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
    const int m0 = blockIdx.x * CT, n0 = blockIdx.y * CT;
    // gather role: pixel gm of the tile, k quad gq of the stage (one float4 = 4 consecutive ci of
    // one (kh, kw): Cin is a multiple of 4).  A wave's lanes hold 64 pixels: conflict-free stores.
    const int gm = tid & 63, gq = tid >> 6;
    const int m = m0 + gm;
    const bool mv = m < M;
    const int mm = mv ? m : 0;
    const int wo = mm % Wo, ho = (mm / Wo) % Ho, img = mm / (Wo * Ho);
    const int iy0 = ho * stride - pad, ix0 = wo * stride - pad;
    const float* ximg = x + (size_t)img * H * W * Cin;
    // filter role: row bk of the stage, 4 channels from bc
    const int bk = tid >> 4, bc = (tid & 15) * 4;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    auto load_a = [&](int k0) -> float4 {
        const int k = k0 + 4 * gq;
        if (!mv || k >= K) return zero;
        const int pos = k / Cin, ci = k - pos * Cin;
        const int kh = pos / KW, kw = pos - kh * KW;
        const int iy = iy0 + kh, ix = ix0 + kw;
        if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) return zero;   // the zero border
        return *(const float4*)(ximg + ((size_t)iy * W + ix) * Cin + ci);
    };
    auto load_b = [&](int k0) -> float4 {
        const int k = k0 + bk;
        return k < K ? *(const float4*)(wp + (size_t)k * Cout + n0 + bc) : zero;
    };
    f32x4 acc[4], l2[4], l1[4], blk[4];          // the running sum, the 512-k and 64-k blocks, the stage
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = l2[j] = l1[j] = blk[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 ra = load_a(0), rb = load_b(0);
    const int ar = lane >> 4, ac = lane & 15;
    for (int k0 = 0; k0 < K; k0 += CK) {
        As[4 * gq + 0][gm] = ra.x;
        As[4 * gq + 1][gm] = ra.y;
        As[4 * gq + 2][gm] = ra.z;
        As[4 * gq + 3][gm] = ra.w;
        *(float4*)&Bs[bk][bc] = rb;
        __syncthreads();
        if (k0 + CK < K) ra = load_a(k0 + CK), rb = load_b(k0 + CK);
#pragma unroll
        for (int kk = 0; kk < CK / 4; ++kk) {
            const float a = As[kk * 4 + ar][16 * w + ac];            // A[row lane & 15][k lane >> 4]
#pragma unroll
            for (int j = 0; j < 4; ++j)                               // B[k lane >> 4][col lane & 15]
                blk[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[kk * 4 + ar][16 * j + ac], blk[j], 0, 0, 0);
        }
        const int st = k0 / CK;
#pragma unroll
        for (int j = 0; j < 4; ++j) l1[j] += blk[j], blk[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if ((st & 3) == 3) {
#pragma unroll
            for (int j = 0; j < 4; ++j) l2[j] += l1[j], l1[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if ((st & 31) == 31) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += l2[j], l2[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += l2[j] + l1[j];              // the unfinished blocks
    // C/D: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int mr = m0 + 16 * w + 4 * ar + r;
        if (mr >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + 16 * j + ac;
            float v = acc[j][r];
            if (bias) v += bias[n];
            if (relu) v = fmaxf(v, 0.f);
            y[(size_t)mr * Cout + n] = v;
        }
    }
}

// wp[(kh KW + kw) Cin_pad + ci][co] = w[co][ci][kh][kw] (torch OIHW), 0 for ci >= Cin
__global__ __launch_bounds__(256) void k_conv2d_pack(int Cout, int Cin, int KHW, int Cin_pad,
                                                     const float* __restrict__ w, float* __restrict__ wp) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)KHW * Cin_pad * Cout) return;
    const int co = (int)(i % Cout);
    const size_t k = i / Cout;
    const int ci = (int)(k % Cin_pad), pos = (int)(k / Cin_pad);
    wp[i] = ci < Cin ? w[((size_t)co * Cin + ci) * KHW + pos] : 0.f;
}

// ------------------------------------------------------------------------------------------
// the pool: y[n][ho][wo][c] = max over the 3x3 window at (2 ho, 2 wo); torch's rule for the
// running maximum (a larger value or a NaN replaces it)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_maxpool3s2(int N, int H, int W, int Ho, int Wo, int C,
                                                    const float* __restrict__ x, float* __restrict__ y) {
    const int G = C / 4;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * Ho * Wo * G) return;
    const int g = (int)(i % G);
    const size_t po = i / G;
    const int wo = (int)(po % Wo), ho = (int)((po / Wo) % Ho), n = (int)(po / ((size_t)Wo * Ho));
    const float* p = x + (((size_t)n * H + 2 * ho) * W + 2 * wo) * C + g * 4;
    float mx[4], v[4];
    ld4<float>(p, mx);
#pragma unroll
    for (int k = 1; k < 9; ++k) {
        ld4<float>(p + ((size_t)(k / 3) * W + k % 3) * C, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) mx[j] = (v[j] > mx[j] || v[j] != v[j]) ? v[j] : mx[j];
    }
    st4<float>(y + po * C + g * 4, mx);
}

// ------------------------------------------------------------------------------------------
// the input: the range flag, then the stacked NHWC-4 batch
// ------------------------------------------------------------------------------------------
constexpr int MINB = 256;          // blocks (and partial minima) of the min reduction
constexpr int W_FLAG = 0, W_MIN = 1, W_PART = 320;   // workspace layout, in floats

// the smaller of the two; a NaN wins and stays (torch's min propagates NaN, and NaN >= 0 is false).
// An exact operation: the order of a min reduction cannot change its result.
__device__ __forceinline__ float nanmin(float a, float b) { return (b < a || b != b) ? b : a; }

__device__ __forceinline__ float block_min(float v, float* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = nanmin(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return nanmin(nanmin(red[0], red[1]), nanmin(red[2], red[3]));
}

__global__ __launch_bounds__(256) void k_lpips_min_part(size_t n, const float* __restrict__ pred,
                                                        float* __restrict__ part) {
    __shared__ float red[4];
    float v = INFINITY;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) v = nanmin(v, pred[i]);
    v = block_min(v, red);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// flag = pred.min() >= 0
__global__ __launch_bounds__(256) void k_lpips_flag(const float* __restrict__ part, int* __restrict__ flag) {
    __shared__ float red[4];
    const float v = block_min(part[threadIdx.x], red);
    if (threadIdx.x == 0) *flag = v >= 0.f ? 1 : 0;
}

// x0[n][h][w][0..2] = ((flag ? 2 v - 1 : v) - shift[c]) / scale[c], channel 3 = 0; images
// 0 .. B-1 from pred, B .. 2B-1 from target
__global__ __launch_bounds__(256) void k_lpips_prep(int B, size_t HW, const float* __restrict__ pred,
                                                    const float* __restrict__ target, const int* __restrict__ flag,
                                                    float* __restrict__ x0) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * (size_t)B * HW) return;
    const size_t n = i / HW, p = i - n * HW;
    const float* src = n < (size_t)B ? pred + n * 3 * HW : target + (n - B) * 3 * HW;
    const bool rescale = *flag != 0;
    const float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};
    float o[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = src[c * HW + p];
        if (rescale) v = __fsub_rn(__fmul_rn(v, 2.f), 1.f);
        o[c] = __fdiv_rn(__fsub_rn(v, shift[c]), scale[c]);
    }
    o[3] = 0.f;
    st4<float>(x0 + i * 4, o);
}

// ------------------------------------------------------------------------------------------
// the head
// ------------------------------------------------------------------------------------------
// AlexNet features on an H x W input: the five ReLU outputs
struct LpipsGeom {
    int h[5], w[5], c[5];
    int nchunk[5];      // head blocks per image and tap
    int off[5];         // chunks of the taps before this one (per image)
    int total;          // chunks of one image over all taps
};
constexpr int HD_PPB = 64;          // pixels per head block: 16 per wave
constexpr int HD_MAXJ = 6;          // channels per lane: C <= 384

// false for a shape that is refused
bool lpips_geom(int B, int H, int W, LpipsGeom* g) {
    if (B <= 0 || H < 31 || W < 31 || B > 32767) return false;
    if ((size_t)2 * B * H * W > (size_t)1 << 28) return false;       // every index below fits an int
    const int h1 = (H + 4 - 11) / 4 + 1, w1 = (W + 4 - 11) / 4 + 1;
    const int h2 = (h1 - 3) / 2 + 1, w2 = (w1 - 3) / 2 + 1;
    const int h3 = (h2 - 3) / 2 + 1, w3 = (w2 - 3) / 2 + 1;
    const int hs[5] = {h1, h2, h3, h3, h3}, ws[5] = {w1, w2, w3, w3, w3}, cs[5] = {64, 192, 384, 256, 256};
    int off = 0;
    for (int k = 0; k < 5; ++k) {
        g->h[k] = hs[k], g->w[k] = ws[k], g->c[k] = cs[k];
        g->nchunk[k] = (hs[k] * ws[k] + HD_PPB - 1) / HD_PPB;
        g->off[k] = off;
        off += g->nchunk[k];
    }
    g->total = off;
    return true;
}

// feat [2B][npix][C]: image b against image B + b.  Block (chunk, b): wave w takes pixels
// chunk * 64 + 16 w + i in order; per pixel the lanes hold the C channels (C / 64 each), the two
// squared norms and the weighted squared difference go through the wave tree.  part[b][chunk] =
// the block's sum, the four waves in order.
__global__ __launch_bounds__(256) void k_lpips_head(int B, int npix, int C, const float* __restrict__ feat,
                                                    const float* __restrict__ lin, float* __restrict__ part) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, w = wave_id();
    const int b = blockIdx.y, chunk = blockIdx.x;
    const float* fa = feat + (size_t)b * npix * C;
    const float* fb = feat + (size_t)(B + b) * npix * C;
    float l[HD_MAXJ];
#pragma unroll
    for (int j = 0; j < HD_MAXJ; ++j) l[j] = lane + 64 * j < C ? lin[lane + 64 * j] : 0.f;
    float tot = 0.f;
    for (int i = 0; i < HD_PPB / 4; ++i) {
        const int p = chunk * HD_PPB + w * (HD_PPB / 4) + i;      // wave-uniform
        if (p >= npix) break;
        float av[HD_MAXJ], bv[HD_MAXJ], sa = 0.f, sb = 0.f;
#pragma unroll
        for (int j = 0; j < HD_MAXJ; ++j) {
            const int c = lane + 64 * j;
            av[j] = c < C ? fa[(size_t)p * C + c] : 0.f;
            bv[j] = c < C ? fb[(size_t)p * C + c] : 0.f;
            sa = fmaf(av[j], av[j], sa);
            sb = fmaf(bv[j], bv[j], sb);
        }
        const float na = sqrtf(wave_sum(sa)) + 1e-10f, nb = sqrtf(wave_sum(sb)) + 1e-10f;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < HD_MAXJ; ++j) {
            const float d = __fdiv_rn(av[j], na) - __fdiv_rn(bv[j], nb);
            s = fmaf(l[j], d * d, s);
        }
        tot += wave_sum(s);
    }
    if (lane == 0) red[w] = tot;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + chunk] = ((red[0] + red[1]) + red[2]) + red[3];
}

// One block, one wave per image in turn: tap by tap the image's chunk sums lane-strided, the
// wave tree, the division by the tap's pixel count; the five means added in tap order.
__global__ __launch_bounds__(256) void k_lpips_finish(int B, const LpipsGeom g, const float* __restrict__ part,
                                                      float* __restrict__ out) {
    const int lane = threadIdx.x & 63, w = wave_id();
    for (int b = w; b < B; b += 4) {
        float total = 0.f;
        for (int k = 0; k < 5; ++k) {
            const float* q = part + (size_t)B * g.off[k] + (size_t)b * g.nchunk[k];
            float s = 0.f;
            for (int i = lane; i < g.nchunk[k]; i += 64) s += q[i];
            total += wave_sum(s) / (float)(g.h[k] * g.w[k]);
        }
        if (lane == 0) out[b] = total;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

#define STREAM ((hipStream_t)stream)

extern "C" int fen_conv2d_f32_pack(int Cout, int Cin, int KH, int KW, int Cin_pad, const float* w, float* wp,
                                   void* stream) {
    if (!w || !wp || Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0 || Cin_pad < Cin) return FEN_EINVAL;
    if ((size_t)KH * KW * Cin_pad * Cout > (size_t)1 << 30) return FEN_EUNSUPPORTED;
    const size_t n = (size_t)KH * KW * Cin_pad * Cout;
    hipLaunchKernelGGL(k_conv2d_pack, dim3(nblk(n)), dim3(256), 0, STREAM, Cout, Cin, KH * KW, Cin_pad, w, wp);
    FEN_CHECK_LAUNCH();
    return FEN_OK;
}

extern "C" int fen_conv2d_f32(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                              const float* x, const float* wp, const float* bias, int relu, float* y, void* stream) {
    if (!x || !wp || !y || !aligned16(x) || !aligned16(wp) || !aligned16(y)) return FEN_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad < 0)
        return FEN_EINVAL;
    if (Cout % CT || Cin % 4) return FEN_EUNSUPPORTED;               // (Cin % 4: K a multiple of 4, float4 gathers)
    if (H + 2 * pad < KH || W + 2 * pad < KW) return FEN_EUNSUPPORTED;   // an empty output
    const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
    const size_t M = (size_t)N * Ho * Wo, K = (size_t)KH * KW * Cin;
    if (M > ((size_t)1 << 30) || K > ((size_t)1 << 24) || (size_t)N * H * W > ((size_t)1 << 30) ||
        Cout / CT > 65535)
        return FEN_EUNSUPPORTED;
    const dim3 grid((unsigned)((M + CT - 1) / CT), (unsigned)(Cout / CT));
    hipLaunchKernelGGL(k_conv2d_f32, grid, dim3(256), 0, STREAM, (int)M, H, W, Cin, Ho, Wo, Cout, KW, (int)K, stride,
                       pad, x, wp, bias, relu, y);
    FEN_CHECK_LAUNCH();
    return FEN_OK;
}

extern "C" int fen_maxpool3s2_f32(int N, int H, int W, int C, const float* x, float* y, void* stream) {
    if (!x || !y || !aligned16(x) || !aligned16(y) || N <= 0 || H <= 0 || W <= 0 || C <= 0) return FEN_EINVAL;
    if (C % 4 || H < 3 || W < 3 || (size_t)N * H * W * (C / 4) > (size_t)1 << 40) return FEN_EUNSUPPORTED;
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    const size_t n = (size_t)N * Ho * Wo * (C / 4);
    if (n > (size_t)1 << 38) return FEN_EUNSUPPORTED;
    hipLaunchKernelGGL(k_maxpool3s2, dim3(nblk(n)), dim3(256), 0, STREAM, N, H, W, Ho, Wo, C, x, y);
    FEN_CHECK_LAUNCH();
    return FEN_OK;
}

extern "C" size_t fen_lpips_work_floats(int B, int H, int W) {
    LpipsGeom g;
    if (!lpips_geom(B, H, W, &g)) return 0;
    return (size_t)W_PART + (size_t)B * g.total;
}

extern "C" int fen_lpips_prep(int B, int H, int W, const float* pred, const float* target, float* work,
                              size_t work_floats, float* x0, void* stream) {
    if (!pred || !target || !work || !x0 || !aligned16(x0)) return FEN_EINVAL;
    LpipsGeom g;
    if (!lpips_geom(B, H, W, &g)) return FEN_EUNSUPPORTED;
    if (work_floats < fen_lpips_work_floats(B, H, W)) return FEN_EINVAL;
    const size_t HW = (size_t)H * W;
    hipLaunchKernelGGL(k_lpips_min_part, dim3(MINB), dim3(256), 0, STREAM, (size_t)B * 3 * HW, pred, work + W_MIN);
    hipLaunchKernelGGL(k_lpips_flag, dim3(1), dim3(256), 0, STREAM, work + W_MIN, (int*)(work + W_FLAG));
    hipLaunchKernelGGL(k_lpips_prep, dim3(nblk(2 * (size_t)B * HW)), dim3(256), 0, STREAM, B, HW, pred, target,
                       (const int*)(work + W_FLAG), x0);
    FEN_CHECK_LAUNCH();
    return FEN_OK;
}

extern "C" int fen_lpips_head(int B, int H, int W, int tap, const float* feat, const float* lin, float* work,
                              size_t work_floats, void* stream) {
    if (!feat || !lin || !work || tap < 0 || tap > 4) return FEN_EINVAL;
    LpipsGeom g;
    if (!lpips_geom(B, H, W, &g)) return FEN_EUNSUPPORTED;
    if (work_floats < fen_lpips_work_floats(B, H, W)) return FEN_EINVAL;
    static_assert(64 * HD_MAXJ >= 384, "the widest tap");
    hipLaunchKernelGGL(k_lpips_head, dim3(g.nchunk[tap], B), dim3(256), 0, STREAM, B, g.h[tap] * g.w[tap], g.c[tap],
                       feat, lin, work + W_PART + (size_t)B * g.off[tap]);
    FEN_CHECK_LAUNCH();
    return FEN_OK;
}

extern "C" int fen_lpips_finish(int B, int H, int W, const float* work, size_t work_floats, float* out,
                                void* stream) {
    if (!work || !out) return FEN_EINVAL;
    LpipsGeom g;
    if (!lpips_geom(B, H, W, &g)) return FEN_EUNSUPPORTED;
    if (work_floats < fen_lpips_work_floats(B, H, W)) return FEN_EINVAL;
    hipLaunchKernelGGL(k_lpips_finish, dim3(1), dim3(256), 0, STREAM, B, g, work + W_PART, out);
    FEN_CHECK_LAUNCH();
    return FEN_OK;
}

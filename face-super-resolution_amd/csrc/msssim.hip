// MS-SSIM (reference src/losses/ssim_loss.py:101-171): levels x_0 = input, x_{i+1} = 2x2
// average pooling (floor mode) of x_i; at every level the zero-padded 11-tap Gaussian terms of
// ssim.hip; M_i = the batch mean of the contrast-structure map cs = (2 spt + C2)/(spp + stt + C2)
// for i < L-1, V = the batch mean of the full SSIM map at the last level; the value
// V * prod_{i<L-1} M_i^{w_i}.  Its gradient w.r.t. pred in closed form: per level
// g_i = d(sum map_i)/dx_i = G*a + 2 p G*b + t G*c from the map's coefficients a, b, c (ssim.hip),
// pulled back through the pooling (each level-i pixel spreads 1/4^i over its 2^i x 2^i block).
//
// Launches, all on one stream, no atomics, no host round trip: L-1 pooling launches (pred and
// target together), L level launches (tile sums + g_i), one one-block finish (fixed-order sums,
// M_i, V, the value and the per-level factors k_i), one combine over the full-resolution pixels.
#include "ssim_common.h"

#include <math.h>

#include <type_traits>

namespace {

constexpr int ML = 8;       // most levels

struct MsGeom {
    int H[ML], W[ML];
    size_t goff[ML];        // level i's g_i inside the gradient maps
    int poff[ML], pcnt[ML]; // level i's tile sums inside the parts
    float inv_n[ML];        // 1 / (B C H_i W_i)
    float pull[ML];         // 1 / (B C H_i W_i 4^i)
};

// x_{i+1} = avg_pool2d(x_i, 2, 2) of pred and target: one thread per output pixel of a plane
__global__ __launch_bounds__(256) void k_ms_pool(size_t n, int Hi, int Wi, int Ho, int Wo,
                                                 const float* __restrict__ p, const float* __restrict__ t,
                                                 float* __restrict__ po, float* __restrict__ to) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int xo = (int)(i % Wo), yo = (int)((i / Wo) % Ho);
    const size_t plane = i / ((size_t)Wo * Ho);
    const size_t e = (plane * Hi + 2 * yo) * Wi + 2 * xo;     // 2 yo + 1 < Hi, 2 xo + 1 < Wi (floor mode)
    po[i] = 0.25f * (((p[e] + p[e + 1]) + p[e + Wi]) + p[e + Wi + 1]);
    to[i] = 0.25f * (((t[e] + t[e + 1]) + t[e + Wi]) + t[e + Wi + 1]);
}

// One level: k_ssim's one-launch form (ssim.hip) for one 32x32 tile of one plane per block --
// inputs on the tile + 10 px (GRAD; + 5 px without) in LDS, the separable passes, the map and
// its tile sum; with GRAD the coefficients a, b, c on the tile + 5 px, their filtered combination
// g = G*a + 2 p G*b + t G*c on the tile, written unscaled (fp32, the level's NCHW shape).
// LAST: the full SSIM map lum * cs; otherwise cs alone, with
//   c = 2 / B2,  b = -cs / B2,  a = (2 mp cs - 2 mt) / B2     (B2 = spp + stt + C2).
template <bool GRAD, bool LAST>
__global__ __launch_bounds__(256) void k_ms_level(int H, int W, const float* __restrict__ pred,
                                                  const float* __restrict__ target, const SsimWin win, float C1,
                                                  float C2, float* __restrict__ part, float* __restrict__ g) {
    constexpr int E1 = GRAD ? ST + 2 * SR : ST;   // where the map (and a, b, c) is needed
    constexpr int E2 = E1 + 2 * SR;               // where the inputs are needed
    constexpr int O1 = GRAD ? SR : 0;             // tile offset inside E1
    constexpr int CW = GRAD ? 7 : 8;              // register block of the map passes
    constexpr int NCH = E1 / CW;
    constexpr int CWV = GRAD ? CW : 4, NCHV = E1 / CWV;
    constexpr int CW2 = 8, NCH2 = ST / CW2;       // horizontal gradient pass: 8-column chunks
    constexpr int RV = 4, NRV = ST / RV;          // vertical gradient pass: 4-row chunks
    constexpr int PS = E2 + 1;
    static_assert(NCH * CW == E1 && NCHV * CWV == E1, "whole register blocks");
    static_assert(3 * E1 * (E1 + 1) <= 2 * E2 * PS, "a/b/c alias");
    static_assert(ST * NRV == 256, "one vertical gradient item per thread");
    __shared__ float sb[2 * E2 * PS];             // p, t on E2 x E2; after the first pass a / b / c on E1 x E1
    __shared__ float hp[5][E2][E1 + 1];           // horizontal sums (reused for a, b, c)
    __shared__ float red[4];
    float* sp = sb;
    float* st = sb + E2 * PS;
    float (*abc)[E1][E1 + 1] = (float (*)[E1][E1 + 1])sb;
    const int tid = threadIdx.x;
    const int h0 = blockIdx.y * ST, w0 = blockIdx.x * ST;
    const int gy0 = h0 - O1 - SR, gx0 = w0 - O1 - SR;     // image coords of E2's (0, 0)
    const size_t pl = (size_t)blockIdx.z * H * W;
    const float* pp = pred + pl;
    const float* tp = target + pl;
    for (int i = tid; i < E2 * E2; i += 256) {
        const int r = i / E2, c = i % E2, gy = gy0 + r, gx = gx0 + c;
        const bool in = (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
        const size_t e = in ? (size_t)gy * W + gx : 0;
        sp[r * PS + c] = in ? pp[e] : 0.f;
        st[r * PS + c] = in ? tp[e] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < E2 * NCH; i += 256) {
        const int r = i / NCH, c0 = (i % NCH) * CW;
        float o[5][CW];
        hrow<CW>(win, sp + r * PS + c0, st + r * PS + c0, o);
#pragma unroll
        for (int k = 0; k < 5; ++k)
#pragma unroll
            for (int c = 0; c < CW; ++c) hp[k][r][c0 + c] = o[k][c];
    }
    __syncthreads();
    // vertical pass: thread = (column, CWV-row chunk); the map, its sum over the tile's own
    // pixels, and (GRAD) a, b, c over sb
    float acc = 0.f;
    for (int i = tid; i < E1 * NCHV; i += 256) {
        const int c = i % E1, r0 = (i / E1) * CWV;
        f32x2 m01[CWV], m23[CWV];
        float m4[CWV];
#pragma unroll
        for (int o = 0; o < CWV; ++o) m01[o] = m23[o] = f32x2{0.f, 0.f}, m4[o] = 0.f;
#pragma unroll
        for (int rr = 0; rr < CWV + 2 * SR; ++rr) {
            const f32x2 v01 = {hp[0][r0 + rr][c], hp[1][r0 + rr][c]};
            const f32x2 v23 = {hp[2][r0 + rr][c], hp[3][r0 + rr][c]};
            const float v4 = hp[4][r0 + rr][c];
#pragma unroll
            for (int o = 0; o < CWV; ++o) {
                const int j = rr - o;
                if (j >= 0 && j <= 2 * SR) {
                    const f32x2 g2 = {win.g[j], win.g[j]};
                    m01[o] = pfma(g2, v01, m01[o]);
                    m23[o] = pfma(g2, v23, m23[o]);
                    m4[o] = fmaf(win.g[j], v4, m4[o]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < CWV; ++o) {
            const int r = r0 + o;
            const float mp = m01[o].x, mt = m01[o].y;
            const float spp = m23[o].x - mp * mp, stt = m23[o].y - mt * mt, spt = m4[o] - mp * mt;
            const float A2 = 2.f * spt + C2, B2 = spp + stt + C2;
            // v_rcp_f32 as in k_ssim: B1 >= C1 > 0, B2 >= C2 > 0 up to rounding
            const float r2 = __builtin_amdgcn_rcpf(B2);
            float S, ca, cb, cc;
            if constexpr (LAST) {
                const float A1 = 2.f * mp * mt + C1, B1 = mp * mp + mt * mt + C1;
                const float r1 = __builtin_amdgcn_rcpf(B1), iB = r1 * r2;
                S = (A1 * A2) * iB;
                ca = 2.f * mt * (A2 - A1) * iB - 2.f * mp * S * (r1 - r2);
                cb = -S * r2;
                cc = 2.f * A1 * iB;
            } else {
                S = A2 * r2;
                ca = (2.f * mp * S - 2.f * mt) * r2;
                cb = -S * r2;
                cc = 2.f * r2;
            }
            const int gy = h0 - O1 + r, gx = w0 - O1 + c;
            const bool in = (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
            const bool own = r >= O1 && r < O1 + ST && c >= O1 && c < O1 + ST;
            if (in && own) acc += S;
            if constexpr (GRAD) {
                abc[0][r][c] = in ? ca : 0.f;
                abc[1][r][c] = in ? cb : 0.f;
                abc[2][r][c] = in ? cc : 0.f;
            }
        }
    }
    if constexpr (GRAD) {
        __syncthreads();
        for (int i = tid; i < E1 * NCH2; i += 256) {          // horizontal pass of a, b (packed) and c
            const int r = i / NCH2, c0 = (i % NCH2) * CW2;
            f32x2 vab[CW2 + 2 * SR];
            float vc[CW2 + 2 * SR];
#pragma unroll
            for (int q = 0; q < CW2 + 2 * SR; ++q) vab[q] = f32x2{abc[0][r][c0 + q], abc[1][r][c0 + q]}, vc[q] = abc[2][r][c0 + q];
#pragma unroll
            for (int c = 0; c < CW2; ++c) {
                f32x2 sab = {0.f, 0.f};
                float sc = 0.f;
#pragma unroll
                for (int j = 0; j < 2 * SR + 1; ++j) {
                    sab = pfma(f32x2{win.g[j], win.g[j]}, vab[c + j], sab);
                    sc = fmaf(win.g[j], vc[c + j], sc);
                }
                hp[0][r][c0 + c] = sab.x;
                hp[1][r][c0 + c] = sab.y;
                hp[2][r][c0 + c] = sc;
            }
        }
        __syncthreads();
        {                                                     // vertical pass + the gradient: one item per thread
            const int c = tid % ST, r0 = (tid / ST) * RV, gx = w0 + c;
            f32x2 mab[RV];
            float mc[RV];
#pragma unroll
            for (int o = 0; o < RV; ++o) mab[o] = f32x2{0.f, 0.f}, mc[o] = 0.f;
#pragma unroll
            for (int rr = 0; rr < RV + 2 * SR; ++rr) {
                const f32x2 vab = {hp[0][r0 + rr][c], hp[1][r0 + rr][c]};
                const float vc = hp[2][r0 + rr][c];
#pragma unroll
                for (int o = 0; o < RV; ++o) {
                    const int j = rr - o;
                    if (j >= 0 && j <= 2 * SR) {
                        mab[o] = pfma(f32x2{win.g[j], win.g[j]}, vab, mab[o]);
                        mc[o] = fmaf(win.g[j], vc, mc[o]);
                    }
                }
            }
#pragma unroll
            for (int o = 0; o < RV; ++o) {
                const int gy = h0 + r0 + o;
                if (gx < W && gy < H) {
                    const size_t e = (size_t)gy * W + gx;
                    g[pl + e] = ssim_dcomb(mab[o], mc[o], pp[e], tp[e]);   // L2-hot: this block staged them
                }
            }
        }
    }
    // the tile's sum: wave sums (fixed tree), then the 4 waves in order
    acc = wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0)
        part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// One block: each level's tile sums in a fixed order (thread-strided, wave tree, the 4 waves in
// order), then out[1 + i] = M_i (V at the last level), out[0] = V prod M_i^{w_i} and the combine
// kernel's factors kf[i] = d(ms)/d(sum map_i) / 4^i: w_i ms / (M_i n_i 4^i), ms / (V n_i 4^i) at
// the last level.  A negative M_i gives NaN (powf), as the reference's ** does.
__global__ __launch_bounds__(256) void k_ms_finish(int levels, const MsGeom gm, const float* __restrict__ part,
                                                   const float* __restrict__ weights, float* __restrict__ out,
                                                   float* __restrict__ kf) {
    __shared__ float red[ML][4];
    const int tid = threadIdx.x;
    for (int i = 0; i < levels; ++i) {
        const float* q = part + gm.poff[i];
        float s = 0.f;
        for (int k = tid; k < gm.pcnt[i]; k += 256) s += q[k];
        s = wave_sum(s);
        if ((tid & 63) == 0) red[i][tid >> 6] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    float mean[ML];
    float ms = 1.f;
    for (int i = 0; i < levels; ++i) {
        mean[i] = (((red[i][0] + red[i][1]) + red[i][2]) + red[i][3]) * gm.inv_n[i];
        ms *= i + 1 < levels ? powf(mean[i], weights[i]) : mean[i];
        out[1 + i] = mean[i];
    }
    out[0] = ms;
    for (int i = 0; i < levels; ++i) kf[i] = (i + 1 < levels ? weights[i] : 1.f) * ms / mean[i] * gm.pull[i];
}

// d(ms)/d(pred) at full resolution: sum_i kf[i] g_i[y >> i][x >> i] over the levels that hold the
// pixel (floor pooling drops an odd last row / column), one thread per pixel (b, y, x), every
// channel.  MODE 1: grad NCHW fp32 = grad_scale * that (written).  MODE 2 (C <= 3): added to
// channels 0..C-1 of the NHWC16 buffer, channels 0..3 of the pixel in one read-modify-write
// (channels >= C written back as read).
template <typename T, int MODE>
__global__ __launch_bounds__(256) void k_ms_combine(int B, int C, int H, int W, int levels, const MsGeom gm,
                                                    const float* __restrict__ gmaps, const float* __restrict__ kf,
                                                    void* __restrict__ grad, float grad_scale) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * H * W) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), b = (int)(i / ((size_t)W * H));
    auto pixel = [&](int ch) {
        float s = 0.f;
        for (int l = 0; l < levels; ++l) {
            const int yl = y >> l, xl = x >> l, Hl = gm.H[l], Wl = gm.W[l];
            if (yl < Hl && xl < Wl) s = fmaf(kf[l], gmaps[gm.goff[l] + ((size_t)(b * C + ch) * Hl + yl) * Wl + xl], s);
        }
        return grad_scale * s;
    };
    if constexpr (MODE == 1) {
        for (int ch = 0; ch < C; ++ch) ((float*)grad)[((size_t)(b * C + ch) * H + y) * W + x] = pixel(ch);
    } else {
        typedef typename std::conditional<sizeof(T) == 2, uint2, float4>::type GV;
        GV* q = (GV*)((T*)grad + i * 16);
        GV u = *q;
        T* v = (T*)&u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            if (ch < C) v[ch] = fromf<T>(tof<T>(v[ch]) + pixel(ch));
        *q = u;
    }
}

// levels, sizes and offsets; false when the shape is refused.  Workspace (floats): the pooled
// pred and target of levels 1..L-1, g_0..g_{L-1}, the tile sums of every level, kf[ML].
struct MsPlan {
    MsGeom gm;
    size_t pyr[ML];         // level i >= 1: its pooled pred (target follows, planes * H_i * W_i on)
    size_t gbase, pbase, kbase, total;
};
bool ms_plan(int B, int C, int H, int W, int levels, MsPlan* pl) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || levels < 1 || levels > ML) return false;
    if ((H < W ? H : W) < (1 << levels) || (size_t)B * C > 65535) return false;
    const size_t planes = (size_t)B * C;
    size_t off = 0, goff = 0;
    int poff = 0;
    for (int i = 0; i < levels; ++i) {
        const int Hi = H >> i, Wi = W >> i;
        const size_t n = planes * Hi * Wi;
        pl->gm.H[i] = Hi, pl->gm.W[i] = Wi;
        pl->pyr[i] = off;
        if (i > 0) off += 2 * n;
        pl->gm.goff[i] = goff;
        goff += n;
        const size_t tiles = planes * ((Hi + ST - 1) / ST) * ((Wi + ST - 1) / ST);
        if (tiles > (size_t)1 << 27) return false;
        pl->gm.poff[i] = poff, pl->gm.pcnt[i] = (int)tiles;
        poff += (int)tiles;
        pl->gm.inv_n[i] = (float)(1.0 / (double)n);
        pl->gm.pull[i] = (float)(1.0 / ((double)n * (double)((size_t)1 << (2 * i))));
    }
    pl->gbase = off;
    pl->pbase = pl->gbase + goff;
    pl->kbase = pl->pbase + poff;
    pl->total = pl->kbase + ML;
    return true;
}

}  // namespace

#define STREAM ((hipStream_t)stream)

extern "C" size_t fen_msssim_work_floats(int B, int C, int H, int W, int levels) {
    MsPlan pl;
    return ms_plan(B, C, H, W, levels, &pl) ? pl.total : 0;
}

extern "C" int fen_msssim(int dtype, int B, int C, int H, int W, const float* pred, const float* target,
                          const float* window1d, int window_size, float C1, float C2, const float* weights_dev,
                          int levels, float* work, float* out, void* grad, float grad_scale, int grad_mode,
                          void* stream) {
    if (!pred || !target || !window1d || !weights_dev || !work || !out || B <= 0 || C <= 0 || H <= 0 || W <= 0)
        return FEN_EINVAL;
    if (grad_mode < 0 || grad_mode > 2 || (grad_mode && !grad)) return FEN_EINVAL;
    if (const int st = fen_detail::check_dtype(dtype)) return st;
    if (grad_mode == 2 && (C > 3 || (dtype != FEN_F32 && dtype != FEN_BF16))) return FEN_EINVAL;
    if (window_size != 2 * SR + 1) return FEN_EUNSUPPORTED;
    if (levels < 1 || levels > ML) return FEN_EUNSUPPORTED;
    if ((H < W ? H : W) < (1 << levels)) return FEN_EUNSUPPORTED;
    MsPlan pl;
    if (!ms_plan(B, C, H, W, levels, &pl)) return FEN_EUNSUPPORTED;
    SsimWin w;
    for (int j = 0; j < 2 * SR + 1; ++j) w.g[j] = window1d[j];
    const MsGeom& gm = pl.gm;
    const size_t planes = (size_t)B * C;
    float* gmaps = work + pl.gbase;
    float* part = work + pl.pbase;
    float* kf = work + pl.kbase;
    const float* lp = pred;
    const float* lt = target;
    for (int i = 0; i < levels; ++i) {
        const int Hi = gm.H[i], Wi = gm.W[i];
        if (i > 0) {
            const size_t n = planes * Hi * Wi;
            float* po = work + pl.pyr[i];
            hipLaunchKernelGGL(k_ms_pool, dim3(nblk(n)), dim3(256), 0, STREAM, n, gm.H[i - 1], gm.W[i - 1], Hi, Wi, lp, lt,
                               po, po + n);
            lp = po, lt = po + n;
        }
        const dim3 grid((Wi + ST - 1) / ST, (Hi + ST - 1) / ST, (unsigned)planes);
        float* pi = part + gm.poff[i];
        float* gi = gmaps + gm.goff[i];
        const bool last = i + 1 == levels;
        if (grad_mode && last)
            hipLaunchKernelGGL((k_ms_level<true, true>), grid, dim3(256), 0, STREAM, Hi, Wi, lp, lt, w, C1, C2, pi, gi);
        else if (grad_mode)
            hipLaunchKernelGGL((k_ms_level<true, false>), grid, dim3(256), 0, STREAM, Hi, Wi, lp, lt, w, C1, C2, pi, gi);
        else if (last)
            hipLaunchKernelGGL((k_ms_level<false, true>), grid, dim3(256), 0, STREAM, Hi, Wi, lp, lt, w, C1, C2, pi, gi);
        else
            hipLaunchKernelGGL((k_ms_level<false, false>), grid, dim3(256), 0, STREAM, Hi, Wi, lp, lt, w, C1, C2, pi, gi);
    }
    hipLaunchKernelGGL(k_ms_finish, dim3(1), dim3(256), 0, STREAM, levels, gm, part, weights_dev, out, kf);
    if (grad_mode) {
        const dim3 grid(nblk((size_t)B * H * W));
        if (grad_mode == 1)
            hipLaunchKernelGGL((k_ms_combine<float, 1>), grid, dim3(256), 0, STREAM, B, C, H, W, levels, gm, gmaps, kf,
                               grad, grad_scale);
        else if (dtype == FEN_F32)
            hipLaunchKernelGGL((k_ms_combine<float, 2>), grid, dim3(256), 0, STREAM, B, C, H, W, levels, gm, gmaps, kf,
                               grad, grad_scale);
        else
            hipLaunchKernelGGL((k_ms_combine<bf16, 2>), grid, dim3(256), 0, STREAM, B, C, H, W, levels, gm, gmaps, kf,
                               grad, grad_scale);
    }
    FEN_CHECK_LAUNCH();
    return FEN_OK;
}

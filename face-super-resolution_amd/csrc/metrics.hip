// Per-image evaluation metrics (reference src/evaluation/metrics.py: psnr_batch 37-52, the SSIM
// module 67-78, MetricCalculator.evaluate_dataset 171-224) in one pass over SR and HR: the tile
// geometry and passes of ssim.hip's value-only form (ssim_common.h) -- one block = one 32x32 tile
// of one image plane, inputs on the tile + 5 px in LDS, the separable 11-tap passes, the SSIM map
// and its tile sum -- and, from the same registers the inputs were loaded into, the squared-error
// sum over the tile's own pixels.  pred may be clamped to [0, data_range] and quantised to 8 bits
// as it is loaded (flags): both sums see the transformed values, no extra pass over memory.
//
// A one-block finish reduces the tile sums per image in a fixed order (no atomics) to
// out[3][B] = mse, PSNR in dB, mean SSIM, and appends the valid images' PSNR / SSIM to a
// dataset-long table at a cursor kept in device memory, so a captured replay per batch serves a
// whole dataset with one host read at the end.
#include "ssim_common.h"

#include <math.h>

namespace {

constexpr int MF_CLAMP = 1, MF_QUANT = 2;

// pred as the metric sees it.  Quantisation as the reference's to_numpy (scripts/test_model.py:
// np.clip(x * 255, 0, 255).astype(uint8)) / 255: after the clamp to [0, 1], floor of the fp32
// product -- an explicit round-to-nearest multiply, so no contraction with a neighbouring add
// can change a code -- and an IEEE division.
__device__ __forceinline__ float metric_pred(float v, float data_range, int flags) {
    if (flags & MF_CLAMP) v = fminf(fmaxf(v, 0.f), data_range);
    if (flags & MF_QUANT) v = __fdiv_rn(floorf(__fmul_rn(v, 255.f)), 255.f);
    return v;
}

// part_ssim / part_sse [B * C][ntile]: this tile's sum of the SSIM map and of (pred - target)^2
// over the tile's own in-image pixels (each pixel of the plane in exactly one tile; the halo
// only feeds the filter).
__global__ __launch_bounds__(256) void k_metrics_tile(int H, int W, const float* __restrict__ pred,
                                                      const float* __restrict__ target, const SsimWin win, float C1,
                                                      float C2, float data_range, int flags,
                                                      float* __restrict__ part_ssim, float* __restrict__ part_sse) {
    constexpr int E2 = ST + 2 * SR;               // where the inputs are needed
    constexpr int CW = 8, NCH = ST / CW;          // horizontal pass: 8-column chunks
    constexpr int CWV = 4, NCHV = ST / CWV;       // vertical pass: 4-row chunks
    constexpr int PS = E2 + 1;
    constexpr int NSB = 2 * E2 * PS, NHP = 5 * E2 * (ST + 1);
    static_assert(E2 * NCH <= 256, "one horizontal item per thread");
    static_assert(ST * NCHV == 256, "one vertical item per thread");
    // the horizontal sums overwrite the staged inputs (every item takes its window into registers
    // before the barrier), as in k_ssim's value-only form: 27.7 KB of LDS
    __shared__ float sbuf[NSB > NHP ? NSB : NHP];
    __shared__ float red[2][4];
    float* sp = sbuf;
    float* st = sbuf + E2 * PS;
    float (*hp)[E2][ST + 1] = (float (*)[E2][ST + 1])sbuf;
    const int tid = threadIdx.x;
    const int h0 = blockIdx.y * ST, w0 = blockIdx.x * ST;
    const size_t pl = (size_t)blockIdx.z * H * W;
    constexpr int NLD = (E2 * E2 + 255) / 256;
    float lp[NLD], lt[NLD];
    float sse = 0.f;
#pragma unroll
    for (int k = 0; k < NLD; ++k) {               // every load issued before the first LDS write
        const int i = tid + k * 256;
        const int r = i / E2, c = i % E2, gy = h0 - SR + r, gx = w0 - SR + c;
        const bool in = i < E2 * E2 && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
        const size_t e = in ? pl + (size_t)gy * W + gx : 0;
        lp[k] = in ? metric_pred(pred[e], data_range, flags) : 0.f;
        lt[k] = in ? target[e] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
        const int i = tid + k * 256;
        if (i < E2 * E2) {
            const int r = i / E2, c = i % E2;
            sp[r * PS + c] = lp[k];
            st[r * PS + c] = lt[k];
            // the tile's own pixels (outside the image both values are 0)
            if (r >= SR && r < SR + ST && c >= SR && c < SR + ST) {
                const float d = lp[k] - lt[k];
                sse = fmaf(d, d, sse);
            }
        }
    }
    __syncthreads();
    {
        const int r = tid / NCH, c0 = (tid % NCH) * CW;
        const bool item = tid < E2 * NCH;
        float pw[CW + 2 * SR], tw[CW + 2 * SR];
        if (item) {
#pragma unroll
            for (int k = 0; k < CW + 2 * SR; ++k) pw[k] = sp[r * PS + c0 + k], tw[k] = st[r * PS + c0 + k];
        }
        __syncthreads();                          // every window in registers: sbuf is hp's now
        if (item) {
            float o[5][CW];
            hrow<CW>(win, pw, tw, o);
#pragma unroll
            for (int k = 0; k < 5; ++k)
#pragma unroll
                for (int c = 0; c < CW; ++c) hp[k][r][c0 + c] = o[k][c];
        }
    }
    __syncthreads();
    float acc = 0.f;
    {                                             // vertical pass + the map: one item per thread
        const int c = tid % ST, r0 = (tid / ST) * CWV;
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
            const float mp = m01[o].x, mt = m01[o].y;
            const float spp = m23[o].x - mp * mp, stt = m23[o].y - mt * mt, spt = m4[o] - mp * mt;
            const float A1 = 2.f * mp * mt + C1, A2 = 2.f * spt + C2;
            const float B1 = mp * mp + mt * mt + C1, B2 = spp + stt + C2;
            // v_rcp_f32 as in k_ssim: B1 >= C1 > 0, B2 >= C2 > 0 up to rounding
            const float S = (A1 * A2) * (__builtin_amdgcn_rcpf(B1) * __builtin_amdgcn_rcpf(B2));
            if (h0 + r0 + o < H && w0 + c < W) acc += S;
        }
    }
    // the tile's two sums: wave sums (fixed tree), then the 4 waves in order
    acc = wave_sum(acc);
    sse = wave_sum(sse);
    if ((tid & 63) == 0) red[0][tid >> 6] = acc, red[1][tid >> 6] = sse;
    __syncthreads();
    if (tid == 0) {
        const size_t q = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        part_ssim[q] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        part_sse[q] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

// One block, one wave per image in turn: the image's np = C * ntile tile sums lane-strided, then
// the wave tree -- a fixed order.  out[0][b] = mse, out[1][b] = 10 log10(range^2 / (mse + 1e-10))
// (psnr_batch), out[2][b] = mean SSIM.  With a table: images 0..n-1 (n = *nvalid, or B) go to
// table[0][c + i] (PSNR) and table[1][c + i] (SSIM), c = *cursor, entries below table_cap only;
// then *cursor = c + n whether they fitted or not.
__global__ __launch_bounds__(256) void k_metrics_finish(int B, int np, float count, float data_range,
                                                        const float* __restrict__ part_ssim,
                                                        const float* __restrict__ part_sse, float* __restrict__ out,
                                                        float* __restrict__ table, int table_cap, int* cursor,
                                                        const int* __restrict__ nvalid) {
    const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
    int c = 0, n = 0;
    if (table) {
        c = *cursor;
        n = nvalid ? *nvalid : B;
        n = n < 0 ? 0 : (n > B ? B : n);
    }
    for (int b = w; b < B; b += 4) {
        const float* qs = part_ssim + (size_t)b * np;
        const float* qe = part_sse + (size_t)b * np;
        float s = 0.f, e = 0.f;
        for (int k = lane; k < np; k += 64) s += qs[k], e += qe[k];
        s = wave_sum(s);
        e = wave_sum(e);
        if (lane == 0) {
            const float mse = e / count;
            const float psnr = 10.f * log10f(data_range * data_range / (mse + 1e-10f));
            const float ssim = s / count;
            out[b] = mse;
            out[B + b] = psnr;
            out[2 * B + b] = ssim;
            const long long idx = (long long)c + b;
            if (table && b < n && idx >= 0 && idx < table_cap) {
                table[idx] = psnr;
                table[(size_t)table_cap + idx] = ssim;
            }
        }
    }
    __syncthreads();                              // every wave has read *cursor
    if (table && tid == 0) *cursor = c + n;
}

// tiles per plane, or 0 when the shape is refused
size_t metrics_tiles(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (size_t)B * C > 65535) return 0;
    const size_t ntile = (size_t)((H + ST - 1) / ST) * ((W + ST - 1) / ST);
    if (ntile * C > (size_t)1 << 27 || (size_t)C * H * W > (size_t)1 << 31) return 0;
    return ntile;
}

}  // namespace

#define STREAM ((hipStream_t)stream)

extern "C" size_t fen_image_metrics_work_floats(int B, int C, int H, int W) {
    return 2 * (size_t)B * C * metrics_tiles(B, C, H, W);
}

extern "C" int fen_image_metrics(int B, int C, int H, int W, const float* pred, const float* target,
                                 const float* window1d, int window_size, float C1, float C2, float data_range,
                                 int flags, float* work, float* out, float* table, int table_cap, int* cursor,
                                 const int* nvalid, void* stream) {
    if (!pred || !target || !window1d || !work || !out) return FEN_EINVAL;
    if (table && (!cursor || table_cap <= 0)) return FEN_EINVAL;
    if ((flags & ~(MF_CLAMP | MF_QUANT)) || !(data_range > 0.f)) return FEN_EINVAL;
    if ((flags & MF_QUANT) && (!(flags & MF_CLAMP) || data_range != 1.f)) return FEN_EINVAL;
    if (window_size != 2 * SR + 1) return FEN_EUNSUPPORTED;
    const size_t ntile = metrics_tiles(B, C, H, W);
    if (!ntile) return FEN_EUNSUPPORTED;
    SsimWin w;
    for (int j = 0; j < 2 * SR + 1; ++j) w.g[j] = window1d[j];
    const size_t nparts = (size_t)B * C * ntile;
    const dim3 grid((W + ST - 1) / ST, (H + ST - 1) / ST, (unsigned)(B * C));
    hipLaunchKernelGGL(k_metrics_tile, grid, dim3(256), 0, STREAM, H, W, pred, target, w, C1, C2, data_range, flags,
                       work, work + nparts);
    hipLaunchKernelGGL(k_metrics_finish, dim3(1), dim3(256), 0, STREAM, B, (int)(C * ntile),
                       (float)((double)C * H * W), data_range, work, work + nparts, out, table, table_cap, cursor,
                       nvalid);
    FEN_CHECK_LAUNCH();
    return FEN_OK;
}

// ESRGAN baseline (RRDBNet, reference src/models/esrgan.py:17-103): 3x3 / stride 1 / pad 1
// convolutions over a GROWING CHANNEL CONCATENATION, as implicit GEMMs on MFMA (gfx950).
// The forward first; the dense blocks' backward (k_rrdb_dgrad, fen_rrdb_dgrad, fen_rrdb_block_bwd:
// the transfer model's stages 2 and 3) follows it, and its weight gradients are in wgrad.hip.
//
// A ResidualDenseBlock (esrgan.py:85-103) lives in ONE NHWC buffer of 192 channels per pixel,
//     x (0..63) | x1 (64..95) | x2 (96..127) | x3 (128..159) | x4 (160..191),
// which is torch.cat's channel order, so no concatenation is ever copied: conv k (k = 1..5)
// reads channels [0, 64 + 32(k-1)) of each pixel -- the pixel stride is 192, not Cin -- and
// conv 1..4 write their 32 outputs (bias + LeakyReLU(0.2)) into their own slice [64 + 32(k-1),
// 64 + 32k) of the same buffer.  THE READ AND WRITTEN CHANNEL RANGES OF ONE LAUNCH ARE DISJOINT
// (fen_rrdb_conv refuses a launch whose output slice of the input buffer starts below Cin), so
// the tiles of a launch are independent although a tile's halo is other tiles' output pixels.
// conv5's epilogue writes 0.2 v + x -- for the third block of an RRDB (esrgan.py:78-82)
// (0.2 v + x) 0.2 + x_rrdb, each product rounded before its sum as the reference's separate
// aten ops do -- straight into channels 0..63 of the NEXT block's buffer: no elementwise launch
// sits between two convs.  The buffers rotate through four, so the buffer a conv5 writes is
// never one of the RRDB's three inputs nor the holder of x_rrdb.
//
// The same kernel runs the network's other strided or gathered convs: conv_body (input = the
// last block's channels 0..63 at stride 192, epilogue + feat), conv_up1 / conv_up2 with the
// nearest x2 upsample folded into the gather (output pixel (h, w) taps input pixels ((h + dh)
// >> 1, (w + dw) >> 1): the upsampled tensor is never materialised), and conv_last (NCHW fp32
// store of the 3 real rows of a 16-row tile; no skip, no clamp).
//
// k_rrdb_conv: 256 threads = 4 waves, output tile 16 x 16 pixels x COT channels (64, 32 or
// 16), wave w owns rows 4w..4w+3: MT = COT / 16 by 4 accumulators of v_mfma_f32_16x16x32_
// {bf16,f16} (fp32: 4 x v_mfma_f32_16x16x4_f32 per 16 B, exact fp32 products).  K runs over Cin
// panels of 128 B (64 16-bit / 32 fp32 channels) x 9 taps.  A panel's 18 x 18 halo is staged
// through registers (zero padding, ragged tiles and channels >= Cin are ZEROS, never loaded:
// the slices past Cin hold another conv's output or stale data) into an LDS image with the
// column-keyed XOR swizzle of fen_common.h (conflict-free ds_read_b128); the next panel's halo
// loads are in flight during this panel's taps.  Weights ([9][Cout_pad][Cin], fen_pack_conv_w
// mode 0) stream per tap through a double-buffered LDS tile, one barrier per tap.  LDS 41.5 KB
// + 2 x COT x 128 B (57.9 KB at COT 64): two blocks per CU.  fp32 accumulation; no atomics,
// fixed order: two runs are bit-identical; every launch on the caller's stream.
#include "fen_common.h"

namespace {

constexpr int RRDB_FEAT = 64, RRDB_GROW = 32, RRDB_STRIDE = RRDB_FEAT + 4 * RRDB_GROW;
constexpr float RRDB_SLOPE = 0.2f;

// MFMAs of one tap: weight tile wt ([COT rows][128 B], swz) x halo image (hcol); the wave reads
// weight rows m*16 + c16 and halo rows wave*4 + n + kh, columns c16 + kw
template <typename T, int MT>
__device__ __forceinline__ void rrdb_tap(f32x4 (&acc)[MT][4], const char* wt, const char* halo, int tap, int wave,
                                         int q, int c16) {
    const int kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int chunk = kk * 4 + q;
        uint4 A[MT], Bf[4];
#pragma unroll
        for (int m = 0; m < MT; ++m) A[m] = *(const uint4*)(wt + swz(m * 16 + c16, chunk));
        const char* hb = halo + hcol(c16 + kw, chunk);
#pragma unroll
        for (int n = 0; n < 4; ++n) Bf[n] = *(const uint4*)(hb + (wave * 4 + n + kh) * (HALO * 128));
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) mma16<T>(acc[m][n], A[m], Bf[n]);
    }
}

template <typename T, int COT>
__global__ __launch_bounds__(256, 2) void k_rrdb_conv(const fen_rrdb_conv_desc d) {
    __shared__ __attribute__((aligned(16))) char halo[HALO_BYTES];
    __shared__ __attribute__((aligned(16))) char wbuf[2 * COT * 128];
    constexpr int MT = COT / 16;
    constexpr int WCH = COT * 8;               // 16-B weight chunks per (tap, panel)
    constexpr int WPT = (WCH + 255) / 256;
    constexpr int HPT = (HP * 8 + 255) / 256;  // 11 halo chunks per thread

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4, c16 = lane & 15;
    const int H = d.H, W = d.W, Cin = d.Cin, Cout = d.Cout;
    const int twn = (W + 15) >> 4, tpi = twn * ((H + 15) >> 4);
    const int tb = xcd_block();
    const int b = tb / tpi, tile = tb - b * tpi;
    const int h0 = (tile / twn) << 4, w0 = (tile % twn) << 4;
    const int co0 = blockIdx.y * COT;
    const int coutp = (Cout + 15) & ~15;
    // the input image: the output's size, or half of it under the fused nearest x2 upsample
    const int sh = d.up2 ? 1 : 0;
    const int Hin = H >> sh, Win = W >> sh;
    const char* xb = (const char*)d.x;
    const char* wb = (const char*)d.w;
    const size_t xpix = (size_t)d.x_stride * sizeof(T);   // bytes between pixels (>= the Cin read)
    const int cinb = Cin * (int)sizeof(T);                // bytes of a pixel this conv reads
    const int npan = (cinb + 127) >> 7;

    f32x4 acc[MT][4];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    uint4 hv[HPT];
    auto halo_load = [&](int pn) {
#pragma unroll
        for (int j = 0; j < HPT; ++j) {
            const int i = tid + j * 256;
            const int p = i >> 3, ch = i & 7;
            const int hr = p / HALO, hc = p - hr * HALO;
            const int gh = h0 + hr - 1, gw = w0 + hc - 1;    // output-grid coordinates of the tap
            const bool ok = i < HP * 8 && (unsigned)gh < (unsigned)H && (unsigned)gw < (unsigned)W &&
                            pn * 128 + ch * 16 < cinb;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (ok) v = *(const uint4*)(xb + ((size_t)(b * Hin + (gh >> sh)) * Win + (gw >> sh)) * xpix + pn * 128 + ch * 16);
            hv[j] = v;
        }
    };
    auto halo_store = [&]() {
#pragma unroll
        for (int j = 0; j < HPT; ++j) {
            const int i = tid + j * 256;
            if (i < HP * 8) *(uint4*)(halo + hswz(i >> 3, i & 7)) = hv[j];
        }
    };
    uint4 wr[WPT];
    // chunk index wrapped (COT 16: 128 chunks, duplicates store the same value twice)
    auto load_w = [&](int pn, int tap) {
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int i = (tid + j * 256) % WCH;
            const int r = i >> 3, ch = i & 7;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (pn * 128 + ch * 16 < cinb)
                v = *(const uint4*)(wb + (size_t)(tap * coutp + co0 + r) * cinb + pn * 128 + ch * 16);
            wr[j] = v;
        }
    };
    auto store_w = [&](char* dst) {
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int i = (tid + j * 256) % WCH;
            *(uint4*)(dst + swz(i >> 3, i & 7)) = wr[j];
        }
    };

    halo_load(0);
    for (int pn = 0; pn < npan; ++pn) {
        // the previous panel's last tap ended with a barrier: halo and wbuf[0] are free
        halo_store();
        load_w(pn, 0);
        store_w(wbuf);
        __syncthreads();
        if (pn + 1 < npan) halo_load(pn + 1);   // lands under this panel's MFMAs
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            if (tap < 8) load_w(pn, tap + 1);
            rrdb_tap<T, MT>(acc, wbuf + (tap & 1) * COT * 128, halo, tap, wave, q, c16);
            if (tap < 8) store_w(wbuf + ((tap + 1) & 1) * COT * 128);
            __syncthreads();
        }
    }

    // ---- epilogue: acc[m][n][r] = D[co0 + m*16 + 4q + r][pixel (h0 + 4 wave + n, w0 + c16)] ----
    const int w_ = w0 + c16;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int cob = co0 + m * 16 + q * 4;
        if (cob >= Cout) continue;
        float bias4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) bias4[r] = cob + r < Cout ? d.bias[cob + r] : 0.f;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int h = h0 + wave * 4 + n;
            if (h >= H || w_ >= W) continue;
            const size_t pix = (size_t)(b * H + h) * W + w_;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = acc[m][n][r] + bias4[r];
                if (d.lrelu) v[r] = prelu_f(v[r], RRDB_SLOPE);
            }
            // v * s + r with the product rounded first (the reference's `out * 0.2 + x` is two ops)
            if (d.r1) {
                float rv[4];
                ld4<T>((const char*)d.r1 + (pix * d.r1_stride + cob) * sizeof(T), rv);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = __fadd_rn(__fmul_rn(v[r], d.s1), rv[r]);
            }
            if (d.r2) {
                float rv[4];
                ld4<T>((const char*)d.r2 + (pix * d.r2_stride + cob) * sizeof(T), rv);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = __fadd_rn(__fmul_rn(v[r], d.s2), rv[r]);
            }
            if (d.nchw_out) {
                float* yf = (float*)d.y;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (cob + r < Cout) yf[(((size_t)b * Cout + cob + r) * H + h) * W + w_] = v[r];
            } else {
                st4<T>((char*)d.y + (pix * d.y_stride + d.y_off + cob) * sizeof(T), v);
            }
        }
    }
}

// conv_first (esrgan.py:36,55): NCHW fp32 [B,Ci,H,W] -> channels 0..63 of the first block's buffer
// (pixel stride ys) and, the same values, a dense NHWC [B,H,W,64] copy y2 (the `feat` of
// `feat + body_feat`, which the rotating buffers do not keep).  One thread = one pixel x 4
// channels; the filter transposed to [Ci*9][64] in LDS; fp32 sums in (ci, kh, kw) order.
template <typename T>
__global__ __launch_bounds__(256) void k_rrdb_first(int B, int Ci, int H, int W, const float* __restrict__ x,
                                                    const float* __restrict__ w, const float* __restrict__ bias,
                                                    T* __restrict__ y, int ys, T* __restrict__ y2) {
    __shared__ __attribute__((aligned(16))) float sw[8 * 9 * RRDB_FEAT];
    const int K = Ci * 9;
    for (int i = threadIdx.x; i < K * RRDB_FEAT; i += 256) {
        const int k = i / RRDB_FEAT, co = i - k * RRDB_FEAT;
        sw[i] = w[co * K + k];
    }
    __syncthreads();
    const size_t npx = (size_t)B * H * W;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t pix = gid >> 4;
    const int cg = (int)(gid & 15) * 4;
    if (pix >= npx) return;
    const int w_ = (int)(pix % W);
    const int h = (int)((pix / W) % H);
    const int b = (int)(pix / ((size_t)W * H));
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = bias[cg + r];
    for (int ci = 0; ci < Ci; ++ci) {
        const float* xp = x + ((size_t)b * Ci + ci) * H * W;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int ih = h + t / 3 - 1, iw = w_ + t % 3 - 1;
            const float xv = ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) ? xp[(size_t)ih * W + iw] : 0.f;
            const float4 wv = *(const float4*)(sw + (ci * 9 + t) * RRDB_FEAT + cg);
            v[0] += xv * wv.x; v[1] += xv * wv.y; v[2] += xv * wv.z; v[3] += xv * wv.w;
        }
    }
    st4<T>(y + pix * ys + cg, v);
    if (y2) st4<T>(y2 + pix * RRDB_FEAT + cg, v);
}

template <typename T, int COT>
int launch_rrdb(const fen_rrdb_conv_desc* d, hipStream_t s) {
    const int tpi = ((d->W + 15) >> 4) * ((d->H + 15) >> 4);
    const int coutp = (d->Cout + 15) & ~15;
    hipLaunchKernelGGL((k_rrdb_conv<T, COT>), dim3((unsigned)(d->B * tpi), coutp / COT), dim3(256), 0, s, *d);
    FEN_CHECK_LAUNCH();
    return FEN_OK;
}

template <typename T>
int dispatch_rrdb(const fen_rrdb_conv_desc* d, hipStream_t s) {
    if (d->Cout == 64) return launch_rrdb<T, 64>(d, s);
    if (d->Cout == 32) return launch_rrdb<T, 32>(d, s);
    return launch_rrdb<T, 16>(d, s);
}

// ---- backward: the data gradient of a dense block's conv (fen_rrdb_dgrad) ----
// dx[.., 0:Cout) (+)= s * conv(dy[.., dy_off : dy_off + Cin); wt), wt = fen_pack_conv_w mode 2
// ([9][Cout][Cin], taps flipped): the forward's implicit GEMM with a NARROW K (Cin = 32 or 64:
// one 128-B panel in 16 bits, one or two in fp32) and a WIDE N (Cout = 64..192).  The dy halo --
// every panel of it -- is therefore staged in LDS ONCE per 16 x 16 tile and the 64-row output-
// channel tiles loop over it; only the weights stream, per (channel tile, panel, tap), through
// the forward's double-buffered LDS tile with one barrier per step.  Rows >= Cout of the last
// channel tile (Cout = 96, 160) are zero weights, never stored.  Epilogue per 4 channels: v =
// s acc (+ what dx holds) (+ s1 r1 + s2 r2 on channels 0..63), times LeakyReLU'(act) -- act > 0 ?
// 1 : 0.2 on the stored forward output -- on the top 32 channels written; one store in dtype.
// A tile reads dy's channel range of its halo and rewrites only its own pixels of dx's [0, Cout):
// the ranges are disjoint (refused otherwise), so tiles are independent; no atomics, fixed order.
// LDS: NPAN x 41.5 KB halo + 16 KB weights (bf16 56.5 KB, two blocks per CU; fp32 97 KB, one).
template <typename T, int NPAN>
__global__ __launch_bounds__(256) void k_rrdb_dgrad(const fen_rrdb_dgrad_desc d) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* halo = smem;                          // [NPAN][HALO_BYTES]
    char* wbuf = smem + NPAN * HALO_BYTES;      // [2][64 rows][128 B]
    constexpr int COT = 64, MT = 4;
    constexpr int WPT = COT * 8 / 256;          // 2 weight chunks per thread and step
    constexpr int HPT = (HP * 8 + 255) / 256;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4, c16 = lane & 15;
    const int H = d.H, W = d.W, Cout = d.Cout;
    const int twn = (W + 15) >> 4, tpi = twn * ((H + 15) >> 4);
    const int tb = xcd_block();
    const int b = tb / tpi, tile = tb - b * tpi;
    const int h0 = (tile / twn) << 4, w0 = (tile % twn) << 4;
    const char* yb = (const char*)d.dy + (size_t)d.dy_off * sizeof(T);
    const char* wb = (const char*)d.w;
    const size_t ypix = (size_t)d.dy_stride * sizeof(T);
    const int cinb = d.Cin * (int)sizeof(T);    // bytes of a pixel's dy slice: 64, 128 or 256
    const int npan = (cinb + 127) >> 7;         // <= NPAN (dispatch)
    const int nct = (Cout + COT - 1) / COT;

    uint4 wr[WPT];
    auto load_w = [&](int ct, int pn, int tap) {
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int i = tid + j * 256;
            const int r = i >> 3, ch = i & 7;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (ct * COT + r < Cout && pn * 128 + ch * 16 < cinb)
                v = *(const uint4*)(wb + (size_t)(tap * Cout + ct * COT + r) * cinb + pn * 128 + ch * 16);
            wr[j] = v;
        }
    };
    auto store_w = [&](char* dst) {
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int i = tid + j * 256;
            *(uint4*)(dst + swz(i >> 3, i & 7)) = wr[j];
        }
    };

    // the whole dy halo, once: zero padding, ragged tiles and chunks past Cin are zeros
    load_w(0, 0, 0);
    for (int pn = 0; pn < npan; ++pn) {
        uint4 hv[HPT];
#pragma unroll
        for (int j = 0; j < HPT; ++j) {
            const int i = tid + j * 256;
            const int p = i >> 3, ch = i & 7;
            const int hr = p / HALO, hc = p - hr * HALO;
            const int gh = h0 + hr - 1, gw = w0 + hc - 1;
            const bool ok = i < HP * 8 && (unsigned)gh < (unsigned)H && (unsigned)gw < (unsigned)W &&
                            pn * 128 + ch * 16 < cinb;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (ok) v = *(const uint4*)(yb + ((size_t)(b * H + gh) * W + gw) * ypix + pn * 128 + ch * 16);
            hv[j] = v;
        }
#pragma unroll
        for (int j = 0; j < HPT; ++j) {
            const int i = tid + j * 256;
            if (i < HP * 8) *(uint4*)(halo + pn * HALO_BYTES + hswz(i >> 3, i & 7)) = hv[j];
        }
    }
    store_w(wbuf);
    __syncthreads();

    const int w_ = w0 + c16;
    const int act0 = Cout - RRDB_GROW;          // first channel the activation derivative scales
    int par = 0;
    for (int ct = 0; ct < nct; ++ct) {
        f32x4 acc[MT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int pn = 0; pn < npan; ++pn) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                // the step after this one: next tap, next panel, or the next channel tile's first
                const bool more = tap < 8 || pn + 1 < npan || ct + 1 < nct;
                if (more) {
                    if (tap < 8) load_w(ct, pn, tap + 1);
                    else if (pn + 1 < npan) load_w(ct, pn + 1, 0);
                    else load_w(ct + 1, 0, 0);
                }
                rrdb_tap<T, MT>(acc, wbuf + par * (COT * 128), halo + pn * HALO_BYTES, tap, wave, q, c16);
                if (more) store_w(wbuf + (par ^ 1) * (COT * 128));
                __syncthreads();
                par ^= 1;
            }
        }
        // ---- epilogue: acc[m][n][r] = D[ct*64 + m*16 + 4q + r][pixel (h0 + 4 wave + n, w0 + c16)] ----
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int cob = ct * COT + m * 16 + q * 4;
            if (cob >= Cout) continue;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                // one pixel's loads at a time: hoisted together, the 16 x 4 operand loads of the
                // tile's epilogue spill
                __builtin_amdgcn_sched_barrier(0);
                const int h = h0 + wave * 4 + n;
                if (h >= H || w_ >= W) continue;
                const size_t pix = (size_t)(b * H + h) * W + w_;
                char* dxp = (char*)d.dx + (pix * d.dx_stride + cob) * sizeof(T);
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = acc[m][n][r] * d.s;
                if (d.accumulate) {
                    float o[4];
                    ld4<T>(dxp, o);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] += o[r];
                }
                if (cob < RRDB_FEAT) {
                    if (d.r1) {
                        float rv[4];
                        ld4<T>((const char*)d.r1 + (pix * d.r1_stride + cob) * sizeof(T), rv);
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] += d.s1 * rv[r];
                    }
                    if (d.r2) {
                        float rv[4];
                        ld4<T>((const char*)d.r2 + (pix * d.r2_stride + cob) * sizeof(T), rv);
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] += d.s2 * rv[r];
                    }
                }
                if (d.act && cob >= act0) {
                    float a[4];
                    ld4<T>((const char*)d.act + (pix * d.act_stride + cob) * sizeof(T), a);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = prelu_bwd_f(v[r], a[r], RRDB_SLOPE);
                }
                st4<T>(dxp, v);
            }
        }
    }
}

template <typename T, int NPAN>
int launch_rrdb_dgrad(const fen_rrdb_dgrad_desc* d, hipStream_t s) {
    constexpr int LDS = NPAN * HALO_BYTES + 2 * 64 * 128;
    const int tpi = ((d->W + 15) >> 4) * ((d->H + 15) >> 4);
    fen_detail::opt_in_lds<k_rrdb_dgrad<T, NPAN>>(LDS);
    hipLaunchKernelGGL((k_rrdb_dgrad<T, NPAN>), dim3((unsigned)(d->B * tpi)), dim3(256), LDS, s, *d);
    FEN_CHECK_LAUNCH();
    return FEN_OK;
}

// pixel indices and the grid's x dimension are ints in the kernels
bool pixels_ok(int B, int H, int W) { return (size_t)B * (size_t)H * (size_t)W < ((size_t)1 << 31); }

}  // namespace

extern "C" int fen_rrdb_conv(const fen_rrdb_conv_desc* d, void* stream) {
    if (!d || !d->x || !d->w || !d->bias || !d->y) return FEN_EINVAL;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->Cin <= 0 || d->Cout <= 0) return FEN_EINVAL;
    if (fen_detail::check_dtype(d->dtype) != FEN_OK) return FEN_EINVAL;
    if (((uintptr_t)d->x | (uintptr_t)d->w | (uintptr_t)d->y | (uintptr_t)d->r1 | (uintptr_t)d->r2) & 15) return FEN_EINVAL;
    const int esz = d->dtype == FEN_F32 ? 4 : 2;
    // the network's channel counts only: inputs 64 + 32 j, outputs 32 / 64, or <= 16 planes of NCHW fp32
    if (d->Cin < RRDB_FEAT || d->Cin > RRDB_STRIDE || (d->Cin - RRDB_FEAT) % RRDB_GROW) return FEN_EUNSUPPORTED;
    if (d->nchw_out ? d->Cout > 16 : (d->Cout != RRDB_GROW && d->Cout != RRDB_FEAT)) return FEN_EUNSUPPORTED;
    if (d->x_stride < d->Cin || (d->x_stride * esz) % 16) return FEN_EINVAL;
    if (!d->nchw_out && (d->y_off < 0 || d->y_stride < d->y_off + d->Cout || d->y_stride % 4 || d->y_off % 4))
        return FEN_EINVAL;
    if ((d->r1 && (d->r1_stride < d->Cout || d->r1_stride % 4)) || (d->r2 && (d->r2_stride < d->Cout || d->r2_stride % 4)))
        return FEN_EINVAL;
    if (d->up2 && ((d->H | d->W) & 1)) return FEN_EINVAL;
    // in place (a dense block's conv 1..4): the written slice lies past every channel read
    if (d->x == d->y && (d->nchw_out || d->y_off < d->Cin)) return FEN_EINVAL;
    if (!pixels_ok(d->B, d->H, d->W)) return FEN_EUNSUPPORTED;
    return fen_detail::with_dtype(d->dtype, [&](auto tag) { return dispatch_rrdb<decltype(tag)>(d, (hipStream_t)stream); });
}

extern "C" int fen_rrdb_block(const fen_rrdb_block_desc* d, void* stream) {
    if (!d || !d->buf || !d->next) return FEN_EINVAL;
    for (int k = 0; k < 5; ++k)
        if (!d->w[k] || !d->bias[k]) return FEN_EINVAL;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->num_feat <= 0 || d->num_grow_ch <= 0) return FEN_EINVAL;
    if (fen_detail::check_dtype(d->dtype) != FEN_OK) return FEN_EINVAL;
    if (d->next == d->buf || (d->x_rrdb && d->x_rrdb == d->next)) return FEN_EINVAL;
    if (d->num_feat != RRDB_FEAT || d->num_grow_ch != RRDB_GROW) return FEN_EUNSUPPORTED;
    if (!pixels_ok(d->B, d->H, d->W)) return FEN_EUNSUPPORTED;
    for (int k = 0; k < 5; ++k) {
        fen_rrdb_conv_desc c = {};
        c.dtype = d->dtype;
        c.B = d->B; c.H = d->H; c.W = d->W;
        c.Cin = RRDB_FEAT + RRDB_GROW * k;
        c.x = d->buf; c.x_stride = RRDB_STRIDE;
        c.w = d->w[k]; c.bias = d->bias[k];
        c.y_stride = RRDB_STRIDE;
        if (k < 4) {
            c.Cout = RRDB_GROW;
            c.y = d->buf; c.y_off = c.Cin;
            c.lrelu = 1;
        } else {
            c.Cout = RRDB_FEAT;
            c.y = d->next; c.y_off = 0;
            c.r1 = d->buf; c.r1_stride = RRDB_STRIDE; c.s1 = RRDB_SLOPE;      // x5 * 0.2 + x
            if (d->x_rrdb) { c.r2 = d->x_rrdb; c.r2_stride = RRDB_STRIDE; c.s2 = RRDB_SLOPE; }   // out * 0.2 + x
        }
        const int rc = fen_rrdb_conv(&c, stream);
        if (rc != FEN_OK) return rc;
    }
    return FEN_OK;
}

extern "C" int fen_rrdb_first(int dtype, int B, int Ci, int H, int W, const float* x, const float* w,
                              const float* bias, void* y, int y_stride, void* y2, void* stream) {
    if (!x || !w || !bias || !y || B <= 0 || Ci <= 0 || H <= 0 || W <= 0) return FEN_EINVAL;
    if (fen_detail::check_dtype(dtype) != FEN_OK || y_stride < RRDB_FEAT || y_stride % 4) return FEN_EINVAL;
    if (Ci > 8 || !pixels_ok(B, H, W)) return FEN_EUNSUPPORTED;
    const size_t nthr = (size_t)B * H * W * 16;
    const unsigned nb = (unsigned)((nthr + 255) / 256);
    return fen_detail::with_dtype(dtype, [&](auto tag) -> int {
        using T = decltype(tag);
        hipLaunchKernelGGL(k_rrdb_first<T>, dim3(nb), dim3(256), 0, (hipStream_t)stream, B, Ci, H, W, x, w, bias, (T*)y,
                           y_stride, (T*)y2);
        FEN_CHECK_LAUNCH();
        return FEN_OK;
    });
}

extern "C" int fen_rrdb_dgrad(const fen_rrdb_dgrad_desc* d, void* stream) {
    if (!d || !d->dy || !d->w || !d->dx) return FEN_EINVAL;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->Cin <= 0 || d->Cout <= 0) return FEN_EINVAL;
    if (fen_detail::check_dtype(d->dtype) != FEN_OK) return FEN_EINVAL;
    if (d->dtype == FEN_F16) return FEN_EUNSUPPORTED;   // fp16 is inference-only
    if (((uintptr_t)d->dy | (uintptr_t)d->w | (uintptr_t)d->dx | (uintptr_t)d->r1 | (uintptr_t)d->r2 |
         (uintptr_t)d->act) & 15)
        return FEN_EINVAL;
    const int esz = d->dtype == FEN_F32 ? 4 : 2;
    if ((d->Cin != RRDB_GROW && d->Cin != RRDB_FEAT) || d->Cout < RRDB_FEAT || d->Cout > RRDB_STRIDE ||
        (d->Cout - RRDB_FEAT) % RRDB_GROW)
        return FEN_EUNSUPPORTED;
    if (d->dy_off < 0 || d->dy_stride < d->dy_off + d->Cin || (d->dy_stride * esz) % 16 || (d->dy_off * esz) % 16)
        return FEN_EINVAL;
    if (d->dx_stride < d->Cout || (d->dx_stride * esz) % 16) return FEN_EINVAL;
    if ((d->r1 && (d->r1_stride < RRDB_FEAT || (d->r1_stride * esz) % 16)) ||
        (d->r2 && (d->r2_stride < RRDB_FEAT || (d->r2_stride * esz) % 16)) ||
        (d->act && (d->act_stride < d->Cout || (d->act_stride * esz) % 16)))
        return FEN_EINVAL;
    // in place (a block's gradient buffer): the slice read lies past every channel written
    if (d->dy == d->dx && d->dy_off < d->Cout) return FEN_EINVAL;
    if (!pixels_ok(d->B, d->H, d->W)) return FEN_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (d->dtype == FEN_BF16) return launch_rrdb_dgrad<bf16, 1>(d, s);
    return d->Cin * 4 <= 128 ? launch_rrdb_dgrad<float, 1>(d, s) : launch_rrdb_dgrad<float, 2>(d, s);
}

extern "C" size_t fen_rrdb_block_bwd_work_floats(int dtype, int B, int H, int W) {
    size_t need = 0;
    for (int k = 0; k < 5; ++k) {
        fen_rrdb_wgrad_desc g = {};
        g.dtype = dtype; g.B = B; g.H = H; g.W = W;
        g.Cin = RRDB_FEAT + RRDB_GROW * k;
        g.Cout = k < 4 ? RRDB_GROW : RRDB_FEAT;
        const size_t n = fen_rrdb_wgrad_work_floats(&g);
        if (n > need) need = n;
    }
    return need;
}

extern "C" int fen_rrdb_block_bwd(const fen_rrdb_block_bwd_desc* d, void* stream) {
    if (!d || !d->buf || !d->D || !d->g) return FEN_EINVAL;
    bool any_w = false;
    for (int k = 0; k < 5; ++k) {
        if (!d->wt[k]) return FEN_EINVAL;
        if (d->db[k] && !d->dw[k]) return FEN_EINVAL;
        any_w = any_w || d->dw[k];
    }
    if (any_w && !d->work) return FEN_EINVAL;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->num_feat <= 0 || d->num_grow_ch <= 0) return FEN_EINVAL;
    if (fen_detail::check_dtype(d->dtype) != FEN_OK) return FEN_EINVAL;
    if (d->dtype == FEN_F16) return FEN_EUNSUPPORTED;
    if (d->D == d->buf || d->g == d->D || d->g_rrdb == d->D) return FEN_EINVAL;
    if (d->num_feat != RRDB_FEAT || d->num_grow_ch != RRDB_GROW) return FEN_EUNSUPPORTED;
    if (!pixels_ok(d->B, d->H, d->W)) return FEN_EUNSUPPORTED;
    // the third block of an RRDB sits behind `out * 0.2 + x_rrdb`: its incoming gradient is 0.2 g
    const float gs = d->third ? RRDB_SLOPE : 1.f;
    for (int k = 4; k >= 0; --k) {
        fen_rrdb_dgrad_desc c = {};
        c.dtype = d->dtype;
        c.B = d->B; c.H = d->H; c.W = d->W;
        c.Cout = RRDB_FEAT + RRDB_GROW * k;
        c.w = d->wt[k];
        c.dx = d->D; c.dx_stride = RRDB_STRIDE;
        if (k == 4) {      // conv5: D = 0.2 dgrad(g) on all 192 channels, + g on the first 64
            c.Cin = RRDB_FEAT;
            c.dy = d->g; c.dy_stride = d->g_stride; c.dy_off = 0;
            c.s = RRDB_SLOPE * gs;
            c.r1 = d->g; c.r1_stride = d->g_stride; c.s1 = gs;
        } else {           // conv k + 1: D[0 : Cout) += dgrad(dpre), dpre = D's slice at Cout
            c.Cin = RRDB_GROW;
            c.dy = d->D; c.dy_stride = RRDB_STRIDE; c.dy_off = c.Cout;
            c.s = 1.f;
            c.accumulate = 1;
            if (k == 0 && d->g_rrdb) { c.r2 = d->g_rrdb; c.r2_stride = d->g_rrdb_stride; c.s2 = 1.f; }
        }
        if (k > 0) { c.act = d->buf; c.act_stride = RRDB_STRIDE; }   // completes x_k's slice
        const int rc = fen_rrdb_dgrad(&c, stream);
        if (rc != FEN_OK) return rc;
    }
    // the weight gradients: x = the forward buffer, dy = D's slices (dpre_1..4) and 0.2 gs g (dpre_5)
    for (int k = 0; k < 5; ++k) {
        if (!d->dw[k]) continue;
        fen_rrdb_wgrad_desc g = {};
        g.dtype = d->dtype;
        g.B = d->B; g.H = d->H; g.W = d->W;
        g.Cin = RRDB_FEAT + RRDB_GROW * k;
        g.x = d->buf; g.x_stride = RRDB_STRIDE;
        if (k < 4) {
            g.Cout = RRDB_GROW;
            g.dy = d->D; g.dy_stride = RRDB_STRIDE; g.dy_off = g.Cin;
            g.scale = 1.f;
        } else {
            g.Cout = RRDB_FEAT;
            g.dy = d->g; g.dy_stride = d->g_stride; g.dy_off = 0;
            g.scale = RRDB_SLOPE * gs;
        }
        g.dw = d->dw[k]; g.db = d->db[k];
        g.accumulate = d->accumulate;
        g.work = d->work;
        const int rc = fen_rrdb_wgrad(&g, stream);
        if (rc != FEN_OK) return rc;
    }
    return FEN_OK;
}

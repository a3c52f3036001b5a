// ESRGAN baseline (RRDBNet, reference src/models/esrgan.py:17-103): 3x3 / stride 1 / pad 1
// convolutions over a GROWING CHANNEL CONCATENATION, as implicit GEMMs on MFMA (gfx950).
// Inference only.
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

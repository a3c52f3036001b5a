// Host-side AddressSanitizer check of the C-ABI ("Race detection /
// sanitizers"): `make asan` builds libfen_hip with the HOST half of every HIP source
// instrumented (-Xarch_host -fsanitize=address; device code is untouched) and this driver,
// linked with the ASan runtime, calls every host path of include/fen.h that runs without a GPU:
// the pure queries, each entry point's argument validation, the multi-job table builders
// (fen_pack_table, fen_wgrad_multi_work_floats), the chained group launch's descriptor checks,
// table build and hash (fen_group_strip_chain_prepare up to its launch), the status word
// exchange and the RCCL entry points' refusals and library resolution.  Any heap / stack
// overflow, use-after-free or leak in those paths aborts the run with an ASan report; a wrong
// return code fails an expectation.  Not product code: nothing links it but the asan target.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fen.h"

static int g_fail = 0;
#define EXPECT(c)                                                          \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                      \
        }                                                                  \
    } while (0)

static void* fake(size_t i) { return (void*)(uintptr_t)(0x10000 * (i + 1)); }

static void pure_queries() {
    for (int c = -8; c <= 1; ++c) EXPECT(fen_status_string(c) != nullptr && std::strlen(fen_status_string(c)) > 0);
    EXPECT(std::strstr(fen_build_info(), "gfx950") != nullptr);
    EXPECT(fen_last_hip_error() != nullptr);
    EXPECT(fen_packed_elems(0, 3, 64) == 9 * 16 * 64);
    EXPECT(fen_packed_elems(2, 256, 64) == 9 * 64 * 256);
    EXPECT(fen_pool_parts(4096) == 64);
    EXPECT(fen_sumsq_parts(5115651) == 1024);
    EXPECT(fen_feat_loss_parts() > 0);
    EXPECT(fen_ssim_parts(2, 3, 64, 64) > 0 && fen_ssim_work_floats(2, 3, 64, 64) == (size_t)3 * 2 * 3 * 64 * 64);
    EXPECT(fen_bn_work_floats(64) > 0);
    {   // grouped BN refusals (host checks only: no launch)
        float f = 0.f;
        EXPECT(fen_bn_stats_n(FEN_BF16, 0, 16, 64, &f, 1e-5f, 0.1f, &f, nullptr, nullptr, &f, nullptr) == FEN_EINVAL);
        EXPECT(fen_bn_stats_n(FEN_BF16, 2, 16, 60, &f, 1e-5f, 0.1f, &f, nullptr, nullptr, &f, nullptr) == FEN_EINVAL);
        EXPECT(fen_bn_stats_n(FEN_BF16, 2, 16, 64, &f, 1e-5f, 0.1f, &f, &f, nullptr, &f, nullptr) == FEN_EINVAL);
        EXPECT(fen_bn_apply_n(FEN_BF16, 2, 16, 64, &f, &f, &f, 32, &f, &f, 0.2f, &f, nullptr) == FEN_EINVAL);
        EXPECT(fen_bn_apply_n(FEN_BF16, 1, 16, 2048, &f, &f, &f, 0, &f, &f, 0.2f, &f, nullptr) == FEN_EUNSUPPORTED);
        EXPECT(fen_bn_bwd_n(FEN_BF16, 0, 16, 64, &f, &f, &f, &f, &f, 0.2f, &f, &f, &f, 0, &f, nullptr) == FEN_EINVAL);
        EXPECT(fen_bn_bwd_n(FEN_BF16, 2, 16, 64, &f, &f, &f, &f, &f, 0.2f, &f, &f, &f, 0, nullptr, nullptr) == FEN_EINVAL);
    }
    EXPECT(fen_conv_first_work_floats(2, 3, 64, 64, 64) > 0);
    EXPECT(fen_conv_last_dgrad_part_rows(2, 256, 256) > 0);
    EXPECT(fen_group_strip_work_bytes(32, 64) > 0 && fen_group_strip_bwd_work_bytes(32, 64) > 0);
    EXPECT(fen_group_strip_bwd_dal_rows(32, 64) > 0);
    EXPECT(fen_rcab_c128_tiles(128, 128) > 0);
    EXPECT(fen_group_strip_supported(FEN_BF16, 32, 64, 64, 64, 16, 10) == 1);
    EXPECT(fen_group_strip_supported(FEN_F32, 32, 64, 64, 64, 16, 10) == 0);
    EXPECT(fen_rcab_deferred_supported(FEN_BF16, 32, 64, 64, 64, 16) == 1);
    EXPECT(fen_rcab_deferred_supported(FEN_BF16, 32, 64, 64, 128, 32) == 0);
}

static void conv_refusals() {
    EXPECT(fen_conv3x3(nullptr, nullptr) == FEN_EINVAL);
    fen_conv_desc d;
    std::memset(&d, 0, sizeof d);
    d.dtype = FEN_BF16, d.B = 1, d.H = 8, d.W = 8, d.Cin = 36, d.Cout = 64;   // 72-B rows
    d.x = d.w = d.y = fake(0);
    EXPECT(fen_conv3x3(&d, nullptr) == FEN_EUNSUPPORTED);
    d.Cin = 64;
    d.epi = FEN_EPI_DOT;
    EXPECT(fen_conv3x3(&d, nullptr) == FEN_EINVAL);                      // no pre_in / part
    d.pre_in = fake(1), d.part = (float*)fake(2);
    d.epi = FEN_EPI_DOT | FEN_EPI_POOL;
    EXPECT(fen_conv3x3(&d, nullptr) == FEN_EUNSUPPORTED);
    d.epi = FEN_EPI_SHUFFLE | FEN_EPI_UNSHUFFLE;
    EXPECT(fen_conv3x3(&d, nullptr) == FEN_EUNSUPPORTED);
    d.epi = 0, d.s2d_in = 48;
    EXPECT(fen_conv3x3(&d, nullptr) == FEN_EINVAL);
    d.s2d_in = 0, d.dtype = 7;
    EXPECT(fen_conv3x3(&d, nullptr) == FEN_EINVAL);
    d.dtype = FEN_BF16, d.pre_in = nullptr, d.part = nullptr;
    d.epi = FEN_EPI_RELU_BWD;
    EXPECT(fen_conv3x3(&d, nullptr) == FEN_EINVAL);                      // no pre_in
    d.pre_in = fake(1), d.part = (float*)fake(2);
    d.epi = FEN_EPI_RELU_BWD | FEN_EPI_PRELU_BWD;
    d.alpha = (const float*)fake(3);
    EXPECT(fen_conv3x3(&d, nullptr) == FEN_EUNSUPPORTED);
    d.epi = 1 << 20;
    EXPECT(fen_conv3x3(&d, nullptr) == FEN_EINVAL);                      // unknown flag
    d.epi = 0, d.y_images = 1;
    EXPECT(fen_conv3x3(&d, nullptr) == FEN_EINVAL);                      // y_images without y_pool
    d.y_images = 0, d.y_pool = fake(4);
    EXPECT(fen_conv3x3(&d, nullptr) == FEN_EUNSUPPORTED);                // y_pool without PReLU
}

static void wgrad_tables() {
    std::vector<fen_wgrad_desc> a(FEN_WGRAD_MAXJOBS + 1);
    for (auto& d : a) {
        std::memset(&d, 0, sizeof d);
        d.dtype = FEN_BF16, d.B = 32, d.H = 64, d.W = 64, d.Cin = 64, d.Cout = 64, d.cout_valid = 64;
        d.x = d.dy = fake(0), d.dw = (float*)fake(1), d.work = (float*)fake(2);
    }
    EXPECT(fen_wgrad3x3_multi(0, a.data(), nullptr) == FEN_EINVAL);
    EXPECT(fen_wgrad3x3_multi(FEN_WGRAD_MAXJOBS + 1, a.data(), nullptr) == FEN_EINVAL);
    EXPECT(fen_wgrad_multi_work_floats(FEN_WGRAD_MAXJOBS + 1, a.data()) == 0);
    const size_t one = fen_wgrad_work_floats(&a[0]);
    EXPECT(one == (size_t)256 * (64 * 64 * 9 + 64));
    EXPECT(fen_wgrad_multi_work_floats(4, a.data()) == one);
    for (int n : {1, 7, FEN_WGRAD_MAXJOBS}) EXPECT(fen_wgrad_multi_work_floats(n, a.data()) > 0);
    a[2].H = 32;
    EXPECT(fen_wgrad3x3_multi(4, a.data(), nullptr) == FEN_EINVAL);
    a[2].H = 64, a[3].x = nullptr;
    EXPECT(fen_wgrad3x3_multi(4, a.data(), nullptr) == FEN_EINVAL);
}

static void pack_tables() {
    // the post-step re-pack table of a full 6x10 network's 131 convs + the upsampler / tail
    const int nj = 140;
    std::vector<fen_pack_job> jobs(nj);
    for (int i = 0; i < nj; ++i)
        jobs[i] = fen_pack_job{(const float*)fake(2 * i), fake(2 * i + 1), i % 3, i % 3 == 1 ? 256 : 64, 64};
    std::vector<char> tab(fen_pack_table_bytes(nj));
    size_t total = 0;
    EXPECT(fen_pack_table(FEN_BF16, nj, jobs.data(), tab.data(), &total) == FEN_OK && total > 0);
    EXPECT(fen_pack_table(FEN_BF16, 0, jobs.data(), tab.data(), &total) == FEN_EINVAL);
    jobs[5].mode = 3;
    EXPECT(fen_pack_table(FEN_BF16, nj, jobs.data(), tab.data(), &total) == FEN_EINVAL);
    EXPECT(fen_pack_multi(FEN_BF16, 0, nullptr, 0, nullptr) == FEN_EINVAL);
}

static void chain_tables() {
    const int B = 2, H = 64, nb = 10, G = 6;
    const size_t nbytes = fen_group_strip_chain_work_bytes(B, H, G);
    EXPECT(nbytes > fen_group_strip_work_bytes(B, H));
    EXPECT(fen_group_strip_chain_work_bytes(B, 12, G) == 0);
    std::vector<fen_group_strip_desc> ds(G);
    for (int g = 0; g < G; ++g) {
        fen_group_strip_desc& d = ds[g];
        std::memset(&d, 0, sizeof d);
        d.dtype = FEN_BF16, d.B = B, d.H = H, d.W = 64, d.C = 64, d.Cr = 16, d.nb = nb, d.res_scale = 0.2f;
        d.x = fake(g + 1), d.y = fake(g + 2);
        for (int j = 0; j < nb; ++j) {
            d.w1[j] = d.w2[j] = fake(100 + j);
            d.b1[j] = d.b2[j] = d.alpha[j] = d.fc1[j] = d.fc2[j] = (const float*)fake(200 + j);
        }
        d.wg = fake(300), d.bg = (const float*)fake(301);
        d.work = fake(400), d.work_bytes = nbytes;
    }
    ds[1].x = fake(90);                                                  // not a chain
    EXPECT(fen_group_strip_chain(ds.data(), G, nullptr, nullptr) == FEN_EINVAL);
    EXPECT(fen_group_strip_chain_prepare(ds.data(), G, nullptr, nullptr) == FEN_EINVAL);
    ds[1].x = ds[0].y;
    fen_group_strip_chain_tail t{fake(500), (const float*)fake(501), ds[0].x, ds[G - 1].y};
    EXPECT(fen_group_strip_chain_prepare(ds.data(), G, &t, nullptr) == FEN_EINVAL);   // tail writes the body's output
    t.y = fake(600);
    // a valid chain: the table is built and hashed on the host; without a GPU the copy-kernel
    // launch then fails (FEN_EHIP) -- ASan covers everything before it
    const int rc = fen_group_strip_chain_prepare(ds.data(), G, &t, nullptr);
    EXPECT(rc == FEN_OK || rc == FEN_EHIP);
    std::vector<fen_group_strip_desc> big(13, ds[0]);
    for (int g = 0; g < 13; ++g) big[g].nb = 19, big[g].x = fake(g + 1), big[g].y = fake(g + 2);
    EXPECT(fen_group_strip_chain_prepare(big.data(), 13, nullptr, nullptr) == FEN_EUNSUPPORTED);
}

static void status_and_rccl() {
    EXPECT(std::strncmp(fen_status_string(FEN_ERCCL), "FEN_ERCCL", 9) == 0);
    EXPECT(fen_rccl_allreduce_bucket(nullptr, nullptr, 16, nullptr) == FEN_EINVAL);
    EXPECT(fen_rccl_init(nullptr, nullptr, 1, 0, 0) == FEN_EINVAL);
    void* h = nullptr;
    unsigned char uid[128] = {0};
    EXPECT(fen_rccl_init(&h, uid, 2, 2, 0) == FEN_EINVAL);
    EXPECT(fen_rccl_check(nullptr) == FEN_EINVAL);
    EXPECT(fen_rccl_destroy(nullptr) == FEN_OK);
    EXPECT(fen_rccl_library() != nullptr);                               // dlopen / dlsym path
    EXPECT(fen_last_rccl_error() != nullptr);
    int* w = (int*)std::malloc(sizeof(int));
    *w = 3;
    EXPECT(fen_status_take(w) == 3 && *w == 0);
    EXPECT(fen_status_take(w) == 0);
    EXPECT(fen_status_take(nullptr) == 0);
    std::free(w);
}

static void misc_refusals() {
    EXPECT(fen_rcab_deferred(nullptr, nullptr) == FEN_EINVAL);
    EXPECT(fen_group_strip(nullptr, nullptr) == FEN_EINVAL);
    EXPECT(fen_group_strip_bwd(nullptr, nullptr) == FEN_EINVAL);
    EXPECT(fen_rcab_c128(nullptr, nullptr) == FEN_EINVAL);
    EXPECT(fen_rcab_bwd(nullptr, nullptr) == FEN_EINVAL);
    EXPECT(fen_colsum_multi(0, nullptr, nullptr) == FEN_EINVAL);
    EXPECT(fen_ssim_ex(FEN_BF16, 2, 3, 64, 64, nullptr, nullptr, nullptr, 11, 1e-4f, 9e-4f, nullptr, nullptr, 1.f, 2,
                       (float*)fake(0), nullptr) == FEN_EINVAL);
    EXPECT(fen_bicubic_down4(0, 3, 256, 256, nullptr, nullptr, nullptr) == FEN_EINVAL);
    {   // fen_msssim: every refusal is a host check before the first launch
        float* f = (float*)fake(0);
        EXPECT(fen_msssim_work_floats(2, 3, 64, 64, 5) > 0 && fen_msssim_work_floats(2, 3, 16, 16, 5) == 0);
        EXPECT(fen_msssim(FEN_F32, 2, 3, 64, 64, nullptr, f, f, 11, 1e-4f, 9e-4f, f, 5, f, f, nullptr, 0.f, 0, nullptr) == FEN_EINVAL);
        EXPECT(fen_msssim(FEN_F32, 2, 3, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, nullptr, 5, f, f, nullptr, 0.f, 0, nullptr) == FEN_EINVAL);
        EXPECT(fen_msssim(FEN_F32, 2, 3, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, f, 5, nullptr, f, nullptr, 0.f, 0, nullptr) == FEN_EINVAL);
        EXPECT(fen_msssim(FEN_F32, 2, 3, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, f, 5, f, nullptr, nullptr, 0.f, 0, nullptr) == FEN_EINVAL);
        EXPECT(fen_msssim(FEN_F32, 2, 3, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, f, 5, f, f, nullptr, 1.f, 1, nullptr) == FEN_EINVAL);
        EXPECT(fen_msssim(FEN_F32, 2, 3, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, f, 5, f, f, f, 1.f, 3, nullptr) == FEN_EINVAL);
        EXPECT(fen_msssim(FEN_BF16, 2, 4, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, f, 5, f, f, f, 1.f, 2, nullptr) == FEN_EINVAL);
        EXPECT(fen_msssim(FEN_F32, 2, 3, 64, 64, f, f, f, 7, 1e-4f, 9e-4f, f, 5, f, f, nullptr, 0.f, 0, nullptr) == FEN_EUNSUPPORTED);
        EXPECT(fen_msssim(FEN_F32, 2, 3, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, f, 9, f, f, nullptr, 0.f, 0, nullptr) == FEN_EUNSUPPORTED);
        EXPECT(fen_msssim(FEN_F32, 2, 3, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, f, 0, f, f, nullptr, 0.f, 0, nullptr) == FEN_EUNSUPPORTED);
        EXPECT(fen_msssim(FEN_F32, 2, 3, 16, 16, f, f, f, 11, 1e-4f, 9e-4f, f, 5, f, f, nullptr, 0.f, 0, nullptr) == FEN_EUNSUPPORTED);
    }
    {   // fen_image_metrics: likewise
        float* f = (float*)fake(0);
        int* ip = (int*)fake(1);
        EXPECT(fen_image_metrics_work_floats(2, 3, 40, 72) == (size_t)2 * 2 * 3 * 2 * 3);
        EXPECT(fen_image_metrics_work_floats(0, 3, 64, 64) == 0 && fen_image_metrics_work_floats(2, 3, 64, -1) == 0);
        EXPECT(fen_image_metrics_work_floats(30000, 3, 64, 64) == 0);
        EXPECT(fen_image_metrics(2, 3, 64, 64, nullptr, f, f, 11, 1e-4f, 9e-4f, 1.f, 0, f, f, nullptr, 0, nullptr, nullptr, nullptr) == FEN_EINVAL);
        EXPECT(fen_image_metrics(2, 3, 64, 64, f, nullptr, f, 11, 1e-4f, 9e-4f, 1.f, 0, f, f, nullptr, 0, nullptr, nullptr, nullptr) == FEN_EINVAL);
        EXPECT(fen_image_metrics(2, 3, 64, 64, f, f, nullptr, 11, 1e-4f, 9e-4f, 1.f, 0, f, f, nullptr, 0, nullptr, nullptr, nullptr) == FEN_EINVAL);
        EXPECT(fen_image_metrics(2, 3, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, 1.f, 0, nullptr, f, nullptr, 0, nullptr, nullptr, nullptr) == FEN_EINVAL);
        EXPECT(fen_image_metrics(2, 3, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, 1.f, 0, f, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == FEN_EINVAL);
        EXPECT(fen_image_metrics(2, 3, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, 1.f, 1, f, f, f, 8, nullptr, nullptr, nullptr) == FEN_EINVAL);   // table, no cursor
        EXPECT(fen_image_metrics(2, 3, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, 1.f, 1, f, f, f, 0, ip, nullptr, nullptr) == FEN_EINVAL);        // table_cap 0
        EXPECT(fen_image_metrics(2, 3, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, 1.f, 2, f, f, nullptr, 0, nullptr, nullptr, nullptr) == FEN_EINVAL);   // quantise without clamp
        EXPECT(fen_image_metrics(2, 3, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, 255.f, 3, f, f, nullptr, 0, nullptr, nullptr, nullptr) == FEN_EINVAL); // quantise, range != 1
        EXPECT(fen_image_metrics(2, 3, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, 1.f, 4, f, f, nullptr, 0, nullptr, nullptr, nullptr) == FEN_EINVAL);   // unknown flag
        EXPECT(fen_image_metrics(2, 3, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, 0.f, 0, f, f, nullptr, 0, nullptr, nullptr, nullptr) == FEN_EINVAL);
        EXPECT(fen_image_metrics(2, 3, 64, 64, f, f, f, 7, 1e-4f, 9e-4f, 1.f, 0, f, f, nullptr, 0, nullptr, nullptr, nullptr) == FEN_EUNSUPPORTED);
        EXPECT(fen_image_metrics(30000, 3, 64, 64, f, f, f, 11, 1e-4f, 9e-4f, 1.f, 0, f, f, nullptr, 0, nullptr, nullptr, nullptr) == FEN_EUNSUPPORTED);
        EXPECT(fen_image_metrics(2, 3, 0, 64, f, f, f, 11, 1e-4f, 9e-4f, 1.f, 0, f, f, nullptr, 0, nullptr, nullptr, nullptr) == FEN_EUNSUPPORTED);
    }
}

// fen_rrdb_conv / fen_rrdb_block / fen_rrdb_first: every refusal is decided on the host, before
// any launch
static void rrdb_refusals() {
    EXPECT(fen_rrdb_conv(nullptr, nullptr) == FEN_EINVAL);
    fen_rrdb_conv_desc d;
    std::memset(&d, 0, sizeof d);
    d.dtype = FEN_F16, d.B = 1, d.H = 8, d.W = 8, d.Cin = 64, d.Cout = 32;
    d.x = d.y = fake(0), d.w = fake(1), d.bias = (const float*)fake(2);
    d.x_stride = d.y_stride = 192, d.y_off = 32;
    EXPECT(fen_rrdb_conv(&d, nullptr) == FEN_EINVAL);                    // in place inside the read range
    d.y = fake(3), d.Cin = 80;
    EXPECT(fen_rrdb_conv(&d, nullptr) == FEN_EUNSUPPORTED);
    d.Cin = 64, d.Cout = 48;
    EXPECT(fen_rrdb_conv(&d, nullptr) == FEN_EUNSUPPORTED);
    d.Cout = 32, d.x_stride = 60;
    EXPECT(fen_rrdb_conv(&d, nullptr) == FEN_EINVAL);
    d.x_stride = 192, d.B = 1 << 11, d.H = 1 << 10, d.W = 1 << 10;
    EXPECT(fen_rrdb_conv(&d, nullptr) == FEN_EUNSUPPORTED);              // 2^31 pixels
    d.B = 1, d.H = 7, d.W = 8, d.up2 = 1;
    EXPECT(fen_rrdb_conv(&d, nullptr) == FEN_EINVAL);
    d.up2 = 0, d.dtype = 9;
    EXPECT(fen_rrdb_conv(&d, nullptr) == FEN_EINVAL);
    d.dtype = FEN_F32, d.bias = nullptr;
    EXPECT(fen_rrdb_conv(&d, nullptr) == FEN_EINVAL);
    d.bias = (const float*)fake(2), d.x = (const char*)fake(0) + 8;
    EXPECT(fen_rrdb_conv(&d, nullptr) == FEN_EINVAL);                    // not 16-B aligned
    d.x = fake(0), d.nchw_out = 1, d.Cout = 17;
    EXPECT(fen_rrdb_conv(&d, nullptr) == FEN_EUNSUPPORTED);

    EXPECT(fen_rrdb_block(nullptr, nullptr) == FEN_EINVAL);
    fen_rrdb_block_desc b;
    std::memset(&b, 0, sizeof b);
    b.dtype = FEN_BF16, b.B = 1, b.H = 8, b.W = 8, b.num_feat = 64, b.num_grow_ch = 16;
    b.buf = fake(0), b.next = fake(1);
    for (int k = 0; k < 5; ++k) b.w[k] = fake(2), b.bias[k] = (const float*)fake(3);
    EXPECT(fen_rrdb_block(&b, nullptr) == FEN_EUNSUPPORTED);
    b.num_feat = 32, b.num_grow_ch = 32;
    EXPECT(fen_rrdb_block(&b, nullptr) == FEN_EUNSUPPORTED);
    b.num_feat = 64, b.next = b.buf;
    EXPECT(fen_rrdb_block(&b, nullptr) == FEN_EINVAL);
    b.next = fake(1), b.x_rrdb = b.next;
    EXPECT(fen_rrdb_block(&b, nullptr) == FEN_EINVAL);
    b.x_rrdb = nullptr, b.bias[4] = nullptr;
    EXPECT(fen_rrdb_block(&b, nullptr) == FEN_EINVAL);
    b.bias[4] = (const float*)fake(3), b.W = 0;
    EXPECT(fen_rrdb_block(&b, nullptr) == FEN_EINVAL);

    const float* f = (const float*)fake(0);
    EXPECT(fen_rrdb_first(FEN_F32, 1, 3, 8, 8, nullptr, f, f, fake(1), 192, nullptr, nullptr) == FEN_EINVAL);
    EXPECT(fen_rrdb_first(FEN_F32, 1, 3, 8, 8, f, f, f, fake(1), 48, nullptr, nullptr) == FEN_EINVAL);
    EXPECT(fen_rrdb_first(FEN_F32, 0, 3, 8, 8, f, f, f, fake(1), 192, nullptr, nullptr) == FEN_EINVAL);
    EXPECT(fen_rrdb_first(FEN_F32, 1, 9, 8, 8, f, f, f, fake(1), 192, nullptr, nullptr) == FEN_EUNSUPPORTED);
}

// every entry point that takes a dtype refuses a code that is no fen_dtype with FEN_EINVAL before
// any launch (tests/test_abi.py holds the same calls)
static void unknown_dtype_refusals() {
    void* p = fake(0);
    float* f = (float*)fake(0);
    const float win[11] = {0.f};
    for (int dt : {3, -1}) {
        fen_conv_desc c;
        std::memset(&c, 0, sizeof c);
        c.dtype = dt, c.B = 1, c.H = 16, c.W = 16, c.Cin = 64, c.Cout = 64, c.x = c.w = c.y = p;
        EXPECT(fen_conv3x3(&c, nullptr) == FEN_EINVAL);
        fen_wgrad_desc wg[2];
        std::memset(wg, 0, sizeof wg);
        for (auto& w : wg) {
            w.dtype = dt, w.B = 1, w.H = 16, w.W = 16, w.Cin = 64, w.Cout = 64, w.cout_valid = 64;
            w.x = w.dy = p, w.dw = w.work = f;
        }
        EXPECT(fen_wgrad3x3(&wg[0], nullptr) == FEN_EINVAL);
        EXPECT(fen_wgrad3x3_multi(2, wg, nullptr) == FEN_EINVAL);
        fen_rcab_deferred_desc r;
        std::memset(&r, 0, sizeof r);
        r.dtype = dt, r.B = 1, r.H = 16, r.W = 16, r.C = 64, r.Cr = 16;
        r.x = r.w1 = r.w2 = r.t = p, r.b1 = r.b2 = r.alpha = f, r.part = f;
        EXPECT(fen_rcab_deferred(&r, nullptr) == FEN_EINVAL);
        r.tp = p, r.pp = r.pfc1 = r.pfc2 = f;
        EXPECT(fen_rcab_group_end(&r, p, f, p, p, nullptr) == FEN_EINVAL);
        fen_rcab_bwd_desc rb;
        std::memset(&rb, 0, sizeof rb);
        rb.dtype = dt, rb.B = 1, rb.H = 16, rb.W = 16, rb.C = 64;
        rb.dt = rb.w2t = rb.w1t = rb.z1 = p, rb.dy = p, rb.alpha = f, rb.dz1 = rb.dx = p, rb.dalpha_part = f;
        EXPECT(fen_rcab_bwd(&rb, nullptr) == FEN_EINVAL);
        std::vector<fen_group_strip_desc> gs(2);
        for (int g = 0; g < 2; ++g) {
            fen_group_strip_desc& d = gs[g];
            std::memset(&d, 0, sizeof d);
            d.dtype = dt, d.B = 1, d.H = 64, d.W = 64, d.C = 64, d.Cr = 16, d.nb = 1, d.res_scale = 0.2f;
            d.x = fake(g + 1), d.y = fake(g + 2);
            d.w1[0] = d.w2[0] = p, d.b1[0] = d.b2[0] = d.alpha[0] = d.fc1[0] = d.fc2[0] = f;
            d.wg = p, d.bg = f, d.work = fake(400), d.work_bytes = fen_group_strip_chain_work_bytes(1, 64, 2);
        }
        EXPECT(fen_group_strip(&gs[0], nullptr) == FEN_EINVAL);
        EXPECT(fen_group_strip_chain_prepare(gs.data(), 2, nullptr, nullptr) == FEN_EINVAL);
        EXPECT(fen_group_strip_chain(gs.data(), 2, nullptr, nullptr) == FEN_EINVAL);
        fen_group_strip_bwd_desc gb;
        std::memset(&gb, 0, sizeof gb);
        gb.dtype = dt, gb.B = 1, gb.H = 64, gb.W = 64, gb.C = 64, gb.Cr = 16, gb.nb = 1, gb.res_scale = 0.2f;
        gb.dy = fake(1), gb.dx = fake(2), gb.wgt = p, gb.work = fake(400);
        gb.work_bytes = fen_group_strip_bwd_work_bytes(1, 64);
        gb.w1t[0] = gb.w2t[0] = gb.z1[0] = gb.t[0] = gb.a1[0] = p, gb.dt[0] = gb.dz1[0] = p;
        gb.alpha[0] = gb.fc1[0] = gb.fc2[0] = gb.s[0] = gb.mean[0] = gb.hid[0] = f;
        gb.dalpha_part[0] = gb.dw1p[0] = gb.dw2p[0] = f;
        EXPECT(fen_group_strip_bwd(&gb, nullptr) == FEN_EINVAL);
        fen_rcab_c128_desc c128;
        std::memset(&c128, 0, sizeof c128);
        c128.dtype = dt, c128.B = 1, c128.H = 16, c128.W = 16, c128.C = 128, c128.Cr = 16, c128.mode = 3;
        c128.x = c128.w = c128.res = fake(1), c128.bias = f, c128.y = fake(2);
        EXPECT(fen_rcab_c128(&c128, nullptr) == FEN_EINVAL);
        fen_rrdb_conv_desc rc;
        std::memset(&rc, 0, sizeof rc);
        rc.dtype = dt, rc.B = 1, rc.H = 8, rc.W = 8, rc.Cin = 64, rc.Cout = 32;
        rc.x = rc.w = fake(1), rc.bias = f, rc.y = fake(2), rc.x_stride = rc.y_stride = 192, rc.y_off = 64;
        EXPECT(fen_rrdb_conv(&rc, nullptr) == FEN_EINVAL);
        fen_rrdb_block_desc blk;
        std::memset(&blk, 0, sizeof blk);
        blk.dtype = dt, blk.B = 1, blk.H = 8, blk.W = 8, blk.num_feat = 64, blk.num_grow_ch = 32;
        blk.buf = fake(1), blk.next = fake(2);
        for (int k = 0; k < 5; ++k) blk.w[k] = p, blk.bias[k] = f;
        EXPECT(fen_rrdb_block(&blk, nullptr) == FEN_EINVAL);
        EXPECT(fen_rrdb_first(dt, 1, 3, 16, 16, f, f, f, p, 192, nullptr, nullptr) == FEN_EINVAL);
        EXPECT(fen_conv_first_fwd(dt, 1, 3, 16, 16, 64, f, f, f, p, nullptr) == FEN_EINVAL);
        EXPECT(fen_conv_first_fwd_ex(dt, 1, 3, 16, 16, 64, f, f, f, f, f, 0.2f, p, nullptr) == FEN_EINVAL);
        EXPECT(fen_conv_first_wgrad(dt, 1, 3, 16, 16, 64, f, p, f, f, 0, f, nullptr) == FEN_EINVAL);
        EXPECT(fen_conv_last_dgrad(dt, 1, 16, 16, 64, 3, p, f, p, p, f, p, f, nullptr) == FEN_EINVAL);
        EXPECT(fen_conv_last_bwd(dt, 1, 16, 16, 64, 3, p, f, p, p, f, p, f, f, f, nullptr) == FEN_EINVAL);
        EXPECT(fen_se_fused(dt, 1, 256, 64, 16, 4, 1.f / 256, f, f, f, f, f, f, p, 0.2f, p, p, nullptr) == FEN_EINVAL);
        EXPECT(fen_se_apply(dt, 1, 256, 64, p, f, 0.2f, p, p, nullptr) == FEN_EINVAL);
        EXPECT(fen_pool_dot(dt, 1, 256, 64, p, p, f, nullptr) == FEN_EINVAL);
        EXPECT(fen_se_bwd_fused(dt, 1, 256, 64, 16, 4, 1.f / 256, 0.2f, f, f, f, f, f, f, p, f, f, f, p, nullptr) == FEN_EINVAL);
        EXPECT(fen_se_bwd_apply(dt, 1, 256, 64, p, f, 0.2f, f, p, nullptr) == FEN_EINVAL);
        EXPECT(fen_pack_conv_w(dt, 0, 64, 64, f, p, nullptr) == FEN_EINVAL);
        {
            fen_pack_job job{f, p, 0, 64, 64};
            std::vector<char> tab(fen_pack_table_bytes(1));
            size_t total = 0;
            EXPECT(fen_pack_table(dt, 1, &job, tab.data(), &total) == FEN_EINVAL);
        }
        EXPECT(fen_pack_multi(dt, 1, p, 256, nullptr) == FEN_EINVAL);
        EXPECT(fen_nchw_to_nhwc(dt, 1, 3, 16, 16, 8, f, p, nullptr) == FEN_EINVAL);
        EXPECT(fen_nhwc_to_nchw(dt, 1, 3, 16, 16, p, f, nullptr) == FEN_EINVAL);
        EXPECT(fen_prelu_bwd_unshuffle(dt, 1, 16, 16, 64, p, p, f, p, f, nullptr) == FEN_EINVAL);
        EXPECT(fen_maxpool2(dt, 1, 16, 16, 64, p, p, nullptr) == FEN_EINVAL);
        EXPECT(fen_maxpool2_bwd_relu(dt, 1, 16, 16, 64, p, p, p, nullptr) == FEN_EINVAL);
        EXPECT(fen_feat_loss(dt, 64, p, 0, 1.f, p, 0, f, nullptr) == FEN_EINVAL);
        EXPECT(fen_ssim(dt, 1, 3, 16, 16, f, f, win, 11, 1e-4f, 9e-4f, f, p, 1.f, 2, nullptr) == FEN_EINVAL);
        EXPECT(fen_ssim_ex(dt, 1, 3, 16, 16, f, f, win, 11, 1e-4f, 9e-4f, f, p, 1.f, 2, f, nullptr) == FEN_EINVAL);
        EXPECT(fen_msssim(dt, 1, 3, 32, 32, f, f, win, 11, 1e-4f, 9e-4f, f, 2, f, f, p, 1.f, 1, nullptr) == FEN_EINVAL);
        EXPECT(fen_bn_stats(dt, 64, 64, p, 1e-5f, 0.1f, f, nullptr, nullptr, f, nullptr) == FEN_EINVAL);
        EXPECT(fen_bn_stats_n(dt, 2, 64, 64, p, 1e-5f, 0.1f, f, nullptr, nullptr, f, nullptr) == FEN_EINVAL);
        EXPECT(fen_bn_apply(dt, 64, 64, p, f, f, f, f, 0.2f, p, nullptr) == FEN_EINVAL);
        EXPECT(fen_bn_apply_n(dt, 2, 64, 64, p, f, f, 64, f, f, 0.2f, p, nullptr) == FEN_EINVAL);
        EXPECT(fen_bn_bwd(dt, 64, 64, p, p, f, f, f, 0.2f, p, f, f, 0, f, nullptr) == FEN_EINVAL);
        EXPECT(fen_bn_bwd_n(dt, 2, 64, 64, p, p, f, f, f, 0.2f, p, f, f, 0, f, nullptr) == FEN_EINVAL);
        EXPECT(fen_subsample2(dt, 1, 16, 16, 64, p, p, nullptr) == FEN_EINVAL);
        EXPECT(fen_s2d2(dt, 1, 16, 16, 64, p, p, 0, nullptr) == FEN_EINVAL);
        EXPECT(fen_zero_insert2(dt, 1, 8, 8, 64, p, p, nullptr) == FEN_EINVAL);
    }
}

// `asan_check overflow`: hands fen_pack_table a table one job too short -- the library's own
// write past it must be caught (proves the host half of libfen_hip_asan.so is instrumented)
static int overflow_selftest() {
    const int nj = 8;
    std::vector<fen_pack_job> jobs(nj, fen_pack_job{(const float*)fake(0), fake(1), 0, 64, 64});
    char* tab = (char*)std::malloc(fen_pack_table_bytes(nj - 1));
    size_t total = 0;
    const int rc = fen_pack_table(FEN_BF16, nj, jobs.data(), tab, &total);
    std::free(tab);
    std::printf("overflow self-test NOT caught (rc %d)\n", rc);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "overflow") == 0) return overflow_selftest();
    pure_queries();
    conv_refusals();
    wgrad_tables();
    pack_tables();
    chain_tables();
    status_and_rccl();
    misc_refusals();
    rrdb_refusals();
    unknown_dtype_refusals();
    if (g_fail) {
        std::fprintf(stderr, "asan_check: %d expectation(s) failed\n", g_fail);
        return 1;
    }
    std::printf("asan_check: all host paths clean under AddressSanitizer\n");
    return 0;
}

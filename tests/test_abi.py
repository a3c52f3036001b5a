"""The C-ABI library loads on CPU and exports every entry point include/fen.h declares."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "fen.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fen_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported():
    from src.hip import lib as L
    lib = L.load()
    names = _declared()
    assert len(names) >= 25
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(L.EXPORTED), set(names) ^ set(L.EXPORTED)


def test_status_strings_and_pure_queries():
    from src.hip import lib as L
    lib = L.load()
    assert lib.fen_status_string(-2).startswith(b"FEN_EUNSUPPORTED")
    assert b"gfx950" in lib.fen_build_info()
    assert lib.fen_packed_elems(0, 3, 64) == 9 * 16 * 64
    assert lib.fen_packed_elems(2, 256, 64) == 9 * 64 * 256
    assert lib.fen_pool_parts(4096) == 64
    assert lib.fen_sumsq_parts(5115651) == 1024


def test_bad_args_rejected_without_gpu():
    """Argument validation happens before any launch, so it is testable on CPU."""
    from src.hip import lib as L
    lib = L.load()
    d = L.ConvDesc()
    assert lib.fen_conv3x3(None, None) == L.load().fen_conv3x3(None, None) == -1
    d.dtype, d.B, d.H, d.W, d.Cin, d.Cout = 1, 1, 8, 8, 36, 64  # 72-B pixel rows: not whole 16-B chunks
    d.x = d.w = d.y = 16
    assert lib.fen_conv3x3(d, None) == -2
    with pytest.raises(L.FenError):
        L.check(-2, "conv")


def test_rcab_deferred_validation_without_gpu():
    from src.hip import lib as L
    lib = L.load()
    assert lib.fen_rcab_deferred(None, None) == -1
    assert lib.fen_rcab_deferred_supported(L.BF16, 32, 64, 64, 64, 16) == 1
    assert lib.fen_rcab_deferred_supported(L.F16, 32, 64, 64, 64, 16) == 1
    assert lib.fen_rcab_deferred_supported(L.F32, 32, 64, 64, 64, 16) == 0      # 16-bit only
    assert lib.fen_rcab_deferred_supported(L.BF16, 32, 64, 60, 64, 16) == 0     # W % 16
    assert lib.fen_rcab_deferred_supported(L.BF16, 32, 64, 64, 128, 32) == 0    # C = 64 only
    d = L.RcabDeferredDesc()
    d.dtype, d.B, d.H, d.W, d.C, d.Cr = L.BF16, 2, 32, 32, 64, 16
    d.x = d.w1 = d.w2 = d.b1 = d.b2 = d.alpha = d.t = d.part = 16
    d.tp = 16                       # deferred input without part_{j-1} / fc weights / x_j out
    assert lib.fen_rcab_deferred(d, None) == -1
    d.tp, d.z1 = 0, 16              # z1 without a1
    assert lib.fen_rcab_deferred(d, None) == -1


def test_wgrad_multi_validation_without_gpu():
    """fen_wgrad3x3_multi: job count bounds, one shape per launch, workspace size (n jobs of
    the persistent kernel share the ~256 slabs of one job)."""
    import ctypes
    from src.hip import lib as L
    lib = L.load()
    arr = (L.WgradDesc * 33)()                                    # FEN_WGRAD_MAXJOBS + 1
    for d in arr:
        d.dtype, d.B, d.H, d.W, d.Cin, d.Cout, d.cout_valid = L.BF16, 32, 64, 64, 64, 64, 64
        d.x = d.dy = d.dw = d.work = 16
    p = ctypes.cast(arr, ctypes.c_void_p)
    assert lib.fen_wgrad3x3_multi(0, p, None) == -1
    assert lib.fen_wgrad3x3_multi(33, p, None) == -1
    assert lib.fen_wgrad_multi_work_floats(33, p) == 0
    one = lib.fen_wgrad_work_floats(ctypes.byref(arr[0]))
    assert one == 256 * (64 * 64 * 9 + 64)
    assert lib.fen_wgrad_multi_work_floats(4, p) == one          # 4 jobs x 64 chunks
    arr[2].H = 32                                                 # shapes differ
    assert lib.fen_wgrad3x3_multi(4, p, None) == -1
    arr[2].H = 64
    arr[3].x = None
    assert lib.fen_wgrad3x3_multi(4, p, None) == -1
    arr[3].x = 16
    # njobs x (Cout/64) x (Cin/64) > 256 even at one chunk per job: the launch geometry must
    # terminate (one chunk per job, more than one wave of blocks) rather than spin on the host
    for n, c in ((5, 512), (17, 256)):
        for d in arr:
            d.Cin = d.Cout = d.cout_valid = c
        assert lib.fen_wgrad_multi_work_floats(n, p) == n * (c * c * 9 + c)


def test_conv_dot_epilogue_validation_without_gpu():
    """FEN_EPI_DOT needs pre_in (the dotted tensor) and part, and is one partial-sum stream:
    not combinable with POOL / PRELU_BWD, SHUFFLE / UNSHUFFLE or LAST."""
    from src.hip import lib as L
    lib = L.load()
    d = L.ConvDesc()
    d.dtype, d.B, d.H, d.W, d.Cin, d.Cout = L.BF16, 1, 16, 16, 64, 64
    d.x = d.w = d.y = 16
    d.epi = L.EPI_DOT
    assert lib.fen_conv3x3(d, None) == -1            # no pre_in / part
    d.pre_in = d.part = 16
    d.epi = L.EPI_DOT | L.EPI_POOL
    assert lib.fen_conv3x3(d, None) == -2
    d.epi = L.EPI_DOT | L.EPI_UNSHUFFLE
    assert lib.fen_conv3x3(d, None) == -2


def test_conv_relu_bwd_and_pool_validation_without_gpu():
    """FEN_EPI_RELU_BWD needs pre_in and excludes the other pre_in modes; y_images needs y_pool;
    y_pool needs the PReLU epilogue and even H, W (all refused before any launch)."""
    from src.hip import lib as L
    lib = L.load()
    d = L.ConvDesc()
    d.dtype, d.B, d.H, d.W, d.Cin, d.Cout = L.BF16, 2, 16, 16, 64, 64
    d.x = d.w = d.y = 16
    d.epi = L.EPI_RELU_BWD
    assert lib.fen_conv3x3(d, None) == -1            # no pre_in
    d.pre_in = d.part = d.alpha = 16
    d.epi = L.EPI_RELU_BWD | L.EPI_PRELU_BWD
    assert lib.fen_conv3x3(d, None) == -2
    d.epi = L.EPI_RELU_BWD | L.EPI_SHUFFLE
    assert lib.fen_conv3x3(d, None) == -2
    d.epi = 1 << 20
    assert lib.fen_conv3x3(d, None) == -1            # unknown flag
    d.epi, d.y_images = L.EPI_PRELU, 1
    assert lib.fen_conv3x3(d, None) == -1            # y_images without y_pool
    d.y_pool, d.y_images = 16, 3
    assert lib.fen_conv3x3(d, None) == -1            # y_images > B
    d.epi, d.y_images = 0, 0
    assert lib.fen_conv3x3(d, None) == -2            # y_pool without PReLU
    d.epi, d.H = L.EPI_PRELU, 15
    assert lib.fen_conv3x3(d, None) == -2            # odd H


def test_group_strip_chain_validation_without_gpu():
    """fen_group_strip_chain's host checks run before any copy or launch: a broken chain, too many
    step tags and a tail aliasing the body's buffers are refused on CPU (a launch without a
    matching prepared table is refused on the GPU, by the kernel: test_gpu_group_chain.py)."""
    from src.hip import lib as L
    lib = L.load()
    B, H, nb, G = 2, 64, 2, 3
    nbytes = lib.fen_group_strip_chain_work_bytes(B, H, G)
    assert nbytes > lib.fen_group_strip_work_bytes(B, H)
    assert lib.fen_group_strip_chain_work_bytes(B, 12, G) == 0          # H not a multiple of 8
    ds = (L.GroupStripDesc * G)()
    for g in range(G):
        d = ds[g]
        d.dtype, d.B, d.H, d.W, d.C, d.Cr, d.nb, d.res_scale = 1, B, H, 64, 64, 16, nb, 0.2
        d.x, d.y = 0x10000 * (g + 1), 0x10000 * (g + 2)                  # group g's output = g+1's input
        for j in range(nb):
            d.w1[j] = d.b1[j] = d.alpha[j] = d.w2[j] = d.b2[j] = d.fc1[j] = d.fc2[j] = 0x1000
        d.wg = d.bg = 0x1000
        d.work, d.work_bytes = 0x100000, nbytes
    # not a chain: group 1's input is not group 0's output
    ds[1].x = 0x90000
    assert lib.fen_group_strip_chain(ds, G, None, None) == -1
    assert lib.fen_group_strip_chain_prepare(ds, G, None, None) == -1
    ds[1].x = ds[0].y
    # the conv_after_body step may not write the body's output or its skip
    t = L.GroupStripChainTail()
    t.w = t.bias = 0x1000
    t.skip, t.y = ds[0].x, ds[G - 1].y
    assert lib.fen_group_strip_chain_prepare(ds, G, t, None) == -1
    # more steps than the 8-bit step tags hold: (nb + 1) * groups > 254
    big = (L.GroupStripDesc * 13)()
    for g in range(13):
        big[g] = ds[0]
        big[g].nb = 19
        big[g].x, big[g].y = 0x10000 * (g + 1), 0x10000 * (g + 2)
    assert lib.fen_group_strip_chain_prepare(big, 13, None, None) == -2


def test_rccl_and_status_entry_points_without_gpu():
    """fen_rccl_* validate their arguments before touching RCCL; fen_status_take reads and
    clears a word in one atomic exchange (here on plain host memory)."""
    import ctypes
    from src.hip import lib as L
    lib = L.load()
    assert lib.fen_status_string(-4).startswith(b"FEN_ERCCL")
    assert lib.fen_rccl_allreduce_bucket(None, None, 16, None) == -1
    assert lib.fen_rccl_init(None, None, 1, 0, 0) == -1
    h = ctypes.c_void_p()
    uid = (ctypes.c_uint8 * 128)()
    assert lib.fen_rccl_init(ctypes.byref(h), uid, 2, 2, 0) == -1       # rank outside nranks
    assert lib.fen_rccl_check(None) == -1
    assert lib.fen_rccl_destroy(None) == 0
    w = ctypes.c_int32(3)
    assert lib.fen_status_take(ctypes.addressof(w)) == 3 and w.value == 0
    assert lib.fen_status_take(ctypes.addressof(w)) == 0
    assert lib.fen_status_take(None) == 0


def test_unknown_dtype_rejected_by_every_entry_point_without_gpu():
    """Every exported function that takes a dtype -- a plain `int dtype` or a descriptor's field --
    answers a code that is no fen_dtype with FEN_EINVAL, given otherwise valid non-null arguments.
    The refusal precedes any launch (and any read through a pointer), so it runs on CPU."""
    import ctypes
    from src.hip import lib as L
    lib = L.load()
    P = 0x10000                                                   # never dereferenced
    win = (ctypes.c_float * 11)(*([1.0 / 11] * 11))               # (the SSIM window is read on the host)
    winp = ctypes.cast(win, ctypes.c_void_p)
    jobs = (L.PackJob * 1)()
    jobs[0].w, jobs[0].out, jobs[0].mode, jobs[0].Cout, jobs[0].Cin = P, P, 0, 64, 64
    table = ctypes.create_string_buffer(lib.fen_pack_table_bytes(1))
    total = ctypes.c_size_t(0)

    def descs(dt):
        c = L.ConvDesc()
        c.dtype, c.B, c.H, c.W, c.Cin, c.Cout = dt, 1, 16, 16, 64, 64
        c.x = c.w = c.y = P
        wg = (L.WgradDesc * 2)()
        for w in wg:
            w.dtype, w.B, w.H, w.W, w.Cin, w.Cout, w.cout_valid = dt, 1, 16, 16, 64, 64, 64
            w.x = w.dy = w.dw = w.work = P
        r = L.RcabDeferredDesc()
        r.dtype, r.B, r.H, r.W, r.C, r.Cr = dt, 1, 16, 16, 64, 16
        r.x = r.w1 = r.w2 = r.b1 = r.b2 = r.alpha = r.t = r.part = P
        ge = L.RcabDeferredDesc()
        ge.dtype, ge.B, ge.H, ge.W, ge.C, ge.Cr = dt, 1, 16, 16, 64, 16
        ge.x = ge.tp = ge.pp = ge.pfc1 = ge.pfc2 = P
        rb = L.RcabBwdDesc()
        rb.dtype, rb.B, rb.H, rb.W, rb.C = dt, 1, 16, 16, 64
        rb.dt = rb.w2t = rb.w1t = rb.z1 = rb.alpha = rb.dz1 = rb.dalpha_part = rb.dx = rb.dy = P
        gs = (L.GroupStripDesc * 2)()
        nbytes = lib.fen_group_strip_chain_work_bytes(1, 64, 2)
        for g, d in enumerate(gs):
            d.dtype, d.B, d.H, d.W, d.C, d.Cr, d.nb, d.res_scale = dt, 1, 64, 64, 64, 16, 1, 0.2
            d.x, d.y = P * (g + 1), P * (g + 2)
            d.w1[0] = d.b1[0] = d.alpha[0] = d.w2[0] = d.b2[0] = d.fc1[0] = d.fc2[0] = P
            d.wg = d.bg = P
            d.work, d.work_bytes = 0x100000, nbytes
        gb = L.GroupStripBwdDesc()
        gb.dtype, gb.B, gb.H, gb.W, gb.C, gb.Cr, gb.nb, gb.res_scale = dt, 1, 64, 64, 64, 16, 1, 0.2
        gb.dy, gb.dx, gb.wgt, gb.work = P, 2 * P, P, 0x100000
        gb.work_bytes = lib.fen_group_strip_bwd_work_bytes(1, 64)
        for f in ("w1t", "w2t", "alpha", "fc1", "fc2", "z1", "t", "s", "mean", "hid", "dt", "dz1", "dalpha_part",
                  "dw1p", "dw2p", "a1"):
            getattr(gb, f)[0] = P
        c128 = L.RcabC128Desc()
        c128.dtype, c128.B, c128.H, c128.W, c128.C, c128.Cr, c128.mode = dt, 1, 16, 16, 128, 16, 3
        c128.x, c128.w, c128.bias, c128.res, c128.y = P, P, P, P, 2 * P
        rc = L.RrdbConvDesc()
        rc.dtype, rc.B, rc.H, rc.W, rc.Cin, rc.Cout = dt, 1, 8, 8, 64, 32
        rc.x, rc.w, rc.bias, rc.y, rc.x_stride, rc.y_stride, rc.y_off = P, P, P, 2 * P, 192, 192, 64
        blk = L.RrdbBlockDesc()
        blk.dtype, blk.B, blk.H, blk.W, blk.num_feat, blk.num_grow_ch = dt, 1, 8, 8, 64, 32
        blk.buf, blk.next = P, 2 * P
        for k in range(5):
            blk.w[k] = blk.bias[k] = P
        return c, wg, r, ge, rb, gs, gb, c128, rc, blk

    for dt in (3, -1):
        c, wg, r, ge, rb, gs, gb, c128, rc, blk = descs(dt)
        calls = {
            "fen_conv3x3": lambda: lib.fen_conv3x3(c, None),
            "fen_wgrad3x3": lambda: lib.fen_wgrad3x3(wg[0], None),
            "fen_wgrad3x3_multi": lambda: lib.fen_wgrad3x3_multi(2, ctypes.cast(wg, ctypes.c_void_p), None),
            "fen_rcab_deferred": lambda: lib.fen_rcab_deferred(r, None),
            "fen_rcab_group_end": lambda: lib.fen_rcab_group_end(ge, P, P, P, P, None),
            "fen_rcab_bwd": lambda: lib.fen_rcab_bwd(rb, None),
            "fen_group_strip": lambda: lib.fen_group_strip(gs[0], None),
            "fen_group_strip_chain_prepare": lambda: lib.fen_group_strip_chain_prepare(gs, 2, None, None),
            "fen_group_strip_chain": lambda: lib.fen_group_strip_chain(gs, 2, None, None),
            "fen_group_strip_bwd": lambda: lib.fen_group_strip_bwd(gb, None),
            "fen_rcab_c128": lambda: lib.fen_rcab_c128(c128, None),
            "fen_rrdb_conv": lambda: lib.fen_rrdb_conv(rc, None),
            "fen_rrdb_block": lambda: lib.fen_rrdb_block(blk, None),
            "fen_rrdb_first": lambda: lib.fen_rrdb_first(dt, 1, 3, 16, 16, P, P, P, P, 192, None, None),
            "fen_conv_first_fwd": lambda: lib.fen_conv_first_fwd(dt, 1, 3, 16, 16, 64, P, P, P, P, None),
            "fen_conv_first_fwd_ex": lambda: lib.fen_conv_first_fwd_ex(dt, 1, 3, 16, 16, 64, P, P, P, P, P, 0.2, P, None),
            "fen_conv_first_wgrad": lambda: lib.fen_conv_first_wgrad(dt, 1, 3, 16, 16, 64, P, P, P, P, 0, P, None),
            "fen_conv_last_dgrad": lambda: lib.fen_conv_last_dgrad(dt, 1, 16, 16, 64, 3, P, P, P, P, P, P, P, None),
            "fen_conv_last_bwd": lambda: lib.fen_conv_last_bwd(dt, 1, 16, 16, 64, 3, P, P, P, P, P, P, P, P, P, None),
            "fen_se_fused": lambda: lib.fen_se_fused(dt, 1, 256, 64, 16, 4, 1 / 256, P, P, P, P, P, P, P, 0.2, P, P, None),
            "fen_se_apply": lambda: lib.fen_se_apply(dt, 1, 256, 64, P, P, 0.2, P, P, None),
            "fen_pool_dot": lambda: lib.fen_pool_dot(dt, 1, 256, 64, P, P, P, None),
            "fen_se_bwd_fused": lambda: lib.fen_se_bwd_fused(dt, 1, 256, 64, 16, 4, 1 / 256, 0.2, P, P, P, P, P, P, P, P,
                                                             P, P, P, None),
            "fen_se_bwd_apply": lambda: lib.fen_se_bwd_apply(dt, 1, 256, 64, P, P, 0.2, P, P, None),
            "fen_pack_conv_w": lambda: lib.fen_pack_conv_w(dt, 0, 64, 64, P, P, None),
            "fen_pack_table": lambda: lib.fen_pack_table(dt, 1, ctypes.cast(jobs, ctypes.c_void_p),
                                                         ctypes.cast(table, ctypes.c_void_p), ctypes.byref(total)),
            "fen_pack_multi": lambda: lib.fen_pack_multi(dt, 1, P, 256, None),
            "fen_nchw_to_nhwc": lambda: lib.fen_nchw_to_nhwc(dt, 1, 3, 16, 16, 8, P, P, None),
            "fen_nhwc_to_nchw": lambda: lib.fen_nhwc_to_nchw(dt, 1, 3, 16, 16, P, P, None),
            "fen_prelu_bwd_unshuffle": lambda: lib.fen_prelu_bwd_unshuffle(dt, 1, 16, 16, 64, P, P, P, P, P, None),
            "fen_maxpool2": lambda: lib.fen_maxpool2(dt, 1, 16, 16, 64, P, P, None),
            "fen_maxpool2_bwd_relu": lambda: lib.fen_maxpool2_bwd_relu(dt, 1, 16, 16, 64, P, P, P, None),
            "fen_feat_loss": lambda: lib.fen_feat_loss(dt, 64, P, 0, 1.0, P, 0, P, None),
            "fen_ssim": lambda: lib.fen_ssim(dt, 1, 3, 16, 16, P, P, winp, 11, 1e-4, 9e-4, P, P, 1.0, 2, None),
            "fen_ssim_ex": lambda: lib.fen_ssim_ex(dt, 1, 3, 16, 16, P, P, winp, 11, 1e-4, 9e-4, P, P, 1.0, 2, P, None),
            "fen_msssim": lambda: lib.fen_msssim(dt, 1, 3, 32, 32, P, P, winp, 11, 1e-4, 9e-4, P, 2, P, P, P, 1.0, 1, None),
            "fen_bn_stats": lambda: lib.fen_bn_stats(dt, 64, 64, P, 1e-5, 0.1, P, None, None, P, None),
            "fen_bn_stats_n": lambda: lib.fen_bn_stats_n(dt, 2, 64, 64, P, 1e-5, 0.1, P, None, None, P, None),
            "fen_bn_apply": lambda: lib.fen_bn_apply(dt, 64, 64, P, P, P, P, P, 0.2, P, None),
            "fen_bn_apply_n": lambda: lib.fen_bn_apply_n(dt, 2, 64, 64, P, P, P, 64, P, P, 0.2, P, None),
            "fen_bn_bwd": lambda: lib.fen_bn_bwd(dt, 64, 64, P, P, P, P, P, 0.2, P, P, P, 0, P, None),
            "fen_bn_bwd_n": lambda: lib.fen_bn_bwd_n(dt, 2, 64, 64, P, P, P, P, P, 0.2, P, P, P, 0, P, None),
            "fen_subsample2": lambda: lib.fen_subsample2(dt, 1, 16, 16, 64, P, P, None),
            "fen_s2d2": lambda: lib.fen_s2d2(dt, 1, 16, 16, 64, P, P, 0, None),
            "fen_zero_insert2": lambda: lib.fen_zero_insert2(dt, 1, 8, 8, 64, P, P, None),
        }
        got = {name: call() for name, call in calls.items()}
        wrong = {name: rc_ for name, rc_ in got.items() if rc_ != -1}
        assert not wrong, (dt, wrong)
    # the list is the header's: every status-returning function with a dtype parameter or descriptor
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fen.h")).read(), flags=re.S)
    takes = set(re.findall(r"\bint (fen_[a-z0-9_]+)\s*\(\s*(?:int dtype|const fen_(?:conv|wgrad|rcab_deferred|"
                           r"group_strip|rcab_c128|group_strip_bwd|rcab_bwd|rrdb_conv|rrdb_block)_desc\*)", hdr))
    takes -= {n for n in takes if n.endswith("_supported")}      # 0 / 1 queries, not statuses
    takes.add("fen_wgrad3x3_multi")                               # (int n, const fen_wgrad_desc* ds, ...)
    assert takes == set(calls), takes ^ set(calls)

"""The direct (non-GEMM) entry points of csrc/misc.hip, csrc/norm.hip and csrc/f32.hip, host side (no GPU): every
CID_CHECK_ARG clause refuses its argument with -22 and its own message before anything is launched.  Addresses are dummy
non-null values (tests/test_abi.py, tests/test_safety_host.py); tests/test_gpu_direct_kernels.py runs the same entry points
at the edges these clauses leave open."""
import ctypes as C

import pytest

A = 64        # a 16-byte-aligned stand-in address


def _refused(lib, rc, fragment):
    msg = lib.cid_last_error()
    assert rc == -22 and fragment in msg, (rc, msg)


def test_linear_small_refusals(lib):
    def lin(x=A, ldx=1280, w=A, b=A, add=None, ldadd=0, out=A, ldo=1000, M=4, N=1000, K=1280):
        return lib.cid_linear_small_f16(x, ldx, w, b, add, ldadd, out, ldo, M, N, K, 0, 0, None)

    for kw in (dict(x=None), dict(w=None), dict(out=None)):
        _refused(lib, lin(**kw), b"cid_linear_small_f16: null pointer")
    for kw in (dict(M=0), dict(M=65), dict(N=0), dict(K=0, ldx=0), dict(K=1284, ldx=1288), dict(ldx=1284)):
        _refused(lib, lin(**kw), b"cid_linear_small_f16: bad shape")
    # the pitches: a row of x holds K values, a row of out N, `add` is one shared row (0) or a row per m
    _refused(lib, lin(ldx=1272), b"cid_linear_small_f16: bad pitch ldx=1272")
    _refused(lib, lin(ldo=999), b"cid_linear_small_f16: bad pitch")
    _refused(lib, lin(add=A, ldadd=999), b"ldadd 0 or >= N")
    _refused(lib, lin(add=A, ldadd=-8), b"ldadd 0 or >= N")


def test_small_attn_refusals(lib):
    def att(q=A, ldq=192, kv1=A, n1=60, kv2=A, n2=4, ldkv=384, out=A, ldo=192, B=2, Lq=4, heads=3, dim_head=64):
        return lib.cid_small_attn_f16(q, ldq, kv1, n1, kv2, n2, ldkv, out, ldo, B, Lq, heads, dim_head, 0.125, None)

    for kw in (dict(q=None), dict(kv1=None), dict(out=None), dict(kv2=None)):
        _refused(lib, att(**kw), b"cid_small_attn_f16: null pointer")
    _refused(lib, att(dim_head=40), b"head width must be 64 (got 40)")
    for kw in (dict(B=0), dict(Lq=0), dict(heads=0), dict(n1=0), dict(n2=-1), dict(n1=1021), dict(ldq=196), dict(ldkv=388)):
        _refused(lib, att(**kw), b"cid_small_attn_f16: bad shape (at most 1024 keys)")
    # the kernel reads q / writes out at h * 64 of a row and V at heads * 64 of a key row
    _refused(lib, att(ldq=184), b"cid_small_attn_f16: bad pitch ldq=184")
    _refused(lib, att(ldkv=376), b"cid_small_attn_f16: bad pitch")
    _refused(lib, att(ldkv=192), b"ldkv >= twice that")
    _refused(lib, att(ldo=191), b"cid_small_attn_f16: bad pitch")
    _refused(lib, att(ldo=0), b"ldo=0")


def test_conv_in_refusals(lib):
    def cin(sample=A, out=A, w=A, bias=A, B=2, Bin=1, cin=4, H=8, W=8, cout=320):
        return lib.cid_conv_in_f16(sample, out, w, bias, B, Bin, cin, H, W, cout, None, None)

    for kw in (dict(sample=None), dict(out=None), dict(w=None), dict(bias=None)):
        _refused(lib, cin(**kw), b"cid_conv_in_f16: null pointer")
    for kw in (dict(B=0), dict(Bin=0), dict(cin=0), dict(cin=10), dict(cout=324), dict(cout=328), dict(H=0), dict(W=0)):
        _refused(lib, cin(**kw), b"cid_conv_in_f16: bad shape (cin <= 9, cout <= 320)")
    _refused(lib, cin(B=3, Bin=2), b"cid_conv_in_f16: B must be a multiple of Bin")

    def cat(sample=A, cin1=4, extra=A, cin2=5, out=A, w=A, bias=A, B=2, Bin=1, H=8, W=8, cout=320):
        return lib.cid_conv_in_cat_f16(sample, cin1, extra, cin2, out, w, bias, B, Bin, H, W, cout, None, None)

    for kw in (dict(sample=None), dict(extra=None), dict(out=None), dict(w=None), dict(bias=None)):
        _refused(lib, cat(**kw), b"cid_conv_in_cat_f16: null pointer")
    for kw in (dict(cin1=0), dict(cin2=0), dict(cin1=5), dict(cout=4), dict(cout=328), dict(H=0), dict(W=-1), dict(B=0), dict(Bin=0)):
        _refused(lib, cat(**kw), b"cid_conv_in_cat_f16: bad shape (cin1 + cin2 <= 9, cout <= 320)")
    _refused(lib, cat(B=4, Bin=3), b"cid_conv_in_cat_f16: B must be a multiple of Bin")


def test_small_conv_and_conv_out_refusals(lib):
    def c3(x=A, out=A, w=A, bias=A, B=1, Hi=8, Wi=8, cin=3, cout=16, stride=1):
        return lib.cid_conv3x3_small_f16(x, out, w, bias, B, Hi, Wi, cin, cout, stride, 0, None)

    for kw in (dict(x=None), dict(out=None), dict(w=None), dict(bias=None)):
        _refused(lib, c3(**kw), b"cid_conv3x3_small_f16: null pointer")
    for kw in (dict(B=0), dict(Hi=0), dict(Wi=0), dict(cin=0), dict(cout=0), dict(cout=12), dict(stride=0), dict(stride=3)):
        _refused(lib, c3(**kw), b"cid_conv3x3_small_f16: bad shape")

    def co(x=A, out=A, w=A, bias=A, B=1, H=8, W=8, cin=320, cout=4):
        return lib.cid_conv_out_f16(x, out, w, bias, B, H, W, cin, cout, None)

    for kw in (dict(x=None), dict(out=None), dict(w=None), dict(bias=None)):
        _refused(lib, co(**kw), b"cid_conv_out_f16: null pointer")
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(cin=324), dict(cout=0), dict(cout=5)):
        _refused(lib, co(**kw), b"cid_conv_out_f16: bad shape (cout <= 4)")
    _refused(lib, co(cin=920), b"cin = 920 is too wide")        # 9 taps x 115 chunks x 64 bytes > 64 KB of LDS


def test_elementwise_refusals(lib):
    for n in (0, -8, 12):
        _refused(lib, lib.cid_gelu_f16(A, n, None), b"cid_gelu_f16: n must be a positive multiple of 8")
    _refused(lib, lib.cid_gelu_f16(None, 8, None), b"cid_gelu_f16")
    _refused(lib, lib.cid_quick_gelu_f16(None, 8, None), b"cid_quick_gelu_f16: null pointer")
    _refused(lib, lib.cid_quick_gelu_f16(A, 0, None), b"cid_quick_gelu_f16: n must be a positive multiple of 8 (got 0)")

    def add(y=A, a=A, n=64, na=32):
        return lib.cid_add_inplace_f16(y, a, n, na, None)

    for kw in (dict(y=None), dict(a=None), dict(n=0), dict(na=0), dict(n=60), dict(na=12, n=24), dict(n=64, na=24)):
        _refused(lib, add(**kw), b"cid_add_inplace_f16: sizes must be multiples of 8")

    def emb(ids=A, B=1, T=77, Tp=80, tok=A, pos=A, out=A, V=100, Cc=768):
        return lib.cid_text_embed_f16(ids, B, T, Tp, tok, pos, out, V, Cc, None)

    for kw in (dict(ids=None), dict(tok=None), dict(pos=None), dict(out=None)):
        _refused(lib, emb(**kw), b"cid_text_embed_f16: null pointer")
    for kw in (dict(B=0), dict(T=0), dict(Tp=76), dict(V=0), dict(Cc=0), dict(Cc=772)):
        _refused(lib, emb(**kw), b"cid_text_embed_f16: bad shape")


def test_step_kernels_refusals(lib):
    def ddim(eps=A, lat=A, coef=A, mask=None, init=None, noise=None, B=2, per=64):
        return lib.cid_cfg_ddim_step_f16(eps, lat, coef, 7.5, mask, init, noise, B, per, None)

    for kw in (dict(eps=None), dict(lat=None), dict(coef=None)):
        _refused(lib, ddim(**kw), b"cid_cfg_ddim_step_f16: null pointer")
    for kw in (dict(mask=A), dict(init=A), dict(noise=A), dict(mask=A, init=A), dict(init=A, noise=A)):
        _refused(lib, ddim(**kw), b"cid_cfg_ddim_step_f16: mask/init/noise must come together")
    for kw in (dict(B=0), dict(per=0), dict(B=1, per=12), dict(B=3, per=4)):
        _refused(lib, ddim(**kw), b"cid_cfg_ddim_step_f16: B * per_sample must be a multiple of 8")

    def multi(eps=A, lat=A, hist=A, saved=A, z=None, z_rows=0, row=A, mask=None, init=None, noise=None, B=2, per=64):
        return lib.cid_cfg_multistep_step_f16(eps, lat, hist, saved, z, z_rows, row, 7.5, mask, init, noise, B, per, None)

    for kw in (dict(eps=None), dict(lat=None), dict(hist=None), dict(saved=None), dict(row=None)):
        _refused(lib, multi(**kw), b"cid_cfg_multistep_step_f16: null pointer")
    for kw in (dict(z=A), dict(z_rows=2), dict(z=A, z_rows=-1)):
        _refused(lib, multi(**kw), b"cid_cfg_multistep_step_f16: z and z_rows must come together")
    for kw in (dict(mask=A), dict(mask=A, noise=A)):
        _refused(lib, multi(**kw), b"cid_cfg_multistep_step_f16: mask/init/noise must come together")
    for kw in (dict(B=0), dict(per=0), dict(B=1, per=20)):
        _refused(lib, multi(**kw), b"cid_cfg_multistep_step_f16: B * per_sample must be a multiple of 8")


def test_residual_accum_refusals(lib):
    from consistentid_amd._lib import AccumSeg

    def seg(y=A, n=64, nr=64, r=(A,)):
        s = AccumSeg()
        s.y, s.n, s.nr = y, n, nr
        for k, a in enumerate(r):
            s.r[k] = a
        return s

    def acc(segs, n_nets=1, scales=A, n_segs=None):
        arr = (AccumSeg * max(len(segs), 1))(*segs)
        return lib.cid_residual_accum_f16(arr, len(segs) if n_segs is None else n_segs, n_nets, scales, None)

    _refused(lib, lib.cid_residual_accum_f16(None, 1, 1, A, None), b"cid_residual_accum_f16: null pointer")
    _refused(lib, acc([seg()], scales=None), b"cid_residual_accum_f16: null pointer")
    _refused(lib, acc([seg()], n_segs=0), b"cid_residual_accum_f16: 0 segments (1..16)")
    _refused(lib, acc([seg()] * 17), b"cid_residual_accum_f16: 17 segments (1..16)")
    _refused(lib, acc([seg()], n_nets=0), b"cid_residual_accum_f16: 0 nets (1..4)")
    _refused(lib, acc([seg(r=(A,) * 4)], n_nets=5), b"cid_residual_accum_f16: 5 nets (1..4)")
    _refused(lib, acc([seg(), seg(y=None)]), b"segment 1: y is null or not 16-byte aligned")
    _refused(lib, acc([seg(y=A + 8)]), b"segment 0: y is null or not 16-byte aligned")
    for kw in (dict(n=0), dict(nr=0), dict(n=60, nr=60), dict(n=64, nr=12), dict(n=64, nr=24)):
        _refused(lib, acc([seg(**kw)]), b"segment 0: n = ")
    _refused(lib, acc([seg(r=(A, None))], n_nets=2), b"segment 0: residual of net 1 is null or not 16-byte aligned")
    _refused(lib, acc([seg(r=(A + 2,))]), b"segment 0: residual of net 0 is null or not 16-byte aligned")


def test_fp16_norm_refusals(lib):
    def ln(x=A, ldx=320, out=A, ldo=320, g=A, b=A, M=4, Cc=320):
        return lib.cid_layernorm_ld_f16(x, ldx, out, ldo, g, b, M, Cc, 1e-5, None)

    for kw in (dict(x=None), dict(out=None), dict(g=None), dict(b=None)):
        _refused(lib, ln(**kw), b"cid_layernorm_ld_f16: null pointer")
    for kw in (dict(M=0), dict(Cc=0, ldx=8, ldo=8), dict(Cc=324, ldx=328, ldo=328)):
        _refused(lib, ln(**kw), b"cid_layernorm_ld_f16: bad shape")
    _refused(lib, ln(Cc=1544, ldx=1544, ldo=1544), b"cid_layernorm_ld_f16: bad shape M=4 C=1544")
    for kw in (dict(ldx=312), dict(ldo=312), dict(ldx=324), dict(ldo=324)):
        _refused(lib, ln(**kw), b"cid_layernorm_ld_f16: bad pitch")
    _refused(lib, lib.cid_layernorm_f16(A, A, A, A, 4, 1544, 1e-5, None), b"cid_layernorm_ld_f16: bad shape")

    def sm(x=A, rows=4, cols=256, ld=256):
        return lib.cid_softmax_rows_f16(x, rows, cols, ld, None)

    for kw in (dict(x=None), dict(rows=0), dict(cols=0), dict(cols=252), dict(ld=248), dict(ld=260)):
        _refused(lib, sm(**kw), b"cid_softmax_rows_f16: bad shape")

    def gn(x1=A, x2=None, c1=320, c2=0, out=A, g=A, b=A, B=2, HW=64, groups=32, ws=A):
        return lib.cid_groupnorm_f16(x1, x2, c1, c2, out, g, b, B, HW, groups, 1e-5, 1, ws, None)

    for kw in (dict(x1=None), dict(out=None), dict(g=None), dict(b=None), dict(ws=None)):
        _refused(lib, gn(**kw), b"cid_groupnorm_f16: null pointer")
    for kw in (dict(c1=0), dict(c1=324), dict(c2=-8), dict(c2=4, x2=A), dict(c2=320)):
        _refused(lib, gn(**kw), b"cid_groupnorm_f16: bad channels")
    for kw in (dict(groups=0), dict(groups=65, c1=520), dict(groups=48), dict(c1=1280, c2=1288, x2=A, groups=8)):
        _refused(lib, gn(**kw), b"cid_groupnorm_f16: bad groups/C")
    for kw in (dict(B=0), dict(HW=0), dict(HW=1024 * 1024 + 1)):
        _refused(lib, gn(**kw), b"cid_groupnorm_f16: bad B/HW")

    def gs(x1=A, x2=A, c1=320, c2=320, out=A, g=A, b=A, B=2, HW=4096, groups=32, st1=A, rows1=256, st2=A, rows2=128):
        return lib.cid_groupnorm_stats_f16(x1, x2, c1, c2, out, g, b, B, HW, groups, 1e-5, 1, st1, rows1, st2, rows2, None)

    for kw in (dict(x1=None), dict(out=None), dict(g=None), dict(b=None), dict(st1=None)):
        _refused(lib, gs(**kw), b"cid_groupnorm_stats_f16: null pointer")
    for kw in (dict(c1=0), dict(c1=324), dict(c2=-8), dict(x2=None), dict(st2=None)):
        _refused(lib, gs(**kw), b"cid_groupnorm_stats_f16: bad channels")
    # 2568 > GN_MAXC; groups that straddle the two sources; a group smaller than a statistics unit (c / 32 channels)
    for kw in (dict(c1=1280, c2=1288), dict(c1=320, c2=64, groups=32), dict(c1=320, c2=0, x2=None, st2=None, groups=64),
               dict(groups=0), dict(c1=328, c2=312)):
        _refused(lib, gs(**kw), b"are not whole statistics units of one source")
    for kw in (dict(B=0), dict(HW=0), dict(rows1=0), dict(rows1=384), dict(rows2=0), dict(rows2=96)):
        _refused(lib, gs(**kw), b"cid_groupnorm_stats_f16: a statistics block must lie inside one sample")


def test_fp32_refusals(lib):
    def gm(x=A, w=A, out=A, res=None, M=64, N=64, c=32, taps=1, ldx=32, ldo=64, ldr=64, Hi=0, Wi=0, Ho=0, Wo=0, up=0):
        return lib.cid_gemm_f32(x, w, None, res, out, M, N, c, taps, ldx, ldo, ldr, Hi, Wi, Ho, Wo, up, None)

    for kw in (dict(x=None), dict(w=None), dict(out=None)):
        _refused(lib, gm(**kw), b"cid_gemm_f32: null pointer")
    for kw in (dict(M=0), dict(N=0), dict(c=0), dict(taps=3), dict(ldx=28), dict(ldo=60)):
        _refused(lib, gm(**kw), b"cid_gemm_f32: bad shape")
    _refused(lib, gm(ldx=34), b"cid_gemm_f32: ldx must be a multiple of 4 when c is")
    _refused(lib, gm(res=A, ldr=60), b"cid_gemm_f32: bad residual pitch")
    geo = dict(taps=9, Hi=8, Wi=8, Ho=8, Wo=8)
    for kw in (dict(Hi=0), dict(Wi=0), dict(Ho=16), dict(Wo=4), dict(up=1), dict(M=96)):
        _refused(lib, gm(**{**geo, **kw}), b"cid_gemm_f32: 3x3 geometry")

    def gn(x=A, out=A, g=A, b=A, B=1, HW=64, Cc=128, groups=32, ws=A):
        return lib.cid_groupnorm_f32(x, out, g, b, B, HW, Cc, groups, 1e-6, 1, ws, None)

    for kw in (dict(x=None), dict(out=None), dict(g=None), dict(b=None), dict(ws=None)):
        _refused(lib, gn(**kw), b"cid_groupnorm_f32: null pointer")
    for kw in (dict(B=0), dict(HW=0), dict(Cc=0), dict(Cc=130, groups=13), dict(Cc=2052, groups=4), dict(groups=0),
               dict(groups=128), dict(groups=24)):
        _refused(lib, gn(**kw), b"cid_groupnorm_f32: bad shape")

    for x, rows, cols, ld in ((None, 2, 8, 8), (A, 0, 8, 8), (A, 2, 0, 8), (A, 2, 8, 7)):
        _refused(lib, lib.cid_softmax_rows_f32(x, rows, cols, ld, None), b"cid_softmax_rows_f32: bad shape")

"""The entry points of the kernels that run once per generation (csrc/parsing.hip, csrc/vae_enc.hip, the time embedding and
the step table of csrc/misc.hip, the packers of csrc/xattn.hip and csrc/xattn3.hip), host side (no GPU): every CID_CHECK_ARG
clause that tests/test_face_parsing_host.py, tests/test_vae_encode_host.py and tests/test_abi.py do not reach refuses its
argument with -22 and its own message before anything is launched, and the clauses they reach by return code alone are held
to their text here.  Addresses are dummy non-null values; tests/test_gpu_preloop_kernels.py runs the same entry points at the
edges these clauses leave open."""
from test_direct_kernels_host import A, _refused

OFF = A + 8       # an address that is not 16-byte aligned


def test_parse_stem_refusals(lib):
    def stem(img=A, out=A, w=A, bias=A, B=1, H=64, W=96):
        return lib.cid_parse_stem_f16(img, out, w, bias, B, H, W, None)

    for kw in (dict(out=None), dict(w=None), dict(bias=None)):
        _refused(lib, stem(**kw), b"cid_parse_stem_f16: null pointer")
    for kw in (dict(B=0), dict(B=16384), dict(H=0), dict(W=16), dict(W=100)):
        _refused(lib, stem(**kw), b"cid_parse_stem_f16: H and W must be positive multiples of 32, 1 <= B <= 16383")
    _refused(lib, stem(B=16384), b"(got B 16384, 64 x 96)")
    _refused(lib, stem(out=OFF), b"cid_parse_stem_f16: out must be 16-byte aligned")


def test_chan_mean_refusals(lib):
    def mean(x=A, out=A, B=2, HW=100, C=128, ld=200):
        return lib.cid_chan_mean_f16(x, out, B, HW, C, ld, None)

    for kw in (dict(x=None), dict(out=None)):
        _refused(lib, mean(**kw), b"cid_chan_mean_f16: null pointer")
    for kw in (dict(B=0), dict(B=65536), dict(HW=0), dict(C=0), dict(C=132, ld=136), dict(ld=120), dict(ld=132)):
        _refused(lib, mean(**kw), b"cid_chan_mean_f16: bad shape")
    _refused(lib, mean(ld=120), b"(B 2, HW 100, C 128, ld 120; C % 8 == 0, ld >= C, ld % 8 == 0)")
    _refused(lib, mean(x=OFF), b"cid_chan_mean_f16: x must be 16-byte aligned")


def test_chan_gate_refusals(lib):
    def gate(mean=A, out=A, w1=A, b1=A, w2=None, b2=None, B=2, K=256, N1=128, N=128, act=2):
        return lib.cid_chan_gate_f32(mean, out, w1, b1, w2, b2, B, K, N1, N, act, None)

    for kw in (dict(mean=None), dict(out=None), dict(w1=None)):
        _refused(lib, gate(**kw), b"cid_chan_gate_f32: null pointer")
    for kw in (dict(B=0), dict(K=0), dict(K=513), dict(N1=0), dict(N1=513, N=513), dict(N=0, w2=A), dict(N=513, w2=A), dict(N=64)):
        _refused(lib, gate(**kw), b"cid_chan_gate_f32: bad shape")
    _refused(lib, gate(N=64), b"(B 2, K 256, N1 128, N 64; at most 512 each, N == N1 without w2)")
    _refused(lib, gate(b2=A), b"cid_chan_gate_f32: b2 without w2")
    for act in (-1, 3):
        _refused(lib, gate(act=act), b"cid_chan_gate_f32: bad act %d (0 none, 1 ReLU, 2 sigmoid)" % act)


def test_chan_affine_refusals(lib):
    def aff(x=A, s=A, t=None, res=None, out=A, B=2, HW=16, C=64):
        return lib.cid_chan_affine_f16(x, s, t, res, out, B, HW, C, None)

    for kw in (dict(x=None), dict(s=None), dict(out=None)):
        _refused(lib, aff(**kw), b"cid_chan_affine_f16: null pointer")
    for kw in (dict(B=0), dict(HW=0), dict(C=0), dict(C=60)):
        _refused(lib, aff(**kw), b"cid_chan_affine_f16: bad shape")
    _refused(lib, aff(C=60), b"(B 2, HW 16, C 60; C % 8 == 0)")
    for kw in (dict(x=OFF), dict(res=OFF), dict(out=OFF), dict(x=OFF, out=OFF)):          # (x == out: the in-place call)
        _refused(lib, aff(**kw), b"cid_chan_affine_f16: x / res / out must be 16-byte aligned")


def test_parse_head_refusals(lib):
    def head(logits=A, ld=32, ncls=19, B=1, h=64, w=64, H=512, W=512, labels=A):
        return lib.cid_parse_head_f16(logits, ld, ncls, B, h, w, H, W, labels, None, None)

    for kw in (dict(logits=None), dict(labels=None)):
        _refused(lib, head(**kw), b"cid_parse_head_f16: null pointer")
    for kw in (dict(ncls=0), dict(ncls=257, ld=264), dict(ld=18), dict(B=0), dict(h=0), dict(w=0), dict(H=0), dict(W=0)):
        _refused(lib, head(**kw), b"cid_parse_head_f16: bad shape")
    _refused(lib, head(ld=18), b"(ncls 19, ld 18, B 1, 64 x 64 -> 512 x 512; 0 < ncls <= min(ld, 256))")


def test_vae_encode_refusals(lib):
    def ein(image=A, Bi=2, mask=A, Bm=1, out=A, w=A, bias=A, H=64, W=48, cout=128, blocks=3, mlat=None):
        return lib.cid_vae_encode_in_f16(image, Bi, mask, Bm, out, w, bias, H, W, cout, 1, blocks, mlat, None)

    for kw in (dict(w=None), dict(bias=None)):
        _refused(lib, ein(**kw), b"cid_vae_encode_in_f16: null pointer")
    for kw in (dict(Bi=0), dict(H=0), dict(W=0), dict(cout=0), dict(cout=132), dict(cout=328)):
        _refused(lib, ein(**kw), b"cid_vae_encode_in_f16: bad shape")
    _refused(lib, ein(cout=328), b"(Bi=2 H=64 W=48 cout=328; cout % 8 == 0, cout <= 320)")
    for blocks in (0, 4):
        _refused(lib, ein(blocks=blocks), b"blocks must be 1 (image), 2 (masked image) or 3 (both), got %d" % blocks)
    _refused(lib, ein(mask=None, blocks=2), b"cid_vae_encode_in_f16: the masked image and mask_latents need a mask")
    _refused(lib, ein(Bm=0), b"cid_vae_encode_in_f16: mask batch Bm=0 must be 1 or Bi=2")
    _refused(lib, ein(W=44, mlat=A), b"mask_latents need H and W multiples of 8 (got 64 x 44)")
    for kw in (dict(out=OFF), dict(bias=OFF)):
        _refused(lib, ein(**kw), b"cid_vae_encode_in_f16: out / bias must be 16-byte aligned")

    def eout(x=A, out=A, w=A, bias=A, B=1, H=12, W=10, cin=512, L=4):
        return lib.cid_vae_encode_out_f16(x, out, None, w, bias, None, B, H, W, cin, L, 0.18215, None)

    for kw in (dict(out=None), dict(w=None)):
        _refused(lib, eout(**kw), b"cid_vae_encode_out_f16: null pointer")
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(cin=0), dict(cin=500), dict(L=0), dict(L=5)):
        _refused(lib, eout(**kw), b"cid_vae_encode_out_f16: bad shape")
    _refused(lib, eout(L=5), b"(B=1 H=12 W=10 cin=512 L=5; cin % 8 == 0, L <= 4)")
    for kw in (dict(x=OFF), dict(w=OFF)):
        _refused(lib, eout(**kw), b"cid_vae_encode_out_f16: x / w must be 16-byte aligned")


def test_sincos_embed_refusals(lib):
    for v, out, rows, dim in ((None, A, 1, 320), (A, None, 1, 320), (A, A, 0, 320), (A, A, -1, 320), (A, A, 1, 0), (A, A, 1, 321)):
        _refused(lib, lib.cid_sincos_embed_f16(v, out, rows, dim, None), b"cid_sincos_embed_f16: bad arguments")


def test_step_select_refusals(lib):
    from consistentid_amd._lib import StepSeg

    def sel(table=A, row_bytes=64, n_rows=3, counter=A, segs=((A, 4, 12),), n_segs=None, null_segs=False):
        arr = (StepSeg * max(len(segs), 1))(*[StepSeg(d, o, n) for d, o, n in segs])
        return lib.cid_step_select(table, row_bytes, n_rows, counter, None if null_segs else arr,
                                   len(segs) if n_segs is None else n_segs, None)

    for kw in (dict(table=None), dict(counter=None), dict(null_segs=True)):
        _refused(lib, sel(**kw), b"cid_step_select: null pointer")
    for kw in (dict(n_rows=0), dict(row_bytes=0), dict(row_bytes=62), dict(n_segs=0), dict(segs=((A, 0, 4),) * 9)):
        _refused(lib, sel(**kw), b"cid_step_select: bad table")
    _refused(lib, sel(segs=((A, 0, 4),) * 9), b"(3 rows of 64 bytes, 9 segments; at most 8)")
    for seg in ((None, 4, 12), (A, -4, 12), (A, 6, 12), (A, 4, 0), (A, 4, 10), (A, 56, 12)):
        _refused(lib, sel(segs=(seg,)), b"cid_step_select: segment 0 does not fit the row")
    _refused(lib, sel(segs=((A, 4, 12), (A + 4, 20, 24), (A, 60, 8))), b"cid_step_select: segment 2 does not fit the row")


def test_packer_refusals(lib):
    def gather(a=A, b=A, idx=A, dst=A, R=3, src_row=4096, n_idx=777):
        return lib.cid_gather_pack_f16(a, b, idx, dst, R, src_row, n_idx, None)

    for kw in (dict(a=None), dict(b=None), dict(idx=None), dict(dst=None)):
        _refused(lib, gather(**kw), b"cid_gather_pack_f16: null pointer")
    for kw in (dict(R=0), dict(src_row=0), dict(src_row=1 << 30), dict(n_idx=0)):         # bit 30 of an index names the source
        _refused(lib, gather(**kw), b"cid_gather_pack_f16: bad sizes")

    def wfrag(w=A, wp=A, rows=96, K=1280):
        return lib.cid_pack_wfrag_f16(w, wp, rows, K, None)

    for kw in (dict(w=None), dict(wp=None), dict(rows=0), dict(rows=48), dict(K=0), dict(K=24)):
        _refused(lib, wfrag(**kw), b"cid_pack_wfrag_f16: rows % 32, K % 16 required")

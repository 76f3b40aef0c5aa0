// Two-stream identity cross-attention core over LONG contexts (more than the 96 key slots that xattn_core.h holds in
// registers): weighted / chunked prompts of 77 k rows (+ ID tokens), Consistent_IPAttProcessor.__call__
// (/root/reference/attention.py:259-279) with q already projected and pre-scaled by d^-0.5 * log2(e):
//
//   out_h = softmax2(q_h Kt_h^T) Vt_h + ip_scale * softmax2(q_h Kip_h^T) Vip_h
//
// One wave owns a unit = (sample, head, 32 tokens); four independent waves per workgroup, no LDS, no barrier.  The key axis
// is walked in 32-slot tiles: NT = ceil(n_txt / 32) text tiles under an online softmax (fp32 running maximum m over REAL
// keys only, partial row sums l per lane half, O in fp32 rescaled by 2^(m_old - m_new)), then -- with ID keys -- ONE tile
// that holds the n_ip <= 32 ID keys from its slot 0, handled as xattn_core_unit does: its whole softmax is known, P is
// scaled by ip_scale / l_ip and the product lands in the same accumulators (after O was divided by l).
// Both contractions run transposed, as everywhere in this library (common.h): S^T = K_h Q_h^T puts the token on the lane
// and the tile's 32 keys in the 16 registers of the two lane halves, so the softmax is lane-local plus one lane^32 exchange
// and P^T feeds O^T = V_h^T P^T from the accumulator registers (V^T is packed with the matching key permutation).
// Registers: only the current tile's K / V^T fragments and the next tile's K fragments are held -- at head width 160 the
// whole K image of a long context does not fit (10 fragments per tile).  K of tile t + 1 and V^T of tile t are requested
// before the MFMAs of tile t: K(t + 1) has a whole tile to arrive, V^T(t) has Q K^T and the softmax.
// Masked slots (text padding of the last tile, unused ID slots) get the score -inf BEFORE any maximum or sum: they give
// p = 2^(-inf) = 0 and can never raise a maximum, whatever the real scores are (the packed zeros would score 0).
#include "common.h"
#include "../../include/cid.h"

namespace {

constexpr int XL_WAVES = 4;

template <int D>
__global__ void __launch_bounds__(64 * XL_WAVES)
xattn_long_kernel(const half_t* __restrict__ q, half_t* __restrict__ out, const half_t* __restrict__ kp,
                  const half_t* __restrict__ vp, const int* __restrict__ kvrow, int N, int C, int heads, int n_txt, int n_ip,
                  float ip_scale, long units) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int QKS = (D + 15) / 16;           // k-steps of Q K^T
    constexpr int DVT = (D + 31) / 32;           // 32-row slices of the head dim
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int idx = lane & 31, hi = lane >> 5;
    const long u = (long)blockIdx.x * XL_WAVES + wave;
    if (u >= units) return;                      // wave-uniform; there is no barrier in this kernel
    const int ntt = N / 32;                      // token tiles per sample
    const int tt = (int)(u % ntt);
    const int h = (int)((u / ntt) % heads);
    const int sample = (int)(u / ((long)ntt * heads));
    const int NT = (n_txt + 31) / 32;
    const bool has_ip = n_ip > 0;
    const int NK = NT + (has_ip ? 1 : 0);
    const int KS = 2 * NK;                       // 16-key steps of P V
    const long row = kvrow[sample];
    const half_t* kph = kp + (row * heads + h) * ((long)NK * QKS * 512) + lane * 8;
    const half_t* vph = vp + (row * heads + h) * ((long)DVT * KS * 512) + lane * 8;
    const long tok = (long)sample * N + (long)tt * 32 + idx;

    // Q_h^T fragments (B operand) straight from global memory; head dims >= D are zero (K's padding is zero too, but the
    // neighbouring head's values -- or what lies behind the last row -- must not be read)
    half8 qf[QKS];
#pragma unroll
    for (int kk = 0; kk < QKS; ++kk) {
        const int dc = kk * 16 + hi * 8;
        qf[kk] = (dc < D) ? ld_global_h8(q + tok * C + h * D + dc) : zero_h8();
    }
    half8 kf[QKS];
#pragma unroll
    for (int kk = 0; kk < QKS; ++kk) kf[kk] = ld_global_h8(kph + (long)kk * 512);

    f32x16 o[DVT];
#pragma unroll
    for (int d = 0; d < DVT; ++d) o[d] = zero_f16v();
    float m = -INFINITY, l = 0.f;

    for (int t = 0; t < NT; ++t) {
        // V^T of this tile and K of the next one (the ID tile after the last text tile) travel under this tile's work
        half8 vf[DVT][2];
#pragma unroll
        for (int d = 0; d < DVT; ++d)
#pragma unroll
            for (int g = 0; g < 2; ++g) vf[d][g] = ld_global_h8(vph + ((long)d * KS + 2 * t + g) * 512);
        half8 kn[QKS];
        if (t + 1 < NK) {
#pragma unroll
            for (int kk = 0; kk < QKS; ++kk) kn[kk] = ld_global_h8(kph + ((long)(t + 1) * QKS + kk) * 512);
        }
        f32x16 s = zero_f16v();
#pragma unroll
        for (int kk = 0; kk < QKS; ++kk) s = mfma32(kf[kk], qf[kk], s);
        const int nvalid = n_txt - t * 32;       // >= 1; < 32 only in the last text tile
        float mt = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (crow(r, hi) >= nvalid) s[r] = -INFINITY;
            mt = fmaxf(mt, s[r]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float mn = fmaxf(m, mt);           // finite: slot 0 of every text tile is a real key
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        m = mn;
        float ls = 0.f;
        half8 pf[2];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float p = __builtin_amdgcn_exp2f(s[g * 8 + i] - mn);
                ls += p;
                pf[g][i] = (half_t)p;
            }
        l = l * alpha + ls;
#pragma unroll
        for (int d = 0; d < DVT; ++d) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
#pragma unroll
            for (int g = 0; g < 2; ++g) o[d] = mfma32(vf[d][g], pf[g], o[d]);
        }
        if (t + 1 < NK) {
#pragma unroll
            for (int kk = 0; kk < QKS; ++kk) kf[kk] = kn[kk];
        }
    }
    l += __shfl_xor(l, 32, 64);
    const float il = 1.f / l;
#pragma unroll
    for (int d = 0; d < DVT; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] *= il;

    // the ID tile (kf holds it).  ip_scale == 0 multiplies every ID probability by an exact zero: the tile is skipped
    if (has_ip && ip_scale != 0.f) {
        half8 vf[DVT][2];
#pragma unroll
        for (int d = 0; d < DVT; ++d)
#pragma unroll
            for (int g = 0; g < 2; ++g) vf[d][g] = ld_global_h8(vph + ((long)d * KS + 2 * NT + g) * 512);
        f32x16 s = zero_f16v();
#pragma unroll
        for (int kk = 0; kk < QKS; ++kk) s = mfma32(kf[kk], qf[kk], s);
        float mi = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (crow(r, hi) >= n_ip) s[r] = -INFINITY;
            mi = fmaxf(mi, s[r]);
        }
        mi = fmaxf(mi, __shfl_xor(mi, 32, 64));
        float li = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = __builtin_amdgcn_exp2f(s[r] - mi);
            li += s[r];
        }
        li += __shfl_xor(li, 32, 64);
        const float f = ip_scale / li;
        half8 pf[2];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int i = 0; i < 8; ++i) pf[g][i] = (half_t)(s[g * 8 + i] * f);
#pragma unroll
        for (int d = 0; d < DVT; ++d)
#pragma unroll
            for (int g = 0; g < 2; ++g) o[d] = mfma32(vf[d][g], pf[g], o[d]);
    }

    // O_h^T -> out: lane = token, registers 4 j .. 4 j + 3 = four consecutive head dims
    half_t* op = out + tok * C + h * D;
#pragma unroll
    for (int d = 0; d < DVT; ++d)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int dd = d * 32 + 8 * j + 4 * hi;
            if (dd < D) {                        // D % 8 == 0: a group of four never straddles the head's end
                half4 ov;
#pragma unroll
                for (int i = 0; i < 4; ++i) ov[i] = (half_t)o[d][j * 4 + i];
                *reinterpret_cast<half4*>(op + dd) = ov;
            }
        }
#endif
}

// K image [r][h][kt][kk][lane][8], V^T image [r][h][dt][ks][lane][8]; key tile kt < NT holds text keys 32 kt + slot, tile NT
// (when n_ip > 0) the ID keys from its slot 0.  Every 16-byte chunk of both images is written, absent slots as zeros.
__global__ void __launch_bounds__(256)
kv_pack_long_kernel(const half_t* __restrict__ kv_txt, const half_t* __restrict__ kv_ip, half_t* __restrict__ kp,
                    half_t* __restrict__ vp, int R, int C, int heads, int n_txt, int n_ip, int NT, int NK) {
    const int D = C / heads, L = n_txt + n_ip;
    const int QKS = (D + 15) / 16, DVT = (D + 31) / 32, KS = 2 * NK;
    const long kchunks = (long)heads * NK * QKS * 64, vchunks = (long)heads * DVT * KS * 64;   // 16-B chunks per packed row
    const long total = (long)R * (kchunks + vchunks);
    // source element of key slot `slot` (0 .. 32 NK - 1) of context row r, or nullptr
    auto src_row = [&](int r, int slot) -> const half_t* {
        const int kt = slot >> 5, j = slot & 31;
        if (kt < NT) {
            const int key = kt * 32 + j;
            return key < n_txt ? kv_txt + ((long)r * L + key) * 2 * C : nullptr;
        }
        return j < n_ip ? kv_ip + ((long)r * L + n_txt + j) * 2 * C : nullptr;
    };
    for (long qi = (long)blockIdx.x * 256 + threadIdx.x; qi < total; qi += (long)gridDim.x * 256) {
        const int r = (int)(qi / (kchunks + vchunks));
        long e = qi - (long)r * (kchunks + vchunks);
        half8 o = zero_h8();
        if (e < kchunks) {
            const long e0 = e;
            const int lane = (int)(e & 63); e >>= 6;
            const int kk = (int)(e % QKS); e /= QKS;
            const int kt = (int)(e % NK); const int h = (int)(e / NK);
            const int dc = kk * 16 + (lane >> 5) * 8;
            const half_t* s = src_row(r, kt * 32 + (lane & 31));
            if (s && dc < D) o = ld_global_h8(s + h * D + dc);   // D % 8 == 0, so a chunk never straddles the head
            *reinterpret_cast<half8*>(kp + ((long)r * kchunks + e0) * 8) = o;
        } else {
            e -= kchunks;
            const long e0 = e;
            const int lane = (int)(e & 63); e >>= 6;
            const int ks = (int)(e % KS); e /= KS;
            const int dt = (int)(e % DVT); const int h = (int)(e / DVT);
            const int d = dt * 32 + (lane & 31), hi = lane >> 5;
            if (d < D) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const half_t* s = src_row(r, ks * 16 + 4 * hi + (i & 3) + 8 * (i >> 2));
                    if (s) o[i] = s[C + h * D + d];
                }
            }
            *reinterpret_cast<half8*>(vp + ((long)r * vchunks + e0) * 8) = o;
        }
    }
}

bool long_head_dim(int D) { return D == 32 || D == 40 || D == 64 || D == 80 || D == 160; }

// most text rows next to n_ip ID rows: 33 key tiles at the most either way (a context without ID rows, as a ControlNet sees
// a pipeline's text + ID rows, may use the ID tile's slots for text)
int long_max_txt(int n_ip) { return CID_XATTN_LONG_MAX_TXT + (n_ip > 0 ? 0 : CID_XATTN_LONG_MAX_IP); }

}  // namespace

extern "C" int32_t cid_xattn_long_max_txt(void) { return CID_XATTN_LONG_MAX_TXT; }

extern "C" int64_t cid_kv_pack_long_elems(int32_t C, int32_t heads, int32_t n_txt, int32_t n_ip, int32_t which) {
    if (heads <= 0 || C <= 0 || C % heads || n_txt < 1 || n_txt > long_max_txt(n_ip) || n_ip < 0 || n_ip > CID_XATTN_LONG_MAX_IP)
        return -22;
    const int D = C / heads;
    const int QKS = (D + 15) / 16, DVT = (D + 31) / 32;
    const int NK = (n_txt + 31) / 32 + (n_ip > 0 ? 1 : 0);
    return which == 0 ? (int64_t)heads * NK * QKS * 512 : (int64_t)heads * DVT * 2 * NK * 512;
}

extern "C" int cid_kv_pack_long_f16(const cid_half* kv_txt, const cid_half* kv_ip, cid_half* kp, cid_half* vp,
                                    int32_t R, int32_t C, int32_t heads, int32_t n_txt, int32_t n_ip, cid_stream_t stream) {
    CID_CHECK_ARG(kv_txt && kv_ip && kp && vp, "cid_kv_pack_long_f16: null pointer");
    CID_CHECK_ARG(R > 0 && heads > 0 && C > 0 && C % heads == 0 && (C / heads) % 8 == 0, "cid_kv_pack_long_f16: bad C/heads");
    CID_CHECK_ARG(n_txt >= 1 && n_txt <= long_max_txt(n_ip), "cid_kv_pack_long_f16: 1 to %d text rows (got %d)",
                  long_max_txt(n_ip), n_txt);
    CID_CHECK_ARG(n_ip >= 0 && n_ip <= CID_XATTN_LONG_MAX_IP, "cid_kv_pack_long_f16: 0 to %d ID rows (got %d)",
                  CID_XATTN_LONG_MAX_IP, n_ip);
    const int NT = (n_txt + 31) / 32, NK = NT + (n_ip > 0 ? 1 : 0);
    const long krow = cid_kv_pack_long_elems(C, heads, n_txt, n_ip, 0), vrow = cid_kv_pack_long_elems(C, heads, n_txt, n_ip, 1);
    const long total = (long)R * (krow + vrow) / 8;
    const int grid = (int)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256);
    hipLaunchKernelGGL(kv_pack_long_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const half_t*)kv_txt,
                       (const half_t*)kv_ip, (half_t*)kp, (half_t*)vp, R, C, heads, n_txt, n_ip, NT, NK);
    CID_CHECK_LAUNCH("cid_kv_pack_long_f16");
    return 0;
}

extern "C" int cid_id_xattn_long_f16(const cid_half* q, cid_half* out, const cid_half* kp, const cid_half* vp,
                                     const int32_t* kvrow, int32_t B, int32_t N, int32_t C, int32_t heads,
                                     int32_t n_txt, int32_t n_ip, float ip_scale, cid_stream_t stream) {
    CID_CHECK_ARG(q && out && kp && vp && kvrow, "cid_id_xattn_long_f16: null pointer");
    CID_CHECK_ARG(B > 0 && N > 0 && heads > 0 && C > 0 && C % heads == 0, "cid_id_xattn_long_f16: bad shape");
    CID_CHECK_ARG(N % 32 == 0, "cid_id_xattn_long_f16: N=%d is not a multiple of 32 tokens", N);
    const int D = C / heads;
    CID_CHECK_ARG(long_head_dim(D), "cid_id_xattn_long_f16: no kernel for head_dim=%d (32, 40, 64, 80, 160)", D);
    CID_CHECK_ARG(n_txt >= 1 && n_txt <= long_max_txt(n_ip), "cid_id_xattn_long_f16: 1 to %d text rows (got %d)",
                  long_max_txt(n_ip), n_txt);
    CID_CHECK_ARG(n_ip >= 0 && n_ip <= CID_XATTN_LONG_MAX_IP, "cid_id_xattn_long_f16: 0 to %d ID rows (got %d)",
                  CID_XATTN_LONG_MAX_IP, n_ip);
    const long units = (long)B * heads * (N / 32);
    const long blocks = (units + XL_WAVES - 1) / XL_WAVES;
    CID_CHECK_ARG(blocks <= 0x7fffffffL, "cid_id_xattn_long_f16: too many (sample, head, token tile) units");
#define CID_XL(DD)                                                                                                       \
    case DD:                                                                                                             \
        hipLaunchKernelGGL(xattn_long_kernel<DD>, dim3((unsigned)blocks), dim3(64 * XL_WAVES), 0, (hipStream_t)stream,   \
                           (const half_t*)q, (half_t*)out, (const half_t*)kp, (const half_t*)vp, kvrow, N, C, heads,     \
                           n_txt, n_ip, ip_scale, units);                                                                \
        break;
    switch (D) {
        CID_XL(32) CID_XL(40) CID_XL(64) CID_XL(80) CID_XL(160)
    }
#undef CID_XL
    CID_CHECK_LAUNCH("cid_id_xattn_long_f16");
    return 0;
}

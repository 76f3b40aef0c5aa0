// Self-attention guidance (Hong et al., arXiv 2210.00939): the column mass of a self-attention map, which the
// flash kernels of attn.hip never materialise, and the masked Gaussian blur with re-noising of the latents.  Both are small
// (the mid block's token count, the latent tensor) and sit inside the captured step; the guided update itself is a
// compile-time switch of the step kernels in misc.hip.
#include "common.h"
#include "../../include/cid.h"

namespace {

// ---------------------------------------------------------------- column mass
// mass[b][j] = mean_head sum_{i < n_keys} softmax_j(q_i . k_j)        (scores in the base-2 domain: q carries scale * log2 e)
// One workgroup per sample walks the heads one after another.  Per head, pass 1 gives every wave 32-row tiles of Q: it holds
// the tile's A fragments, streams the K tiles through v_mfma_f32_32x32x16_f16 (operands straight from global memory: a
// fragment is 8 consecutive halves of one row) and keeps a running (max, sum) per lane and row, merged across the 32 lanes of a
// row once per tile -> LDS (max, 1 / sum) per row.  Pass 2 gives every wave 32-column tiles of K, recomputes the scores tile by
// tile and adds 2^(s - max_i) / sum_i down the rows.  Nothing is shared between workgroups and every sum has one fixed
// order (rows inside a lane by register, row tiles ascending, the two lane halves, heads ascending): no atomics, the same
// input gives the same bits.  Keys j >= n_keys are masked to -inf, rows i >= n_keys do not contribute, tiles wholly in the
// padding are skipped.  The row statistics need the whole row before any column sum can start, so a sample's work cannot be
// spread over workgroups without a workspace; at the SDXL mid block (20 heads x 1024^2 x 64) one workgroup computes 2.7 GFLOP twice:
// 5.0 ms measured, against 91 us at SD1.5 512^2 (open work).
constexpr int CM_THREADS = 512;
constexpr int CM_WAVES = CM_THREADS / 64;
constexpr int CM_MAXN = 4096;
constexpr float CM_NEG = -3.0e38f;       // finite "no key yet": (CM_NEG - max) never becomes inf - inf

template <int STEPS>
CID_DEVINL void cm_load_frags(half8 (&f)[STEPS], const half_t* row, int d, int hi) {
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const int k0 = 16 * s + 8 * hi;                 // d % 8 == 0: a fragment lies inside the head or wholly outside it
        f[s] = k0 < d ? ld_global_h8(row + k0) : zero_h8();
    }
}

template <int STEPS>
CID_DEVINL f32x16 cm_scores(const half8 (&a)[STEPS], const half8 (&b)[STEPS]) {
    f32x16 acc = zero_f16v();
#pragma unroll
    for (int s = 0; s < STEPS; ++s) acc = mfma32(a[s], b[s], acc);
    return acc;
}

template <int STEPS>      // ceil(d / 16)
__global__ void __launch_bounds__(CM_THREADS)
attn_colmass_kernel(const half_t* __restrict__ q, int ldq, const half_t* __restrict__ k, int ldk, float* __restrict__ mass,
                    int N, int n_keys, int heads, int d) {
    __shared__ float rmax[CM_MAXN], rinv[CM_MAXN], macc[CM_MAXN];
    const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, idx = lane & 31, hi = lane >> 5;
    const int tiles = (n_keys + 31) >> 5;               // row / column tiles that hold a real token
    const half_t* qb = q + (long)b * N * ldq;
    const half_t* kb = k + (long)b * N * ldk;
    for (int j = threadIdx.x; j < N; j += CM_THREADS) macc[j] = 0.f;
    for (int h = 0; h < heads; ++h) {
        const half_t* qh = qb + h * d;
        const half_t* kh = kb + h * d;
        // pass 1: (max, 1 / sum) of every real row
        for (int rt = wave; rt < tiles; rt += CM_WAVES) {
            half8 a[STEPS];
            cm_load_frags<STEPS>(a, qh + (long)(rt * 32 + idx) * ldq, d, hi);
            float m[16], l[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) { m[r] = CM_NEG; l[r] = 0.f; }
            for (int ct = 0; ct < tiles; ++ct) {
                half8 bf[STEPS];
                cm_load_frags<STEPS>(bf, kh + (long)(ct * 32 + idx) * ldk, d, hi);
                const f32x16 s = cm_scores<STEPS>(a, bf);        // s[r]: row crow(r, hi), column idx of the tile
                if (ct * 32 + idx < n_keys) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float mn = fmaxf(m[r], s[r]);
                        l[r] = l[r] * __builtin_amdgcn_exp2f(m[r] - mn) + __builtin_amdgcn_exp2f(s[r] - mn);
                        m[r] = mn;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {                      // across the 32 lanes that share the row (xor < 32 stays in the half)
                float mm = m[r];
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) mm = fmaxf(mm, __shfl_xor(mm, o, 64));
                float ll = l[r] * __builtin_amdgcn_exp2f(m[r] - mm);
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) ll += __shfl_xor(ll, o, 64);
                if (idx == 0) {
                    const int i = rt * 32 + crow(r, hi);
                    rmax[i] = mm;
                    rinv[i] = 1.f / ll;                          // >= 1 term equals 2^0: ll >= 1
                }
            }
        }
        __syncthreads();
        // pass 2: column sums of the normalised map
        for (int ct = wave; ct < tiles; ct += CM_WAVES) {
            half8 bf[STEPS];
            cm_load_frags<STEPS>(bf, kh + (long)(ct * 32 + idx) * ldk, d, hi);
            float col = 0.f;
            for (int rt = 0; rt < tiles; ++rt) {
                half8 a[STEPS];
                cm_load_frags<STEPS>(a, qh + (long)(rt * 32 + idx) * ldq, d, hi);
                const f32x16 s = cm_scores<STEPS>(a, bf);
                float part = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = rt * 32 + crow(r, hi);
                    const float p = __builtin_amdgcn_exp2f(s[r] - rmax[i]) * rinv[i];
                    part += i < n_keys ? p : 0.f;
                }
                col += part;
            }
            col += __shfl_xor(col, 32, 64);                     // the two halves hold rows 4 hi + ... of the same column
            if (hi == 0) macc[ct * 32 + idx] += col;            // this lane alone touches the slot, in every head
        }
        __syncthreads();                                         // the next head overwrites the row statistics
    }
    const float inv_heads = 1.f / (float)heads;
    for (int j = threadIdx.x; j < N; j += CM_THREADS)
        mass[(long)b * N + j] = j < n_keys ? macc[j] * inv_heads : 0.f;
}

// ---------------------------------------------------------------- degrade
// out = n_d D + n_e ehat,  x0 = p_x x + p_e e,  ehat = q_x x + q_e e,  D = mask ? blur(x0) : x0          (cid.h)
// One workgroup per 16 x 16 pixels of one (sample, channel) plane: x0 of the tile and its 4-pixel halo (reflect) goes to LDS,
// the nine taps run along x into a second LDS image and along y from there.  fp32 throughout, one rounding at the store.
constexpr int DG_T = 16, DG_R = 4, DG_H = DG_T + 2 * DG_R;

CID_DEVINL int reflect_idx(int i, int n) {      // |overshoot| <= 4 < n; the clamp only guards tile pixels beyond the image
    i = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

__global__ void __launch_bounds__(DG_T * DG_T)
sag_degrade_kernel(const half_t* __restrict__ lat, const half_t* __restrict__ eps, const float* __restrict__ mass,
                   half_t* __restrict__ out, const float* __restrict__ coef, int h, int w, int hm, int wm, int C) {
    __shared__ float t0[DG_H][DG_H + 1], t1[DG_H][DG_T + 1];
    const float px = coef[0], pe = coef[1], qx = coef[2], qe = coef[3], nd = coef[4], ne = coef[5];
    // exp(-k^2 / 2), k = 0 .. 4, over their sum with both signs
    constexpr float G0 = 1.f, G1 = 0.60653065971263342f, G2 = 0.13533528323661270f, G3 = 0.011108996538242306f,
                    G4 = 0.00033546262790251185f;
    constexpr float GS = G0 + 2.f * (G1 + G2 + G3 + G4);
    const float tap[9] = {G4 / GS, G3 / GS, G2 / GS, G1 / GS, G0 / GS, G1 / GS, G2 / GS, G3 / GS, G4 / GS};
    const int plane = blockIdx.z, b = plane / C;
    const long base = (long)plane * h * w;
    const int x0 = blockIdx.x * DG_T, y0 = blockIdx.y * DG_T;
    const int tid = threadIdx.x;
    for (int e = tid; e < DG_H * DG_H; e += DG_T * DG_T) {
        const int ly = e / DG_H, lx = e - ly * DG_H;
        const long at = base + (long)reflect_idx(y0 - DG_R + ly, h) * w + reflect_idx(x0 - DG_R + lx, w);
        t0[ly][lx] = px * (float)lat[at] + pe * (float)eps[at];
    }
    __syncthreads();
    for (int e = tid; e < DG_H * DG_T; e += DG_T * DG_T) {
        const int ly = e / DG_T, lx = e - ly * DG_T;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) s += tap[k] * t0[ly][lx + k];
        t1[ly][lx] = s;
    }
    __syncthreads();
    const int ty = tid / DG_T, tx = tid - ty * DG_T, y = y0 + ty, x = x0 + tx;
    if (y < h && x < w) {
        float blur = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) blur += tap[k] * t1[ty + k][tx];
        // nearest neighbour up from the mid block's (hm, wm): source index floor(dst * in / out)
        const int my = (int)((long)y * hm / h), mx = (int)((long)x * wm / w);
        const bool masked = mass[(long)b * hm * wm + my * wm + mx] > 1.0f;
        const long at = base + (long)y * w + x;
        const float xv = (float)lat[at], ev = (float)eps[at];
        const float dv = masked ? blur : t0[ty + DG_R][tx + DG_R];
        out[at] = (half_t)(nd * dv + ne * (qx * xv + qe * ev));
    }
}

}  // namespace

extern "C" int cid_attn_colmass_f16(const cid_half* q, int32_t ldq, const cid_half* k, int32_t ldk, float* mass,
                                    int32_t B, int32_t N, int32_t n_keys, int32_t heads, int32_t d, cid_stream_t stream) {
    CID_CHECK_ARG(q && k && mass, "cid_attn_colmass_f16: null pointer");
    CID_CHECK_ARG(B > 0 && heads > 0 && N > 0 && N % 32 == 0 && N <= CM_MAXN,
                  "cid_attn_colmass_f16: N must be a positive multiple of 32 up to %d (got %d)", CM_MAXN, N);
    CID_CHECK_ARG(n_keys > 0 && n_keys <= N, "cid_attn_colmass_f16: n_keys = %d of N = %d", n_keys, N);
    CID_CHECK_ARG(d > 0 && d % 8 == 0 && ldq % 8 == 0 && ldk % 8 == 0 && ldq >= heads * d && ldk >= heads * d,
                  "cid_attn_colmass_f16: bad head width / pitches (d %% 8, ld %% 8, ld >= heads * d)");
    CID_CHECK_ARG((uintptr_t)q % 16 == 0 && (uintptr_t)k % 16 == 0 && (uintptr_t)mass % 16 == 0,
                  "cid_attn_colmass_f16: every buffer must be 16-byte aligned");
    const half_t* qp = (const half_t*)q;
    const half_t* kp = (const half_t*)k;
#define CID_CM_LAUNCH(S)                                                                                                   \
    hipLaunchKernelGGL(attn_colmass_kernel<S>, dim3(B), dim3(CM_THREADS), 0, (hipStream_t)stream, qp, (int)ldq, kp,        \
                       (int)ldk, mass, (int)N, (int)n_keys, (int)heads, (int)d)
    switch (d) {                             // the head widths of cid_self_attn_f16; STEPS = ceil(d / 16)
        case 32: CID_CM_LAUNCH(2); break;
        case 40: CID_CM_LAUNCH(3); break;
        case 64: CID_CM_LAUNCH(4); break;
        case 80: CID_CM_LAUNCH(5); break;
        case 160: CID_CM_LAUNCH(10); break;
        default:
            cid_set_error("cid_attn_colmass_f16: unsupported head dim %d (32, 40, 64, 80, 160)", d);
            return -22;
    }
#undef CID_CM_LAUNCH
    CID_CHECK_LAUNCH("cid_attn_colmass_f16");
    return 0;
}

extern "C" int cid_sag_degrade_f16(const cid_half* latents, const cid_half* eps_g, const float* mass, cid_half* out,
                                   const float* coef, int32_t B, int32_t C, int32_t h, int32_t w, int32_t hm, int32_t wm,
                                   cid_stream_t stream) {
    CID_CHECK_ARG(latents && eps_g && mass && out && coef, "cid_sag_degrade_f16: null pointer");
    CID_CHECK_ARG(B > 0 && C > 0 && hm > 0 && wm > 0, "cid_sag_degrade_f16: B, C, hm, wm must be positive");
    CID_CHECK_ARG(h >= 5 && w >= 5, "cid_sag_degrade_f16: reflect padding by 4 needs h, w >= 5 (got %d x %d)", h, w);
    CID_CHECK_ARG((long)B * C <= 65535 && (long)B * C * h * w <= 0x7fffffffL, "cid_sag_degrade_f16: tensor too large");
    for (const void* p : {(const void*)latents, (const void*)eps_g, (const void*)mass, (const void*)out, (const void*)coef})
        CID_CHECK_ARG((uintptr_t)p % 16 == 0, "cid_sag_degrade_f16: every buffer must be 16-byte aligned");
    hipLaunchKernelGGL(sag_degrade_kernel, dim3((w + DG_T - 1) / DG_T, (h + DG_T - 1) / DG_T, B * C), dim3(DG_T * DG_T), 0,
                       (hipStream_t)stream, (const half_t*)latents, (const half_t*)eps_g, mass, (half_t*)out, coef, (int)h,
                       (int)w, (int)hm, (int)wm, (int)C);
    CID_CHECK_LAUNCH("cid_sag_degrade_f16");
    return 0;
}

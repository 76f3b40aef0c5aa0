// FreeU (diffusers 0.23 utils/torch_utils.py apply_freeu / fourier_filter, called from UpBlock2D / CrossAttnUpBlock2D.forward
// in front of torch.cat([hidden, skip], 1)) on token-major tensors: the backbone's first c_x / 2 channels times b, and the
// skip tensor through the low-frequency filter.  With threshold = 1 the filter's box holds the four frequencies {-1, 0}^2,
// so per (sample, channel) plane it is seven real sums and a pointwise update (cid.h):
//     phi = {1, cos th, sin th, cos tw, sin tw, cos(th + tw), sin(th + tw)},   th = 2 pi h / H, tw = 2 pi w / W
//     out[h, w] = x[h, w] + (s - 1) / (H W) * sum_k (sum_{h', w'} x[h', w'] phi_k[h', w']) phi_k[h, w]
// No FFT, no permute.  Two launches: the sums (partials per token slice into ws), then the update, which first adds the
// slices' partials in slice order.  fp32 throughout, one rounding at the store, no atomics: the same input gives the same bits.
#include "common.h"
#include "../../include/cid.h"

namespace {

constexpr int FU_SLAB = 64;         // channels per workgroup: 8 lanes x 16 bytes of a token row
constexpr int FU_NPHI = 7;
constexpr int FU_TG = 32;           // token rows in flight per workgroup (256 lanes / 8 lanes per row)
constexpr int FU_MAX_SIDE = 1024;   // H, W: the twiddle table [H + W] sits in LDS
constexpr int FU_WGS = 256;         // workgroups that fill the chip (the MI355X has 256 CUs); a constant, so that the slicing -- and
                                    // with it the order of the sums -- does not depend on the device asked
constexpr int FU_MIN_TOKENS = 64;   // tokens per slice at least

// slices of the token axis: 1 where (sample, slab) workgroups fill the chip already (SD1.5 up block 0 at CFG batch 8: 160 of them,
// 13 KB each: latency either way), otherwise as many as bring the grid to FU_WGS (SDXL up block 1: 2 samples x 5 slabs of
// 64 x 64 tokens -> 26 slices), each at least FU_MIN_TOKENS long
inline int fu_slices(int B, int c_skip, int HW) {
    const long wgs = (long)B * ((c_skip + FU_SLAB - 1) / FU_SLAB);
    const long want = (FU_WGS + wgs - 1) / wgs, most = (HW + FU_MIN_TOKENS - 1) / FU_MIN_TOKENS;
    const long t = want < most ? want : most;
    return (int)(t < 1 ? 1 : t);
}

// (cos, sin) of 2 pi i / n for i < n, accurate to fp32: sincospif on the reduced argument 2 i / n in [0, 2)
CID_DEVINL void fu_twiddles(float2* tab, int H, int W) {
    for (int i = threadIdx.x; i < H + W; i += 256) {
        const int n = i < H ? H : W, k = i < H ? i : i - H;
        float sn, cs;
        sincospif(2.f * (float)k / (float)n, &sn, &cs);
        tab[i] = make_float2(cs, sn);
    }
}

CID_DEVINL void fu_phi(const float2* tab, int t, int H, int W, float* phi) {
    const int h = t / W, w = t - h * W;
    const float2 a = tab[h], b = tab[H + w];
    phi[0] = 1.f;
    phi[1] = a.x; phi[2] = a.y; phi[3] = b.x; phi[4] = b.y;
    phi[5] = a.x * b.x - a.y * b.y;
    phi[6] = a.y * b.x + a.x * b.y;
}

// grid (slice, slab, sample).  ws[((b * nslab + slab) * T + slice) * 7 + k][64]: the slice's sum of x * phi_k per channel of the slab
__global__ void __launch_bounds__(256)
freeu_sums_kernel(const half_t* __restrict__ skip, int c_skip, int H, int W, int chunk, float* __restrict__ ws) {
    __shared__ float2 tab[2 * FU_MAX_SIDE];
    __shared__ float part[4][FU_NPHI][FU_SLAB];
    const int HW = H * W;
    const int slice = blockIdx.x, slab = blockIdx.y, b = blockIdx.z;
    const int cl = threadIdx.x & 7, tg = threadIdx.x >> 3;
    const int c0 = slab * FU_SLAB + cl * 8;
    const int t0 = slice * chunk, t1 = min(t0 + chunk, HW);
    fu_twiddles(tab, H, W);
    __syncthreads();
    float acc[FU_NPHI][8];
#pragma unroll
    for (int k = 0; k < FU_NPHI; ++k)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[k][i] = 0.f;
    if (c0 < c_skip) {
        for (int t = t0 + tg; t < t1; t += FU_TG) {
            const half8 v = ld_global_h8(skip + ((long)b * HW + t) * c_skip + c0);
            float phi[FU_NPHI];
            fu_phi(tab, t, H, W, phi);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float f = (float)v[i];
#pragma unroll
                for (int k = 0; k < FU_NPHI; ++k) acc[k][i] = __builtin_fmaf(f, phi[k], acc[k][i]);
            }
        }
    }
    // the 8 token rows of a wave (lane bits 3..5), then the 4 waves through LDS: a fixed order
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < FU_NPHI; ++k)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float v = acc[k][i];
            v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
            if (lane < 8) part[wave][k][cl * 8 + i] = v;
        }
    __syncthreads();
    float* dst = ws + (((long)b * gridDim.y + slab) * gridDim.x + slice) * (FU_NPHI * FU_SLAB);
    for (int e = threadIdx.x; e < FU_NPHI * FU_SLAB; e += 256) {
        const int k = e / FU_SLAB, c = e - k * FU_SLAB;
        dst[e] = ((part[0][k][c] + part[1][k][c]) + part[2][k][c]) + part[3][k][c];
    }
}

// the same grid.  Every workgroup adds the T partials of its (sample, slab) in slice order, filters its slice of the tokens and
// then takes its share of the backbone's scaled half (a grid-stride walk over [B * HW][c_x / 16] vectors).
__global__ void __launch_bounds__(256)
freeu_apply_kernel(const half_t* skip, half_t* skip_out, int c_skip, int H, int W, int chunk, const float* __restrict__ ws,
                   float gain /* (s - 1) / (H W) */, half_t* __restrict__ x, int c_x, float bscale, long x_vecs /* B * HW * c_x / 16 */) {
    __shared__ float2 tab[2 * FU_MAX_SIDE];
    __shared__ float coef[FU_NPHI][FU_SLAB];
    const int HW = H * W;
    const int slice = blockIdx.x, slab = blockIdx.y, b = blockIdx.z, T = gridDim.x;
    const int cl = threadIdx.x & 7, tg = threadIdx.x >> 3;
    const int c0 = slab * FU_SLAB + cl * 8;
    const int t0 = slice * chunk, t1 = min(t0 + chunk, HW);
    fu_twiddles(tab, H, W);
    const float* src = ws + ((long)b * gridDim.y + slab) * T * (FU_NPHI * FU_SLAB);
    for (int e = threadIdx.x; e < FU_NPHI * FU_SLAB; e += 256) {
        float v = 0.f;
        for (int j = 0; j < T; ++j) v += src[(long)j * (FU_NPHI * FU_SLAB) + e];
        (&coef[0][0])[e] = v * gain;
    }
    __syncthreads();
    if (c0 < c_skip) {
        float cf[FU_NPHI][8];
#pragma unroll
        for (int k = 0; k < FU_NPHI; ++k)
#pragma unroll
            for (int i = 0; i < 8; ++i) cf[k][i] = coef[k][cl * 8 + i];
        for (int t = t0 + tg; t < t1; t += FU_TG) {
            const long at = ((long)b * HW + t) * c_skip + c0;
            const half8 v = ld_global_h8(skip + at);
            float phi[FU_NPHI];
            fu_phi(tab, t, H, W, phi);
            half8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float d = cf[0][i];
#pragma unroll
                for (int k = 1; k < FU_NPHI; ++k) d = __builtin_fmaf(cf[k][i], phi[k], d);
                o[i] = (half_t)((float)v[i] + d);
            }
            *reinterpret_cast<half8*>(skip_out + at) = o;
        }
    }
    const int hv = c_x >> 4;                                   // 16-byte vectors of a row's scaled half
    const long lin = ((long)b * gridDim.y + slab) * T + slice, nwg = (long)gridDim.x * gridDim.y * gridDim.z;
    for (long q = lin * 256 + threadIdx.x; q < x_vecs; q += nwg * 256) {
        const long row = q / hv;
        half_t* p = x + row * c_x + (q - row * hv) * 8;
        half8 v = ld_global_h8(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (half_t)(bscale * (float)v[i]);
        *reinterpret_cast<half8*>(p) = v;
    }
}

}  // namespace

extern "C" int64_t cid_freeu_ws_bytes(int32_t B, int32_t c_skip, int32_t H, int32_t W) {
    if (B <= 0 || c_skip <= 0 || H <= 0 || W <= 0 || H > FU_MAX_SIDE || W > FU_MAX_SIDE) return 0;
    const long nslab = (c_skip + FU_SLAB - 1) / FU_SLAB;
    return (int64_t)B * nslab * fu_slices(B, c_skip, H * W) * FU_NPHI * FU_SLAB * (long)sizeof(float);
}

extern "C" int cid_freeu_f16(cid_half* x, int32_t c_x, float b, const cid_half* skip, cid_half* skip_out, int32_t c_skip,
                             float s, int32_t B, int32_t H, int32_t W, float* ws, cid_stream_t stream) {
    CID_CHECK_ARG(x && skip && skip_out && ws, "cid_freeu_f16: null pointer");
    CID_CHECK_ARG(B > 0 && B <= 65535, "cid_freeu_f16: B must be in 1..65535 (got %d)", B);
    CID_CHECK_ARG(H >= 2 && W >= 2 && H <= FU_MAX_SIDE && W <= FU_MAX_SIDE,
                  "cid_freeu_f16: H and W must be in 2..%d (got %d x %d; the filter's box is empty on a side of 1)", FU_MAX_SIDE, H, W);
    CID_CHECK_ARG(c_x > 0 && c_x % 16 == 0, "cid_freeu_f16: c_x must be a positive multiple of 16 (got %d; the scaled half ends on a 16-byte vector)", c_x);
    CID_CHECK_ARG(c_skip > 0 && c_skip % 8 == 0, "cid_freeu_f16: c_skip must be a positive multiple of 8 (got %d)", c_skip);
    CID_CHECK_ARG(((uintptr_t)x % 16 | (uintptr_t)skip % 16 | (uintptr_t)skip_out % 16 | (uintptr_t)ws % 4) == 0,
                  "cid_freeu_f16: x, skip and skip_out must be 16-byte aligned");
    CID_CHECK_ARG(b == b && s == s && fabsf(b) <= 3.402823466e+38f && fabsf(s) <= 3.402823466e+38f, "cid_freeu_f16: s and b must be finite");
    const int HW = H * W, nslab = (c_skip + FU_SLAB - 1) / FU_SLAB;
    CID_CHECK_ARG(nslab <= 65535, "cid_freeu_f16: c_skip = %d is too wide (at most 65535 slabs of %d channels)", c_skip, FU_SLAB);
    const int T = fu_slices(B, c_skip, HW);
    const int chunk = (HW + T - 1) / T;
    const dim3 grid(T, nslab, B);
    hipLaunchKernelGGL(freeu_sums_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const half_t*)skip, c_skip, H, W, chunk, ws);
    CID_CHECK_LAUNCH("cid_freeu_f16 (sums)");
    hipLaunchKernelGGL(freeu_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const half_t*)skip, (half_t*)skip_out, c_skip, H, W,
                       chunk, (const float*)ws, (float)(((double)s - 1.0) / ((double)H * (double)W)), (half_t*)x, c_x, b,
                       (long)B * HW * (c_x >> 4));
    CID_CHECK_LAUNCH("cid_freeu_f16 (update)");
    return 0;
}

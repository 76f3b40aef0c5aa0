// Safety checker tail (diffusers 0.23 StableDiffusionSafetyChecker.forward, reached through run_safety_checker of
// pipline_StableDiffusion_ConsistentID.py:584-602, StableDIffusionInpaint_ConsistentID.py:371-381 and
// StableDIffusionControlNetInpaint_ConsistentID.py:468-478): everything after the last encoder layer of the CLIP vision
// tower, and the blackout of the flagged images.  Once per generated image, off the denoise step: latency-bound work
// (a [P][C] matrix-vector product per image), written for one launch and no host round trip, not for throughput.
#include "common.h"
#include "../../include/cid.h"

namespace {

constexpr int HEAD_MAXC = 4096;     // CLS row / projection width held in LDS as fp32
constexpr int HEAD_MAXP = 4096;
constexpr int HEAD_MAXK = 64;
constexpr int HEAD_ROWS = 4;        // projection rows one wave has in flight

// sum over the 256 threads of the workgroup, returned to every thread; `red` is 4 floats of LDS owned by this call site
CID_DEVINL float block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// One 256-thread workgroup per image.  fp32 throughout; the one rounding is the fp16 store of embeds.
//   1. LayerNorm of the CLS row (two passes over the row kept in LDS: mean, then the centred sum of squares)
//   2. e = W ln: a wave per output row, HEAD_ROWS rows in flight, lanes stride the row in 16-byte pieces
//   3. inv = 1 / max(|e|, 1e-12)
//   4. cos[k] = inv * (e . c[k]): a wave per concept row (rows L2-normalised by the host)
//   5. thread 0 walks the thresholds in index order (the special-care adjustment is a loop-carried value)
__global__ void __launch_bounds__(256)
clip_head_kernel(const half_t* __restrict__ x, long ldx, const half_t* __restrict__ gamma, const half_t* __restrict__ beta,
                 float eps, const half_t* __restrict__ w, const float* __restrict__ concepts, const float* __restrict__ thr,
                 int C, int P, int K, int n_special, half_t* __restrict__ embeds, float* __restrict__ cos_out,
                 float* __restrict__ scores, int* __restrict__ flags) {
    __shared__ __attribute__((aligned(16))) float ln[HEAD_MAXC];
    __shared__ float e[HEAD_MAXP];
    __shared__ float cosv[HEAD_MAXK];
    __shared__ float red[3][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const half_t* xr = x + (long)b * ldx;
    const int C8 = C >> 3;

    // 1. LayerNorm
    float s = 0.f;
    for (int i = tid; i < C8; i += 256) {
        const half8 h = ld_global_h8(xr + i * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = (float)h[j];
            ln[i * 8 + j] = v;
            s += v;
        }
    }
    const float mean = block_sum(s, red[0]) / (float)C;
    float q = 0.f;
    for (int i = tid; i < C8; i += 256) {          // every thread re-reads the pieces it wrote itself
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float dlt = ln[i * 8 + j] - mean;
            q += dlt * dlt;
        }
    }
    const float rstd = 1.f / sqrtf(block_sum(q, red[1]) / (float)C + eps);
    for (int i = tid; i < C8; i += 256) {
        const half8 g = ld_global_h8(gamma + i * 8), bb = ld_global_h8(beta + i * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) ln[i * 8 + j] = (ln[i * 8 + j] - mean) * rstd * (float)g[j] + (float)bb[j];
    }
    __syncthreads();

    // 2. projection
    for (int p0 = wave * HEAD_ROWS; p0 < P; p0 += 4 * HEAD_ROWS) {
        float acc[HEAD_ROWS];
#pragma unroll
        for (int r = 0; r < HEAD_ROWS; ++r) acc[r] = 0.f;
        for (int i = lane; i < C8; i += 64) {
            half8 wr[HEAD_ROWS];
#pragma unroll
            for (int r = 0; r < HEAD_ROWS; ++r)
                wr[r] = p0 + r < P ? ld_global_h8(w + (long)(p0 + r) * C + i * 8) : zero_h8();
            const f32x4 l0 = *reinterpret_cast<const f32x4*>(ln + i * 8), l1 = *reinterpret_cast<const f32x4*>(ln + i * 8 + 4);
#pragma unroll
            for (int r = 0; r < HEAD_ROWS; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[r] = __builtin_fmaf((float)wr[r][j], l0[j], acc[r]);
                    acc[r] = __builtin_fmaf((float)wr[r][j + 4], l1[j], acc[r]);
                }
        }
#pragma unroll
        for (int r = 0; r < HEAD_ROWS; ++r) {
            const float v = wave_sum(acc[r]);
            if (lane == 0 && p0 + r < P) e[p0 + r] = v;
        }
    }
    __syncthreads();

    // 3. norm of e; image_embeds is e itself (CLIPVisionModelWithProjection does not normalise it)
    float ss = 0.f;
    for (int p = tid; p < P; p += 256) {
        const float v = e[p];
        ss += v * v;
        if (embeds) embeds[(long)b * P + p] = (half_t)v;
    }
    if (K == 0) return;
    const float inv = 1.f / fmaxf(sqrtf(block_sum(ss, red[2])), 1e-12f);

    // 4. cosines
    for (int k = wave; k < K; k += 4) {
        const float* c = concepts + (long)k * P;
        float a = 0.f;
        for (int p = lane; p < P; p += 64) a = __builtin_fmaf(e[p] * inv, c[p], a);
        a = wave_sum(a);
        if (lane == 0) {
            cosv[k] = a;
            cos_out[(long)b * K + k] = a;
        }
    }
    __syncthreads();

    // 5. decision: round(score, 3) > 0 of the Python loop is rintf(score * 1000) >= 1 (half to even at 0.0005)
    if (tid == 0) {
        float adj = 0.f;
        int flagged = 0;
        for (int k = 0; k < K; ++k) {
            const float sc = (cosv[k] - thr[k]) + adj;
            scores[(long)b * K + k] = sc;
            const bool hit = rintf(sc * 1000.f) >= 1.f;
            if (k < n_special) {
                if (hit) adj = 0.01f;          // lifts every LATER entry, special or not
            } else {
                flagged |= hit;
            }
        }
        flags[b] = flagged;
    }
}

// images [B][per_image] fp16: image b becomes zero where flags[b] != 0 (the flags stay on the device); other images are
// not written.  VEC: 16-byte stores (per_image % 8 == 0 and an aligned base), else one half per store.
template <bool VEC>
__global__ void __launch_bounds__(256)
blackout_kernel(half_t* __restrict__ images, const int* __restrict__ flags, long per_image) {
    const int b = blockIdx.y;
    if (flags[b] == 0) return;
    half_t* img = images + (long)b * per_image;
    const long n = VEC ? per_image >> 3 : per_image;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        if (VEC)
            *reinterpret_cast<half8*>(img + i * 8) = zero_h8();
        else
            img[i] = (half_t)0.f;
    }
}

}  // namespace

extern "C" int cid_clip_head_f16(const cid_half* x, int64_t ldx, const cid_half* ln_gamma, const cid_half* ln_beta, float ln_eps,
                                 const cid_half* w_proj, const float* concepts, const float* thresholds, int32_t B, int32_t C,
                                 int32_t P, int32_t K, int32_t n_special, cid_half* embeds, float* cos, float* scores,
                                 int32_t* flags, cid_stream_t stream) {
    CID_CHECK_ARG(x && ln_gamma && ln_beta && w_proj, "cid_clip_head_f16: null pointer (x, ln_gamma, ln_beta, w_proj)");
    CID_CHECK_ARG(B > 0, "cid_clip_head_f16: B must be positive (got %d)", B);
    CID_CHECK_ARG(C > 0 && C % 8 == 0 && C <= HEAD_MAXC, "cid_clip_head_f16: C must be a multiple of 8, at most %d (got %d)",
                  HEAD_MAXC, C);
    CID_CHECK_ARG(P > 0 && P % 8 == 0 && P <= HEAD_MAXP, "cid_clip_head_f16: P must be a multiple of 8, at most %d (got %d)",
                  HEAD_MAXP, P);
    CID_CHECK_ARG(ldx >= C && ldx % 8 == 0, "cid_clip_head_f16: ldx must be a multiple of 8, at least C (got %lld)", (long long)ldx);
    CID_CHECK_ARG(K >= 0 && K <= HEAD_MAXK, "cid_clip_head_f16: K must be in [0, %d] (got %d)", HEAD_MAXK, K);
    CID_CHECK_ARG(n_special >= 0 && n_special <= K, "cid_clip_head_f16: n_special must be in [0, K] (got %d, K = %d)", n_special, K);
    if (K > 0)
        CID_CHECK_ARG(concepts && thresholds && cos && scores && flags,
                      "cid_clip_head_f16: null pointer (concepts, thresholds, cos, scores, flags are required with K > 0)");
    else
        CID_CHECK_ARG(embeds, "cid_clip_head_f16: K == 0 without embeds leaves nothing to compute");
    CID_CHECK_ARG(((uintptr_t)x | (uintptr_t)ln_gamma | (uintptr_t)ln_beta | (uintptr_t)w_proj) % 16 == 0,
                  "cid_clip_head_f16: x, ln_gamma, ln_beta and w_proj must be 16-byte aligned");
    hipLaunchKernelGGL(clip_head_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, (long)ldx,
                       (const half_t*)ln_gamma, (const half_t*)ln_beta, ln_eps, (const half_t*)w_proj, concepts, thresholds, C, P, K,
                       n_special, (half_t*)embeds, cos, scores, (int*)flags);
    CID_CHECK_LAUNCH("cid_clip_head_f16");
    return 0;
}

extern "C" int cid_blackout_f16(cid_half* images, const int32_t* flags, int32_t B, int64_t per_image, cid_stream_t stream) {
    CID_CHECK_ARG(images && flags, "cid_blackout_f16: null pointer");
    CID_CHECK_ARG(B > 0 && B <= 65535 && per_image >= 1, "cid_blackout_f16: B must be in [1, 65535] and per_image at least 1 (got %d, %lld)",
                  B, (long long)per_image);
    CID_CHECK_ARG((uintptr_t)images % 2 == 0, "cid_blackout_f16: images must be 2-byte aligned");
    const bool vec = per_image % 8 == 0 && (uintptr_t)images % 16 == 0;
    const long n = vec ? per_image / 8 : per_image;
    const long want = (n + 255) / 256;
    const dim3 grid((unsigned)(want < 1024 ? want : 1024), (unsigned)B);
    if (vec)
        hipLaunchKernelGGL(blackout_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (half_t*)images, (const int*)flags,
                           (long)per_image);
    else
        hipLaunchKernelGGL(blackout_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (half_t*)images, (const int*)flags,
                           (long)per_image);
    CID_CHECK_LAUNCH("cid_blackout_f16");
    return 0;
}

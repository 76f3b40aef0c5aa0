// Ends of the VAE encoder (D: AutoencoderKL.encode, as the inpaint pipelines call it through prepare_latents /
// prepare_mask_latents, pipelines/StableDIffusionInpaint_ConsistentID.py:231-295, ControlNet variant :254-356):
//   cid_vae_encode_in_f16  the inpaint pre-processing (normalise, binarise the mask, image * (mask < 0.5), fp16) folded into
//                          the loads of encoder.conv_in (3 -> 128, 3x3 pad 1), plus the nearest-sampled mask latents;
//   cid_vae_encode_out_f16 encoder.conv_out (3x3, cin -> 2L) with quant_conv folded into its weights, then the
//                          DiagonalGaussianDistribution: moments, clamp, std, mean + std * eps, times scaling_factor.
// Everything between the two (down blocks, Downsample2D(padding=0), mid block, conv_norm_out) is cid_gemm_f16 /
// cid_groupnorm_f16 / cid_softmax_rows_f16.
#include "common.h"
#include "../../include/cid.h"

namespace {

// ---------------------------------------------------------------- encoder conv_in
// Store-bound: 256 bytes of output per pixel and block (128 channels), 12 input bytes.  Same design as conv_in_kernel
// (misc.hip): eight threads share a pixel; each gathers the pixel's 27 inputs (9 taps x 3 channels, fp32, clamped
// unconditional loads) and the 9 mask values ONCE, rounds them to half pairs, and walks every eighth octet of output
// channels with v_dot2_f32_f16 against weights staged in LDS as [k pair][cout] half2; 16-byte stores.  The masked image
// is the same gather with the taps whose mask is >= 0.5 zeroed, so both blocks come out of one pass.
constexpr int EI_KP = 14;        // half pairs of the 27-long contraction (the last pair's second half is zero)
constexpr int EI_MAXCO = 320;
constexpr int EI_TPP = 8;        // threads per pixel

__global__ void __launch_bounds__(256)
vae_encode_in_kernel(const float* __restrict__ image, const float* __restrict__ mask, half_t* __restrict__ out,
                     const half_t* __restrict__ w, const half_t* __restrict__ bias, half_t* __restrict__ mask_latents,
                     int Bi, int Bm, int H, int W, int cout, int normalize, int blocks) {
    __shared__ half2v wl[EI_KP * EI_MAXCO];
    half_t* wl1 = reinterpret_cast<half_t*>(wl);
    for (int co = threadIdx.x; co < cout; co += 256) {
        const half_t* wr = w + (long)co * 27;
        for (int k = 0; k < 27; ++k) wl1[((k >> 1) * cout + co) * 2 + (k & 1)] = wr[k];
        wl1[((EI_KP - 1) * cout + co) * 2 + 1] = (half_t)0.f;
    }
    __syncthreads();
    const bool want_img = blocks & 1, want_msk = (blocks & 2) != 0;
    const int nco = cout >> 3;
    const int HW = H * W;
    const long npix = (long)Bi * HW;
    const int sub = threadIdx.x & (EI_TPP - 1);
    const long ostride = (long)Bi * HW * cout;           // one batch block of the output
    for (long p = (long)blockIdx.x * (256 / EI_TPP) + (threadIdx.x / EI_TPP); p < npix; p += (long)gridDim.x * (256 / EI_TPP)) {
        const int b = (int)(p / HW);
        const int rem = (int)(p - (long)b * HW);
        const int y = rem / W, x = rem - y * W;
        const float* src = image + (long)b * 3 * HW;
        const float* msrc = mask ? mask + (long)(Bm == 1 ? 0 : b) * HW : nullptr;
        half_t v[2 * EI_KP], vm[2 * EI_KP];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
            const int yc = yy < 0 ? 0 : (yy >= H ? H - 1 : yy), xc = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);
            const long o = (long)yc * W + xc;
            const bool keep = msrc ? (msrc[o] < 0.5f) : true;       // binarised at 0.5, masked_image = image * (mask < 0.5)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float t = src[(long)c * HW + o];
                if (normalize) t = 2.f * t - 1.f;
                const half_t h = ok ? (half_t)t : (half_t)0.f;
                v[tap * 3 + c] = h;
                vm[tap * 3 + c] = keep ? h : (half_t)0.f;
            }
        }
        v[27] = (half_t)0.f;
        vm[27] = (half_t)0.f;
        if (mask_latents && sub == 0 && b < Bm && (y & 7) == 0 && (x & 7) == 0)
            // F.interpolate(mask, size=(H / 8, W / 8)) (nearest: source index 8y, 8x) of the binarised mask
            mask_latents[((long)b * (H >> 3) + (y >> 3)) * (W >> 3) + (x >> 3)] = msrc[rem] < 0.5f ? (half_t)0.f : (half_t)1.f;
        for (int cc = sub; cc < nco; cc += EI_TPP) {
            float ai[8], am[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) { ai[i] = 0.f; am[i] = 0.f; }
#pragma unroll
            for (int kp = 0; kp < EI_KP; ++kp) {
                const half2v* wp = wl + kp * cout + cc * 8;
                const half2v xi = {v[2 * kp], v[2 * kp + 1]}, xm = {vm[2 * kp], vm[2 * kp + 1]};
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const half2v wv = wp[i];
                    if (want_img) ai[i] = __builtin_amdgcn_fdot2(xi, wv, ai[i], false);
                    if (want_msk) am[i] = __builtin_amdgcn_fdot2(xm, wv, am[i], false);
                }
            }
            const half8 bb = ld_global_h8(bias + cc * 8);
            half_t* dst = out + ((long)b * HW + rem) * cout + cc * 8;
            if (want_img) {
                half8 o;
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = (half_t)(ai[i] + (float)bb[i]);
                *reinterpret_cast<half8*>(dst) = o;
                dst += ostride;
            }
            if (want_msk) {
                half8 o;
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = (half_t)(am[i] + (float)bb[i]);
                *reinterpret_cast<half8*>(dst) = o;
            }
        }
    }
}

// ---------------------------------------------------------------- encoder conv_out + quant_conv + posterior
// One wave per latent pixel: lane l accumulates the 16-byte channel chunks l, l + 64, ... of the nine taps against all
// 2L <= 8 folded output rows (weights read through L1/L2: 72 KB at cin = 512), a butterfly reduction leaves every sum in
// every lane, and lane j < L writes latent channel j (and the moments j, j + L).  8192 pixels per 512 x 512 image pair:
// microseconds of work, kept plain.
constexpr int EO_MAXL = 4;

__global__ void __launch_bounds__(256)
vae_encode_out_kernel(const half_t* __restrict__ x, half_t* __restrict__ out, float* __restrict__ moments,
                      const half_t* __restrict__ w, const float* __restrict__ bias, const half_t* __restrict__ eps,
                      int B, int H, int W, int cin, int L, float scale) {
    const int lane = threadIdx.x & 63;
    const int nch = cin >> 3;
    const int HW = H * W;
    const long npix = (long)B * HW;
    const int L2 = 2 * L;
    for (long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6); p < npix; p += (long)gridDim.x * 4) {
        const int b = (int)(p / HW);
        const int rem = (int)(p - (long)b * HW);
        const int y = rem / W, xq = rem - y * W;
        float acc[2 * EO_MAXL];
#pragma unroll
        for (int j = 0; j < 2 * EO_MAXL; ++j) acc[j] = 0.f;
        for (int tap = 0; tap < 9; ++tap) {
            const int yy = y + tap / 3 - 1, xx = xq + tap % 3 - 1;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;           // uniform over the wave
            const half_t* src = x + ((long)b * HW + (long)yy * W + xx) * cin;
            for (int c8 = lane; c8 < nch; c8 += 64) {
                const half8 xv = ld_global_h8(src + c8 * 8);
#pragma unroll
                for (int j = 0; j < 2 * EO_MAXL; ++j) {
                    if (j < L2) {
                        const half8 wv = ld_global_h8(w + ((long)j * 9 + tap) * cin + c8 * 8);
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const half2v a2 = {xv[2 * q], xv[2 * q + 1]}, w2 = {wv[2 * q], wv[2 * q + 1]};
                            acc[j] = __builtin_amdgcn_fdot2(a2, w2, acc[j], false);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 2 * EO_MAXL; ++j) acc[j] = wave_sum(acc[j]);
        if (lane < L) {
            float mean = 0.f, logvar = 0.f;
#pragma unroll
            for (int j = 0; j < EO_MAXL; ++j)
                if (j == lane) { mean = acc[j] + bias[j]; }
#pragma unroll
            for (int j = 0; j < 2 * EO_MAXL; ++j)
                if (j == lane + L) { logvar = acc[j] + bias[j]; }
            const long o = ((long)b * L + lane) * HW + rem;
            if (moments) {
                moments[((long)b * L2 + lane) * HW + rem] = mean;
                moments[((long)b * L2 + L + lane) * HW + rem] = logvar;
            }
            float z = mean;
            if (eps) {
                const float lv = fminf(fmaxf(logvar, -30.f), 20.f);
                z = mean + expf(0.5f * lv) * (float)eps[o];
            }
            out[o] = (half_t)(scale * z);
        }
    }
}

inline int grid_for(long items, int per_block, int cap) {
    long g = (items + per_block - 1) / per_block;
    return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" int cid_vae_encode_in_f16(const float* image, int32_t Bi, const float* mask, int32_t Bm, cid_half* out,
                                     const cid_half* w, const cid_half* bias, int32_t H, int32_t W, int32_t cout,
                                     int32_t normalize, int32_t blocks, cid_half* mask_latents, cid_stream_t stream) {
    CID_CHECK_ARG(image && out && w && bias, "cid_vae_encode_in_f16: null pointer");
    CID_CHECK_ARG(Bi > 0 && H > 0 && W > 0 && cout > 0 && cout % 8 == 0 && cout <= EI_MAXCO,
                  "cid_vae_encode_in_f16: bad shape (Bi=%d H=%d W=%d cout=%d; cout %% 8 == 0, cout <= %d)", Bi, H, W, cout, EI_MAXCO);
    CID_CHECK_ARG(blocks >= 1 && blocks <= 3, "cid_vae_encode_in_f16: blocks must be 1 (image), 2 (masked image) or 3 (both), got %d",
                  blocks);
    CID_CHECK_ARG(mask || (!(blocks & 2) && !mask_latents),
                  "cid_vae_encode_in_f16: the masked image and mask_latents need a mask");
    CID_CHECK_ARG(!mask || Bm == 1 || Bm == Bi, "cid_vae_encode_in_f16: mask batch Bm=%d must be 1 or Bi=%d", Bm, Bi);
    CID_CHECK_ARG(!mask_latents || (H % 8 == 0 && W % 8 == 0),
                  "cid_vae_encode_in_f16: mask_latents need H and W multiples of 8 (got %d x %d)", H, W);
    CID_CHECK_ARG((((uintptr_t)out | (uintptr_t)bias) & 15) == 0, "cid_vae_encode_in_f16: out / bias must be 16-byte aligned");
    const long items = (long)Bi * H * W;
    hipLaunchKernelGGL(vae_encode_in_kernel, dim3(grid_for(items, 256 / EI_TPP, 4096)), dim3(256), 0, (hipStream_t)stream,
                       image, mask, (half_t*)out, (const half_t*)w, (const half_t*)bias, (half_t*)mask_latents, Bi,
                       mask ? Bm : 1, H, W, cout, normalize ? 1 : 0, blocks);
    CID_CHECK_LAUNCH("cid_vae_encode_in_f16");
    return 0;
}

extern "C" int cid_vae_encode_out_f16(const cid_half* x, cid_half* out, float* moments, const cid_half* w, const float* bias,
                                      const cid_half* eps, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t L,
                                      float scale, cid_stream_t stream) {
    CID_CHECK_ARG(x && out && w && bias, "cid_vae_encode_out_f16: null pointer");
    CID_CHECK_ARG(B > 0 && H > 0 && W > 0 && cin > 0 && cin % 8 == 0 && L > 0 && L <= EO_MAXL,
                  "cid_vae_encode_out_f16: bad shape (B=%d H=%d W=%d cin=%d L=%d; cin %% 8 == 0, L <= %d)", B, H, W, cin, L, EO_MAXL);
    CID_CHECK_ARG((((uintptr_t)x | (uintptr_t)w) & 15) == 0 && (cin * 2) % 16 == 0,
                  "cid_vae_encode_out_f16: x / w must be 16-byte aligned");
    const long pix = (long)B * H * W;
    hipLaunchKernelGGL(vae_encode_out_kernel, dim3(grid_for(pix, 4, 8192)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)x, (half_t*)out, moments, (const half_t*)w, bias, (const half_t*)eps, B, H, W, cin, L, scale);
    CID_CHECK_LAUNCH("cid_vae_encode_out_f16");
    return 0;
}

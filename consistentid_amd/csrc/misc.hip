// HBM-/latency-bound ends of the UNet step: conv_in, conv_out, timestep embedding,
// the tiny-M linears of the time path, CFG + DDIM update, residual adds.
// None of these is matrix-core work: they are vectorised (16 B per lane) streaming
// kernels; algorithmic bytes = tensors read once + written once.
#include "common.h"
#include "../../include/cid.h"
#include <stdarg.h>

// ---------------------------------------------------------------- error plumbing
static thread_local char g_err[512] = "";
void cid_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* cid_last_error(void) { return g_err; }
extern "C" int cid_version(void) { return 115; }   // 101: cid_gemm_desc.pad_mode, 102: cid_gemm_desc.act, 103: cid_gemm_desc.w_up4, 104: cid_gemm_plan, 105: cid_cfg_multistep_step_f16, 106: cid_residual_accum_f16, 107: cid_clip_head_f16 / cid_blackout_f16, 108: cid_cfg_rescale_f16 / cid_cfg_*_step_scaled_f16, 109: cid_freeu_f16 (freeu.hip), 110: cid_id_xattn_long_f16 / cid_kv_pack_long_* (xattn_long.hip), 111: cid_multistep_step_f16, 112: cid_tiny_conv64_f16 / cid_tiny_decode_in_f16 / cid_tiny_decode_out_f16 (taesd.hip), 113: cid_tiny_encode_in_f16 / cid_tiny_conv64_s2_f16 / cid_tiny_encode_out_f16, 114: cid_cfg_pag_ddim_step_f16 / cid_cfg_pag_multistep_step_f16 / cid_pag_multistep_step_f16 (perturbed-attention guidance), 115: cid_attn_colmass_f16 / cid_sag_degrade_f16 (sag.hip) / cid_cfg_sag_ddim_step_f16 / cid_cfg_sag_multistep_step_f16 / cid_sag_multistep_step_f16 (self-attention guidance)

namespace {

// ---------------------------------------------------------------- conv_in
// sample NCHW [Bin][cin][H][W] -> token-major [B][H*W][cout], 3x3 pad 1 (diffusers UNet2DConditionModel.conv_in as called from
// /root/reference/pipline_StableDiffusion_ConsistentID.py:552-557 on torch.cat([latents] * 2), :537-539).
// HBM-bound on its output (8 input channels, 320 output channels).  Eight threads share a pixel: each gathers the pixel's
// 9 x cin inputs ONCE as packed half pairs and walks every eighth octet of output channels with v_dot2_f32_f16 against
// weights staged in LDS as [k pair][cout] half2 (read in the weights' own [cout][K] order, transposed on the LDS side).  Batch
// row b reads sample b % Bin: the rows that share a sample are COMPUTED once and stored B / Bin times (the CFG duplication).
// (Rounds 1-5: one thread per (pixel, channel octet) re-gathering the 36 inputs with 2-byte loads and converting every
//  weight it touched -- 50 us at the SD1.5 level-0 shape for 10 MB of output.)
constexpr int CIN_MAXKP = 42;    // half pairs of the contraction: 9 taps x cin1 and 9 taps x cin2, each rounded up to a pair
constexpr int CIN_MAXCO = 320;
constexpr int CIN_TPP = 8;       // threads per pixel

// C1 / C2 > 0: the channel split is a compile-time constant (4 + 0 plain, 9 + 0 and 4 + 5 inpainting): every (tap, channel) of the
// gather is then known at compile time and its loads are unconditional (coordinates clamped, the value zeroed outside the image),
// so that all of a pixel's inputs are in flight together.  C1 = 0: any split <= 9, runtime divisions (slow, correct).
template <int C1, int C2>
__global__ void __launch_bounds__(256)
conv_in_kernel(const half_t* __restrict__ sample, const half_t* __restrict__ extra, half_t* __restrict__ out,
               const half_t* __restrict__ w, const half_t* __restrict__ bias, int B, int Bin, int cin1_, int cin2_, int H, int W,
               int cout, const float* __restrict__ in_scale) {
    const int cin1 = C1 > 0 ? C1 : cin1_, cin2 = C1 > 0 ? C2 : cin2_;
    // channels [0, cin1) come from `sample` (the latents, scaled by in_scale), channels [cin1, cin1 + cin2) from `extra`
    // (mask | masked-image latents of a 9-channel inpainting UNet, inpaint ref :320-321 -- concatenated AFTER
    // scale_model_input there, so they are not scaled); both NCHW, batch row b reads sample b % Bin of either
    const int cin = cin1 + cin2;
    // scheduler.scale_model_input (ref :540): a scalar on the latents, read from device memory so one captured graph
    // serves every step; the convolution is linear, so it is applied to the latent part's tap sum (fp32)
    const float isc = in_scale ? in_scale[0] : 1.f;
    __shared__ half2v wl[CIN_MAXKP * CIN_MAXCO];           // [k pair][cout]: part 1 = (tap, ci < cin1), then part 2
    const int K = 9 * cin, K1 = 9 * cin1, K2 = 9 * cin2;
    const int KP1 = (K1 + 1) >> 1, KP2 = (K2 + 1) >> 1;
    half_t* wl1 = reinterpret_cast<half_t*>(wl);
    // staging: thread co copies weight row co ([tap][ci], 2 K bytes) -- its loads are independent and in flight together, its
    // 2-byte LDS stores land 4 bytes from the neighbouring thread's (conflict free).  (An element-per-thread transpose walked
    // K * cout / 256 = 45 dependent load -> store rounds with two runtime divisions each: 50 of this kernel's 70 us.)
    for (int co = threadIdx.x; co < cout; co += 256) {
        const half_t* wr = w + (long)co * K;
        int tap = 0, ci = 0;
        for (int k = 0; k < K; ++k) {
            const int kk = ci < cin1 ? tap * cin1 + ci : 2 * KP1 + tap * cin2 + (ci - cin1);   // position in the reordered contraction
            wl1[((kk >> 1) * cout + co) * 2 + (kk & 1)] = wr[k];
            if (++ci == cin) { ci = 0; ++tap; }
        }
        if (K1 & 1) wl1[((KP1 - 1) * cout + co) * 2 + 1] = (half_t)0.f;                         // the odd pairs' second halves
        if (K2 & 1) wl1[((KP1 + KP2 - 1) * cout + co) * 2 + 1] = (half_t)0.f;
    }
    __syncthreads();
    const int nco = cout >> 3;
    const int HW = H * W, rep = B / Bin;
    const long npix = (long)Bin * HW;
    const int sub = threadIdx.x & (CIN_TPP - 1);
    for (long p = (long)blockIdx.x * (256 / CIN_TPP) + (threadIdx.x / CIN_TPP); p < npix; p += (long)gridDim.x * (256 / CIN_TPP)) {
        const int b = (int)(p / HW);
        const int rem = (int)(p - (long)b * HW);
        const int y = rem / W, x = rem - y * W;
        const half_t* src = sample + (long)b * cin1 * HW;
        const half_t* src2 = extra + (long)b * cin2 * HW;   // not dereferenced when cin2 == 0
        half2v in[CIN_MAXKP];
#pragma unroll
        for (int kp = 0; kp < CIN_MAXKP; ++kp) {
            half_t v[2] = {(half_t)0.f, (half_t)0.f};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                int kk = 2 * kp + h;
                const bool part2 = kk >= 2 * KP1;
                if (part2) kk -= 2 * KP1;
                const int cpart = part2 ? cin2 : cin1;
                const bool live = kp < KP1 + KP2 && kk < 9 * cpart;
                if (C1 > 0 && !live) continue;                  // (compile-time in the specialised instances)
                const int tap = live ? kk / cpart : 0, ci = live ? kk - tap * cpart : 0;
                const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
                const bool ok = live && yy >= 0 && yy < H && xx >= 0 && xx < W;
                const int yc = yy < 0 ? 0 : (yy >= H ? H - 1 : yy), xc = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);
                const half_t* sp = (part2 && cin2 > 0) ? src2 : src;
                const half_t t = sp[((long)ci * H + yc) * W + xc];      // always a valid address: no branch around the load
                v[h] = ok ? t : (half_t)0.f;
            }
            in[kp] = half2v{v[0], v[1]};
        }
        for (int cc = sub; cc < nco; cc += CIN_TPP) {
            float a1[8], a2[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) { a1[i] = 0.f; a2[i] = 0.f; }
#pragma unroll
            for (int kp = 0; kp < CIN_MAXKP; ++kp) {
                if (kp < KP1 + KP2) {
                    const half2v* wp = wl + kp * cout + cc * 8;
                    const bool p2 = kp >= KP1;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        if (p2) a2[i] = __builtin_amdgcn_fdot2(in[kp], wp[i], a2[i], false);
                        else a1[i] = __builtin_amdgcn_fdot2(in[kp], wp[i], a1[i], false);
                    }
                }
            }
            const half8 bb = ld_global_h8(bias + cc * 8);
            half8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = (half_t)(a1[i] * isc + a2[i] + (float)bb[i]);
            for (int r = 0; r < rep; ++r)
                *reinterpret_cast<half8*>(out + ((long)(b + r * Bin) * HW + rem) * cout + cc * 8) = o;
        }
    }
}


// ---------------------------------------------------------------- small 3x3 conv (ControlNet condition embedding)
// token-major [B][Hi*Wi][cin] -> token-major [B][Ho*Wo][cout], pad 1, stride 1 or 2, optional SiLU.
// Channel counts below the MFMA kernel's 64-multiple rule (3, 16, 32, 96): runs once per generation (the
// control image is constant over the denoising steps), so a plain fp32-accumulating direct conv is enough.
__global__ void __launch_bounds__(256)
conv3x3_small_kernel(const half_t* __restrict__ x, half_t* __restrict__ out, const half_t* __restrict__ w,
                     const half_t* __restrict__ bias, int B, int Hi, int Wi, int Ho, int Wo, int cin, int cout,
                     int stride, int silu) {
    const int nco = cout / 8;
    const long total = (long)B * Ho * Wo * nco;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long)gridDim.x * 256) {
        const long pix = q / nco;
        const int cc = (int)(q - pix * nco);
        const int b = (int)(pix / (Ho * Wo));
        const int rem = (int)(pix - (long)b * Ho * Wo);
        const int y = rem / Wo, xo = rem - y * Wo;
        float acc[8];
        const half8 bb = ld_global_h8(bias + cc * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = (float)bb[i];
        for (int tap = 0; tap < 9; ++tap) {
            const int yy = y * stride + tap / 3 - 1, xx = xo * stride + tap % 3 - 1;
            if (yy < 0 || yy >= Hi || xx < 0 || xx >= Wi) continue;
            const half_t* xp = x + (((long)b * Hi + yy) * Wi + xx) * cin;
            const half_t* wp = w + ((long)(cc * 8) * 9 + tap) * cin;
            if ((cin & 7) == 0) {
                for (int ci = 0; ci < cin; ci += 8) {
                    const half8 xv = ld_global_h8(xp + ci);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const half8 wv = ld_global_h8(wp + (long)i * 9 * cin + ci);
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[i] += (float)xv[j] * (float)wv[j];
                    }
                }
            } else {
                for (int ci = 0; ci < cin; ++ci) {
                    const float v = (float)xp[ci];
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[i] += v * (float)wp[(long)i * 9 * cin + ci];
                }
            }
        }
        half8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (half_t)(silu ? silu_f(acc[i]) : acc[i]);
        *reinterpret_cast<half8*>(out + pix * cout + cc * 8) = o;
    }
}

// ---------------------------------------------------------------- identity-conditioning stack helpers (once per image)
// exact-erf GELU in place (nn.GELU() of functions.py:395, :499 and attention.py:58)
__global__ void __launch_bounds__(256)
gelu_kernel(half_t* __restrict__ x, long n8) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        half8 h = ld_global_h8(x + i * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = (half_t)gelu_erf_f((float)h[k]);
        *reinterpret_cast<half8*>(x + i * 8) = h;
    }
}

// CLIP quick GELU in place: x * sigmoid(1.702 x) = x / (1 + 2^(-1.702 log2(e) x)) in fp32.  For x below about -52 the
// power overflows to +inf and the quotient is -0; for large x it is 0 and the result is x -- never NaN for a finite input.
// (v_rcp_f32 of +inf is +0; the exp2 / rcp error, 1 ulp each in fp32, is far below the fp16 rounding of the result.)
__global__ void __launch_bounds__(256)
quick_gelu_kernel(half_t* __restrict__ x, long n8) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        half8 h = ld_global_h8(x + i * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float v = (float)h[k];
            h[k] = (half_t)(v * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(v * -2.4554670422754636f)));   // 1.702 log2 e
        }
        *reinterpret_cast<half8*>(x + i * 8) = h;
    }
}

// CLIPTextEmbeddings: token row + position row (fp32 add, one rounding), zero rows on the padded tail of the token axis.
// One thread per 8 channels of one output row.  The caller checks the ids on the host; an id outside [0, V) that gets here
// anyway reads nothing and yields a zero token row.
__global__ void __launch_bounds__(256)
text_embed_kernel(const int* __restrict__ ids, int T, int Tp, const half_t* __restrict__ tok, const half_t* __restrict__ pos,
                  half_t* __restrict__ out, int V, int C8, long items) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        const long row = i / C8;
        const int c = (int)(i - row * C8) * 8;
        const int b = (int)(row / Tp), t = (int)(row - (long)b * Tp);
        half8 o = zero_h8();
        if (t < T) {
            const int id = ids[(long)b * T + t];
            const half8 e = (unsigned)id < (unsigned)V ? ld_global_h8(tok + (long)id * (C8 * 8) + c) : zero_h8();
            const half8 p = ld_global_h8(pos + (long)t * (C8 * 8) + c);
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = (half_t)((float)e[k] + (float)p[k]);
        }
        *reinterpret_cast<half8*>(out + row * (C8 * 8) + c) = o;
    }
}

// PerceiverAttention core (functions.py:439-447): a handful of latent queries attend to [image tokens ; latents].
// One wave per (sample, head, query); head width 64 (dim_head is 64 throughout the reference).  Keys live in two row
// blocks (the torch.cat((x, latents)) of :433 without the copy); a row holds [K | V] (to_kv(...).chunk(2), :434).
constexpr int SA_MAXK = 16;     // 64 lanes x 16 = up to 1024 keys
__global__ void __launch_bounds__(256)
small_attn_kernel(const half_t* __restrict__ q, int ldq, const half_t* __restrict__ kv1, int n1,
                  const half_t* __restrict__ kv2, int n2, int ldkv, half_t* __restrict__ out, int ldo,
                  int Lq, int heads, float scale2, int total) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= total) return;
    const int qi = w % Lq, h = (w / Lq) % heads, b = w / (Lq * heads);
    const int inner = heads * 64, n = n1 + n2;
    float qv[64];
    {
        const half_t* qp = q + (long)(b * Lq + qi) * ldq + h * 64;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const half8 t = ld_global_h8(qp + c * 8);
#pragma unroll
            for (int i = 0; i < 8; ++i) qv[c * 8 + i] = (float)t[i];
        }
    }
    auto row = [&](int j) -> const half_t* {
        return j < n1 ? kv1 + (long)(b * n1 + j) * ldkv : kv2 + (long)(b * n2 + (j - n1)) * ldkv;
    };
    float sc[SA_MAXK];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < SA_MAXK; ++t) {
        const int j = t * 64 + lane;
        float s = -INFINITY;
        if (j < n) {
            const half_t* kp = row(j) + h * 64;
            s = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const half8 kk = ld_global_h8(kp + c * 8);
#pragma unroll
                for (int i = 0; i < 8; ++i) s += qv[c * 8 + i] * (float)kk[i];
            }
            s *= scale2;
        }
        sc[t] = s;
        mx = fmaxf(mx, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < SA_MAXK; ++t) { sc[t] = (t * 64 + lane < n) ? __expf(sc[t] - mx) : 0.f; sum += sc[t]; }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    // out[c = lane] = sum_j p_j V[j][c]; p_j is fetched from its owner lane
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < SA_MAXK; ++t) {
        if (t * 64 >= n) break;
        for (int src = 0; src < 64; ++src) {
            const int j = t * 64 + src;
            if (j >= n) break;
            const float p = __shfl(sc[t], src, 64);
            acc += p * (float)row(j)[inner + h * 64 + lane];
        }
    }
    out[(long)(b * Lq + qi) * ldo + h * 64 + lane] = (half_t)(acc * inv);
}

// ---------------------------------------------------------------- conv_out
// token-major [B][H*W][cin] -> NCHW [B][cout<=4][H][W], 3x3 pad 1 (diffusers UNet2DConditionModel.conv_out behind
// conv_norm_out + SiLU, as called from /root/reference/pipline_StableDiffusion_ConsistentID.py:552-557).
// The activation is read once from HBM; the nine taps of a pixel hit in L2 -- 190 MB of L2 -> L1 traffic at the SD1.5 level-0
// shape, which is what its 27 us are (7 TB/s; unconditional clamped loads made it 38 us: more bytes, not fewer round trips).  Eight lanes
// share a pixel pair (each lane every eighth 16-byte channel chunk), the weights [9][cin / 8][4 outputs] sit in LDS and one
// read of a (tap, chunk) serves both pixels; v_dot2_f32_f16 accumulates in fp32; the eight partial sums meet by DPP-style
// shuffles.  (The first version ran one wave per pixel with the weights re-read from L1 per wave and four 64-lane
// reductions per pixel: 63.6 us at the SD1.5 level-0 shape, 0.33 TB/s.)
constexpr int CO_PPL = 2;        // pixels per lane
constexpr int CO_PPW = 8 * CO_PPL;   // pixels per wave

CID_DEVINL float dot8(half8 a, half8 b, float c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const half2v x = {a[2 * j], a[2 * j + 1]}, y = {b[2 * j], b[2 * j + 1]};
        c = __builtin_amdgcn_fdot2(x, y, c, false);
    }
    return c;
}

__global__ void __launch_bounds__(256)
conv_out_kernel(const half_t* __restrict__ x, half_t* __restrict__ out, const half_t* __restrict__ w,
                const half_t* __restrict__ bias, int B, int H, int W, int cin, int cout) {
    extern __shared__ __attribute__((aligned(16))) char co_smem[];
    half8* wl = reinterpret_cast<half8*>(co_smem);          // [9][nch][4]
    const int nch = cin / 8;
    for (int e = threadIdx.x; e < 9 * nch * 4; e += 256) {
        const int co = e & 3, r = e >> 2;
        const int tap = r / nch, c8 = r - tap * nch;
        wl[e] = co < cout ? ld_global_h8(w + ((long)co * 9 + tap) * cin + c8 * 8) : zero_h8();
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pg = lane >> 3, cl = lane & 7;
    const long npix = (long)B * H * W;
    const int HW = H * W;
    for (long p0 = ((long)blockIdx.x * 4 + wave) * CO_PPW; p0 < npix; p0 += (long)gridDim.x * 4 * CO_PPW) {
        int pb[CO_PPL], py[CO_PPL], px[CO_PPL];
        bool pok[CO_PPL];
#pragma unroll
        for (int j = 0; j < CO_PPL; ++j) {
            const long p = p0 + pg * CO_PPL + j;
            pok[j] = p < npix;
            const long q = pok[j] ? p : 0;
            pb[j] = (int)(q / HW);
            const int rem = (int)(q - (long)pb[j] * HW);
            py[j] = rem / W; px[j] = rem - py[j] * W;
        }
        float acc[CO_PPL][4];
#pragma unroll
        for (int j = 0; j < CO_PPL; ++j)
#pragma unroll
            for (int co = 0; co < 4; ++co) acc[j][co] = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
            const half_t* src[CO_PPL];
            bool ok[CO_PPL];
#pragma unroll
            for (int j = 0; j < CO_PPL; ++j) {
                const int yy = py[j] + dy, xx = px[j] + dx;
                ok[j] = pok[j] && yy >= 0 && yy < H && xx >= 0 && xx < W;
                src[j] = x + (((long)pb[j] * H + (ok[j] ? yy : 0)) * W + (ok[j] ? xx : 0)) * cin;
            }
            for (int c8 = cl; c8 < nch; c8 += 8) {
                half8 xv[CO_PPL];
#pragma unroll
                for (int j = 0; j < CO_PPL; ++j) xv[j] = ok[j] ? ld_global_h8(src[j] + c8 * 8) : zero_h8();
                const half8* wp = wl + (tap * nch + c8) * 4;
#pragma unroll
                for (int co = 0; co < 4; ++co) {
                    const half8 wv = wp[co];
#pragma unroll
                    for (int j = 0; j < CO_PPL; ++j) acc[j][co] = dot8(xv[j], wv, acc[j][co]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < CO_PPL; ++j)
#pragma unroll
            for (int co = 0; co < 4; ++co) {
                float v = acc[j][co];
                v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
                acc[j][co] = v;
            }
        if (cl == 0) {
#pragma unroll
            for (int j = 0; j < CO_PPL; ++j)
                if (pok[j])
                    for (int co = 0; co < cout; ++co)
                        out[(((long)pb[j] * cout + co) * H + py[j]) * W + px[j]] = (half_t)(acc[j][co] + (float)bias[co]);
        }
    }
}

// ---------------------------------------------------------------- timestep path
__global__ void sincos_kernel(const float* __restrict__ v, half_t* __restrict__ out, int rows, int dim) {
    const int half_dim = dim / 2;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= rows * half_dim) return;
    const int r = q / half_dim, i = q - r * half_dim;
    const float f = expf(-9.210340371976184f * (float)i / (float)half_dim);   // ln(10000)
    const float a = v[r] * f;
    out[(long)r * dim + i] = (half_t)cosf(a);
    out[(long)r * dim + half_dim + i] = (half_t)sinf(a);
}

constexpr int LS_NPW = 4;   // outputs per wave
constexpr int LS_MS = 8;    // rows per register slab

__global__ void __launch_bounds__(256)
linear_small_kernel(const half_t* __restrict__ x, int ldx, const half_t* __restrict__ w, const half_t* __restrict__ b,
                    const half_t* __restrict__ add, int ldadd, half_t* __restrict__ out, int ldo,
                    int M, int N, int K, int act_in, int act_out) {
    const int lane = threadIdx.x & 63;
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * LS_NPW;
    if (n0 >= N) return;
    const int nk = K / 8;
    for (int m0 = 0; m0 < M; m0 += LS_MS) {
        float acc[LS_NPW][LS_MS];
#pragma unroll
        for (int j = 0; j < LS_NPW; ++j)
#pragma unroll
            for (int m = 0; m < LS_MS; ++m) acc[j][m] = 0.f;
        for (int kc = lane; kc < nk; kc += 64) {
            float xv[LS_MS][8];
#pragma unroll
            for (int m = 0; m < LS_MS; ++m) {
                if (m0 + m < M) {
                    const half8 hh = ld_global_h8(x + (long)(m0 + m) * ldx + kc * 8);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        float f = (float)hh[i];
                        if (act_in == 1) f = silu_f(f);
                        xv[m][i] = f;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i) xv[m][i] = 0.f;
                }
            }
#pragma unroll
            for (int j = 0; j < LS_NPW; ++j) {
                if (n0 + j < N) {
                    const half8 wv = ld_global_h8(w + (long)(n0 + j) * K + kc * 8);
#pragma unroll
                    for (int m = 0; m < LS_MS; ++m)
#pragma unroll
                        for (int i = 0; i < 8; ++i) acc[j][m] += xv[m][i] * (float)wv[i];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < LS_NPW; ++j)
#pragma unroll
            for (int m = 0; m < LS_MS; ++m) {
                const float r = wave_sum(acc[j][m]);
                if (lane == 0 && n0 + j < N && m0 + m < M) {
                    float v = r + (b ? (float)b[n0 + j] : 0.f);
                    if (add) v += (float)add[(long)(m0 + m) * ldadd + n0 + j];
                    if (act_out == 1) v = silu_f(v);
                    out[(long)(m0 + m) * ldo + n0 + j] = (half_t)v;
                }
            }
    }
}

// ---------------------------------------------------------------- loop glue
// SCALED (the *_scaled_f16 entries, guidance_rescale): e is multiplied by escale[sample], the factor cfg_rescale_kernel wrote;
// per_sample % 8 == 0 there, so an 8-half item lies inside one sample.  The trailing two arguments are not read without it:
// the unscaled instantiation is the kernel as it was.
// PAG (the cid_*pag*_step_f16 entries, perturbed-attention guidance): eps holds one more block of rows, the perturbed
// prediction p, behind the conditional one, and e += s (c - p) with s = pag[0], a DEVICE value (a step-table column).  The
// branch on s != 0 is uniform over the grid: at s == 0 the perturbed rows are never addressed (they may hold NaN, and
// 0 * NaN is NaN) and e is the sibling's expression.  pag is not read without PAG: those instantiations are the kernels as they were.
// SAG (the cid_*sag*_step_f16 entries, self-attention guidance): the prediction e_d of the degraded latents comes in a buffer of
// its own, eps_d [B][per_sample], and e += s (guide - e_d), the guide rows being the unconditional ones with CFG and the
// conditional ones without; s is a launch argument.  At s == 0 eps_d is never addressed.  Neither is read without SAG.
template <bool SCALED, bool PAG = false, bool SAG = false>
__global__ void __launch_bounds__(256)
cfg_ddim_kernel(const half_t* __restrict__ eps, half_t* __restrict__ lat, const float* __restrict__ coef,
                float g, const half_t* __restrict__ mask, const half_t* __restrict__ init,
                const half_t* __restrict__ noise, long n /* B * per_sample, multiple of 8 */,
                const float* __restrict__ escale, int sample_items /* 8-half items per sample */,
                const float* __restrict__ pag /* PAG only: one DEVICE value */,
                const half_t* __restrict__ eps_d /* SAG only */, float sag /* SAG only */) {
    float s = 0.f;
    if constexpr (PAG) s = pag[0];
    const bool perturbed = PAG && s != 0.f;
    const bool degraded = SAG && sag != 0.f;
    const float cx = coef[0], ce = coef[1];
    const float ci = mask ? coef[2] : 0.f, cn = mask ? coef[3] : 0.f;
    for (long q = ((long)blockIdx.x * 256 + threadIdx.x) * 8; q < n; q += (long)gridDim.x * 256 * 8) {
        const half8 eu = ld_global_h8(eps + q), ec = ld_global_h8(eps + n + q), xl = ld_global_h8(lat + q);
        half8 ep;
        if constexpr (PAG) { if (perturbed) ep = ld_global_h8(eps + 2 * n + q); }
        half8 ed;
        if constexpr (SAG) { if (degraded) ed = ld_global_h8(eps_d + q); }
        half8 mk, in0, nz;
        if (mask) { mk = ld_global_h8(mask + q); in0 = ld_global_h8(init + q); nz = ld_global_h8(noise + q); }
        float es = 1.f;
        if constexpr (SCALED) es = escale[(unsigned)(q >> 3) / (unsigned)sample_items];   // fewer than 2^31 items: the entry checks
        half8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float u = (float)eu[i], c = (float)ec[i];
            float e = u + g * (c - u);
            if constexpr (PAG) { if (perturbed) e += s * (c - (float)ep[i]); }
            if constexpr (SAG) { if (degraded) e += sag * (u - (float)ed[i]); }
            if constexpr (SCALED) e *= es;
            float v = cx * (float)xl[i] + ce * e;
            if (mask) {
                const float m = (float)mk[i];
                v = (1.f - m) * (ci * (float)in0[i] + cn * (float)nz[i]) + m * v;
            }
            o[i] = (half_t)v;
        }
        *reinterpret_cast<half8*>(lat + q) = o;
    }
}

// CFG + one step of a linear multistep sampler (PNDM, DPM-Solver++ 2M, DDIM with eta > 0): cid.h, "multistep row".  Every
// per-step value -- coefficients, the ring slot that receives m, the save / restore flags, the noise row -- is read from the
// 16-word device row, so the launch is the same for every step.  A ring slot, `saved` and `z` are loaded only where the
// row gives them a non-zero coefficient (wave-uniform branches): an unwritten buffer may hold NaN, and 0 * NaN is NaN.
// CFG = false (cid_multistep_step_f16, the single pass): eps holds ONE model output per sample, [B][per_sample], and e is that
// value -- no second half is loaded (eps + n is past the end of the buffer) and g is not read.
// PAG as cfg_ddim_kernel's: the perturbed rows follow the conditional ones -- [3B] rows with CFG, [2B] without, where
// e = c + s (c - p).  SAG as cfg_ddim_kernel's: e += s (eps row 0 - e_d), the unconditional rows with CFG, the only rows without.
template <bool SCALED, bool CFG = true, bool PAG = false, bool SAG = false>      // SCALED, PAG, SAG as cfg_ddim_kernel's
__global__ void __launch_bounds__(256)
cfg_multistep_kernel(const half_t* __restrict__ eps, half_t* __restrict__ lat, float* hist, half_t* saved,
                     const half_t* __restrict__ z, int z_rows, const float* __restrict__ row, float g,
                     const half_t* __restrict__ mask, const half_t* __restrict__ init, const half_t* __restrict__ noise,
                     long n /* B * per_sample, multiple of 8 */, const float* __restrict__ escale, int sample_items /* 8-half items per sample */,
                     const float* __restrict__ pag /* PAG only: one DEVICE value */,
                     const half_t* __restrict__ eps_d /* SAG only */, float sag /* SAG only */) {
    float s = 0.f;
    if constexpr (PAG) s = pag[0];
    const bool perturbed = PAG && s != 0.f;
    const bool degraded = SAG && sag != 0.f;
    const float a = row[0], b = row[1], cx = row[2], cm = row[3], cz = z ? row[11] : 0.f;
    const float ch[4] = {row[4], row[5], row[6], row[7]};
    const float ci = mask ? row[9] : 0.f, cn = mask ? row[10] : 0.f;
    const int* irow = reinterpret_cast<const int*>(row);
    const int w = irow[12], flags = irow[13];
    const int zr = irow[14] < 0 ? 0 : (irow[14] > z_rows - 1 ? z_rows - 1 : irow[14]);   // a bad row cannot index past z
    const bool put = w >= 0 && w < 4, save = flags & 1, restore = flags & 2;
    for (long q = ((long)blockIdx.x * 256 + threadIdx.x) * 8; q < n; q += (long)gridDim.x * 256 * 8) {
        const half8 eu = ld_global_h8(eps + q);
        half8 ec;
        if constexpr (CFG) ec = ld_global_h8(eps + n + q);
        half8 ep;
        if constexpr (PAG) { if (perturbed) ep = ld_global_h8(eps + (CFG ? 2 : 1) * n + q); }
        half8 ed;
        if constexpr (SAG) { if (degraded) ed = ld_global_h8(eps_d + q); }
        const half8 xl = ld_global_h8(lat + q);
        const half8 src = restore ? ld_global_h8(saved + q) : xl;
        float es = 1.f;
        if constexpr (SCALED) es = escale[(unsigned)(q >> 3) / (unsigned)sample_items];   // fewer than 2^31 items: the entry checks
        float m[8], v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float u = (float)eu[i];
            float e = u;
            if constexpr (CFG) { const float c = (float)ec[i]; e = u + g * (c - u); }
            if constexpr (PAG) { if (perturbed) e += s * ((CFG ? (float)ec[i] : u) - (float)ep[i]); }
            if constexpr (SAG) { if (degraded) e += sag * (u - (float)ed[i]); }
            if constexpr (SCALED) e *= es;
            if constexpr (CFG) m[i] = a * (float)xl[i] + b * e;
            else m[i] = __builtin_fmaf(a, (float)xl[i], b * e);     // the contraction the CFG instantiations compile to: the same bits on equal halves
            v[i] = cx * (float)src[i] + cm * m[i];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (ch[s] != 0.f) {
                const float* hp = hist + (long)s * n + q;
                const f32x4 h0 = *reinterpret_cast<const f32x4*>(hp), h1 = *reinterpret_cast<const f32x4*>(hp + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) { v[i] += ch[s] * h0[i]; v[4 + i] += ch[s] * h1[i]; }
            }
        if (cz != 0.f) {
            const half8 zv = ld_global_h8(z + (long)zr * n + q);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] += cz * (float)zv[i];
        }
        if (put) {                                   // after the reads: the row may still weigh the slot's previous content
            float* hp = hist + (long)w * n + q;
            const f32x4 m0 = {m[0], m[1], m[2], m[3]}, m1 = {m[4], m[5], m[6], m[7]};
            *reinterpret_cast<f32x4*>(hp) = m0;
            *reinterpret_cast<f32x4*>(hp + 4) = m1;
        }
        if (save) *reinterpret_cast<half8*>(saved + q) = xl;
        half8 mk, in0, nz;
        if (mask) { mk = ld_global_h8(mask + q); in0 = ld_global_h8(init + q); nz = ld_global_h8(noise + q); }
        half8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float r = v[i];
            if (mask) {
                const float k = (float)mk[i];
                r = (1.f - k) * (ci * (float)in0[i] + cn * (float)nz[i]) + k * r;
            }
            o[i] = (half_t)r;
        }
        *reinterpret_cast<half8*>(lat + q) = o;
    }
}

// guidance_rescale's factor (cid.h, cid_cfg_rescale_f16): one 1024-thread workgroup per sample walks the sample's conditional
// half c and the guided e = u + g (c - u) once and keeps, for both, a running (count, mean, M2 = sum of squared deviations).
// An 8-half item enters as its own (8, mean, M2) -- the mean taken relative to the item's first value, so that a constant
// item has M2 == 0 exactly -- and every merge, thread-local, across the lanes of a wave and across the 16 waves through LDS, is
// Chan's pairwise update in its delta form: a zero delta leaves the mean untouched, so a constant sample ends at M2 == 0.
// No sum / sum of squares (it cancels at a non-zero mean), no atomics, a fixed merge order: the same input gives the same bits.
struct Moments { float n, mc, sc, me, se; };     // count, mean and M2 of c, mean and M2 of e

CID_DEVINL void moments_merge(Moments& a, const Moments& b) {
    const float n = a.n + b.n;
    if (n > 0.f) {                               // both empty (a thread past a short sample's end): nothing to merge
        const float fb = b.n / n, w = a.n * fb;
        const float dc = b.mc - a.mc, de = b.me - a.me;
        a.mc += dc * fb;  a.sc += b.sc + dc * dc * w;
        a.me += de * fb;  a.se += b.se + de * de * w;
        a.n = n;
    }
}
CID_DEVINL Moments moments_shfl_xor(const Moments& a, int o) {
    Moments b;
    b.n = __shfl_xor(a.n, o, 64);   b.mc = __shfl_xor(a.mc, o, 64); b.sc = __shfl_xor(a.sc, o, 64);
    b.me = __shfl_xor(a.me, o, 64); b.se = __shfl_xor(a.se, o, 64);
    return b;
}

__global__ void __launch_bounds__(1024)
cfg_rescale_kernel(const half_t* __restrict__ eps, float g, float phi, float* __restrict__ escale, long n /* B * per_sample */,
                   int per_sample /* multiple of 8 */) {
    __shared__ Moments part[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const half_t* pu = eps + (long)b * per_sample;
    const half_t* pc = pu + n;
    Moments acc = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int q = tid * 8; q < per_sample; q += 1024 * 8) {
        const half8 eu = ld_global_h8(pu + q), ec = ld_global_h8(pc + q);
        float c[8], e[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float u = (float)eu[i];
            c[i] = (float)ec[i];
            e[i] = u + g * (c[i] - u);
        }
        float dc = 0.f, de = 0.f;
#pragma unroll
        for (int i = 1; i < 8; ++i) { dc += c[i] - c[0]; de += e[i] - e[0]; }
        Moments it = {8.f, c[0] + dc * 0.125f, 0.f, e[0] + de * 0.125f, 0.f};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float rc = c[i] - it.mc, re = e[i] - it.me;
            it.sc += rc * rc;
            it.se += re * re;
        }
        moments_merge(acc, it);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) moments_merge(acc, moments_shfl_xor(acc, o));
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (wave == 0) {
        Moments t = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (lane < 16) t = part[lane];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) moments_merge(t, moments_shfl_xor(t, o));
        // std(c) / std(e): the two share N - 1.  std(e) == 0 (a constant prediction) -> 1.0, where diffusers divides by zero
        if (lane == 0) escale[b] = t.se == 0.f ? 1.f : 1.f - phi + phi * sqrtf(t.sc / t.se);
    }
}

__global__ void __launch_bounds__(256)
add_inplace_kernel(half_t* __restrict__ y, const half_t* __restrict__ a, long n, long na) {
    for (long q = ((long)blockIdx.x * 256 + threadIdx.x) * 8; q < n; q += (long)gridDim.x * 256 * 8) {
        half8 yv = ld_global_h8(y + q);
        const half8 av = ld_global_h8(a + (q % na));
#pragma unroll
        for (int i = 0; i < 8; ++i) yv[i] = (half_t)((float)yv[i] + (float)av[i]);
        *reinterpret_cast<half8*>(y + q) = yv;
    }
}

// Residuals of several ControlNets onto up to 16 tensors in one launch (cid_residual_accum_f16, cid.h).  The segments travel
// by value; `first` holds the prefix sums of their 256-chunk tiles (a chunk = 8 halves = 16 bytes per lane), so a tile lies
// in ONE segment and a workgroup finds it with a wave-uniform walk over at most 16 kernel-argument words.  The grid is capped:
// a workgroup strides over the tiles.  The scales come from device memory (the launch is the same for every step of a captured
// loop); a net whose scale is exactly 0 is skipped by a wave-uniform branch BEFORE its residual is loaded -- a net outside
// its guidance window did not run, its buffers may hold anything, and 0 * NaN is NaN.
constexpr int RA_MAX_SEGS = 16;
constexpr int RA_TILE = 256;        // chunks per tile = lanes per workgroup
struct AccumSegs {
    cid_accum_seg s[RA_MAX_SEGS];
    long first[RA_MAX_SEGS + 1];    // tiles before segment j; first[n] = all tiles
    int n, n_nets;
};
__global__ void __launch_bounds__(256)
residual_accum_kernel(AccumSegs segs, const float* __restrict__ scales) {
    float sc[CID_MAX_CONTROLNETS];
#pragma unroll
    for (int k = 0; k < CID_MAX_CONTROLNETS; ++k) sc[k] = k < segs.n_nets ? scales[k] : 0.f;
    const long tiles = segs.first[segs.n];
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        int j = 0;
        while (j + 1 < segs.n && tile >= segs.first[j + 1]) ++j;
        const long n = segs.s[j].n, nr = segs.s[j].nr;
        const long q = ((tile - segs.first[j]) * RA_TILE + threadIdx.x) * 8;
        if (q >= n) continue;                                   // the tail of a segment's last tile
        const long qr = nr == n ? q : q % nr;                   // B-row residual under the 2B-row batch (CN :418-425)
        half_t* yp = reinterpret_cast<half_t*>(segs.s[j].y) + q;
        const half8 yv = ld_global_h8(yp);
        float acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
        for (int k = 0; k < CID_MAX_CONTROLNETS; ++k)
            if (sc[k] != 0.f) {
                const half8 rv = ld_global_h8(reinterpret_cast<const half_t*>(segs.s[j].r[k]) + qr);
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] += sc[k] * (float)rv[i];
            }
        half8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (half_t)((float)yv[i] + acc[i]);
        *reinterpret_cast<half8*>(yp) = o;
    }
}

// Upsample2D weight fold (cid_upconv_fold_f16): one thread per element of w4[parity][n][tap4][c].  Along an axis, parity p and
// folded tap r take the source taps [lo, hi]: (p, r) = (0, 0): {0}, (0, 1): {1, 2}, (1, 0): {0, 1}, (1, 1): {2}.
__global__ void __launch_bounds__(256)
upconv_fold_kernel(const half_t* __restrict__ w, half_t* __restrict__ w4, int N, int C) {
    const long total = 16L * N * C;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c = (int)(e % C);
        long r = e / C;
        const int tap4 = (int)(r & 3);
        r >>= 2;
        const int n = (int)(r % N), par = (int)(r / N);
        const int py = par >> 1, px = par & 1, ry = tap4 >> 1, rx = tap4 & 1;
        const int ylo = py + ry == 0 ? 0 : (py + ry == 2 ? 2 : (py ? 0 : 1)), yhi = py + ry == 0 ? 0 : (py + ry == 2 ? 2 : (py ? 1 : 2));
        const int xlo = px + rx == 0 ? 0 : (px + rx == 2 ? 2 : (px ? 0 : 1)), xhi = px + rx == 0 ? 0 : (px + rx == 2 ? 2 : (px ? 1 : 2));
        const half_t* src = w + (long)n * 9 * C + c;
        float acc = 0.f;
        bool first = true;
        for (int ty = ylo; ty <= yhi; ++ty)                 // fixed order: ty-major, then tx
            for (int tx = xlo; tx <= xhi; ++tx) {
                const float v = (float)src[(long)(ty * 3 + tx) * C];
                acc = first ? v : __fadd_rn(acc, v);
                first = false;
            }
        w4[e] = (half_t)acc;
    }
}

inline int grid_for(long items, int per_block, int cap) {
    long g = (items + per_block - 1) / per_block;
    return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" int cid_conv_in_f16(const cid_half* sample, cid_half* out, const cid_half* w, const cid_half* bias,
                               int32_t B, int32_t Bin, int32_t cin, int32_t H, int32_t W, int32_t cout,
                               const float* in_scale, cid_stream_t stream) {
    CID_CHECK_ARG(sample && out && w && bias, "cid_conv_in_f16: null pointer");
    CID_CHECK_ARG(B > 0 && Bin > 0 && cin > 0 && cin <= 9 && cout % 8 == 0 && cout <= CIN_MAXCO && H > 0 && W > 0,
                  "cid_conv_in_f16: bad shape (cin <= 9, cout <= 320)");
    CID_CHECK_ARG(B % Bin == 0, "cid_conv_in_f16: B must be a multiple of Bin (batch row b reads sample b %% Bin)");
    const long items = (long)Bin * H * W;                   // pixels computed (rows that share a sample are stored B / Bin times)
    const dim3 grid(grid_for(items, 256 / CIN_TPP, 512));
#define CID_CONV_IN(A, Bc) hipLaunchKernelGGL((conv_in_kernel<A, Bc>), grid, dim3(256), 0, (hipStream_t)stream, (const half_t*)sample, \
                       (const half_t*)sample, (half_t*)out, (const half_t*)w, (const half_t*)bias, B, Bin, cin, 0, H, W, cout, in_scale)
    if (cin == 4) CID_CONV_IN(4, 0);
    else if (cin == 9) CID_CONV_IN(9, 0);
    else CID_CONV_IN(0, 0);
#undef CID_CONV_IN
    CID_CHECK_LAUNCH("cid_conv_in_f16");
    return 0;
}

extern "C" int cid_conv_in_cat_f16(const cid_half* sample, int32_t cin1, const cid_half* extra, int32_t cin2, cid_half* out,
                                   const cid_half* w, const cid_half* bias, int32_t B, int32_t Bin, int32_t H, int32_t W,
                                   int32_t cout, const float* in_scale, cid_stream_t stream) {
    CID_CHECK_ARG(sample && extra && out && w && bias, "cid_conv_in_cat_f16: null pointer");
    CID_CHECK_ARG(B > 0 && Bin > 0 && cin1 > 0 && cin2 > 0 && cin1 + cin2 <= 9 && cout % 8 == 0 && cout <= CIN_MAXCO && H > 0 &&
                  W > 0, "cid_conv_in_cat_f16: bad shape (cin1 + cin2 <= 9, cout <= 320)");
    CID_CHECK_ARG(B % Bin == 0, "cid_conv_in_cat_f16: B must be a multiple of Bin (batch row b reads sample b %% Bin)");
    const long items = (long)Bin * H * W;
    const dim3 grid(grid_for(items, 256 / CIN_TPP, 512));
    if (cin1 == 4 && cin2 == 5)
        hipLaunchKernelGGL((conv_in_kernel<4, 5>), grid, dim3(256), 0, (hipStream_t)stream, (const half_t*)sample, (const half_t*)extra,
                           (half_t*)out, (const half_t*)w, (const half_t*)bias, B, Bin, cin1, cin2, H, W, cout, in_scale);
    else
        hipLaunchKernelGGL((conv_in_kernel<0, 0>), grid, dim3(256), 0, (hipStream_t)stream, (const half_t*)sample, (const half_t*)extra,
                           (half_t*)out, (const half_t*)w, (const half_t*)bias, B, Bin, cin1, cin2, H, W, cout, in_scale);
    CID_CHECK_LAUNCH("cid_conv_in_cat_f16");
    return 0;
}


extern "C" int cid_conv3x3_small_f16(const cid_half* x, cid_half* out, const cid_half* w, const cid_half* bias,
                                     int32_t B, int32_t Hi, int32_t Wi, int32_t cin, int32_t cout, int32_t stride,
                                     int32_t silu, cid_stream_t stream) {
    CID_CHECK_ARG(x && out && w && bias, "cid_conv3x3_small_f16: null pointer");
    CID_CHECK_ARG(B > 0 && Hi > 0 && Wi > 0 && cin > 0 && cout > 0 && cout % 8 == 0 && (stride == 1 || stride == 2),
                  "cid_conv3x3_small_f16: bad shape (cout %% 8, stride 1 or 2)");
    const int Ho = (Hi - 1) / stride + 1, Wo = (Wi - 1) / stride + 1;     // kernel 3, pad 1
    const long items = (long)B * Ho * Wo * (cout / 8);
    hipLaunchKernelGGL(conv3x3_small_kernel, dim3(grid_for(items, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)x, (half_t*)out, (const half_t*)w, (const half_t*)bias, B, Hi, Wi, Ho, Wo, cin, cout,
                       stride, silu);
    CID_CHECK_LAUNCH("cid_conv3x3_small_f16");
    return 0;
}


extern "C" int cid_upconv_fold_f16(const cid_half* w, cid_half* w4, int32_t N, int32_t C, cid_stream_t stream) {
    CID_CHECK_ARG(w && w4 && N > 0 && C > 0 && 16L * N * C < 0x7fffffffL, "cid_upconv_fold_f16: bad arguments (N = %d, C = %d)", N, C);
    hipLaunchKernelGGL(upconv_fold_kernel, dim3(grid_for(16L * N * C, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)w, (half_t*)w4, N, C);
    CID_CHECK_LAUNCH("cid_upconv_fold_f16");
    return 0;
}

extern "C" int cid_gelu_f16(cid_half* x, int64_t n, cid_stream_t stream) {
    CID_CHECK_ARG(x && n > 0 && n % 8 == 0, "cid_gelu_f16: n must be a positive multiple of 8");
    hipLaunchKernelGGL(gelu_kernel, dim3(grid_for(n / 8, 256, 4096)), dim3(256), 0, (hipStream_t)stream, (half_t*)x, (long)(n / 8));
    CID_CHECK_LAUNCH("cid_gelu_f16");
    return 0;
}

extern "C" int cid_quick_gelu_f16(cid_half* x, int64_t n, cid_stream_t stream) {
    CID_CHECK_ARG(x, "cid_quick_gelu_f16: null pointer");
    CID_CHECK_ARG(n > 0 && n % 8 == 0, "cid_quick_gelu_f16: n must be a positive multiple of 8 (got %lld)", (long long)n);
    hipLaunchKernelGGL(quick_gelu_kernel, dim3(grid_for(n / 8, 256, 4096)), dim3(256), 0, (hipStream_t)stream, (half_t*)x,
                       (long)(n / 8));
    CID_CHECK_LAUNCH("cid_quick_gelu_f16");
    return 0;
}

extern "C" int cid_text_embed_f16(const int32_t* ids, int32_t B, int32_t T, int32_t Tp, const cid_half* tok,
                                  const cid_half* pos, cid_half* out, int32_t V, int32_t C, cid_stream_t stream) {
    CID_CHECK_ARG(ids && tok && pos && out, "cid_text_embed_f16: null pointer");
    CID_CHECK_ARG(B > 0 && T > 0 && Tp >= T && V > 0 && C > 0 && C % 8 == 0,
                  "cid_text_embed_f16: bad shape (B %d, T %d, Tp %d, V %d, C %d; Tp >= T, C %% 8 == 0)", B, T, Tp, V, C);
    const long items = (long)B * Tp * (C / 8);
    hipLaunchKernelGGL(text_embed_kernel, dim3(grid_for(items, 256, 4096)), dim3(256), 0, (hipStream_t)stream, (const int*)ids,
                       T, Tp, (const half_t*)tok, (const half_t*)pos, (half_t*)out, V, C / 8, items);
    CID_CHECK_LAUNCH("cid_text_embed_f16");
    return 0;
}

extern "C" int cid_small_attn_f16(const cid_half* q, int32_t ldq, const cid_half* kv1, int32_t n1, const cid_half* kv2,
                                  int32_t n2, int32_t ldkv, cid_half* out, int32_t ldo, int32_t B, int32_t Lq,
                                  int32_t heads, int32_t dim_head, float scale2, cid_stream_t stream) {
    CID_CHECK_ARG(q && kv1 && out && (n2 == 0 || kv2), "cid_small_attn_f16: null pointer");
    CID_CHECK_ARG(dim_head == 64, "cid_small_attn_f16: head width must be 64 (got %d)", dim_head);
    CID_CHECK_ARG(B > 0 && Lq > 0 && heads > 0 && n1 > 0 && n2 >= 0 && n1 + n2 <= 64 * SA_MAXK && ldq % 8 == 0 && ldkv % 8 == 0,
                  "cid_small_attn_f16: bad shape (at most %d keys)", 64 * SA_MAXK);
    // a q / out row holds `heads` heads of 64, a key row [K | V]: the kernel reads V at row + heads * 64
    CID_CHECK_ARG(ldq >= heads * 64 && ldkv >= 2 * heads * 64 && ldo >= heads * 64,
                  "cid_small_attn_f16: bad pitch ldq=%d ldkv=%d ldo=%d (ldq, ldo >= heads * 64 = %d, ldkv >= twice that)", ldq, ldkv, ldo,
                  heads * 64);
    const int total = B * heads * Lq;
    hipLaunchKernelGGL(small_attn_kernel, dim3((total + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const half_t*)q, ldq,
                       (const half_t*)kv1, n1, (const half_t*)kv2, n2, ldkv, (half_t*)out, ldo, Lq, heads, scale2, total);
    CID_CHECK_LAUNCH("cid_small_attn_f16");
    return 0;
}

extern "C" int cid_conv_out_f16(const cid_half* x, cid_half* out, const cid_half* w, const cid_half* bias,
                                int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout, cid_stream_t stream) {
    CID_CHECK_ARG(x && out && w && bias, "cid_conv_out_f16: null pointer");
    CID_CHECK_ARG(B > 0 && H > 0 && W > 0 && cin % 8 == 0 && cout > 0 && cout <= 4, "cid_conv_out_f16: bad shape (cout <= 4)");
    const long pix = (long)B * H * W;
    const int smem = 9 * (cin / 8) * 4 * 16;                 // weights [9][cin / 8][4] x 16 B
    CID_CHECK_ARG(smem <= 64 * 1024, "cid_conv_out_f16: cin = %d is too wide (the weights are held in 64 KB of LDS)", cin);
    hipLaunchKernelGGL(conv_out_kernel, dim3(grid_for(pix, 4 * CO_PPW, 2048)), dim3(256), smem, (hipStream_t)stream,
                       (const half_t*)x, (half_t*)out, (const half_t*)w, (const half_t*)bias, B, H, W, cin, cout);
    CID_CHECK_LAUNCH("cid_conv_out_f16");
    return 0;
}

extern "C" int cid_sincos_embed_f16(const float* v, cid_half* out, int32_t rows, int32_t dim, cid_stream_t stream) {
    CID_CHECK_ARG(v && out && rows > 0 && dim > 0 && dim % 2 == 0, "cid_sincos_embed_f16: bad arguments");
    const int n = rows * (dim / 2);
    hipLaunchKernelGGL(sincos_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, v, (half_t*)out, rows, dim);
    CID_CHECK_LAUNCH("cid_sincos_embed_f16");
    return 0;
}

extern "C" int cid_linear_small_f16(const cid_half* x, int32_t ldx, const cid_half* w, const cid_half* b,
                                    const cid_half* add, int32_t ldadd, cid_half* out, int32_t ldo,
                                    int32_t M, int32_t N, int32_t K, int32_t act_in, int32_t act_out,
                                    cid_stream_t stream) {
    CID_CHECK_ARG(x && w && out, "cid_linear_small_f16: null pointer");
    CID_CHECK_ARG(M > 0 && M <= 64 && N > 0 && K > 0 && K % 8 == 0 && ldx % 8 == 0, "cid_linear_small_f16: bad shape (M <= 64, K %% 8)");
    CID_CHECK_ARG(ldx >= K && ldo >= N && (ldadd == 0 || ldadd >= N),
                  "cid_linear_small_f16: bad pitch ldx=%d ldo=%d ldadd=%d (ldx >= K = %d, ldo >= N = %d, ldadd 0 or >= N)", ldx, ldo, ldadd, K, N);
    const int waves = (N + LS_NPW - 1) / LS_NPW;
    hipLaunchKernelGGL(linear_small_kernel, dim3((waves + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)x, ldx, (const half_t*)w, (const half_t*)b, (const half_t*)add, ldadd,
                       (half_t*)out, ldo, M, N, K, act_in, act_out);
    CID_CHECK_LAUNCH("cid_linear_small_f16");
    return 0;
}

extern "C" int cid_cfg_ddim_step_f16(const cid_half* eps, cid_half* latents, const float* coef, float guidance,
                                     const cid_half* mask, const cid_half* init, const cid_half* noise,
                                     int32_t B, int32_t per_sample, cid_stream_t stream) {
    CID_CHECK_ARG(eps && latents && coef, "cid_cfg_ddim_step_f16: null pointer");
    CID_CHECK_ARG((mask == nullptr) == (init == nullptr) && (mask == nullptr) == (noise == nullptr),
                  "cid_cfg_ddim_step_f16: mask/init/noise must come together");
    const long n = (long)B * per_sample;
    CID_CHECK_ARG(B > 0 && per_sample > 0 && n % 8 == 0, "cid_cfg_ddim_step_f16: B * per_sample must be a multiple of 8");
    hipLaunchKernelGGL(cfg_ddim_kernel<false>, dim3(grid_for(n / 8, 256, 1024)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)eps, (half_t*)latents, coef, guidance, (const half_t*)mask, (const half_t*)init,
                       (const half_t*)noise, n, (const float*)nullptr, 0, (const float*)nullptr, (const half_t*)nullptr, 0.f);
    CID_CHECK_LAUNCH("cid_cfg_ddim_step_f16");
    return 0;
}

extern "C" int cid_cfg_ddim_step_scaled_f16(const cid_half* eps, cid_half* latents, const float* coef, float guidance,
                                            const cid_half* mask, const cid_half* init, const cid_half* noise,
                                            int32_t B, int32_t per_sample, const float* escale, cid_stream_t stream) {
    CID_CHECK_ARG(eps && latents && coef && escale, "cid_cfg_ddim_step_scaled_f16: null pointer");
    CID_CHECK_ARG((mask == nullptr) == (init == nullptr) && (mask == nullptr) == (noise == nullptr),
                  "cid_cfg_ddim_step_scaled_f16: mask/init/noise must come together");
    CID_CHECK_ARG(B > 0 && per_sample > 0 && per_sample % 8 == 0,
                  "cid_cfg_ddim_step_scaled_f16: per_sample must be a multiple of 8 (an 8-half item lies inside one sample)");
    const long n = (long)B * per_sample;
    CID_CHECK_ARG(n / 8 <= 0x7fffffffL, "cid_cfg_ddim_step_scaled_f16: B * per_sample must be below 2^34");
    hipLaunchKernelGGL(cfg_ddim_kernel<true>, dim3(grid_for(n / 8, 256, 1024)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)eps, (half_t*)latents, coef, guidance, (const half_t*)mask, (const half_t*)init,
                       (const half_t*)noise, n, escale, (int)(per_sample / 8), (const float*)nullptr, (const half_t*)nullptr, 0.f);
    CID_CHECK_LAUNCH("cid_cfg_ddim_step_scaled_f16");
    return 0;
}

extern "C" int cid_cfg_rescale_f16(const cid_half* eps, float guidance, float rescale, float* escale, int32_t B,
                                   int32_t per_sample, cid_stream_t stream) {
    CID_CHECK_ARG(eps && escale, "cid_cfg_rescale_f16: null pointer");
    CID_CHECK_ARG(B > 0, "cid_cfg_rescale_f16: B must be positive");
    CID_CHECK_ARG(per_sample > 0 && per_sample % 8 == 0, "cid_cfg_rescale_f16: per_sample must be a positive multiple of 8");
    // the element counts are kept in fp32 (exact up to 2^24) and a sample is indexed with an int
    CID_CHECK_ARG(per_sample <= (1 << 24), "cid_cfg_rescale_f16: per_sample must be at most 2^24 (16777216)");
    CID_CHECK_ARG((uintptr_t)eps % 16 == 0 && (uintptr_t)escale % 4 == 0, "cid_cfg_rescale_f16: eps must be 16-byte aligned");
    CID_CHECK_ARG(rescale >= 0.f && rescale <= 3.402823466e+38f, "cid_cfg_rescale_f16: rescale must be finite and not negative");
    hipLaunchKernelGGL(cfg_rescale_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, (const half_t*)eps, guidance, rescale,
                       escale, (long)B * per_sample, (int)per_sample);
    CID_CHECK_LAUNCH("cid_cfg_rescale_f16");
    return 0;
}

extern "C" int cid_cfg_multistep_step_f16(const cid_half* eps, cid_half* latents, float* hist, cid_half* saved,
                                          const cid_half* z, int32_t z_rows, const void* row, float guidance,
                                          const cid_half* mask, const cid_half* init, const cid_half* noise,
                                          int32_t B, int32_t per_sample, cid_stream_t stream) {
    CID_CHECK_ARG(eps && latents && hist && saved && row, "cid_cfg_multistep_step_f16: null pointer");
    CID_CHECK_ARG((z == nullptr) == (z_rows == 0) && z_rows >= 0, "cid_cfg_multistep_step_f16: z and z_rows must come together");
    CID_CHECK_ARG((mask == nullptr) == (init == nullptr) && (mask == nullptr) == (noise == nullptr),
                  "cid_cfg_multistep_step_f16: mask/init/noise must come together");
    const long n = (long)B * per_sample;
    CID_CHECK_ARG(B > 0 && per_sample > 0 && n % 8 == 0, "cid_cfg_multistep_step_f16: B * per_sample must be a multiple of 8");
    hipLaunchKernelGGL(cfg_multistep_kernel<false>, dim3(grid_for(n / 8, 256, 1024)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)eps, (half_t*)latents, hist, (half_t*)saved, (const half_t*)z, (int)z_rows,
                       (const float*)row, guidance, (const half_t*)mask, (const half_t*)init, (const half_t*)noise, n,
                       (const float*)nullptr, 0, (const float*)nullptr, (const half_t*)nullptr, 0.f);
    CID_CHECK_LAUNCH("cid_cfg_multistep_step_f16");
    return 0;
}

extern "C" int cid_multistep_step_f16(const cid_half* eps, cid_half* latents, float* hist, cid_half* saved,
                                      const cid_half* z, int32_t z_rows, const void* row,
                                      const cid_half* mask, const cid_half* init, const cid_half* noise,
                                      int32_t B, int32_t per_sample, cid_stream_t stream) {
    CID_CHECK_ARG(eps && latents && hist && saved && row, "cid_multistep_step_f16: null pointer");
    CID_CHECK_ARG((z == nullptr) == (z_rows == 0) && z_rows >= 0, "cid_multistep_step_f16: z and z_rows must come together");
    CID_CHECK_ARG((mask == nullptr) == (init == nullptr) && (mask == nullptr) == (noise == nullptr),
                  "cid_multistep_step_f16: mask/init/noise must come together");
    const long n = (long)B * per_sample;
    CID_CHECK_ARG(B > 0 && per_sample > 0 && n % 8 == 0, "cid_multistep_step_f16: B * per_sample must be a multiple of 8");
    for (const void* p : {(const void*)eps, (const void*)latents, (const void*)hist, (const void*)saved, (const void*)z,
                          (const void*)row, (const void*)mask, (const void*)init, (const void*)noise})
        CID_CHECK_ARG((uintptr_t)p % 16 == 0, "cid_multistep_step_f16: every buffer must be 16-byte aligned");
    hipLaunchKernelGGL((cfg_multistep_kernel<false, false>), dim3(grid_for(n / 8, 256, 1024)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)eps, (half_t*)latents, hist, (half_t*)saved, (const half_t*)z, (int)z_rows,
                       (const float*)row, 0.f, (const half_t*)mask, (const half_t*)init, (const half_t*)noise, n,
                       (const float*)nullptr, 0, (const float*)nullptr, (const half_t*)nullptr, 0.f);
    CID_CHECK_LAUNCH("cid_multistep_step_f16");
    return 0;
}

extern "C" int cid_cfg_multistep_step_scaled_f16(const cid_half* eps, cid_half* latents, float* hist, cid_half* saved,
                                                 const cid_half* z, int32_t z_rows, const void* row, float guidance,
                                                 const cid_half* mask, const cid_half* init, const cid_half* noise,
                                                 int32_t B, int32_t per_sample, const float* escale, cid_stream_t stream) {
    CID_CHECK_ARG(eps && latents && hist && saved && row && escale, "cid_cfg_multistep_step_scaled_f16: null pointer");
    CID_CHECK_ARG((z == nullptr) == (z_rows == 0) && z_rows >= 0,
                  "cid_cfg_multistep_step_scaled_f16: z and z_rows must come together");
    CID_CHECK_ARG((mask == nullptr) == (init == nullptr) && (mask == nullptr) == (noise == nullptr),
                  "cid_cfg_multistep_step_scaled_f16: mask/init/noise must come together");
    CID_CHECK_ARG(B > 0 && per_sample > 0 && per_sample % 8 == 0,
                  "cid_cfg_multistep_step_scaled_f16: per_sample must be a multiple of 8 (an 8-half item lies inside one sample)");
    const long n = (long)B * per_sample;
    CID_CHECK_ARG(n / 8 <= 0x7fffffffL, "cid_cfg_multistep_step_scaled_f16: B * per_sample must be below 2^34");
    hipLaunchKernelGGL(cfg_multistep_kernel<true>, dim3(grid_for(n / 8, 256, 1024)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)eps, (half_t*)latents, hist, (half_t*)saved, (const half_t*)z, (int)z_rows,
                       (const float*)row, guidance, (const half_t*)mask, (const half_t*)init, (const half_t*)noise, n,
                       escale, (int)(per_sample / 8), (const float*)nullptr, (const half_t*)nullptr, 0.f);
    CID_CHECK_LAUNCH("cid_cfg_multistep_step_scaled_f16");
    return 0;
}

// perturbed-attention guidance: the three step entries with a third (second, without CFG) block of eps rows; cid.h
#define CID_PAG_STEP_CHECKS(NAME)                                                                                          \
    CID_CHECK_ARG((mask == nullptr) == (init == nullptr) && (mask == nullptr) == (noise == nullptr),                      \
                  NAME ": mask/init/noise must come together");                                                           \
    const long n = (long)B * per_sample;                                                                                   \
    CID_CHECK_ARG(B > 0 && per_sample > 0 && n % 8 == 0, NAME ": B * per_sample must be a multiple of 8")

extern "C" int cid_cfg_pag_ddim_step_f16(const cid_half* eps, cid_half* latents, const float* coef, float guidance,
                                         const float* pag, const cid_half* mask, const cid_half* init, const cid_half* noise,
                                         int32_t B, int32_t per_sample, cid_stream_t stream) {
    CID_CHECK_ARG(eps && latents && coef && pag, "cid_cfg_pag_ddim_step_f16: null pointer");
    CID_PAG_STEP_CHECKS("cid_cfg_pag_ddim_step_f16");
    hipLaunchKernelGGL((cfg_ddim_kernel<false, true>), dim3(grid_for(n / 8, 256, 1024)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)eps, (half_t*)latents, coef, guidance, (const half_t*)mask, (const half_t*)init,
                       (const half_t*)noise, n, (const float*)nullptr, 0, pag, (const half_t*)nullptr, 0.f);
    CID_CHECK_LAUNCH("cid_cfg_pag_ddim_step_f16");
    return 0;
}

#define CID_PAG_MULTISTEP_CHECKS(NAME)                                                                                     \
    CID_CHECK_ARG(eps && latents && hist && saved && row && pag, NAME ": null pointer");                                  \
    CID_CHECK_ARG((z == nullptr) == (z_rows == 0) && z_rows >= 0, NAME ": z and z_rows must come together");              \
    CID_PAG_STEP_CHECKS(NAME)

extern "C" int cid_cfg_pag_multistep_step_f16(const cid_half* eps, cid_half* latents, float* hist, cid_half* saved,
                                              const cid_half* z, int32_t z_rows, const void* row, float guidance,
                                              const float* pag, const cid_half* mask, const cid_half* init,
                                              const cid_half* noise, int32_t B, int32_t per_sample, cid_stream_t stream) {
    CID_PAG_MULTISTEP_CHECKS("cid_cfg_pag_multistep_step_f16");
    hipLaunchKernelGGL((cfg_multistep_kernel<false, true, true>), dim3(grid_for(n / 8, 256, 1024)), dim3(256), 0,
                       (hipStream_t)stream, (const half_t*)eps, (half_t*)latents, hist, (half_t*)saved, (const half_t*)z,
                       (int)z_rows, (const float*)row, guidance, (const half_t*)mask, (const half_t*)init,
                       (const half_t*)noise, n, (const float*)nullptr, 0, pag, (const half_t*)nullptr, 0.f);
    CID_CHECK_LAUNCH("cid_cfg_pag_multistep_step_f16");
    return 0;
}

extern "C" int cid_pag_multistep_step_f16(const cid_half* eps, cid_half* latents, float* hist, cid_half* saved,
                                          const cid_half* z, int32_t z_rows, const void* row, const float* pag,
                                          const cid_half* mask, const cid_half* init, const cid_half* noise,
                                          int32_t B, int32_t per_sample, cid_stream_t stream) {
    CID_PAG_MULTISTEP_CHECKS("cid_pag_multistep_step_f16");
    for (const void* p : {(const void*)eps, (const void*)latents, (const void*)hist, (const void*)saved, (const void*)z,
                          (const void*)row, (const void*)mask, (const void*)init, (const void*)noise})       // as cid_multistep_step_f16
        CID_CHECK_ARG((uintptr_t)p % 16 == 0, "cid_pag_multistep_step_f16: every buffer must be 16-byte aligned");
    hipLaunchKernelGGL((cfg_multistep_kernel<false, false, true>), dim3(grid_for(n / 8, 256, 1024)), dim3(256), 0,
                       (hipStream_t)stream, (const half_t*)eps, (half_t*)latents, hist, (half_t*)saved, (const half_t*)z,
                       (int)z_rows, (const float*)row, 0.f, (const half_t*)mask, (const half_t*)init,
                       (const half_t*)noise, n, (const float*)nullptr, 0, pag, (const half_t*)nullptr, 0.f);
    CID_CHECK_LAUNCH("cid_pag_multistep_step_f16");
    return 0;
}

// self-attention guidance: the three step entries with the degraded prediction in a buffer of its own; cid.h
extern "C" int cid_cfg_sag_ddim_step_f16(const cid_half* eps, cid_half* latents, const float* coef, float guidance,
                                         const cid_half* eps_d, float sag, const cid_half* mask, const cid_half* init,
                                         const cid_half* noise, int32_t B, int32_t per_sample, cid_stream_t stream) {
    CID_CHECK_ARG(eps && latents && coef && eps_d, "cid_cfg_sag_ddim_step_f16: null pointer");
    CID_PAG_STEP_CHECKS("cid_cfg_sag_ddim_step_f16");
    hipLaunchKernelGGL((cfg_ddim_kernel<false, false, true>), dim3(grid_for(n / 8, 256, 1024)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)eps, (half_t*)latents, coef, guidance, (const half_t*)mask, (const half_t*)init,
                       (const half_t*)noise, n, (const float*)nullptr, 0, (const float*)nullptr, (const half_t*)eps_d, sag);
    CID_CHECK_LAUNCH("cid_cfg_sag_ddim_step_f16");
    return 0;
}

#define CID_SAG_MULTISTEP_CHECKS(NAME)                                                                                     \
    CID_CHECK_ARG(eps && latents && hist && saved && row && eps_d, NAME ": null pointer");                                \
    CID_CHECK_ARG((z == nullptr) == (z_rows == 0) && z_rows >= 0, NAME ": z and z_rows must come together");              \
    CID_PAG_STEP_CHECKS(NAME)

extern "C" int cid_cfg_sag_multistep_step_f16(const cid_half* eps, cid_half* latents, float* hist, cid_half* saved,
                                              const cid_half* z, int32_t z_rows, const void* row, float guidance,
                                              const cid_half* eps_d, float sag, const cid_half* mask, const cid_half* init,
                                              const cid_half* noise, int32_t B, int32_t per_sample, cid_stream_t stream) {
    CID_SAG_MULTISTEP_CHECKS("cid_cfg_sag_multistep_step_f16");
    hipLaunchKernelGGL((cfg_multistep_kernel<false, true, false, true>), dim3(grid_for(n / 8, 256, 1024)), dim3(256), 0,
                       (hipStream_t)stream, (const half_t*)eps, (half_t*)latents, hist, (half_t*)saved, (const half_t*)z,
                       (int)z_rows, (const float*)row, guidance, (const half_t*)mask, (const half_t*)init,
                       (const half_t*)noise, n, (const float*)nullptr, 0, (const float*)nullptr, (const half_t*)eps_d, sag);
    CID_CHECK_LAUNCH("cid_cfg_sag_multistep_step_f16");
    return 0;
}

extern "C" int cid_sag_multistep_step_f16(const cid_half* eps, cid_half* latents, float* hist, cid_half* saved,
                                          const cid_half* z, int32_t z_rows, const void* row, const cid_half* eps_d, float sag,
                                          const cid_half* mask, const cid_half* init, const cid_half* noise,
                                          int32_t B, int32_t per_sample, cid_stream_t stream) {
    CID_SAG_MULTISTEP_CHECKS("cid_sag_multistep_step_f16");
    for (const void* p : {(const void*)eps, (const void*)latents, (const void*)hist, (const void*)saved, (const void*)z,
                          (const void*)row, (const void*)eps_d, (const void*)mask, (const void*)init, (const void*)noise})   // as cid_multistep_step_f16
        CID_CHECK_ARG((uintptr_t)p % 16 == 0, "cid_sag_multistep_step_f16: every buffer must be 16-byte aligned");
    hipLaunchKernelGGL((cfg_multistep_kernel<false, false, false, true>), dim3(grid_for(n / 8, 256, 1024)), dim3(256), 0,
                       (hipStream_t)stream, (const half_t*)eps, (half_t*)latents, hist, (half_t*)saved, (const half_t*)z,
                       (int)z_rows, (const float*)row, 0.f, (const half_t*)mask, (const half_t*)init,
                       (const half_t*)noise, n, (const float*)nullptr, 0, (const float*)nullptr, (const half_t*)eps_d, sag);
    CID_CHECK_LAUNCH("cid_sag_multistep_step_f16");
    return 0;
}
#undef CID_SAG_MULTISTEP_CHECKS
#undef CID_PAG_MULTISTEP_CHECKS
#undef CID_PAG_STEP_CHECKS

extern "C" int cid_add_inplace_f16(cid_half* y, const cid_half* a, int64_t n, int64_t na, cid_stream_t stream) {
    CID_CHECK_ARG(y && a && n > 0 && na > 0 && n % 8 == 0 && na % 8 == 0 && n % na == 0, "cid_add_inplace_f16: sizes must be multiples of 8");
    hipLaunchKernelGGL(add_inplace_kernel, dim3(grid_for(n / 8, 256, 2048)), dim3(256), 0, (hipStream_t)stream,
                       (half_t*)y, (const half_t*)a, (long)n, (long)na);
    CID_CHECK_LAUNCH("cid_add_inplace_f16");
    return 0;
}

extern "C" int cid_residual_accum_f16(const cid_accum_seg* segs, int32_t n_segs, int32_t n_nets, const float* scales,
                                      cid_stream_t stream) {
    CID_CHECK_ARG(segs && scales, "cid_residual_accum_f16: null pointer");
    CID_CHECK_ARG(n_segs >= 1 && n_segs <= RA_MAX_SEGS, "cid_residual_accum_f16: %d segments (1..%d)", n_segs, RA_MAX_SEGS);
    CID_CHECK_ARG(n_nets >= 1 && n_nets <= CID_MAX_CONTROLNETS, "cid_residual_accum_f16: %d nets (1..%d)", n_nets,
                  CID_MAX_CONTROLNETS);
    AccumSegs sg;
    sg.n = n_segs;
    sg.n_nets = n_nets;
    long tiles = 0;
    for (int j = 0; j < RA_MAX_SEGS; ++j) {
        sg.first[j] = tiles;
        if (j >= n_segs) { sg.s[j] = cid_accum_seg{}; continue; }
        const cid_accum_seg& s = segs[j];
        CID_CHECK_ARG(s.y && ((uintptr_t)s.y & 15) == 0, "cid_residual_accum_f16: segment %d: y is null or not 16-byte aligned", j);
        CID_CHECK_ARG(s.n > 0 && s.nr > 0 && s.n % 8 == 0 && s.nr % 8 == 0 && s.n % s.nr == 0,
                      "cid_residual_accum_f16: segment %d: n = %lld, nr = %lld (positive multiples of 8, n %% nr == 0)", j,
                      (long long)s.n, (long long)s.nr);
        for (int k = 0; k < n_nets; ++k)
            CID_CHECK_ARG(s.r[k] && ((uintptr_t)s.r[k] & 15) == 0,
                          "cid_residual_accum_f16: segment %d: residual of net %d is null or not 16-byte aligned", j, k);
        sg.s[j] = s;
        for (int k = n_nets; k < CID_MAX_CONTROLNETS; ++k) sg.s[j].r[k] = nullptr;
        tiles += (s.n / 8 + RA_TILE - 1) / RA_TILE;
    }
    sg.first[RA_MAX_SEGS] = tiles;
    for (int j = n_segs; j <= RA_MAX_SEGS; ++j) sg.first[j] = tiles;
    hipLaunchKernelGGL(residual_accum_kernel, dim3(grid_for(tiles, 1, 2048)), dim3(256), 0, (hipStream_t)stream, sg, scales);
    CID_CHECK_LAUNCH("cid_residual_accum_f16");
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Per-step values of the denoise loop (t, scheduler coefficients, embed-set rows, time-embedding row, SDXL pooled embeds):
// row *counter of a device table -> the buffers the captured step reads; then ++*counter.  One workgroup.
namespace {
struct StepSegs { cid_step_seg s[8]; int n; };
__global__ void __launch_bounds__(1024)
step_select_kernel(const unsigned* __restrict__ table, long row_words, int n_rows, int* counter, StepSegs segs) {
    int row = *counter;
    if (row < 0) row = 0;
    if (row > n_rows - 1) row = n_rows - 1;
    __syncthreads();                           // every thread has read the counter before it moves on
    const unsigned* src = table + (long)row * row_words;
    // one workgroup (the counter update needs no second launch), 1024 lanes, 16 bytes per lane where the segment and its
    // place in the row are 16-byte aligned: a 40-KB time-embedding row is 2.5 load rounds instead of 40 dependent ones
    for (int k = 0; k < segs.n; ++k) {
        unsigned* dst = reinterpret_cast<unsigned*>(segs.s[k].dst);
        const long w0 = segs.s[k].offset >> 2, nw = segs.s[k].nbytes >> 2;
        const bool wide = (((uintptr_t)dst | (uintptr_t)(src + w0)) & 15) == 0;
        long done = 0;
        if (wide) {
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            const long nq = nw >> 2;
            for (long i = threadIdx.x; i < nq; i += 1024)
                reinterpret_cast<u32x4*>(dst)[i] = reinterpret_cast<const u32x4*>(src + w0)[i];
            done = nq << 2;
        }
        for (long i = done + threadIdx.x; i < nw; i += 1024) dst[i] = src[w0 + i];
    }
    if (threadIdx.x == 0) *counter = row + 1;
}
}  // namespace

extern "C" int cid_step_select(const void* table, int64_t row_bytes, int32_t n_rows, int32_t* counter, const cid_step_seg* segs,
                               int32_t n_segs, cid_stream_t stream) {
    CID_CHECK_ARG(table && counter && segs, "cid_step_select: null pointer");
    CID_CHECK_ARG(n_rows > 0 && row_bytes > 0 && row_bytes % 4 == 0 && n_segs > 0 && n_segs <= 8,
                  "cid_step_select: bad table (%d rows of %ld bytes, %d segments; at most 8)", n_rows, (long)row_bytes, n_segs);
    StepSegs sg;
    sg.n = n_segs;
    for (int k = 0; k < n_segs; ++k) {
        CID_CHECK_ARG(segs[k].dst && segs[k].offset >= 0 && segs[k].nbytes > 0 && segs[k].offset % 4 == 0 && segs[k].nbytes % 4 == 0 &&
                      segs[k].offset + segs[k].nbytes <= row_bytes, "cid_step_select: segment %d does not fit the row", k);
        sg.s[k] = segs[k];
    }
    hipLaunchKernelGGL(step_select_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const unsigned*)table,
                       (long)(row_bytes >> 2), n_rows, counter, sg);
    CID_CHECK_LAUNCH("cid_step_select");
    return 0;
}

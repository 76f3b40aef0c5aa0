// Face parser (BiSeNet, models/BiSeNet/model.py + resnet.py), run once per reference image by
// pipline_StableDiffusion_ConsistentID.py:229-244.  Its convolutions are cid_gemm_f16 calls (BatchNorm folded on the host,
// ReLU in the epilogue: cid_gemm_desc.act); these kernels fill the gaps around them:
//   parse_stem_kernel    uint8 RGB -> ToTensor / Normalize -> conv 7x7/2 (+ folded BN) -> ReLU -> maxpool 3x3/2, one launch
//   chan_mean_kernel     F.avg_pool2d(x, x.size()[2:]) of a token-major fp16 tensor, fp32 out
//   chan_gate_kernel     the 1x1 convolutions on those means (conv_avg, the ARM attention, the FFM squeeze / excite)
//   chan_affine_kernel   x * s[b][c] + (t[b][c] | res | x): the ARM / FFM products and sums
//   parse_head_kernel    F.interpolate(bilinear, align_corners=True) of the logits + argmax over the classes
// None of these is matrix-core work: the stem is 1.2 GFLOP of fp32 FMAs at 512 x 512, the rest streams a few MB.
#include "common.h"
#include "../../include/cid.h"

namespace {

// ---------------------------------------------------------------- stem
// One workgroup: an 8 x 8 tile of pooled outputs x 16 channels.  That tile pools conv rows / columns 2 p0 - 1 .. 2 p0 + 15
// (17, the first one the pool's padding at p0 = 0), which read input rows / columns 4 p0 - 5 .. 4 p0 + 33 (39).  The
// normalised input tile and the 16 filters sit in LDS; the conv tile goes to LDS after its ReLU and the pool reads it back.
constexpr int ST_P = 8;                    // pooled outputs per tile side
constexpr int ST_C = 2 * ST_P + 1;         // conv outputs per tile side
constexpr int ST_I = 4 * ST_P + 7;         // input pixels per tile side
constexpr int ST_G = 16;                   // output channels per workgroup
constexpr int ST_K = 7 * 7 * 3;            // taps x input channels

__global__ void __launch_bounds__(256)
parse_stem_kernel(const unsigned char* __restrict__ img, half_t* __restrict__ out, const float* __restrict__ w,
                  const float* __restrict__ bias, int H, int W) {
    __shared__ float xin[ST_I * ST_I * 3];
    __shared__ __attribute__((aligned(16))) float ws[ST_K * ST_G];    // [k][channel of the group]
    __shared__ float cv[ST_C * ST_C * ST_G];
    const int tid = threadIdx.x;
    const int px0 = blockIdx.x * ST_P, py0 = blockIdx.y * ST_P;
    const int b = blockIdx.z >> 2, g = blockIdx.z & 3;
    const int Hc = H >> 1, Wc = W >> 1, Hp = H >> 2, Wp = W >> 2;
    // torchvision ToTensor + Normalize with the reference's ImageNet constants (pipline_StableDiffusion_ConsistentID.py:233);
    // the convolution's zero padding lies in the normalised image
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    const unsigned char* src = img + (long)b * H * W * 3;
    for (int e = tid; e < ST_I * ST_I * 3; e += 256) {
        const int p = e / 3, c = e - p * 3;
        const int r = p / ST_I, q = p - r * ST_I;
        const int iy = 4 * py0 - 5 + r, ix = 4 * px0 - 5 + q;
        float v = 0.f;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = ((float)src[((long)iy * W + ix) * 3 + c] / 255.f - mean[c]) / stdv[c];
        xin[e] = v;
    }
    for (int e = tid; e < ST_K * ST_G; e += 256) {
        const int k = e / ST_G, o = e - k * ST_G;
        ws[e] = w[(long)(g * ST_G + o) * ST_K + k];
    }
    __syncthreads();
    for (int p = tid; p < ST_C * ST_C; p += 256) {
        const int ry = p / ST_C, rx = p - ry * ST_C;
        const int cy = 2 * py0 - 1 + ry, cx = 2 * px0 - 1 + rx;
        float acc[ST_G];
        if (cy < 0 || cy >= Hc || cx < 0 || cx >= Wc) {
            // outside the conv output: the pool's padding.  Every real value is >= 0 after the ReLU, so 0 never wins a window
#pragma unroll
            for (int o = 0; o < ST_G; ++o) acc[o] = 0.f;
        } else {
#pragma unroll
            for (int o = 0; o < ST_G; ++o) acc[o] = bias[g * ST_G + o];
            // conv output (cy, cx) reads input (2 cy - 3 + ky, 2 cx - 3 + kx): tile row 2 ry + ky, column 2 rx + kx
            for (int ky = 0; ky < 7; ++ky) {
                const float* xr = xin + ((2 * ry + ky) * ST_I + 2 * rx) * 3;
                const float* wr = ws + ky * 21 * ST_G;
#pragma unroll
                for (int j = 0; j < 21; ++j) {
                    const float v = xr[j];
#pragma unroll
                    for (int o = 0; o < ST_G; ++o) acc[o] = __builtin_fmaf(v, wr[j * ST_G + o], acc[o]);
                }
            }
#pragma unroll
            for (int o = 0; o < ST_G; ++o) acc[o] = __builtin_fmaxf(acc[o], 0.f);
        }
#pragma unroll
        for (int o = 0; o < ST_G; ++o) cv[p * ST_G + o] = acc[o];
    }
    __syncthreads();
    // pool: thread = one pooled pixel x 4 channels; pooled (py, px) reads conv rows 2 py - 1 + dy: tile row 2 (py - py0) + dy
    const int pp = tid >> 2, cq = tid & 3;
    const int ly = pp / ST_P, lx = pp - ly * ST_P;
    float m[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float* c = cv + ((2 * ly + dy) * ST_C + 2 * lx + dx) * ST_G + 4 * cq;
#pragma unroll
            for (int i = 0; i < 4; ++i) m[i] = __builtin_fmaxf(m[i], c[i]);
        }
    half4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (half_t)m[i];
    const long row = (long)b * Hp * Wp + (long)(py0 + ly) * Wp + px0 + lx;
    *reinterpret_cast<half4*>(out + row * 64 + g * ST_G + 4 * cq) = o;
}

// ---------------------------------------------------------------- per-(sample, channel) mean
// Workgroup = one sample x 64 channels: 8 lanes of 8 channels x 32 row lanes, fp32 partial sums, a fixed-order fold.
__global__ void __launch_bounds__(256)
chan_mean_kernel(const half_t* __restrict__ x, float* __restrict__ out, int HW, int C, int ld) {
    __shared__ float part[32][64];
    const int tid = threadIdx.x, cg = tid & 7, r = tid >> 3;
    const int b = blockIdx.y, c0 = blockIdx.x * 64 + cg * 8;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c0 < C) {
        const half_t* p = x + (long)b * HW * ld + c0;
        for (int t = r; t < HW; t += 32) {
            const half8 v = *reinterpret_cast<const half8*>(p + (long)t * ld);
#pragma unroll
            for (int i = 0; i < 8; ++i) s[i] += (float)v[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) part[r][cg * 8 + i] = s[i];
    __syncthreads();
    if (tid < 64 && blockIdx.x * 64 + tid < C) {
        float t = 0.f;
        for (int j = 0; j < 32; ++j) t += part[j][tid];
        out[(long)b * C + blockIdx.x * 64 + tid] = t / (float)HW;
    }
}

// ---------------------------------------------------------------- channel gate
CID_DEVINL float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// y[n] = sum_k W[n][k] v[k] (+ b[n]) for n < N: one wave per output row, lanes over k, a butterfly fold
CID_DEVINL void gate_layer(const float* v, const float* __restrict__ w, const float* __restrict__ b, float* y, int K, int N) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int n = wave; n < N; n += 4) {
        float s = 0.f;
        for (int k = lane; k < K; k += 64) s = __builtin_fmaf(w[(long)n * K + k], v[k], s);
        s = wave_sum(s);
        if (lane == 0) y[n] = s + (b ? b[n] : 0.f);
    }
}

__global__ void __launch_bounds__(256)
chan_gate_kernel(const float* __restrict__ mean, float* __restrict__ out, const float* __restrict__ w1,
                 const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                 int K, int N1, int N, int act) {
    __shared__ float v[512], h[512], y[512];
    const int b = blockIdx.x;
    for (int k = threadIdx.x; k < K; k += 256) v[k] = mean[(long)b * K + k];
    __syncthreads();
    gate_layer(v, w1, b1, w2 ? h : y, K, N1);
    __syncthreads();
    if (w2) {
        for (int n = threadIdx.x; n < N1; n += 256) h[n] = __builtin_fmaxf(h[n], 0.f);
        __syncthreads();
        gate_layer(h, w2, b2, y, N1, N);
        __syncthreads();
    }
    for (int n = threadIdx.x; n < N; n += 256) {
        float t = y[n];
        if (act == 1) t = __builtin_fmaxf(t, 0.f);
        else if (act == 2) t = 1.f / (1.f + __expf(-t));
        out[(long)b * N + n] = t;
    }
}

// ---------------------------------------------------------------- channel affine
// out = x * s[b][c] + add, add = t[b][c] | res[b][p][c] | x[b][p][c]; fp32, rounded once.  8 channels per thread.
__global__ void __launch_bounds__(256)
chan_affine_kernel(const half_t* x, const float* __restrict__ s, const float* __restrict__ t, const half_t* res,
                   half_t* out, long HW, int C8, long items) {     // (out may be x: no restrict on x / res / out)
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < items; e += (long)gridDim.x * blockDim.x) {
        const long row = e / C8;
        const int c = (int)(e - row * C8) * 8;
        const long b = row / HW;
        const int C = C8 * 8;
        const half8 xv = *reinterpret_cast<const half8*>(x + row * C + c);
        half8 av = xv;
        if (res) av = *reinterpret_cast<const half8*>(res + row * C + c);
        const float* sp = s + b * C + c;
        half8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float add = t ? t[b * C + c + i] : (float)av[i];
            o[i] = (half_t)((float)xv[i] * sp[i] + add);
        }
        *reinterpret_cast<half8*>(out + row * C + c) = o;
    }
}

// ---------------------------------------------------------------- head: bilinear (align_corners=True) + argmax
// One thread per output pixel.  The source coordinate and the weights follow D: torch's upsample_bilinear2d with
// align_corners=True: scale = (in - 1) / (out - 1) in fp32, src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1),
// l1 = src - i0, l0 = 1 - l1, value = l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11).  First maximum wins (numpy's rule).
__global__ void __launch_bounds__(256)
parse_head_kernel(const half_t* __restrict__ lg, int ld, int ncls, int h, int w, int H, int W, float sh, float sw,
                  unsigned char* __restrict__ labels, float* __restrict__ lout, long items) {
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < items; e += (long)gridDim.x * blockDim.x) {
        const long bY = e / W;
        const int X = (int)(e - bY * W);
        const long b = bY / H;
        const int Y = (int)(bY - b * H);
        const float sy = sh * (float)Y, sx = sw * (float)X;
        const int y0 = (int)sy, x0 = (int)sx;
        const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
        const float ly1 = sy - (float)y0, lx1 = sx - (float)x0;
        const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
        const half_t* base = lg + b * (long)h * w * ld;
        const half_t* p00 = base + ((long)y0 * w + x0) * ld;
        const half_t* p01 = base + ((long)y0 * w + x1) * ld;
        const half_t* p10 = base + ((long)y1 * w + x0) * ld;
        const half_t* p11 = base + ((long)y1 * w + x1) * ld;
        float best = 0.f;
        int arg = 0;
        for (int c = 0; c < ncls; ++c) {
            const float v = ly0 * (lx0 * (float)p00[c] + lx1 * (float)p01[c]) + ly1 * (lx0 * (float)p10[c] + lx1 * (float)p11[c]);
            if (c == 0 || v > best) { best = v; arg = c; }
            if (lout) lout[((b * ncls + c) * H + Y) * (long)W + X] = v;
        }
        labels[e] = (unsigned char)arg;
    }
}

int grid_for(long items, int block, int cap) {
    long g = (items + block - 1) / block;
    return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" int cid_parse_stem_f16(const uint8_t* img, cid_half* out, const float* w, const float* bias, int32_t B, int32_t H,
                                  int32_t W, cid_stream_t stream) {
    CID_CHECK_ARG(img && out && w && bias, "cid_parse_stem_f16: null pointer");
    CID_CHECK_ARG(B > 0 && H >= 32 && W >= 32 && H % 32 == 0 && W % 32 == 0 && B <= 65535 / 4,
                  "cid_parse_stem_f16: H and W must be positive multiples of 32, 1 <= B <= 16383 (got B %d, %d x %d)", B, H, W);
    CID_CHECK_ARG(((uintptr_t)out & 15) == 0, "cid_parse_stem_f16: out must be 16-byte aligned");
    hipLaunchKernelGGL(parse_stem_kernel, dim3(W / 4 / ST_P, H / 4 / ST_P, B * 4), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)img, (half_t*)out, w, bias, H, W);
    CID_CHECK_LAUNCH("cid_parse_stem_f16");
    return 0;
}

extern "C" int cid_chan_mean_f16(const cid_half* x, float* out, int32_t B, int32_t HW, int32_t C, int32_t ld,
                                 cid_stream_t stream) {
    CID_CHECK_ARG(x && out, "cid_chan_mean_f16: null pointer");
    CID_CHECK_ARG(B > 0 && B <= 65535 && HW > 0 && C > 0 && C % 8 == 0 && ld >= C && ld % 8 == 0,
                  "cid_chan_mean_f16: bad shape (B %d, HW %d, C %d, ld %d; C %% 8 == 0, ld >= C, ld %% 8 == 0)", B, HW, C, ld);
    CID_CHECK_ARG(((uintptr_t)x & 15) == 0, "cid_chan_mean_f16: x must be 16-byte aligned");
    hipLaunchKernelGGL(chan_mean_kernel, dim3((C + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, out,
                       HW, C, ld);
    CID_CHECK_LAUNCH("cid_chan_mean_f16");
    return 0;
}

extern "C" int cid_chan_gate_f32(const float* mean, float* out, const float* w1, const float* b1, const float* w2,
                                 const float* b2, int32_t B, int32_t K, int32_t N1, int32_t N, int32_t act,
                                 cid_stream_t stream) {
    CID_CHECK_ARG(mean && out && w1, "cid_chan_gate_f32: null pointer");
    CID_CHECK_ARG(B > 0 && K > 0 && K <= 512 && N1 > 0 && N1 <= 512 && N > 0 && N <= 512 && (w2 || N == N1),
                  "cid_chan_gate_f32: bad shape (B %d, K %d, N1 %d, N %d; at most 512 each, N == N1 without w2)", B, K, N1, N);
    CID_CHECK_ARG(w2 || !b2, "cid_chan_gate_f32: b2 without w2");
    CID_CHECK_ARG(act >= 0 && act <= 2, "cid_chan_gate_f32: bad act %d (0 none, 1 ReLU, 2 sigmoid)", act);
    hipLaunchKernelGGL(chan_gate_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, mean, out, w1, b1, w2, b2, K, N1, N, act);
    CID_CHECK_LAUNCH("cid_chan_gate_f32");
    return 0;
}

extern "C" int cid_chan_affine_f16(const cid_half* x, const float* s, const float* t, const cid_half* res, cid_half* out,
                                   int32_t B, int32_t HW, int32_t C, cid_stream_t stream) {
    CID_CHECK_ARG(x && s && out, "cid_chan_affine_f16: null pointer");
    CID_CHECK_ARG(!(t && res), "cid_chan_affine_f16: give t or res, not both");
    CID_CHECK_ARG(B > 0 && HW > 0 && C > 0 && C % 8 == 0, "cid_chan_affine_f16: bad shape (B %d, HW %d, C %d; C %% 8 == 0)",
                  B, HW, C);
    CID_CHECK_ARG((((uintptr_t)x | (uintptr_t)res | (uintptr_t)out) & 15) == 0,
                  "cid_chan_affine_f16: x / res / out must be 16-byte aligned");
    const long items = (long)B * HW * (C / 8);
    hipLaunchKernelGGL(chan_affine_kernel, dim3(grid_for(items, 256, 4096)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)x, s, t, (const half_t*)res, (half_t*)out, (long)HW, C / 8, items);
    CID_CHECK_LAUNCH("cid_chan_affine_f16");
    return 0;
}

extern "C" int cid_parse_head_f16(const cid_half* logits, int32_t ld, int32_t ncls, int32_t B, int32_t h, int32_t w,
                                  int32_t H, int32_t W, uint8_t* labels, float* logits_out, cid_stream_t stream) {
    CID_CHECK_ARG(logits && labels, "cid_parse_head_f16: null pointer");
    CID_CHECK_ARG(ncls > 0 && ncls <= 256 && ld >= ncls && B > 0 && h > 0 && w > 0 && H > 0 && W > 0,
                  "cid_parse_head_f16: bad shape (ncls %d, ld %d, B %d, %d x %d -> %d x %d; 0 < ncls <= min(ld, 256))", ncls,
                  ld, B, h, w, H, W);
    const float sh = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f;
    const float sw = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    const long items = (long)B * H * W;
    hipLaunchKernelGGL(parse_head_kernel, dim3(grid_for(items, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)logits, ld, ncls, h, w, H, W, sh, sw, (unsigned char*)labels, logits_out, items);
    CID_CHECK_LAUNCH("cid_parse_head_f16");
    return 0;
}

// AutoencoderTiny (TAESD / taesdxl) decoder (D: diffusers 0.23 models/autoencoder_tiny.py, vae.DecoderTiny): a 64-channel,
// attention-free ReLU conv net that stands in for AutoencoderKL.decode in few-step generation.
//   cid_tiny_decode_in_f16   tanh(z / 3) * 3, conv 4 -> 64, bias, ReLU: NCHW latents -> token-major
//   cid_tiny_conv64_f16      the 64 -> 64 body convolution, weight-stationary (below)
//   cid_tiny_decode_out_f16  conv 64 -> 3, bias, then 2x - 1 or clamp(x, 0, 1): token-major -> NCHW image
// and its encoder (vae.EncoderTiny), the decoder's mirror image, which reuses cid_tiny_conv64_f16 for every Block:
//   cid_tiny_encode_in_f16   the inpaint pre-processing, (v + 1) / 2, conv 3 -> 64, bias: fp32 NCHW image -> token-major
//   cid_tiny_conv64_s2_f16   the stride-2, bias-less 64 -> 64 convolution between levels, weight-stationary (below)
//   cid_tiny_encode_out_f16  conv 64 -> 4, bias, times scale: token-major -> NCHW latents
// The body is memory-bound at full resolution (128 bytes in, 128 bytes out and 73.7 kFLOP per pixel), so the kernel is built
// around touching each activation once: cid_gemm_f16 at N = 64, K = 576 re-stages the 72 KiB weight for every 128-token
// tile and gathers every input pixel nine times.
#include "common.h"
#include "../../include/cid.h"

namespace {

// ---------------------------------------------------------------- body: 64 -> 64, 3x3, weight-stationary
// One workgroup of 8 waves per CU (152,064 bytes of LDS).  The whole weight sits in LDS as [tap][cout][cin] for every tile the
// workgroup walks (tiles blockIdx.x, + gridDim.x, ...); an output tile is TC_TH x TC_TW pixels and its input is staged with a
// one-pixel halo, (TC_TH + 2) x (TC_TW + 2) pixels of 128 bytes, zeros outside the image.  With `up` the halo is filled through
// the nearest-2x map (output pixel (y, x) reads input (y >> 1, x >> 1)), so the upsampled tensor exists in LDS only.
// Both LDS images keep 128-byte rows and XOR the 16-byte slot of a row with bits 1..3 of the row index: the sixteen lanes that a
// ds_read_b128 serves together read sixteen consecutive rows at one slot, which the XOR spreads over all sixteen 16-byte
// columns of the 256-byte bank row.
// Wave w computes tile rows 2w and 2w + 1 (two 32-pixel column tiles) against both 32-channel row tiles: A = weights (rows =
// output channels), B = pixels, so a lane ends up with 4 consecutive channels of one pixel per register quad (8-byte stores).
// The halo of the NEXT tile is loaded into registers before the MFMAs of this one and written to LDS after them.
// Deterministic: one workgroup owns an output tile, the contraction order is fixed (tap-major, then channel), no atomics.
constexpr int TC_TH = 16, TC_TW = 32;
constexpr int TC_THREADS = 512;
constexpr int TC_HH = TC_TH + 2, TC_HW = TC_TW + 2;
constexpr int TC_HPIX = TC_HH * TC_HW;                         // 612 halo pixels
constexpr int TC_HCHUNKS = TC_HPIX * 8;                        // 16-byte chunks of the halo image
constexpr int TC_NLD = (TC_HCHUNKS + TC_THREADS - 1) / TC_THREADS;   // 10 chunks per thread
constexpr int TC_WBYTES = 9 * 64 * 128;                        // 73,728
constexpr int TC_SMEM = TC_WBYTES + TC_HPIX * 128;             // 152,064
constexpr int TC_GRID_CAP = 256;                               // one workgroup per CU
static_assert(TC_SMEM <= 160 * 1024, "LDS budget");

CID_DEVINL int tc_swz(int row, int slot) { return row * 128 + ((slot ^ ((row >> 1) & 7)) << 4); }

struct TinyConvArgs {
    const half_t* x; const half_t* w; const half_t* bias; const half_t* res; half_t* out;
    int B, H, W;            // OUTPUT grid
    int Hi, Wi;             // input grid (H >> up, W >> up)
    int up, relu;
    int tiles_x, tiles_y, ntiles;
};

CID_DEVINL void tc_tile_origin(const TinyConvArgs& a, int t, int& b, int& y0, int& x0) {
    const int per = a.tiles_x * a.tiles_y;
    b = t / per;
    const int r = t - b * per;
    const int ty = r / a.tiles_x;
    y0 = ty * TC_TH;
    x0 = (r - ty * a.tiles_x) * TC_TW;
}

CID_DEVINL void tc_load_halo(const TinyConvArgs& a, int t, half8 (&v)[TC_NLD]) {
    int b, y0, x0;
    tc_tile_origin(a, t, b, y0, x0);
    const half_t* src = a.x + (long)b * a.Hi * a.Wi * 64;
#pragma unroll
    for (int i = 0; i < TC_NLD; ++i) {
        const int ch = (int)threadIdx.x + i * TC_THREADS;
        const int p = ch >> 3, s = ch & 7;
        const int hy = p / TC_HW, hx = p - hy * TC_HW;
        const int y = y0 - 1 + hy, x = x0 - 1 + hx;
        half8 val = zero_h8();
        if (ch < TC_HCHUNKS && y >= 0 && y < a.H && x >= 0 && x < a.W)
            val = ld_global_h8(src + ((long)(y >> a.up) * a.Wi + (x >> a.up)) * 64 + s * 8);
        v[i] = val;
    }
}

__global__ void __launch_bounds__(TC_THREADS)
tiny_conv64_kernel(const TinyConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tc_lds[];
    unsigned char* wl = tc_lds;
    unsigned char* hl = tc_lds + TC_WBYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int idx = lane & 31, hi = lane >> 5;

    // weights: global [cout][tap][cin] -> LDS [tap][cout][cin], once
    for (int ch = tid; ch < 64 * 72; ch += TC_THREADS) {
        const int n = ch / 72, rem = ch - n * 72;
        const int tap = rem >> 3, s = rem & 7;
        *reinterpret_cast<half8*>(wl + tc_swz(tap * 64 + n, s)) = ld_global_h8(a.w + (long)ch * 8);
    }

    half8 pre[TC_NLD];
    int t = blockIdx.x;
    if (t < a.ntiles) tc_load_halo(a, t, pre);
    while (t < a.ntiles) {
        __syncthreads();                    // the previous tile's reads of the halo image are done
#pragma unroll
        for (int i = 0; i < TC_NLD; ++i) {
            const int ch = tid + i * TC_THREADS;
            if (ch < TC_HCHUNKS) *reinterpret_cast<half8*>(hl + tc_swz(ch >> 3, ch & 7)) = pre[i];
        }
        __syncthreads();
        const int tn = t + gridDim.x;
        if (tn < a.ntiles) tc_load_halo(a, tn, pre);

        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = zero_f16v();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap % 3;
            const int p0 = (2 * wave + dy) * TC_HW + idx + dx;          // halo pixel of column tile 0; tile 1 is one row down
            const int p1 = p0 + TC_HW;
            const int n0 = tap * 64 + idx, n1 = n0 + 32;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                const int s = kb * 2 + hi;
                const half8 a0 = *reinterpret_cast<const half8*>(wl + tc_swz(n0, s));
                const half8 a1 = *reinterpret_cast<const half8*>(wl + tc_swz(n1, s));
                const half8 b0 = *reinterpret_cast<const half8*>(hl + tc_swz(p0, s));
                const half8 b1 = *reinterpret_cast<const half8*>(hl + tc_swz(p1, s));
                acc[0][0] = mfma32(a0, b0, acc[0][0]);
                acc[0][1] = mfma32(a0, b1, acc[0][1]);
                acc[1][0] = mfma32(a1, b0, acc[1][0]);
                acc[1][1] = mfma32(a1, b1, acc[1][1]);
            }
        }

        // epilogue: lane = pixel idx of tile row 2 * wave + j; registers 4g .. 4g + 3 of row tile i = channels 32i + 8g + 4hi + (0..3)
        int b, y0, x0;
        tc_tile_origin(a, t, b, y0, x0);
        const int x = x0 + idx;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int y = y0 + 2 * wave + j;
            if (y < a.H && x < a.W) {
                const long o = (((long)b * a.H + y) * a.W + x) * 64;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int c = 32 * i + 8 * g + 4 * hi;
                        float v[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) v[q] = acc[i][j][4 * g + q];
                        if (a.bias) {
                            const half4 bb = *reinterpret_cast<const half4*>(a.bias + c);
#pragma unroll
                            for (int q = 0; q < 4; ++q) v[q] += (float)bb[q];
                        }
                        if (a.res) {
                            const half4 rr = *reinterpret_cast<const half4*>(a.res + o + c);
#pragma unroll
                            for (int q = 0; q < 4; ++q) v[q] += (float)rr[q];
                        }
                        half4 ov;
#pragma unroll
                        for (int q = 0; q < 4; ++q) ov[q] = (half_t)(a.relu ? fmaxf(v[q], 0.f) : v[q]);
                        *reinterpret_cast<half4*>(a.out + o + c) = ov;
                    }
            }
        }
        t = tn;
    }
}

// ---------------------------------------------------------------- encoder: 64 -> 64, 3x3, stride 2, pad 1, weight-stationary
// The body kernel's design on an 8 x 16 output tile: output (y, x) reads input (2y - 1 + dy, 2x - 1 + dx), so the tile's input is
// a (2 * 8 + 1) x (2 * 16 + 1) = 17 x 33 halo, zeros outside the image on all four sides; the weight leaves 90,112 bytes of the
// 160 KiB, 704 pixels (16 x 32 outputs would need 33 x 65).  Wave w owns the 32 pixels of tile rows 2 (w >> 1) and
// 2 (w >> 1) + 1 (B operand: lane idx = 16 * row + column) against the 32 output channels of row tile w & 1: one accumulator.
// With the body kernel's halo image the sixteen lanes of a ds_read_b128 group would read every SECOND 128-byte row, two lanes per
// 16-byte column of the bank row.  The halo is therefore staged de-interleaved by column parity, in rows of TS_LW = 40 pixels:
// even halo columns 0, 2 .. 32 at 0 .. 16, odd ones 1, 3 .. 31 at 17 .. 32 (33 .. 39 are never written or read).  Tap dx = 0 of
// output column x then reads row-pixel x, dx = 1 reads 17 + x, dx = 2 reads x + 1: consecutive 128-byte rows along x, and the
// second tile row of a B operand sits 2 * TS_LW = 80 = 0 (mod 16) rows further on, so every 16-lane group ({0-3, 12-15, 20-27},
// ...) reads sixteen rows that are distinct mod 16, which tc_swz spreads over all sixteen columns as in the body kernel.
constexpr int TS_TH = 8, TS_TW = 16;
constexpr int TS_HH = 2 * TS_TH + 1, TS_HW = 2 * TS_TW + 1;   // 17 x 33 halo
constexpr int TS_LW = 40;                                      // LDS pixels per halo row
constexpr int TS_ODD = TS_TW + 1;                              // where the odd columns start
constexpr int TS_HCHUNKS = TS_HH * TS_HW * 8;                  // 4,488 16-byte chunks are loaded
constexpr int TS_NLD = (TS_HCHUNKS + TC_THREADS - 1) / TC_THREADS;   // 9 per thread
constexpr int TS_SMEM = TC_WBYTES + TS_HH * TS_LW * 128;       // 160,768
static_assert(TS_SMEM <= 160 * 1024, "LDS budget");
static_assert((2 * TS_LW) % 16 == 0 && TS_LW >= TS_HW && TS_TH * TS_TW * 2 == 32 * 8, "tile / wave / swizzle assumptions");

struct TinyS2Args {
    const half_t* x; const half_t* w; half_t* out;
    int B, Hi, Wi, Ho, Wo;
    int tiles_x, tiles_y, ntiles;
};

CID_DEVINL void ts_tile_origin(const TinyS2Args& a, int t, int& b, int& y0, int& x0) {
    const int per = a.tiles_x * a.tiles_y;
    b = t / per;
    const int r = t - b * per;
    const int ty = r / a.tiles_x;
    y0 = ty * TS_TH;
    x0 = (r - ty * a.tiles_x) * TS_TW;
}

CID_DEVINL void ts_load_halo(const TinyS2Args& a, int t, half8 (&v)[TS_NLD]) {
    int b, y0, x0;
    ts_tile_origin(a, t, b, y0, x0);
    const half_t* src = a.x + (long)b * a.Hi * a.Wi * 64;
#pragma unroll
    for (int i = 0; i < TS_NLD; ++i) {
        const int ch = (int)threadIdx.x + i * TC_THREADS;
        const int p = ch >> 3, s = ch & 7;
        const int hy = p / TS_HW, hx = p - hy * TS_HW;
        const int y = 2 * y0 - 1 + hy, x = 2 * x0 - 1 + hx;
        half8 val = zero_h8();
        if (ch < TS_HCHUNKS && y >= 0 && y < a.Hi && x >= 0 && x < a.Wi)
            val = ld_global_h8(src + ((long)y * a.Wi + x) * 64 + s * 8);
        v[i] = val;
    }
}

__global__ void __launch_bounds__(TC_THREADS)
tiny_conv64_s2_kernel(const TinyS2Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tc_lds[];
    unsigned char* wl = tc_lds;
    unsigned char* hl = tc_lds + TC_WBYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int idx = lane & 31, hi = lane >> 5;
    const int pt = wave >> 1, ct = wave & 1;
    const int ly = 2 * pt + (idx >> 4), lx = idx & 15;           // this lane's output pixel within the tile

    for (int ch = tid; ch < 64 * 72; ch += TC_THREADS) {
        const int n = ch / 72, rem = ch - n * 72;
        const int tap = rem >> 3, s = rem & 7;
        *reinterpret_cast<half8*>(wl + tc_swz(tap * 64 + n, s)) = ld_global_h8(a.w + (long)ch * 8);
    }

    half8 pre[TS_NLD];
    int t = blockIdx.x;
    if (t < a.ntiles) ts_load_halo(a, t, pre);
    while (t < a.ntiles) {
        __syncthreads();                    // the previous tile's reads of the halo image are done
#pragma unroll
        for (int i = 0; i < TS_NLD; ++i) {
            const int ch = tid + i * TC_THREADS;
            if (ch < TS_HCHUNKS) {
                const int p = ch >> 3;
                const int hy = p / TS_HW, hx = p - hy * TS_HW;
                const int row = hy * TS_LW + ((hx & 1) ? TS_ODD + (hx >> 1) : (hx >> 1));
                *reinterpret_cast<half8*>(hl + tc_swz(row, ch & 7)) = pre[i];
            }
        }
        __syncthreads();
        const int tn = t + gridDim.x;
        if (tn < a.ntiles) ts_load_halo(a, tn, pre);

        f32x16 acc = zero_f16v();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap % 3;
            const int p0 = (2 * ly + dy) * TS_LW + lx + (dx == 1 ? TS_ODD : (dx >> 1));
            const int n0 = tap * 64 + 32 * ct + idx;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                const int s = kb * 2 + hi;
                const half8 a0 = *reinterpret_cast<const half8*>(wl + tc_swz(n0, s));
                const half8 b0 = *reinterpret_cast<const half8*>(hl + tc_swz(p0, s));
                acc = mfma32(a0, b0, acc);
            }
        }

        // epilogue: registers 4g .. 4g + 3 = channels 32 ct + 8g + 4hi + (0..3) of this lane's pixel
        int b, y0, x0;
        ts_tile_origin(a, t, b, y0, x0);
        const int y = y0 + ly, x = x0 + lx;
        if (y < a.Ho && x < a.Wo) {
            const long o = (((long)b * a.Ho + y) * a.Wo + x) * 64;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                half4 ov;
#pragma unroll
                for (int q = 0; q < 4; ++q) ov[q] = (half_t)acc[4 * g + q];
                *reinterpret_cast<half4*>(a.out + o + 32 * ct + 8 * g + 4 * hi) = ov;
            }
        }
        t = tn;
    }
}

// ---------------------------------------------------------------- the ends
// tanh(z / 3) * 3 in fp32, finite and good to fp32 rounding for every finite input: the odd series below 1/8 (the quotient form
// cancels there: 1 - t with t -> 1), (1 - t) / (1 + t) with t = exp(-2|x|) above it -- t underflows to 0, never overflows, so
// |z| = 65504 gives exactly 3.
CID_DEVINL float tanh3_f(float z) {
    const float x = z * 0.33333333333333333f;
    const float ax = __builtin_fabsf(x);
    float r;
    if (ax < 0.125f) {
        const float x2 = x * x;
        float p = __builtin_fmaf(x2, -0.053968253968253971f, 0.13333333333333333f);   // -17/315, 2/15
        p = __builtin_fmaf(x2, p, -0.33333333333333333f);
        r = __builtin_fmaf(x * x2, p, x);
    } else {
        const float t = __builtin_amdgcn_exp2f(ax * -2.8853900817779268f);            // exp(-2|x|)
        r = __builtin_copysignf((1.f - t) / (1.f + t), x);
    }
    return 3.f * r;
}

// decode_in: eight threads per latent pixel, each gathers the pixel's 36 inputs (9 taps x 4 channels, tanh applied, zero outside)
// and computes 8 of the 64 output channels in fp32 against weights held in LDS as fp32 [k][cout]; one 16-byte store each.
constexpr int DI_K = 36;

__global__ void __launch_bounds__(256)
tiny_decode_in_kernel(const half_t* __restrict__ z, half_t* __restrict__ out, const half_t* __restrict__ w,
                      const half_t* __restrict__ bias, int B, int H, int W) {
    __shared__ float wl[DI_K * 64];
    for (int i = threadIdx.x; i < DI_K * 64; i += 256) {
        const int co = i / DI_K, k = i - co * DI_K;             // w: [cout][tap][4] = [cout][k]
        wl[k * 64 + co] = (float)w[i];
    }
    __syncthreads();
    const long HW = (long)H * W;
    const long p = (long)blockIdx.x * 32 + (threadIdx.x >> 3);
    if (p >= (long)B * HW) return;
    const int sub = threadIdx.x & 7;
    const int b = (int)(p / HW);
    const int rem = (int)(p - (long)b * HW);
    const int y = rem / W, x = rem - y * W;
    const half_t* src = z + (long)b * 4 * HW;
    float acc[8];
    {
        const half8 bb = ld_global_h8(bias + sub * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = (float)bb[i];
    }
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        const long o = (long)yy * W + xx;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float v = tanh3_f((float)src[c * HW + o]);
            const float* wp = wl + (tap * 4 + c) * 64 + sub * 8;
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(v, wp[i], acc[i]);
        }
    }
    half8 ov;
#pragma unroll
    for (int i = 0; i < 8; ++i) ov[i] = (half_t)fmaxf(acc[i], 0.f);
    *reinterpret_cast<half8*>(out + p * 64 + sub * 8) = ov;
}

// encode_in: vae_encode_in_kernel's (vae_enc.hip) pre-processing in front of decode_in's arithmetic.  Eight threads per pixel
// gather the 27 inputs and 9 mask values once: v = half(normalize ? 2x - 1 : x), the masked image is v where mask < 0.5 and 0
// elsewhere, then u = half(v + 1) / 2 (ONE fp16 rounding, of v + 1: the halving is exact), TAESD's [0, 1] range.  The conv's zero
// padding applies to u: a tap outside the image is 0, which is -1 in image space and so cannot be folded into the bias; a masked
// pixel is u = 0.5.  fp32 accumulation against weights in LDS as fp32 [k][cout], bias, no activation, 16-byte stores.
constexpr int NI_K = 27;

__global__ void __launch_bounds__(256)
tiny_encode_in_kernel(const float* __restrict__ image, const float* __restrict__ mask, half_t* __restrict__ out,
                      const half_t* __restrict__ w, const half_t* __restrict__ bias, half_t* __restrict__ mask_latents,
                      int Bi, int Bm, int H, int W, int normalize, int blocks) {
    __shared__ float wl[NI_K * 64];
    for (int i = threadIdx.x; i < NI_K * 64; i += 256) {
        const int co = i / NI_K, k = i - co * NI_K;             // w: [cout][tap][3] = [cout][k]
        wl[k * 64 + co] = (float)w[i];
    }
    __syncthreads();
    const bool want_img = blocks & 1, want_msk = (blocks & 2) != 0;
    const int HW = H * W;
    const long npix = (long)Bi * HW;
    const int sub = threadIdx.x & 7;
    const long ostride = npix * 64;                             // one batch block of the output
    for (long p = (long)blockIdx.x * 32 + (threadIdx.x >> 3); p < npix; p += (long)gridDim.x * 32) {
        const int b = (int)(p / HW);
        const int rem = (int)(p - (long)b * HW);
        const int y = rem / W, x = rem - y * W;
        const float* src = image + (long)b * 3 * HW;
        const float* msrc = mask ? mask + (long)(Bm == 1 ? 0 : b) * HW : nullptr;
        float ai[8], am[8];
        {
            const half8 bb = ld_global_h8(bias + sub * 8);
#pragma unroll
            for (int i = 0; i < 8; ++i) ai[i] = am[i] = (float)bb[i];
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;  // u = 0 outside the image
            const long o = (long)yy * W + xx;
            const bool keep = msrc ? (msrc[o] < 0.5f) : true;       // binarised at 0.5, masked_image = image * (mask < 0.5)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float t = src[(long)c * HW + o];
                if (normalize) t = 2.f * t - 1.f;
                const half_t v = (half_t)t;
                const float ui = 0.5f * (float)(half_t)((float)v + 1.f);
                const float um = keep ? ui : 0.5f;
                const float* wp = wl + (tap * 3 + c) * 64 + sub * 8;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (want_img) ai[i] = __builtin_fmaf(ui, wp[i], ai[i]);
                    if (want_msk) am[i] = __builtin_fmaf(um, wp[i], am[i]);
                }
            }
        }
        if (mask_latents && sub == 0 && b < Bm && (y & 7) == 0 && (x & 7) == 0)
            // F.interpolate(mask, size=(H / 8, W / 8)) (nearest: source index 8y, 8x) of the binarised mask
            mask_latents[((long)b * (H >> 3) + (y >> 3)) * (W >> 3) + (x >> 3)] = msrc[rem] < 0.5f ? (half_t)0.f : (half_t)1.f;
        half_t* dst = out + p * 64 + sub * 8;
        if (want_img) {
            half8 ov;
#pragma unroll
            for (int i = 0; i < 8; ++i) ov[i] = (half_t)ai[i];
            *reinterpret_cast<half8*>(dst) = ov;
            dst += ostride;
        }
        if (want_msk) {
            half8 ov;
#pragma unroll
            for (int i = 0; i < 8; ++i) ov[i] = (half_t)am[i];
            *reinterpret_cast<half8*>(dst) = ov;
        }
    }
}

// decode_out / encode_out: eight threads per pixel, thread s takes channels 8s .. 8s + 7 of the nine taps (the eight 16-byte
// loads of a pixel are one 128-byte line) against the NO output rows in LDS (fp32 [cout][tap][cin]); a butterfly over the eight
// lanes leaves every sum in every lane and lane s < NO writes plane s.  NO = 3: the image, 2v - 1 or clamp(v, 0, 1); NO = 4: the
// encoder's latents, v * scale.
template <int NO>
__global__ void __launch_bounds__(256)
tiny_out_kernel(const half_t* __restrict__ xin, half_t* __restrict__ out, const half_t* __restrict__ w,
                const half_t* __restrict__ bias, int B, int H, int W, int clamp01, float scale) {
    __shared__ float wl[NO * 576];
    for (int i = threadIdx.x; i < NO * 576; i += 256) wl[i] = (float)w[i];
    __syncthreads();
    const long HW = (long)H * W;
    long p = (long)blockIdx.x * 32 + (threadIdx.x >> 3);
    const bool live = p < (long)B * HW;
    if (!live) p = (long)B * HW - 1;                           // keep the whole wave in the shuffles
    const int sub = threadIdx.x & 7;
    const int b = (int)(p / HW);
    const int rem = (int)(p - (long)b * HW);
    const int y = rem / W, x = rem - y * W;
    float acc[NO];
#pragma unroll
    for (int j = 0; j < NO; ++j) acc[j] = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        const half8 v = ld_global_h8(xin + ((long)b * HW + (long)yy * W + xx) * 64 + sub * 8);
#pragma unroll
        for (int j = 0; j < NO; ++j) {
            const float* wp = wl + j * 576 + tap * 64 + sub * 8;
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[j] = __builtin_fmaf((float)v[i], wp[i], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < NO; ++j)
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
    if (live && sub < NO) {
        float v = acc[0];
#pragma unroll
        for (int j = 1; j < NO; ++j) v = sub == j ? acc[j] : v;
        v += (float)bias[sub];
        if (NO == 3) v = clamp01 ? fminf(fmaxf(v, 0.f), 1.f) : __builtin_fmaf(2.f, v, -1.f);
        else v *= scale;
        out[((long)b * NO + sub) * HW + rem] = (half_t)v;
    }
}

}  // namespace

extern "C" void cid_tiny_conv64_tile(int32_t* tile_h, int32_t* tile_w, int32_t* grid_cap) {
    if (tile_h) *tile_h = TC_TH;
    if (tile_w) *tile_w = TC_TW;
    if (grid_cap) *grid_cap = TC_GRID_CAP;
}

extern "C" int cid_tiny_conv64_f16(const cid_half* x, cid_half* out, const cid_half* w, const cid_half* bias,
                                   const cid_half* res, int32_t B, int32_t H, int32_t W, int32_t up, int32_t relu,
                                   cid_stream_t stream) {
    CID_CHECK_ARG(x && out && w, "cid_tiny_conv64_f16: null pointer");
    CID_CHECK_ARG(B > 0 && H > 0 && W > 0, "cid_tiny_conv64_f16: bad shape (B=%d H=%d W=%d)", B, H, W);
    CID_CHECK_ARG(up == 0 || up == 1, "cid_tiny_conv64_f16: up must be 0 or 1 (got %d)", up);
    CID_CHECK_ARG(relu == 0 || relu == 1, "cid_tiny_conv64_f16: relu must be 0 or 1 (got %d)", relu);
    CID_CHECK_ARG((((uintptr_t)x | (uintptr_t)out | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)res) & 15) == 0,
                  "cid_tiny_conv64_f16: x / out / w / bias / res must be 16-byte aligned");
    CID_CHECK_ARG(x != out && res != out, "cid_tiny_conv64_f16: out must not alias x or res (tiles read their neighbours' halo)");
    const int Ho = up ? 2 * H : H, Wo = up ? 2 * W : W;
    CID_CHECK_ARG((long)B * Ho * Wo * 64 < 0x7fffffffL * 2, "cid_tiny_conv64_f16: tensor exceeds 4 GiB");
    TinyConvArgs a;
    a.x = (const half_t*)x; a.w = (const half_t*)w; a.bias = (const half_t*)bias; a.res = (const half_t*)res;
    a.out = (half_t*)out;
    a.B = B; a.H = Ho; a.W = Wo; a.Hi = H; a.Wi = W; a.up = up; a.relu = relu;
    a.tiles_x = (Wo + TC_TW - 1) / TC_TW;
    a.tiles_y = (Ho + TC_TH - 1) / TC_TH;
    const long nt = (long)B * a.tiles_x * a.tiles_y;
    CID_CHECK_ARG(nt < 0x7fffffffL, "cid_tiny_conv64_f16: too many tiles");
    a.ntiles = (int)nt;
    static bool configured = false;
    if (!configured) {
        hipError_t herr = hipFuncSetAttribute((const void*)tiny_conv64_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TC_SMEM);
        if (herr != hipSuccess) {
            cid_set_error("cid_tiny_conv64_f16: cannot reserve %d bytes of LDS (%s)", TC_SMEM, hipGetErrorString(herr));
            return -5;
        }
        configured = true;
    }
    const int grid = a.ntiles < TC_GRID_CAP ? a.ntiles : TC_GRID_CAP;
    hipLaunchKernelGGL(tiny_conv64_kernel, dim3(grid), dim3(TC_THREADS), TC_SMEM, (hipStream_t)stream, a);
    CID_CHECK_LAUNCH("cid_tiny_conv64_f16");
    return 0;
}

extern "C" int cid_tiny_decode_in_f16(const cid_half* z, cid_half* out, const cid_half* w, const cid_half* bias,
                                      int32_t B, int32_t H, int32_t W, cid_stream_t stream) {
    CID_CHECK_ARG(z && out && w && bias, "cid_tiny_decode_in_f16: null pointer");
    CID_CHECK_ARG(B > 0 && H > 0 && W > 0, "cid_tiny_decode_in_f16: bad shape (B=%d H=%d W=%d)", B, H, W);
    CID_CHECK_ARG((((uintptr_t)out | (uintptr_t)bias) & 15) == 0, "cid_tiny_decode_in_f16: out / bias must be 16-byte aligned");
    const long pix = (long)B * H * W;
    CID_CHECK_ARG(pix < 0x7fffffffL, "cid_tiny_decode_in_f16: too many pixels");
    hipLaunchKernelGGL(tiny_decode_in_kernel, dim3((unsigned)((pix + 31) / 32)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)z, (half_t*)out, (const half_t*)w, (const half_t*)bias, B, H, W);
    CID_CHECK_LAUNCH("cid_tiny_decode_in_f16");
    return 0;
}

extern "C" int cid_tiny_decode_out_f16(const cid_half* x, cid_half* out, const cid_half* w, const cid_half* bias,
                                       int32_t B, int32_t H, int32_t W, int32_t mode, cid_stream_t stream) {
    CID_CHECK_ARG(x && out && w && bias, "cid_tiny_decode_out_f16: null pointer");
    CID_CHECK_ARG(B > 0 && H > 0 && W > 0, "cid_tiny_decode_out_f16: bad shape (B=%d H=%d W=%d)", B, H, W);
    CID_CHECK_ARG(mode == 0 || mode == 1, "cid_tiny_decode_out_f16: mode must be 0 (2x - 1) or 1 (clamp to [0, 1]), got %d", mode);
    CID_CHECK_ARG(((uintptr_t)x & 15) == 0, "cid_tiny_decode_out_f16: x must be 16-byte aligned");
    const long pix = (long)B * H * W;
    CID_CHECK_ARG(pix < 0x7fffffffL, "cid_tiny_decode_out_f16: too many pixels");
    hipLaunchKernelGGL(tiny_out_kernel<3>, dim3((unsigned)((pix + 31) / 32)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)x, (half_t*)out, (const half_t*)w, (const half_t*)bias, B, H, W, mode, 1.f);
    CID_CHECK_LAUNCH("cid_tiny_decode_out_f16");
    return 0;
}

// ---------------------------------------------------------------- encoder entries
extern "C" void cid_tiny_conv64_s2_tile(int32_t* tile_h, int32_t* tile_w, int32_t* grid_cap) {
    if (tile_h) *tile_h = TS_TH;
    if (tile_w) *tile_w = TS_TW;
    if (grid_cap) *grid_cap = TC_GRID_CAP;
}

extern "C" int cid_tiny_conv64_s2_f16(const cid_half* x, cid_half* out, const cid_half* w, int32_t B, int32_t Hi, int32_t Wi,
                                      cid_stream_t stream) {
    CID_CHECK_ARG(x && out && w, "cid_tiny_conv64_s2_f16: null pointer");
    CID_CHECK_ARG(B > 0 && Hi > 0 && Wi > 0, "cid_tiny_conv64_s2_f16: bad shape (B=%d Hi=%d Wi=%d)", B, Hi, Wi);
    CID_CHECK_ARG((((uintptr_t)x | (uintptr_t)out | (uintptr_t)w) & 15) == 0, "cid_tiny_conv64_s2_f16: x / out / w must be 16-byte aligned");
    CID_CHECK_ARG(x != out, "cid_tiny_conv64_s2_f16: out must not alias x (tiles read their neighbours' halo)");
    CID_CHECK_ARG((long)B * Hi * Wi * 64 < 0x7fffffffL * 2, "cid_tiny_conv64_s2_f16: tensor exceeds 4 GiB");
    TinyS2Args a;
    a.x = (const half_t*)x; a.w = (const half_t*)w; a.out = (half_t*)out;
    a.B = B; a.Hi = Hi; a.Wi = Wi; a.Ho = (Hi + 1) / 2; a.Wo = (Wi + 1) / 2;
    a.tiles_x = (a.Wo + TS_TW - 1) / TS_TW;
    a.tiles_y = (a.Ho + TS_TH - 1) / TS_TH;
    const long nt = (long)B * a.tiles_x * a.tiles_y;
    CID_CHECK_ARG(nt < 0x7fffffffL, "cid_tiny_conv64_s2_f16: too many tiles");
    a.ntiles = (int)nt;
    static bool configured = false;
    if (!configured) {
        hipError_t herr = hipFuncSetAttribute((const void*)tiny_conv64_s2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TS_SMEM);
        if (herr != hipSuccess) {
            cid_set_error("cid_tiny_conv64_s2_f16: cannot reserve %d bytes of LDS (%s)", TS_SMEM, hipGetErrorString(herr));
            return -5;
        }
        configured = true;
    }
    const int grid = a.ntiles < TC_GRID_CAP ? a.ntiles : TC_GRID_CAP;
    hipLaunchKernelGGL(tiny_conv64_s2_kernel, dim3(grid), dim3(TC_THREADS), TS_SMEM, (hipStream_t)stream, a);
    CID_CHECK_LAUNCH("cid_tiny_conv64_s2_f16");
    return 0;
}

extern "C" int cid_tiny_encode_in_f16(const float* image, int32_t Bi, const float* mask, int32_t Bm, cid_half* out,
                                      const cid_half* w, const cid_half* bias, int32_t H, int32_t W, int32_t normalize,
                                      int32_t blocks, cid_half* mask_latents, cid_stream_t stream) {
    CID_CHECK_ARG(image && out && w && bias, "cid_tiny_encode_in_f16: null pointer");
    CID_CHECK_ARG(Bi > 0 && H > 0 && W > 0, "cid_tiny_encode_in_f16: bad shape (Bi=%d H=%d W=%d)", Bi, H, W);
    CID_CHECK_ARG(blocks >= 1 && blocks <= 3, "cid_tiny_encode_in_f16: blocks must be 1 (image), 2 (masked image) or 3 (both), got %d",
                  blocks);
    CID_CHECK_ARG(mask || (!(blocks & 2) && !mask_latents), "cid_tiny_encode_in_f16: the masked image and mask_latents need a mask");
    CID_CHECK_ARG(!mask || Bm == 1 || Bm == Bi, "cid_tiny_encode_in_f16: mask batch Bm=%d must be 1 or Bi=%d", Bm, Bi);
    CID_CHECK_ARG(!mask_latents || (H % 8 == 0 && W % 8 == 0),
                  "cid_tiny_encode_in_f16: mask_latents need H and W multiples of 8 (got %d x %d)", H, W);
    CID_CHECK_ARG((((uintptr_t)out | (uintptr_t)bias) & 15) == 0, "cid_tiny_encode_in_f16: out / bias must be 16-byte aligned");
    const long pix = (long)Bi * H * W;
    CID_CHECK_ARG((long)H * W < 0x7fffffffL && pix * ((blocks & 1) + (blocks >> 1)) < 0x7fffffffL, "cid_tiny_encode_in_f16: too many pixels");
    const long nb = (pix + 31) / 32;
    hipLaunchKernelGGL(tiny_encode_in_kernel, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, (hipStream_t)stream,
                       image, mask, (half_t*)out, (const half_t*)w, (const half_t*)bias, (half_t*)mask_latents, Bi, Bm, H, W,
                       normalize != 0, blocks);
    CID_CHECK_LAUNCH("cid_tiny_encode_in_f16");
    return 0;
}

extern "C" int cid_tiny_encode_out_f16(const cid_half* x, cid_half* out, const cid_half* w, const cid_half* bias, int32_t B,
                                       int32_t H, int32_t W, float scale, cid_stream_t stream) {
    CID_CHECK_ARG(x && out && w && bias, "cid_tiny_encode_out_f16: null pointer");
    CID_CHECK_ARG(B > 0 && H > 0 && W > 0, "cid_tiny_encode_out_f16: bad shape (B=%d H=%d W=%d)", B, H, W);
    CID_CHECK_ARG(((uintptr_t)x & 15) == 0, "cid_tiny_encode_out_f16: x must be 16-byte aligned");
    const long pix = (long)B * H * W;
    CID_CHECK_ARG(pix < 0x7fffffffL, "cid_tiny_encode_out_f16: too many pixels");
    hipLaunchKernelGGL(tiny_out_kernel<4>, dim3((unsigned)((pix + 31) / 32)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)x, (half_t*)out, (const half_t*)w, (const half_t*)bias, B, H, W, 0, scale);
    CID_CHECK_LAUNCH("cid_tiny_encode_out_f16");
    return 0;
}

/* cid.h -- C ABI of libcid.so: hand-written HIP kernels (gfx950 / MI355X) for the
 * ConsistentID UNet-denoise hot path.
 *
 * The reference (JackAILab/ConsistentID) has no FFI of its own: its plugin boundary
 * is diffusers' Python attention-processor protocol plus the UNet call signature
 * (SURVEY.md section 8b).  Each entry point below names the reference interface it
 * replaces (file:line relative to /root/reference; "D:" marks diffusers==0.23.0
 * internals that the reference calls but does not vendor).  INTEGRATION.md shows the
 * ctypes binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless it says "host"; fp16 tensors are
 *     IEEE binary16, row-major, token-major ("NHWC": [batch, H*W, C]);
 *   - no allocation, no retained pointers, no host synchronisation inside;
 *     everything is enqueued on `stream` (a hipStream_t) and is graph-capturable;
 *   - return 0 on success, negative errno-style code on failure
 *     (-22 bad argument, -5 launch failure); cid_last_error() gives the text;
 *   - 16-byte alignment is required for every tensor base and row pitch.
 */
#ifndef CID_H
#define CID_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* cid_stream_t;      /* hipStream_t */
typedef uint16_t cid_half;       /* IEEE binary16 bit pattern */

int cid_version(void);          /* 115: cid_attn_colmass_f16, cid_sag_degrade_f16, cid_cfg_sag_ddim_step_f16, cid_cfg_sag_multistep_step_f16, cid_sag_multistep_step_f16 added (self-attention guidance).  114: cid_cfg_pag_ddim_step_f16, cid_cfg_pag_multistep_step_f16, cid_pag_multistep_step_f16 added (perturbed-attention guidance).  113: cid_tiny_encode_in_f16, cid_tiny_conv64_s2_f16, cid_tiny_conv64_s2_tile, cid_tiny_encode_out_f16 added (AutoencoderTiny encoder).  112: cid_tiny_conv64_f16, cid_tiny_decode_in_f16, cid_tiny_decode_out_f16, cid_tiny_conv64_tile added (AutoencoderTiny decoder).  111: cid_multistep_step_f16 added.  110: cid_id_xattn_long_f16, cid_kv_pack_long_f16, cid_kv_pack_long_elems, cid_xattn_long_max_txt added (contexts beyond 96 keys).  109: cid_freeu_f16, cid_freeu_ws_bytes added.  108: cid_cfg_rescale_f16, cid_cfg_ddim_step_scaled_f16, cid_cfg_multistep_step_scaled_f16 added.  107: cid_clip_head_f16, cid_blackout_f16 added.  106: cid_residual_accum_f16.  105: cid_cfg_multistep_step_f16 added.  104: cid_gemm_plan added (host-only query; no struct changed).  103: cid_gemm_desc grew a trailing w_up4
                                 * pointer (102: act, 101: pad_mode; set them or zero the struct) */
const char* cid_last_error(void);

/* ---------------------------------------------------------------------------
 * Implicit GEMM:  out[m][n] = epilogue( sum_k A(m,k) * W[n][k] )
 * Replaces (D:) nn.Linear / nn.Conv2d 1x1 / 3x3 (stride 1|2, pad 1) / nearest-2x
 * upsample + conv, i.e. ResnetBlock2D.conv1/conv2/conv_shortcut, Downsample2D,
 * Upsample2D, Transformer2DModel.proj_in/out, Attention.to_q/to_k/to_v/to_out,
 * FeedForward (GEGLU) -- SURVEY.md 8a rows a5-a9; LoRA of attention.py:139-162,
 * :236-282 is merged into W by the host.
 *   c1 + c2 must be a multiple of 64 (and c1 too when c2 > 0); N a multiple of 32;
 *   row pitches ld1, ld2, ldo multiples of 8 halfs (rows start 16-byte aligned).
 *   A(m, k): k = tap * (c1 + c2) + c ; for taps == 9 the row m = (b, y, x) of the
 *   OUTPUT grid reads input pixel (y*stride + dy - 1, x*stride + dx - 1) of the
 *   (optionally 2x nearest-upsampled) input, zero outside.  Channels [0, c1) come
 *   from x1, [c1, c1 + c2) from x2 (skip concat without a copy).
 *   mode 0: out[m][n] = acc + bias[n] + rowbias[m / rows_per_sample][n] + res[m][n]
 *           (taps == 9, stride 1, up 0|1, N % 160 == 0: ResnetBlock2D.conv1 / conv2 and Upsample2D.conv run on csrc/conv3x3.hip
 *            -- 32 x 32 MFMA tiles, loader / compute wave roles -- wherever its tiles fill the chip unsplit; same arithmetic)
 *   mode 1: GEGLU. W rows are interleaved in blocks of 16 (value block, gate block);
 *           out[m][j] = (val + bias_v) * gelu_erf(gate + bias_g), out width N / 2;
 *           bias is interleaved the same way.
 *   mode 2: fused QKV for self-attention. Columns [0, n_vt0) are written row-major
 *           to out; columns [n_vt0, N) (the V third) are written TRANSPOSED to
 *           vt[b][head][d][pos(token)] (see cid_self_attn_f16).
 *   mode 3: the QUERY projection of the identity cross-attention with the attention as its epilogue
 *           (Consistent_IPAttProcessor.__call__, attention.py:236 `query = attn.to_q(hidden_states) + lora` followed by
 *           :259-279, the two softmaxes over the text and the ID keys): W = the merged to_q weight pre-multiplied by
 *           d^-0.5 * log2(e), N = heads * dhead; out[m][h * dhead + j] = the attention output of head h BEFORE to_out
 *           (what cid_id_xattn_core_f16 writes) -- q never goes to memory.  att_kp / att_vp: the packed K / V^T of
 *           cid_kv_pack_f16, att_kvrow[b] the context row of sample b, ntok tokens per sample (a multiple of 64; of 128 for dhead 64),
 *           the reference's 77 + 4 context, dhead in {64, 80, 160}.  No bias / rowbias / res / split-K; the LayerNorm
 *           fold applies (norm2 in front of to_q).
 */
typedef struct cid_gemm_desc {
    const cid_half* x1; const cid_half* x2;
    int32_t c1, c2, ld1, ld2;
    const cid_half* w;            /* [N][taps * (c1 + c2)] */
    cid_half* out; int32_t ldo;
    const cid_half* bias;         /* [N] or NULL */
    const cid_half* rowbias; int32_t ld_rowbias; int32_t rows_per_sample; /* or NULL */
    const cid_half* res; int32_t ldr;                                      /* or NULL; 16-byte aligned, ldr % 8 == 0 (like out / ldo) */
    int32_t M, N;
    int32_t taps;                 /* 1 or 9 */
    int32_t Hi, Wi, Ho, Wo, stride, up; /* conv geometry (taps == 9) */
    int32_t mode;
    cid_half* vt; int32_t n_vt0, heads, dhead, dvp, ntok; /* mode 2 */
    void* ws; int64_t ws_bytes;   /* optional fp32 scratch for split-K (small M, deep K); NULL => never split */
    /* LayerNorm folded into the projection (D: BasicTransformerBlock.norm1 / norm2 / norm3 in front of
     * Attention.to_q/to_k/to_v, to_q and FeedForward's GEGLU; attention.py:133-147, :236): x1 is the RAW residual stream,
     * W = W0 diag(gamma) rounded to fp16, ln_s[n] = sum_k W[n][k] (fp32, of the rounded W), ln_b[n] = (W0 beta)[n] +
     * bias[n] (fp32); the kernel computes mean / rstd of every row of x1 on the fly and writes
     * rstd * (acc - mean * ln_s[n]) + ln_b[n] through the mode's epilogue.  taps == 1, c2 == 0, bias == NULL. */
    const float* ln_s; const float* ln_b; float ln_eps;   /* both NULL => no LayerNorm */
    /* GroupNorm statistics of `out` for its consumer (D: ResnetBlock2D.norm1 / norm2, Transformer2DModel.norm,
     * conv_norm_out read what a conv / proj_out just wrote): fp32 [M / rows][32][2] = (sum, sum of squares) of the fp16
     * outputs over `rows` consecutive tokens x N / 32 consecutive channels, rows = cid_gemm_stats_rows(d) (> 0 required);
     * consumed by cid_groupnorm_stats_f16.  mode 0 only.  (A launch that runs from w_up4 blocks them by its tiles instead:
     * `rows` outputs of ONE parity of one image, ordered image, parity, tile -- the same sums per sample.) */
    float* gn_stats;
    /* mode 3 */
    const cid_half* att_kp; const cid_half* att_vp; const int32_t* att_kvrow;
    int32_t att_n_txt, att_n_ip; float att_ip_scale;
    /* Second destination (or NULL): every output row is stored to out2 + m * ldo as well -- the CFG `torch.cat([x] * 2)`
     * of a tensor both halves of the batch share (ref pipline_StableDiffusion_ConsistentID.py:537-539) written by its
     * producer instead of by a copy launch.  mode 0 only. */
    cid_half* out2;
    /* Padding of a 3x3 convolution (since cid_version() 101, which grew the struct by this field):
     *   0: symmetric pad 1 (the rule above; a zero-initialised descriptor keeps it);
     *   1: D: Downsample2D(padding=0) of the VAE encoder's DownEncoderBlock2D -- F.pad(x, (0, 1, 0, 1)) then a stride-2 conv
     *      without padding: output (y, x) reads input (2y + dy, 2x + dx), dy, dx in {0, 1, 2}; row Hi and column Wi read as
     *      zero.  Only with mode 0, taps 9, stride 2, up 0, even Hi / Wi, Ho = Hi / 2, Wo = Wi / 2 (else -22); split-K allowed. */
    int32_t pad_mode;
    /* Activation of the plain epilogue (since cid_version() 102, which grew the struct by this field):
     *   0: none (a zero-initialised descriptor keeps it);
     *   1: ReLU after bias + rowbias + res, before the fp16 rounding and the stores (out and out2) -- the ConvBNReLU /
     *      BasicBlock `F.relu(bn(conv(x)) [+ shortcut])` of the face parser (models/BiSeNet/model.py:26-29, resnet.py:36-48,
     *      run once per image by pipline_StableDiffusion_ConsistentID.py:243).  Mode 0 only, without gn_stats, ws
     *      (split-K) or ln_s (else -22); the launch runs on the gather kernels of every tile width. */
    int32_t act;
    /* Folded weights of an Upsample2D convolution (since cid_version() 103, which grew the struct by this field), or NULL:
     * W4[parity][N][tap4][c1] as written by cid_upconv_fold_f16 from w.  After a nearest 2x upsample the three taps along an
     * axis touch two input rows / columns, so the outputs of one parity (Y & 1, X & 1) are a 2x2 convolution of the INPUT
     * image with summed taps: 4/9 of the multiplications.  Only with taps 9, up 1, stride 1, mode 0 and no res (else -22).
     * The launch uses it where csrc/conv3x3.hip can tile the image by parity (N % 160 == 0, one source, no rowbias, whole input
     * rows per tile, enough tiles to fill the chip); every other launch computes from w as if the field were NULL, and with
     * NULL the call is what it was before 103, bit for bit.  The sums are rounded to fp16 once, so the two paths differ by
     * that rounding (relative L2 ~ 1.5e-4).  CID_UPCONV_FOLD=0 in the environment ignores the field (A/B switch). */
    const cid_half* w_up4;
} cid_gemm_desc;
int cid_gemm_f16(const cid_gemm_desc* d, cid_stream_t stream);
/* Token rows per statistics block if cid_gemm_f16(d) can emit gn_stats (its tile height), 0 if it cannot (split-K,
 * tile widths off the 160-channel grid, ragged M): the caller then lets cid_groupnorm_f16 take its own statistics. */
int cid_gemm_stats_rows(const cid_gemm_desc* d);
/* What cid_gemm_f16(d) would launch (since cid_version() 104).  Host code only: it runs the same argument checks and the same
 * plan and kernel choice as the call itself (one function decides both), launches nothing and needs no GPU; pointers are only
 * tested for NULL and alignment.  Returns what cid_gemm_f16 would return before launching (0, or -22 with cid_last_error()). */
enum {
    CID_GEMM_FAMILY_IGEMM = 0,           /* gather kernel (csrc/gemm.hip igemm_kernel) */
    CID_GEMM_FAMILY_IGEMM_HALO = 1,      /* stride-1 3x3 halo kernel (igemm_halo_kernel) */
    CID_GEMM_FAMILY_CONV_H32 = 2,        /* csrc/conv3x3.hip, nine taps */
    CID_GEMM_FAMILY_CONV_H32_PHASE = 3,  /* csrc/conv3x3.hip, four 2x2 phase convolutions from w_up4 */
    CID_GEMM_FAMILY_GEGLU_H32 = 4,       /* csrc/linear_h32.hip */
    CID_GEMM_FAMILY_IGEMM_ATT = 5        /* gather kernel with the attention epilogue (mode 3) */
};
typedef struct cid_gemm_plan_info {
    int32_t family;            /* CID_GEMM_FAMILY_* */
    int32_t bm, bn;            /* tile: token rows x weight rows (mode 1: interleaved value / gate rows) */
    int32_t splitk;            /* K partitions (gridDim.z); > 1 needs ws */
    int32_t nloop;             /* n-tiles walked by one workgroup (GEGLU launches) */
    int32_t nbuf;              /* LDS ring stages of the gather kernels (2 | 3); 0 for the families that fix their own staging */
    int32_t ln, act, vmode;    /* LayerNorm-fold instance; ReLU instance; a second launch writes the transposed V third (mode 2) */
    int32_t splitk_epilogue;   /* the split-K reduction kernel follows the launch */
    int32_t stats_rows;        /* cid_gemm_stats_rows(d): tile height if gn_stats can be emitted, else 0 */
} cid_gemm_plan_info;
int cid_gemm_plan(const cid_gemm_desc* d, cid_gemm_plan_info* out);
/* Fold the packed nine-tap weights w[N][9][C] (tap = 3 ty + tx) of an Upsample2D convolution into w4[4][N][4][C] for
 * cid_gemm_desc.w_up4: parity = 2 py + px, tap4 = 2 ry + rx.  Along y, parity 0 reads input rows (y - 1, y) with taps
 * ({0}, {1, 2}), parity 1 reads rows (y, y + 1) with taps ({0, 1}, {2}); the same along x.  Every entry is the fp32 sum of
 * its 1, 2 or 4 source taps added in the order ty-major, then tx, rounded to fp16 once.  Run once when weights are packed. */
int cid_upconv_fold_f16(const cid_half* w, cid_half* w4, int32_t N, int32_t C, cid_stream_t stream);

/* ---------------------------------------------------------------------------
 * Self-attention core (replaces the softmax(QK^T)V of Consistent_AttProcessor,
 * attention.py:149-159; q/k/v/out projections incl. LoRA are cid_gemm_f16 calls).
 *   q : [B][N][ldq] slice, head h at columns h*d .. ; pre-multiplied by
 *       scale * log2(e) (folded into the merged to_q weight by the host)
 *   k : same layout;  vt : [B][heads][dvp][N] fp16 with the token axis permuted
 *       inside every group of 16:  pos = (t & ~15) | (8*((t>>2)&1) + 4*((t>>3)&1) + (t&3))
 *   out[b][n][h*d + j].   N % 64 == 0;  d in {40, 64, 80, 160}.
 */
int cid_self_attn_f16(const cid_half* q, const cid_half* k, const cid_half* vt, cid_half* out,
                      int32_t B, int32_t N, int32_t heads, int32_t d,
                      int32_t ldq, int32_t ldk, int32_t dvp, int32_t ldo, cid_stream_t stream);
/* Same, with only the first n_keys (<= N) keys of every sample real and the rest padding (scores -inf): token counts
 * that are not a multiple of 64 -- the 257 tokens of the CLIP-ViT-H vision tower whose hidden_states[-2] the reference
 * feeds to ProjPlusModel / FacialEncoder (pipline_StableDiffusion_ConsistentID.py:182-183, :200-201).  Rows beyond n_keys
 * of q / out are computed like any other and are for the caller to ignore.  The padding rows of k may hold any finite
 * values (their scores never enter a maximum or a sum); the padding columns of vt must be finite (they are multiplied by
 * probabilities that are exactly zero). */
int cid_self_attn_keys_f16(const cid_half* q, const cid_half* k, const cid_half* vt, cid_half* out,
                           int32_t B, int32_t N, int32_t heads, int32_t d, int32_t ldq, int32_t ldk,
                           int32_t dvp, int32_t ldo, int32_t n_keys, cid_stream_t stream);
/* Causal form for the CLIP text towers (D: CLIPTextTransformer's causal mask, read by the reference's text_encoder calls
 * pipline_StableDiffusion_ConsistentID.py:467, SDXL :514-521): key j is visible to query i iff j <= i and j < n_keys.
 * Same arguments as cid_self_attn_keys_f16; d == 64 only (CLIP-L 12 x 64, OpenCLIP bigG 20 x 64).  Query rows beyond n_keys
 * come out finite (they see keys 0 .. n_keys - 1) and are for the caller to ignore. */
int cid_self_attn_causal_f16(const cid_half* q, const cid_half* k, const cid_half* vt, cid_half* out,
                             int32_t B, int32_t N, int32_t heads, int32_t d, int32_t ldq, int32_t ldk,
                             int32_t dvp, int32_t ldo, int32_t n_keys, cid_stream_t stream);

/* ---------------------------------------------------------------------------
 * Fused identity cross-attention = Consistent_IPAttProcessor.__call__
 * (attention.py:207-294) with LoRA merged:
 *   q   = LN?(x) Wq'^T                               (:236)
 *   o   = softmax(q Kt^T) Vt + ip_scale * softmax(q Kip^T) Vip   (:259-279)
 *   out = o Wo'^T + bo (+ residual)                  (:282)
 * K/V of both streams come pre-projected and pre-packed (cid_kv_pack_f16) because
 * encoder_hidden_states is step-invariant.  One launch, x read once, out written
 * once.  `kvrow[s]` selects the packed K/V row used by sample s.
 *   x, out, residual : [B][N][C] fp16 (ld = C).  ln_gamma/ln_beta NULL => no LN.
 *   wq, wo  : merged [C][C] weights, row-major ([out][in]); wq additionally
 *             pre-scaled by d^-0.5 * log2(e).
 */
int cid_id_xattn_f16(const cid_half* x, cid_half* out, const cid_half* residual,
                     const cid_half* ln_gamma, const cid_half* ln_beta, float ln_eps,
                     const cid_half* wq, const cid_half* wo, const cid_half* bo,
                     const cid_half* kp, const cid_half* vp, const int32_t* kvrow,
                     int32_t B, int32_t N, int32_t C, int32_t heads,
                     int32_t n_txt, int32_t n_ip, float ip_scale, cid_stream_t stream);
/* Attention core only (same two-stream softmax.V, no projections): q already projected and
 * pre-scaled, out = o.  Used for the 1280-channel levels, where [tokens x C] tiles are too
 * large to keep resident and the projections run as cid_gemm_f16 calls instead. */
int cid_id_xattn_core_f16(const cid_half* q, cid_half* out, const cid_half* kp, const cid_half* vp,
                          const int32_t* kvrow, int32_t B, int32_t N, int32_t C, int32_t heads,
                          int32_t n_txt, int32_t n_ip, float ip_scale, cid_stream_t stream);
/* bytes of one packed K row / V row (per embed row) for (C, heads) */
int64_t cid_kv_pack_elems(int32_t C, int32_t heads, int32_t which /*0=K,1=V*/);
/* kv_txt, kv_ip: [R][L][2C] = [K | V] projections of all L = n_txt + n_ip context
 * rows with the text weights resp. the to_k_ip/to_v_ip weights (attention.py:249-250,
 * :266-269); packs rows < n_txt from kv_txt and rows >= n_txt from kv_ip. */
int cid_kv_pack_f16(const cid_half* kv_txt, const cid_half* kv_ip, cid_half* kp, cid_half* vp,
                    int32_t R, int32_t C, int32_t heads, int32_t n_txt, int32_t n_ip,
                    cid_stream_t stream);
/* [rows][K] fp16 row-major -> MFMA A-fragment order [rows/32][K/16][64 lanes][8]. */
int cid_pack_wfrag_f16(const cid_half* w, cid_half* wp, int32_t rows, int32_t K, cid_stream_t stream);

/* ---------------------------------------------------------------------------
 * Long contexts (csrc/xattn_long.hip, since cid_version() 110): the attention core of cid_id_xattn_core_f16 over
 * 1 <= n_txt <= CID_XATTN_LONG_MAX_TXT text rows and 0 <= n_ip <= CID_XATTN_LONG_MAX_IP ID rows -- weighted / chunked
 * prompts of 77 k rows.  The key axis is walked in 32-slot tiles under an online softmax (fp32), the ID keys sit on a
 * tile of their own behind the last text tile:
 *   out = softmax2(q Kt^T) Vt + ip_scale * softmax2(q Kip^T) Vip        (attention.py:259-279; the ID term is absent for n_ip = 0)
 *   q, out : [B][N][C] fp16 (ld = C), q projected and pre-scaled by d^-0.5 * log2(e); N % 32 == 0;
 *            head width C / heads in {32, 40, 64, 80, 160};  kvrow[s] = packed context row of sample s.
 * Without ID rows (n_ip == 0) the text stream may be CID_XATTN_LONG_MAX_TXT + CID_XATTN_LONG_MAX_IP rows long -- the same
 * 33 key tiles at the most: a ControlNet is handed a pipeline's text AND ID rows as one text stream.
 * Deterministic (no atomics).  Everything else is refused with -22 before any launch. */
#define CID_XATTN_LONG_MAX_TXT 1024
#define CID_XATTN_LONG_MAX_IP 32
int32_t cid_xattn_long_max_txt(void);      /* CID_XATTN_LONG_MAX_TXT of the library that was built */
int cid_id_xattn_long_f16(const cid_half* q, cid_half* out, const cid_half* kp, const cid_half* vp,
                          const int32_t* kvrow, int32_t B, int32_t N, int32_t C, int32_t heads,
                          int32_t n_txt, int32_t n_ip, float ip_scale, cid_stream_t stream);
/* halfs of one packed K row (which = 0) / V^T row (which = 1) of that kernel, per context row; -22 outside the range above.
 * With QKS = ceil(d / 16), DVT = ceil(d / 32), NT = ceil(n_txt / 32), NK = NT + (n_ip > 0):
 *   K   [heads][NK][QKS][64 lanes][8]      lane (idx = lane & 31, hi = lane >> 5), element i: key slot 32 kt + idx,
 *                                          head dim 16 kk + 8 hi + i
 *   V^T [heads][DVT][2 NK][64 lanes][8]    head dim 32 dt + idx, key slot 16 ks + 4 hi + (i & 3) + 8 (i >> 2)
 * Key slot s < 32 NT is text row s (absent for s >= n_txt); slot 32 NT + j is ID row j (absent for j >= n_ip). */
int64_t cid_kv_pack_long_elems(int32_t C, int32_t heads, int32_t n_txt, int32_t n_ip, int32_t which /*0=K,1=V*/);
/* kv_txt, kv_ip as for cid_kv_pack_f16 ([R][L][2C], L = n_txt + n_ip).  Every slot of both images is written; absent
 * key slots and head dims >= d are zero. */
int cid_kv_pack_long_f16(const cid_half* kv_txt, const cid_half* kv_ip, cid_half* kp, cid_half* vp,
                         int32_t R, int32_t C, int32_t heads, int32_t n_txt, int32_t n_ip,
                         cid_stream_t stream);

/* ---------------------------------------------------------------------------
 * Fused identity cross-attention with the BasicTransformerBlock wrapper, ONE launch (csrc/xattn3.hip):
 * Consistent_IPAttProcessor.__call__ (attention.py:207-294) INCLUDING  x + attn2(LayerNorm(x), ehs)
 * (D: diffusers BasicTransformerBlock norm2 / residual; called from pipline_StableDiffusion_ConsistentID.py:552-557
 * through the UNet):
 *   q   = rstd * (x Wq'^T - mean * s) + b'     LayerNorm folded: Wq' = Wq diag(gamma) * d^-0.5 * log2(e)
 *                                              (fp16), s[n] = sum_k Wq'[n][k] (fp32), b' = Wq beta (fp32)
 *   o   = softmax(q Kt^T) Vt + ip_scale * softmax(q Kip^T) Vip            (:259-279)
 *   out = o Wo^T + bo (+ x)                                                (:282)
 * Built for the SD1.5 level-0 geometry (C = 320, 8 heads of 40; cid_id_xattn3_supported tells) with the
 * reference's 77 + 4 context or ControlNet's 81 + 0; N % 64 == 0.  x is read from HBM once, out written once.
 * 64-token tiles, two 4-wave workgroups per CU, weights streamed L2 -> registers in MFMA A-operand order.
 *   q_rowsum, q_bias : fp32 [C] (zeros when there is no LayerNorm);
 *   kp, vp           : context rows in MFMA-fragment order, cid_kv_pack2_elems halfs per row, produced by
 *                      cid_gather_pack_f16 with the host tables of consistentid_amd/xattn_pack.py (key order "reg");
 *   wq_packed, wo_packed : the [C][C] matrices Wq' / Wo re-ordered as [wave 4][k-step 10][row tile 5][lane 64][8]:
 *                          element (wave w, k-step s, tile t, lane l, j) = W[80 w + 16 t + (l & 15)][32 s + 8 (l >> 4) + j]
 *                          (consistentid_amd/xattn_pack.pack_w3; same element count as the plain matrix);
 *   flags            : bit 0 = LayerNorm folded (mean / rstd are computed in-kernel), bit 1 = add x (residual). */
int64_t cid_kv_pack2_elems(int32_t C, int32_t heads, int32_t which /*0=K,1=V*/);
int cid_id_xattn3_supported(int32_t C, int32_t heads, int32_t n_txt, int32_t n_ip);
int cid_id_xattn3_f16(const cid_half* x, cid_half* out, const cid_half* wq_packed, const float* q_rowsum,
                      const float* q_bias, const cid_half* wo_packed, const cid_half* bo, const cid_half* kp,
                      const cid_half* vp, const int32_t* kvrow, int32_t B, int32_t N, int32_t C, int32_t heads,
                      int32_t n_txt, int32_t n_ip, float ip_scale, float ln_eps, int32_t flags,
                      cid_stream_t stream);
/* The same launch with a row pitch for out: ldo halfs (>= C, a multiple of 8); x stays contiguous.  out may be a column
 * block of a wider buffer -- the [M, 5 C] row [ff | h3] that the folded ff2 + proj_out GEMM reads. */
int cid_id_xattn3_ld_f16(const cid_half* x, cid_half* out, int64_t ldo, const cid_half* wq_packed,
                         const float* q_rowsum, const float* q_bias, const cid_half* wo_packed, const cid_half* bo,
                         const cid_half* kp, const cid_half* vp, const int32_t* kvrow, int32_t B, int32_t N,
                         int32_t C, int32_t heads, int32_t n_txt, int32_t n_ip, float ip_scale, float ln_eps,
                         int32_t flags, cid_stream_t stream);
/* dst[r][e] = idx[e] < 0 ? 0 : (bit 30 of idx[e] ? src_b : src_a)[r * src_row_elems + (idx[e] & 0x3fffffff)]
 * for r < R, e < n_idx: the generic "put projected K / V rows into fragment order" step (idx on the device). */
int cid_gather_pack_f16(const cid_half* src_a, const cid_half* src_b, const int32_t* idx, cid_half* dst,
                        int32_t R, int64_t src_row_elems, int64_t n_idx, cid_stream_t stream);

/* ---------------------------------------------------------------------------
 * Normalisation (D: nn.LayerNorm eps 1e-5 in BasicTransformerBlock; nn.GroupNorm
 * 32 groups, eps 1e-5 in ResnetBlock2D / conv_norm_out, 1e-6 in Transformer2DModel),
 * SiLU optionally fused (D: ResnetBlock2D.nonlinearity).  SURVEY.md 8a a5-a7.
 */
int cid_layernorm_f16(const cid_half* x, cid_half* out, const cid_half* gamma, const cid_half* beta,
                      int32_t M, int32_t C, float eps, cid_stream_t stream);
/* The same with row pitches ldx / ldo in halfs (>= C, multiples of 8): x or out may be a column block of a wider buffer. */
int cid_layernorm_ld_f16(const cid_half* x, int64_t ldx, cid_half* out, int64_t ldo, const cid_half* gamma,
                         const cid_half* beta, int32_t M, int32_t C, float eps, cid_stream_t stream);
/* In-place softmax over fp16 rows of BASE-2 logits (fp32 math): replaces the softmax of diffusers' default
 * attention in the VAE mid block (single head of width 512 over all latent pixels), which the reference reaches
 * through self.decode_latents / vae.decode (pipline_StableDiffusion_ConsistentID.py:587,:597).  cols % 8 == 0. */
int cid_softmax_rows_f16(cid_half* x, int32_t rows, int32_t cols, int64_t ld, cid_stream_t stream);

/* x = concat(x1[.., c1], x2[.., c2]) per token; ws: >= cid_groupnorm_ws_bytes() scratch. */
int64_t cid_groupnorm_ws_bytes(int32_t B, int32_t C);
int cid_groupnorm_f16(const cid_half* x1, const cid_half* x2, int32_t c1, int32_t c2,
                      cid_half* out, const cid_half* gamma, const cid_half* beta,
                      int32_t B, int32_t HW, int32_t groups, float eps, int32_t silu,
                      void* ws, cid_stream_t stream);
/* GroupNorm (+ SiLU) whose statistics were emitted by the GEMM epilogue(s) that wrote the input (cid_gemm_desc.gn_stats):
 * ONE launch, x read once -- the statistics pass of cid_groupnorm_f16 is gone.  stats1 / stats2 belong to x1 / x2 (skip
 * concat: two tensors, two producers), rows1 / rows2 = the cid_gemm_stats_rows of their producers; cid_groupnorm_stats_ok
 * tells whether every group is a whole number of c / 32-channel units of one source (it is for every GroupNorm of the
 * SD1.5 / SDXL UNets except the 1280+640 and 640+320 concatenations). */
int cid_groupnorm_stats_ok(int32_t c1, int32_t c2, int32_t groups);
int cid_groupnorm_stats_f16(const cid_half* x1, const cid_half* x2, int32_t c1, int32_t c2,
                            cid_half* out, const cid_half* gamma, const cid_half* beta,
                            int32_t B, int32_t HW, int32_t groups, float eps, int32_t silu,
                            const float* stats1, int32_t rows1, const float* stats2, int32_t rows2,
                            cid_stream_t stream);

/* ---------------------------------------------------------------------------
 * fp32 kernels of the SDXL VAE decode.  The reference upcasts that VAE to float32 before decoding
 * (pipline_StableDiffusionXL_ConsistentID.py:670-676: upcast_vae(), vae.decode(latents / scaling_factor)); these
 * three entry points are the fp32 counterparts of cid_gemm_f16 / cid_groupnorm_f16 / cid_softmax_rows_f16 that the
 * fp32 decoder engine (consistentid_amd/vae.py::HipVAEDecoderF32) is built on.  All tensors fp32, token-major.
 *   cid_gemm_f32: out[m][n] = sum_k A(m,k) W[n][k] + bias[n] + res[m][n], k = tap * c + ch; taps 1 (Linear / 1x1) or
 *     9 (3x3, stride 1, pad 1, `up` = input nearest-upsampled 2x first: Ho = Hi << up); exact f32 accumulation on
 *     v_mfma_f32_32x32x2_f32.  ldx % 4 == 0 when c % 4 == 0.
 *   cid_groupnorm_f32: GroupNorm over [B][HW][C] (+ SiLU); ws >= cid_groupnorm_f32_ws_bytes(B, HW, C).
 *   cid_softmax_rows_f32: in place, base-2 logits. */
int cid_gemm_f32(const float* x, const float* w, const float* bias, const float* res, float* out,
                 int32_t M, int32_t N, int32_t c, int32_t taps, int32_t ldx, int32_t ldo, int32_t ldr,
                 int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t up, cid_stream_t stream);
int64_t cid_groupnorm_f32_ws_bytes(int32_t B, int32_t HW, int32_t C);
int cid_groupnorm_f32(const float* x, float* out, const float* gamma, const float* beta, int32_t B, int32_t HW,
                      int32_t C, int32_t groups, float eps, int32_t silu, void* ws, cid_stream_t stream);
int cid_softmax_rows_f32(float* x, int32_t rows, int32_t cols, int64_t ld, cid_stream_t stream);

/* ---------------------------------------------------------------------------
 * UNet ends (D: UNet2DConditionModel.conv_in / conv_out), HBM-bound direct kernels.
 * conv_in : sample NCHW fp16 [Bin][cin][H][W] -> token-major [B][H*W][cout];
 *           batch b reads sample (b % Bin)  (the CFG torch.cat([latents]*2),
 *           pipline_StableDiffusion_ConsistentID.py:537-539, without the copy);
 *           B % Bin == 0: rows that share a sample are computed once and stored B / Bin times.
 *           w: [cout][9][cin], bias [cout]; cin <= 9, cout % 8 == 0, cout <= 320.
 * conv_out: token-major [B][H*W][cin] -> NCHW fp16 [B][cout<=4][H][W]; w [cout][9][cin].
 */
int cid_conv_in_f16(const cid_half* sample, cid_half* out, const cid_half* w, const cid_half* bias,
                    int32_t B, int32_t Bin, int32_t cin, int32_t H, int32_t W, int32_t cout,
                    const float* in_scale /* device scalar multiplying the sample (scheduler.scale_model_input,
                                             pipline_StableDiffusion_ConsistentID.py:540), or NULL */,
                    cid_stream_t stream);
/* conv_in of a 9-channel inpainting UNet: input channels [0, cin1) from `sample` (latents, scaled by in_scale), channels
 * [cin1, cin1 + cin2) from `extra` (cat([mask, masked_image_latents]) NCHW [Bin][cin2][H][W], NOT scaled) -- the
 * torch.cat([latent_model_input, mask, masked_image_latents], dim=1) of
 * pipelines/StableDIffusionInpaint_ConsistentID.py:320-321 and StableDIffusionControlNetInpaint_ConsistentID.py:415-416
 * without materialising it.  w: [cout][9][cin1 + cin2]. */
int cid_conv_in_cat_f16(const cid_half* sample, int32_t cin1, const cid_half* extra, int32_t cin2, cid_half* out,
                        const cid_half* w, const cid_half* bias, int32_t B, int32_t Bin, int32_t H, int32_t W,
                        int32_t cout, const float* in_scale, cid_stream_t stream);
/* Small-channel 3x3 convolution (pad 1, stride 1 or 2, optional SiLU), token-major in and out; w [cout][9][cin].
 * Replaces the nn.Conv2d + F.silu chain of diffusers' ControlNetConditioningEmbedding (3 -> 16 -> ... -> 256 -> C0)
 * that the reference reaches through self.controlnet(..., controlnet_cond=control_image, ...)
 * (pipelines/StableDIffusionControlNetInpaint_ConsistentID.py:405-412).  cout % 8 == 0; any cin. */
int cid_conv3x3_small_f16(const cid_half* x, cid_half* out, const cid_half* w, const cid_half* bias,
                          int32_t B, int32_t Hi, int32_t Wi, int32_t cin, int32_t cout, int32_t stride,
                          int32_t silu, cid_stream_t stream);
/* Identity-conditioning stack (once per image; ProjPlusModel functions.py:490-522, FacialEncoder attention.py:72-88):
 * its Linears / LayerNorms are cid_gemm_f16 / cid_layernorm_f16; these two fill the gaps.
 *   cid_gelu_f16        in-place exact-erf GELU (nn.GELU(), functions.py:395,:499, attention.py:58); n % 8 == 0
 *   cid_small_attn_f16  PerceiverAttention core (functions.py:439-447): Lq latent queries per sample attend to the keys of
 *                       two row blocks (n1 image tokens, n2 latents: the torch.cat of :433 without the copy); a key row is
 *                       [K | V] as produced by to_kv (:434); out = softmax(scale2 * q k^T) v, head width 64,
 *                       n1 + n2 <= 1024.  q [B*Lq][ldq], kv* [B*n*][ldkv], out [B*Lq][ldo].
 *                       Refused (-EINVAL): ldq or ldo < heads * 64, ldkv < 2 * heads * 64 (V is read at row + heads * 64). */
int cid_gelu_f16(cid_half* x, int64_t n, cid_stream_t stream);
int cid_small_attn_f16(const cid_half* q, int32_t ldq, const cid_half* kv1, int32_t n1, const cid_half* kv2, int32_t n2,
                       int32_t ldkv, cid_half* out, int32_t ldo, int32_t B, int32_t Lq, int32_t heads, int32_t dim_head,
                       float scale2, cid_stream_t stream);
int cid_conv_out_f16(const cid_half* x, cid_half* out, const cid_half* w, const cid_half* bias,
                     int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout, cid_stream_t stream);

/* ---------------------------------------------------------------------------
 * CLIP text towers (once per prompt; the reference's text_encoder / text_encoder_2 calls,
 * pipline_StableDiffusion_ConsistentID.py:467-501, SDXL :514-565, through D: CLIPTextModel / CLIPTextModelWithProjection).
 * Their LayerNorms, projections and MLP are cid_layernorm_f16 / cid_gemm_f16 / cid_linear_small_f16, their attention is
 * cid_self_attn_causal_f16; these two fill the gaps.
 *   cid_quick_gelu_f16  in place x * sigmoid(1.702 x) (D: QuickGELUActivation, hidden_act "quick_gelu" of CLIP-L), fp32 math;
 *                       every finite input gives a finite result (-0 or x where exp overflows).  n % 8 == 0
 *   cid_text_embed_f16  out[b][t] = tok[ids[b][t]] + pos[t] for t < T, zero rows for T <= t < Tp (D: CLIPTextEmbeddings).
 *                       ids int32 [B][T]; tok [V][C], pos [>= T][C], out [B][Tp][C]; C % 8 == 0.  The caller checks
 *                       0 <= id < V on the host (the Python engine raises ValueError); an id outside that range reads
 *                       nothing and gives a zero token row. */
int cid_quick_gelu_f16(cid_half* x, int64_t n, cid_stream_t stream);
int cid_text_embed_f16(const int32_t* ids, int32_t B, int32_t T, int32_t Tp, const cid_half* tok, const cid_half* pos,
                       cid_half* out, int32_t V, int32_t C, cid_stream_t stream);

/* ---------------------------------------------------------------------------
 * Safety checker tail (csrc/safety.hip).  The three SD1.5-family pipelines call run_safety_checker between the VAE decode and
 * the PIL conversion (pipline_StableDiffusion_ConsistentID.py:584-602, pipelines/StableDIffusionInpaint_ConsistentID.py:371-381,
 * pipelines/StableDIffusionControlNetInpaint_ConsistentID.py:468-478) -> D: StableDiffusionSafetyChecker.forward.  The CLIP
 * ViT-L/14 tower runs on the vision engine's launches (quick GELU); these two are what follows its last encoder layer.
 * cid_clip_head_f16: D: CLIPVisionTransformer.post_layernorm on the CLS token, CLIPVisionModelWithProjection.visual_projection,
 *   D: cosine_distance against the concept tables and the threshold loop of the checker, for B images in ONE launch (one
 *   256-thread workgroup per image).  All arithmetic fp32:
 *     ln = LayerNorm(x[b]) (gain / bias ln_gamma / ln_beta fp16 [C], ln_eps);  e = w_proj ln  (w_proj fp16 [P][C], no bias);
 *     embeds[b] = fp16(e)  (image_embeds, not normalised; the one rounding);  cos[b][k] = (e / max(|e|, 1e-12)) . concepts[k];
 *     adj = 0;  for k in index order:  scores[b][k] = (cos[b][k] - thresholds[k]) + adj;  hit = rintf(scores * 1000.f) >= 1.f
 *     (Python's round(np.float32, 3) > 0, half to even);  a hit at k < n_special sets adj = 0.01f for every LATER k and does
 *     not flag;  flags[b] = any hit at k >= n_special.
 *   x: row b at x + b * ldx halfs -- token 0 of a padded [B][Np][C] state with ldx = Np * C.  concepts: fp32 [K][P], rows
 *   L2-normalised by the caller, the n_special special-care rows FIRST; thresholds fp32 [K] in the same order.  cos / scores fp32
 *   [B][K], flags int32 [B]; embeds fp16 [B][P] or NULL.  K == 0 (concepts, thresholds, cos, scores, flags NULL) writes only
 *   embeds.  Refused (-22): a NULL required pointer; C, P or ldx not a multiple of 8; C or P > 4096; ldx < C; K outside [0, 64];
 *   n_special outside [0, K]; B <= 0; x / ln_gamma / ln_beta / w_proj not 16-byte aligned.
 * cid_blackout_f16: `images[idx] = torch.zeros_like(images[idx])` of the checker for every flagged image, reading the flags on
 *   the device: images fp16 [B][per_image], image b zeroed where flags[b] != 0, the others not written.  Any per_image >= 1
 *   (16-byte stores when per_image % 8 == 0 and the base is 16-byte aligned, 2-byte stores otherwise); B <= 65535. */
int cid_clip_head_f16(const cid_half* x, int64_t ldx, const cid_half* ln_gamma, const cid_half* ln_beta, float ln_eps,
                      const cid_half* w_proj, const float* concepts, const float* thresholds, int32_t B, int32_t C, int32_t P,
                      int32_t K, int32_t n_special, cid_half* embeds, float* cos, float* scores, int32_t* flags,
                      cid_stream_t stream);
int cid_blackout_f16(cid_half* images, const int32_t* flags, int32_t B, int64_t per_image, cid_stream_t stream);

/* ---------------------------------------------------------------------------
 * VAE encoder ends (csrc/vae_enc.hip).  The inpaint pipelines encode the init image and the masked image before the loop
 * (pipelines/StableDIffusionInpaint_ConsistentID.py:231-295, StableDIffusionControlNetInpaint_ConsistentID.py:254-356:
 * mask_processor binarisation, masked_image = init_image * (mask < 0.5), then D: prepare_latents / prepare_mask_latents ->
 * AutoencoderKL.encode(...).latent_dist.sample(generator) * scaling_factor and F.interpolate(mask, size=(H / 8, W / 8))).
 * Between these two entries the encoder runs on cid_gemm_f16 (Downsample2D(padding=0): pad_mode 1) / cid_groupnorm_f16 /
 * cid_softmax_rows_f16.
 * cid_vae_encode_in_f16: D: Encoder.conv_in (3 -> cout, 3x3 pad 1) with the pre-processing folded into its loads.
 *   image fp32 NCHW [Bi][3][H][W]; mask fp32 NCHW [Bm][1][H][W], Bm in {1, Bi}, or NULL; normalize != 0: pixel = 2x - 1
 *   (the diffusers rule for [0, 1] tensors); the masked image is pixel * (mask < 0.5); every pixel is rounded to fp16 after
 *   normalisation and masking (the reference feeds an fp16 VAE).  blocks: bit 0 the image, bit 1 the masked image (needs the
 *   mask).  out: token-major fp16 [nblk * Bi][H * W][cout], the image block first; w [cout][9][3], bias [cout];
 *   cout % 8 == 0, cout <= 320.  mask_latents (or NULL; needs the mask, H % 8 == 0, W % 8 == 0): fp16 NCHW [Bm][1][H/8][W/8]
 *   = the binarised mask at (8y, 8x), i.e. F.interpolate(mask >= 0.5, size=(H / 8, W / 8)) (nearest, diffusers
 *   prepare_mask_latents).
 * cid_vae_encode_out_f16: D: Encoder.conv_out + AutoencoderKL.quant_conv + DiagonalGaussianDistribution.sample / .mode.
 *   x token-major fp16 [B][H * W][cin] = SiLU(conv_norm_out(mid)); w [2L][9][cin] fp16 = quant_conv folded into conv_out
 *   (W' = Q W per tap, computed in fp32 and rounded once), bias fp32 [2L] = Q b + q_b; eps fp16 NCHW [B][L][H][W] (the
 *   randn_tensor draw of sample(generator)) or NULL for the mode; out fp16 NCHW [B][L][H][W] =
 *   scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps); moments fp32 NCHW [B][2L][H][W] (mean | logvar before the
 *   clamp, the `parameters` of the distribution) or NULL.  L <= 4, cin % 8 == 0. */
int cid_vae_encode_in_f16(const float* image, int32_t Bi, const float* mask, int32_t Bm, cid_half* out, const cid_half* w,
                          const cid_half* bias, int32_t H, int32_t W, int32_t cout, int32_t normalize, int32_t blocks,
                          cid_half* mask_latents, cid_stream_t stream);
int cid_vae_encode_out_f16(const cid_half* x, cid_half* out, float* moments, const cid_half* w, const float* bias,
                           const cid_half* eps, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t L, float scale,
                           cid_stream_t stream);

/* ---------------------------------------------------------------------------
 * AutoencoderTiny decoder (csrc/taesd.hip, since cid_version() 112).  D: diffusers 0.23 AutoencoderTiny.decode ->
 * vae.DecoderTiny (TAESD / taesdxl), the decoder diffusers documents beside LCM: `tanh(z / 3) * 3`, conv 4 -> 64 + ReLU,
 * AutoencoderTinyBlock x n / nearest 2x / bias-less conv per level, conv 64 -> 3, then `mul(2).sub(1)`.  64 channels
 * everywhere, ReLU, no normalisation, no attention.  All three entries: 3x3, pad 1, stride 1, zeros outside the image, fp32
 * accumulation, one rounding to fp16 at the store; weights [cout][9][cin] (tap = 3 ky + kx); deterministic (no atomics, no
 * split-K, a fixed contraction order); any H, W >= 1.
 * cid_tiny_conv64_f16: the 64 -> 64 body convolution, weight-stationary.  x token-major [B][H * W][64]; out token-major
 *   [B][Ho * Wo][64] with (Ho, Wo) = (H, W), or (2H, 2W) with up = 1: the input is then read through a nearest 2x upsample
 *   (output (y, x) reads input (y >> 1, x >> 1)) that is never materialised.  out = act(acc + bias + res): bias [64] or NULL,
 *   res token-major [B][Ho * Wo][64] or NULL (added BEFORE the activation), relu 0 | 1.  The whole 72 KiB weight is staged in
 *   LDS once per workgroup; an output tile is tile_h x tile_w pixels (cid_tiny_conv64_tile) staged with a one-pixel halo,
 *   ragged at the right and bottom edges; the launch has at most grid_cap workgroups, which loop over the tiles.
 *   Refused (-22): a NULL x / out / w; B, H or W <= 0; up or relu outside {0, 1}; a pointer that is not 16-byte aligned;
 *   out == x or out == res (a tile reads its neighbours' pixels); B * Ho * Wo * 64 >= 2^32 - 2 output elements.
 * cid_tiny_decode_in_f16: z NCHW fp16 [B][4][H][W] (the latents as the denoise loop leaves them) -> relu(conv(tanh(z / 3) * 3)
 *   + bias), token-major [B][H * W][64]; w [64][9][4], bias [64].  tanh is evaluated in fp32 and is finite for every finite
 *   fp16 input (|z| = 65504 gives exactly 3).  out / bias 16-byte aligned.
 * cid_tiny_decode_out_f16: x token-major [B][H * W][64] -> v = conv(x) + bias (w [3][9][64], bias [3]); out NCHW fp16
 *   [B][3][H][W] = 2 v - 1 (mode 0: what AutoencoderTiny.decode returns, in [-1, 1]) or clamp(v, 0, 1) (mode 1: the
 *   `(image / 2 + 0.5).clamp(0, 1)` of StableDiffusionPipeline.decode_latents applied to 2 v - 1, without the extra pass). */
void cid_tiny_conv64_tile(int32_t* tile_h, int32_t* tile_w, int32_t* grid_cap);    /* host query; any pointer may be NULL */
int cid_tiny_conv64_f16(const cid_half* x, cid_half* out, const cid_half* w, const cid_half* bias, const cid_half* res,
                        int32_t B, int32_t H, int32_t W, int32_t up, int32_t relu, cid_stream_t stream);
int cid_tiny_decode_in_f16(const cid_half* z, cid_half* out, const cid_half* w, const cid_half* bias, int32_t B, int32_t H,
                           int32_t W, cid_stream_t stream);
int cid_tiny_decode_out_f16(const cid_half* x, cid_half* out, const cid_half* w, const cid_half* bias, int32_t B, int32_t H,
                            int32_t W, int32_t mode, cid_stream_t stream);

/* ---------------------------------------------------------------------------
 * AutoencoderTiny encoder (csrc/taesd.hip, since cid_version() 113).  D: diffusers 0.23 AutoencoderTiny.encode ->
 * vae.EncoderTiny: `x.add(1).div(2)`, conv 3 -> 64 (no activation), then per level a stride-2 bias-less conv (from the second
 * level on) and AutoencoderTinyBlock x n, conv 64 -> 4.  The Blocks are cid_tiny_conv64_f16 launches; the three entries below
 * are the rest.  fp32 accumulation, one rounding to fp16 at the store, weights [cout][9][cin] (tap = 3 ky + kx),
 * deterministic, any H, W >= 1.
 * cid_tiny_encode_in_f16: the arguments of cid_vae_encode_in_f16 (image fp32 NCHW [Bi][3][H][W]; mask fp32 [Bm][1][H][W], Bm in
 *   {1, Bi}, or NULL; blocks bit 0 = the image, bit 1 = the masked image; out token-major [nblk * Bi][H * W][64], the image
 *   block first; mask_latents fp16 [Bm][1][H / 8][W / 8] = the binarised mask at every 8th pixel, or NULL -- only with H and W
 *   multiples of 8).  Per pixel, in this order: v = half(normalize ? 2x - 1 : x); the masked image is v * (mask < 0.5);
 *   u = half(v + 1) / 2 (one fp16 rounding, of v + 1); conv 3 -> 64 + bias over u with ZERO padding of u (a tap outside the
 *   image is 0 in [0, 1] space, i.e. -1 in image space; a masked pixel is u = 0.5); no activation.  w [64][9][3], bias [64].
 * cid_tiny_conv64_s2_f16: the stride-2, pad-1, bias-less 64 -> 64 convolution.  x token-major [B][Hi * Wi][64]; out token-major
 *   [B][Ho * Wo][64] with Ho = ceil(Hi / 2), Wo = ceil(Wi / 2); output (y, x) reads input (2y - 1 + dy, 2x - 1 + dx), zeros
 *   outside on all four sides (NOT cid_gemm_desc.pad_mode 1).  Weight-stationary like cid_tiny_conv64_f16: one workgroup owns
 *   an output tile of tile_h x tile_w pixels (cid_tiny_conv64_s2_tile), at most grid_cap workgroups loop over the tiles.
 *   Refused (-22): a NULL or misaligned pointer, B, Hi or Wi <= 0, out == x, B * Hi * Wi * 64 >= 2^32 - 2 input elements.
 * cid_tiny_encode_out_f16: x token-major [B][H * W][64] -> (conv(x) + bias) * scale (w [4][9][64], bias [4]), out NCHW fp16
 *   [B][4][H][W]; scale = the config's scaling_factor (1.0 for what AutoencoderTiny.encode returns). */
void cid_tiny_conv64_s2_tile(int32_t* tile_h, int32_t* tile_w, int32_t* grid_cap);  /* host query; any pointer may be NULL */
int cid_tiny_conv64_s2_f16(const cid_half* x, cid_half* out, const cid_half* w, int32_t B, int32_t Hi, int32_t Wi,
                           cid_stream_t stream);
int cid_tiny_encode_in_f16(const float* image, int32_t Bi, const float* mask, int32_t Bm, cid_half* out, const cid_half* w,
                           const cid_half* bias, int32_t H, int32_t W, int32_t normalize, int32_t blocks,
                           cid_half* mask_latents, cid_stream_t stream);
int cid_tiny_encode_out_f16(const cid_half* x, cid_half* out, const cid_half* w, const cid_half* bias, int32_t B, int32_t H,
                            int32_t W, float scale, cid_stream_t stream);

/* ---------------------------------------------------------------------------
 * Face parser (csrc/parsing.hip): BiSeNet (models/BiSeNet/model.py:230-254, resnet.py:58-80) as the reference runs it, once
 * per reference image: `self.bise_net(img)[0]` on a 512 x 512 resize (pipline_StableDiffusion_ConsistentID.py:229-244).
 * Its convolutions are cid_gemm_f16 calls (BatchNorm folded into W and bias on the host, ReLU = cid_gemm_desc.act 1; the
 * 1x1 stride-2 shortcut is a taps-9 stride-2 conv whose weight is zero outside the centre tap); these fill the gaps.
 *   cid_parse_stem_f16  resnet.py:72-74 with ToTensor + Normalize((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)) of
 *                       :231-234 in front: img uint8 NHWC [B][H][W][3] -> (x / 255 - mean) / std -> conv 7x7 / 2 pad 3
 *                       (zero padding of the normalised image; w fp32 [64][7][7][3] = [out][ky][kx][rgb], BN folded;
 *                       bias fp32 [64]) -> ReLU -> maxpool 3x3 / 2 pad 1 -> token-major fp16 [B][(H / 4) (W / 4)][64].
 *                       H, W multiples of 32; 1 <= B <= 16383 (four workgroup layers per image).
 *   cid_chan_mean_f16   F.avg_pool2d(x, x.size()[2:]) (model.py:78, :111, :203): out fp32 [B][C] = mean over the HW tokens
 *                       of x [B][HW][ld] (first C channels); C % 8 == 0, ld % 8 == 0.
 *   cid_chan_gate_f32   the 1x1 convolutions on those means, one launch: y = W1 m (+ b1) (W1 fp32 [N1][K]); with w2:
 *                       y = W2 ReLU(y) (+ b2) (W2 fp32 [N][N1], FFM conv1 / relu / conv2, model.py:204-206); then
 *                       act 0 none, 1 ReLU (conv_avg, :112), 2 sigmoid (ARM conv_atten / bn_atten, :79-81; FFM :207).
 *                       out fp32 [B][N]; K, N1, N <= 512; N == N1 without w2.
 *   cid_chan_affine_f16 out[b][p][c] = x[b][p][c] * s[b][c] + add, add = t[b][c] (fp32 [B][C], ARM32 + conv_avg: :82,
 *                       :115), res[b][p][c] (ARM16 + feat32_up: :120) or x itself when both are NULL (FFM :208-209);
 *                       fp32 math, rounded once; [B][HW][C] contiguous, C % 8 == 0; out may be x.
 *   cid_parse_head_f16  F.interpolate(logits, (H, W), mode='bilinear', align_corners=True) (model.py:251) in fp32, then
 *                       the first-maximum argmax over the classes (numpy's `.argmax(0)`, :244 of the pipeline): logits
 *                       fp16 [B][h * w][ld] (the first ncls channels), labels uint8 [B][H][W]; logits_out (or NULL) fp32
 *                       NCHW [B][ncls][H][W], the upsampled logits (the reference's `out`).  ncls <= min(ld, 256). */
int cid_parse_stem_f16(const uint8_t* img, cid_half* out, const float* w, const float* bias, int32_t B, int32_t H, int32_t W,
                       cid_stream_t stream);
int cid_chan_mean_f16(const cid_half* x, float* out, int32_t B, int32_t HW, int32_t C, int32_t ld, cid_stream_t stream);
int cid_chan_gate_f32(const float* mean, float* out, const float* w1, const float* b1, const float* w2, const float* b2,
                      int32_t B, int32_t K, int32_t N1, int32_t N, int32_t act, cid_stream_t stream);
int cid_chan_affine_f16(const cid_half* x, const float* s, const float* t, const cid_half* res, cid_half* out, int32_t B,
                        int32_t HW, int32_t C, cid_stream_t stream);
int cid_parse_head_f16(const cid_half* logits, int32_t ld, int32_t ncls, int32_t B, int32_t h, int32_t w, int32_t H,
                       int32_t W, uint8_t* labels, float* logits_out, cid_stream_t stream);

/* ---------------------------------------------------------------------------
 * Timestep path (D: get_timestep_embedding flip_sin_to_cos, TimestepEmbedding,
 * ResnetBlock2D.time_emb_proj).  SURVEY.md 8a a4.
 * cid_sincos_embed: out[r][0:dim/2] = cos(v[r] * f_i), out[r][dim/2:] = sin(..),
 *                   f_i = exp(-ln(10000) * i / (dim/2)); v is a DEVICE fp32 array.
 * cid_linear_small: out[m][n] = act_out( sum_k act_in(x[m][k]) W[n][k] + b[n] (+ add[m][n]) )
 *                   for M <= 32 rows; act: 0 none, 1 SiLU.
 *                   Refused (-EINVAL): ldx < K, ldo < N, ldadd neither 0 (one row for every m) nor >= N.
 */
int cid_sincos_embed_f16(const float* v, cid_half* out, int32_t rows, int32_t dim, cid_stream_t stream);
int cid_linear_small_f16(const cid_half* x, int32_t ldx, const cid_half* w, const cid_half* b,
                         const cid_half* add, int32_t ldadd, cid_half* out, int32_t ldo,
                         int32_t M, int32_t N, int32_t K, int32_t act_in, int32_t act_out,
                         cid_stream_t stream);

/* ---------------------------------------------------------------------------
 * Loop glue (pipline_StableDiffusion_ConsistentID.py:561-571; D: DDIMScheduler.step,
 * eta = 0):  eps = eps_u + g (eps_c - eps_u);
 *            x_prev = c_x * x + c_eps * eps   with c_x = sqrt(a_prev)/sqrt(a_t),
 *            c_eps = sqrt(1-a_prev) - sqrt(a_prev) sqrt(1-a_t)/sqrt(a_t).
 * eps: [2B][...] (uncond first), latents [B][...] updated in place.  coef: DEVICE
 * fp32 {c_x, c_eps} so the launch is graph-replayable across timesteps.
 * Optional inpaint blend (pipelines/StableDIffusionControlNetInpaint_ConsistentID.py:
 * 437-449): latents = (1-m) * (c_init*init + c_noise*noise) + m * latents, with
 * coef[2], coef[3] = {c_init, c_noise}; mask/init/noise NULL => skipped.
 */
int cid_cfg_ddim_step_f16(const cid_half* eps, cid_half* latents, const float* coef, float guidance,
                          const cid_half* mask, const cid_half* init, const cid_half* noise,
                          int32_t B, int32_t per_sample, cid_stream_t stream);
/* CFG + one step of a linear multistep sampler: PNDM (skip_prk_steps), DPM-Solver++ 2M, DDIM with eta > 0
 * (consistentid_amd/scheduler.py computes the rows).  eps [2B][per_sample] (uncond first); latents [B][per_sample],
 * updated in place; hist: fp32 ring [4][B * per_sample] of earlier model outputs; saved: fp16 [B * per_sample], the
 * sample PNDM's second evaluation steps from again; z: fp16 [z_rows][B * per_sample] pre-drawn noise or NULL (z_rows 0).
 * row: DEVICE, sixteen 4-byte words (cid_step_select fills it), the "multistep row":
 *    f0 a   f1 b           m = a * x + b * e,  e = eps_u + g (eps_c - eps_u),  x = latents as they come in
 *    f2 c_x f3 c_m         coefficient of the source sample / of m
 *    f4..f7 c_hist[0..3]   coefficient of ring slot 0..3 as it is BEFORE this launch (absolute slots: the host permutes)
 *    f8 c_in               model-input scale: conv_in reads this word through a 16-byte-aligned view, which is why it
 *                          sits here; 1.0 for these samplers, not used by this kernel
 *    f9 c_init f10 c_noise inpaint blend of the NEXT timestep, as in cid_cfg_ddim_step_f16
 *    f11 c_z               coefficient of z[z_row]
 *    i12 w                 ring slot that receives m (written after the reads), none unless 0 <= w < 4
 *    i13 flags             bit0: copy x into `saved`;  bit1: the source sample is `saved` (as it is before this launch), else x
 *    i14 z_row             clamped to [0, z_rows)        i15 0
 *    x' = c_x * src + c_m * m + sum_s c_hist[s] * hist[s] + c_z * z[z_row];
 *    latents = mask ? (1 - mask) * (c_init * init + c_noise * noise) + mask * x' : x'
 * A ring slot with c_hist[s] == 0, z with c_z == 0 and `saved` with bit1 clear are NOT read (they may hold anything, NaN
 * included).  fp32 arithmetic, one rounding to fp16 at the store of latents; hist keeps m in fp32.
 * B * per_sample % 8 == 0; every buffer 16-byte aligned; mask/init/noise come together or not at all. */
int cid_cfg_multistep_step_f16(const cid_half* eps, cid_half* latents, float* hist, cid_half* saved,
                               const cid_half* z, int32_t z_rows, const void* row, float guidance,
                               const cid_half* mask, const cid_half* init, const cid_half* noise,
                               int32_t B, int32_t per_sample, cid_stream_t stream);
/* The single pass (since cid_version() 111): one step of the same row contract WITHOUT classifier-free guidance.
 * eps [B][per_sample] holds ONE model output per sample and e = eps; nothing behind eps + B * per_sample is read.  Every
 * other argument, the multistep row, the ring, `saved`, z and the inpaint blend are cid_cfg_multistep_step_f16's; with
 * eps_u == eps_c that entry gives the same bits at every guidance value (u + g (u - u) is u).  consistentid_amd/scheduler.py
 * LCMScheduler at guidance_scale <= 1 steps with it.
 * -22 before any launch: a null eps / latents / hist / saved / row, z without z_rows or z_rows without z, mask / init / noise
 * not all or none, B <= 0, per_sample <= 0, B * per_sample % 8 != 0, a buffer that is not 16-byte aligned. */
int cid_multistep_step_f16(const cid_half* eps, cid_half* latents, float* hist, cid_half* saved,
                           const cid_half* z, int32_t z_rows, const void* row,
                           const cid_half* mask, const cid_half* init, const cid_half* noise,
                           int32_t B, int32_t per_sample, cid_stream_t stream);
/* guidance_rescale ("Common Diffusion Noise Schedules and Sample Steps Are Flawed", section 3.4; diffusers 0.23
 * rescale_noise_cfg, applied between the CFG combine and scheduler.step): the per-sample factor of the guided prediction.
 * eps: fp16 [2B][per_sample], unconditional half first -- what the step kernels read.  escale: DEVICE fp32 [B], written:
 *    c = eps[B + b],  e = u + g (c - u) in fp32, the step kernels' own expression,
 *    escale[b] = 1 - rescale + rescale * std(c) / std(e)        (both over the whole sample; their N - 1 cancels)
 * so that e * escale[b] = rescale * (e * std(c) / std(e)) + (1 - rescale) * e.  DEVIATION: where std(e) == 0 (a constant
 * prediction) escale[b] = 1.0; diffusers divides by zero there and hands NaN to the scheduler.
 * One launch, one 1024-thread workgroup per sample, nothing on the host and no allocation (graph-capturable).  The
 * variances are merged (count, mean, M2) triples -- Chan's pairwise update per 8-half item, per thread, across lanes and
 * across waves -- not sum / sum of squares, so a mean far from zero costs no accuracy (|relative error| of the ratio
 * ~1e-6 against fp64); no atomics and a fixed merge order: the same input gives the same bits on every launch.
 * -22 before any launch: a null pointer, B <= 0, per_sample <= 0, not a multiple of 8 or above 2^24 (the element counts
 * are fp32, exact up to there; the largest sample of the models is 65 536), eps not 16-byte aligned, rescale negative or
 * not finite. */
int cid_cfg_rescale_f16(const cid_half* eps, float guidance, float rescale, float* escale, int32_t B, int32_t per_sample,
                        cid_stream_t stream);
/* cid_cfg_ddim_step_f16 / cid_cfg_multistep_step_f16 with e = (eps_u + g (eps_c - eps_u)) * escale[sample]; everything
 * downstream of e is as documented there (m = a x + b e, ring, saved sample, z, inpaint blend).  escale: DEVICE fp32 [B]
 * (cid_cfg_rescale_f16 writes it).  per_sample % 8 == 0 here -- an 8-half item must lie inside one sample -- where the
 * unscaled entries ask for B * per_sample % 8 == 0 only, and B * per_sample < 2^34 (the sample of an item is a 32-bit division).  With escale all 1.0 the results are bit-identical to the
 * unscaled entries', which compile to the instructions they had before these existed (one kernel body, a compile-time switch). */
int cid_cfg_ddim_step_scaled_f16(const cid_half* eps, cid_half* latents, const float* coef, float guidance,
                                 const cid_half* mask, const cid_half* init, const cid_half* noise,
                                 int32_t B, int32_t per_sample, const float* escale, cid_stream_t stream);
int cid_cfg_multistep_step_scaled_f16(const cid_half* eps, cid_half* latents, float* hist, cid_half* saved,
                                      const cid_half* z, int32_t z_rows, const void* row, float guidance,
                                      const cid_half* mask, const cid_half* init, const cid_half* noise,
                                      int32_t B, int32_t per_sample, const float* escale, cid_stream_t stream);
/* Perturbed-attention guidance (arXiv 2403.17377; since cid_version() 114): the three step entries above with one more
 * block of eps rows, the prediction p of the perturbed evaluation, behind the conditional rows:
 *    cid_cfg_pag_ddim_step_f16, cid_cfg_pag_multistep_step_f16:  eps [3B][per_sample] = [uncond | cond | perturbed],
 *                                                                e = eps_u + g (eps_c - eps_u) + s (eps_c - eps_p)
 *    cid_pag_multistep_step_f16 (the single pass):               eps [2B][per_sample] = [cond | perturbed],
 *                                                                e = eps_c + s (eps_c - eps_p)
 * s = pag[0], ONE fp32 value on the DEVICE (a step-table column: a captured launch follows it).  Everything downstream of e
 * is the sibling entry's: coefficient row, ring, `saved`, z, inpaint blend; fp32 arithmetic, one rounding at the store of
 * latents.  The kernel branches once, uniformly, on the loaded value: with s == 0 the perturbed rows are NOT read (they may hold
 * anything, NaN included) and the launch runs the sibling's instructions -- latents, ring and `saved` get the sibling's bits.
 * -22 before any launch: exactly what the sibling entry refuses (so cid_pag_multistep_step_f16, like cid_multistep_step_f16,
 * also a buffer that is not 16-byte aligned), and a null pag. */
int cid_cfg_pag_ddim_step_f16(const cid_half* eps, cid_half* latents, const float* coef, float guidance, const float* pag,
                              const cid_half* mask, const cid_half* init, const cid_half* noise,
                              int32_t B, int32_t per_sample, cid_stream_t stream);
int cid_cfg_pag_multistep_step_f16(const cid_half* eps, cid_half* latents, float* hist, cid_half* saved,
                                   const cid_half* z, int32_t z_rows, const void* row, float guidance, const float* pag,
                                   const cid_half* mask, const cid_half* init, const cid_half* noise,
                                   int32_t B, int32_t per_sample, cid_stream_t stream);
int cid_pag_multistep_step_f16(const cid_half* eps, cid_half* latents, float* hist, cid_half* saved,
                               const cid_half* z, int32_t z_rows, const void* row, const float* pag,
                               const cid_half* mask, const cid_half* init, const cid_half* noise,
                               int32_t B, int32_t per_sample, cid_stream_t stream);
/* Self-attention guidance (Hong et al., arXiv 2210.00939; since cid_version() 115).
 * cid_attn_colmass_f16: the column mass of a self-attention map the flash kernels never materialise,
 *    mass[b][j] = 1 / heads * sum_head sum_{i < n_keys} softmax_j(q_i . k_j)          fp32 [B][N]
 * q, k: what the fused QKV GEMM leaves in its [B * N][2c] buffer (head h at columns h * d of either, q pre-multiplied by
 * scale * log2 e as for cid_self_attn_f16; ldq = ldk = 2c there).  Keys j >= n_keys are padding: their columns are written
 * as 0 and their scores enter no maximum or sum; rows i >= n_keys do not contribute.  Row softmax with the row maximum
 * subtracted, fp16 products accumulated in fp32; one workgroup per sample, no atomics, one fixed summation order: the same
 * input gives the same bits on every launch.  -22: null or not 16-byte aligned pointers, N no multiple of 32 or above 4096,
 * n_keys outside 1 .. N, d not in {32, 40, 64, 80, 160}, a pitch that is no multiple of 8 or below heads * d.
 * cid_sag_degrade_f16: mask, blur and re-noise in one launch.  With x = latents, e = eps_g (fp16 [B][C][h][w]) and
 * coef = p_x, p_e, q_x, q_e, n_d, n_e, 0, 0 (eight fp32 words on the DEVICE: a step-table column, a captured launch follows it):
 *    x0 = p_x x + p_e e        ehat = q_x x + q_e e        out = n_d (m ? blur(x0) : x0) + n_e ehat
 *    m(b, y, x) = mass[b][floor(y hm / h) * wm + floor(x wm / w)] > 1.0      (strictly; mass fp32 [B][hm * wm], the same for
 *                                                                            every channel)
 * blur: the separable 9 x 9 Gaussian with sigma 1 (taps exp(-k^2 / 2), k = -4 .. 4, normalised), reflect padding by 4, per
 * channel.  fp32 arithmetic, one rounding at the store.  -22 before any launch: h < 5 or w < 5, a null pointer, a buffer
 * that is not 16-byte aligned, B * C above 65535.
 * The three step entries take the prediction e_d of the degraded latents in a buffer of its own, eps_d [B][per_sample], and
 * the scale s as a launch argument:
 *    cid_cfg_sag_ddim_step_f16, cid_cfg_sag_multistep_step_f16:  eps [2B][per_sample],  e = u + g (c - u) + s (u - e_d)
 *    cid_sag_multistep_step_f16 (the single pass):               eps [B][per_sample],   e = c + s (c - e_d)
 * Everything downstream of e is the sibling entry's.  With s == 0 eps_d is NOT read (it may hold NaN) and latents, ring and
 * `saved` get the sibling's bits.  -22: exactly what the sibling entry refuses, and a null eps_d. */
int cid_attn_colmass_f16(const cid_half* q, int32_t ldq, const cid_half* k, int32_t ldk, float* mass,
                         int32_t B, int32_t N, int32_t n_keys, int32_t heads, int32_t d, cid_stream_t stream);
int cid_sag_degrade_f16(const cid_half* latents, const cid_half* eps_g, const float* mass, cid_half* out, const float* coef,
                        int32_t B, int32_t C, int32_t h, int32_t w, int32_t hm, int32_t wm, cid_stream_t stream);
int cid_cfg_sag_ddim_step_f16(const cid_half* eps, cid_half* latents, const float* coef, float guidance,
                              const cid_half* eps_d, float sag, const cid_half* mask, const cid_half* init,
                              const cid_half* noise, int32_t B, int32_t per_sample, cid_stream_t stream);
int cid_cfg_sag_multistep_step_f16(const cid_half* eps, cid_half* latents, float* hist, cid_half* saved,
                                   const cid_half* z, int32_t z_rows, const void* row, float guidance,
                                   const cid_half* eps_d, float sag, const cid_half* mask, const cid_half* init,
                                   const cid_half* noise, int32_t B, int32_t per_sample, cid_stream_t stream);
int cid_sag_multistep_step_f16(const cid_half* eps, cid_half* latents, float* hist, cid_half* saved,
                               const cid_half* z, int32_t z_rows, const void* row, const cid_half* eps_d, float sag,
                               const cid_half* mask, const cid_half* init, const cid_half* noise,
                               int32_t B, int32_t per_sample, cid_stream_t stream);
/* FreeU (D: utils/torch_utils.py apply_freeu / fourier_filter, called from UpBlock2D / CrossAttnUpBlock2D.forward on the
 * inputs of every resnet of the first two up blocks, in front of torch.cat([hidden, skip], 1)):
 *    x[.., : c_x / 2] *= b          x: fp16 [B*H*W][c_x] in place, fp32 product, one rounding; the upper half is not touched
 *    skip_out = fourier_filter(skip, threshold = 1, scale = s)       skip, skip_out: fp16 [B*H*W][c_skip]; skip_out may BE skip
 * threshold = 1 puts the four frequencies {-1, 0}^2 into the filter's box (even and odd sides alike), so with
 * th = 2 pi h / H, tw = 2 pi w / W and phi = {1, cos th, sin th, cos tw, sin tw, cos(th + tw), sin(th + tw)} per plane
 *    skip_out[h, w] = skip[h, w] + (s - 1) / (H W) * sum_k ( sum_{h', w'} skip[h', w'] phi_k[h', w'] ) phi_k[h, w]
 * -- no FFT and no NCHW permute.  fp32 sums and update, one rounding to fp16 per element; twiddles from sincospif.  Two
 * launches: the seven sums per (sample, channel), as partials over slices of the token axis into ws (as many slices as bring
 * the grid of (sample, 64-channel slab) workgroups to 256), then the update, which adds the partials in slice order.  No atomics:
 * the same input gives the same bits, in place and out of place.  ws: >= cid_freeu_ws_bytes() of DEVICE scratch (fp32).
 * x must not overlap skip or skip_out; skip_out is skip itself or does not overlap it.
 * -22 before any launch: a null pointer, B outside 1..65535, H or W outside 2..1024 (diffusers' slice is empty on a side of 1;
 * the twiddle table sits in LDS), c_x not a positive multiple of 16 (the scaled half ends on a 16-byte vector), c_skip not a
 * positive multiple of 8, a tensor base that is not 16-byte aligned, s or b not finite.  cid_freeu_ws_bytes is host-only and
 * returns 0 for a shape cid_freeu_f16 refuses. */
int64_t cid_freeu_ws_bytes(int32_t B, int32_t c_skip, int32_t H, int32_t W);
int cid_freeu_f16(cid_half* x, int32_t c_x, float b, const cid_half* skip, cid_half* skip_out, int32_t c_skip, float s,
                  int32_t B, int32_t H, int32_t W, float* ws, cid_stream_t stream);
/* y[i] += a[i mod na] (ControlNet residual adds, CN :418-425) */
int cid_add_inplace_f16(cid_half* y, const cid_half* a, int64_t n, int64_t na, cid_stream_t stream);

/* The residuals of several ControlNets (diffusers MultiControlNetModel; CN :397-398 scales, :418-425 the hand-over to
 * the UNet) added to up to 16 destination tensors in ONE launch:
 *    y_j[i] = fp16( fp32(y_j[i]) + sum_k scales[k] * fp32(r_jk[i mod nr_j]) )        j < n_segs, k < n_nets
 * scales: DEVICE, n_nets fp32 values (conditioning scale x keep of the step; cid_step_select fills it in a captured
 * loop) -- no per-step host value enters the launch.  The sum runs in fp32 in net order and is rounded once, at the
 * store.  A net whose scale is exactly 0 adds nothing AND its residuals are NOT read: a net outside its guidance window
 * is not run, so r_jk may then point at anything readable or stale (NaN bit patterns included), but must not be NULL.
 * `i mod nr` is the B-row residual under the 2B-row CFG batch, as in cid_add_inplace_f16.
 * segs: HOST array, copied into the kernel arguments.  Refused before any launch (-22): NULL segs / scales / y / r[k]
 * with k < n_nets; n_segs outside 1..16; n_nets outside 1..CID_MAX_CONTROLNETS; n or nr not a positive multiple of 8;
 * n % nr != 0; y or r[k] not 16-byte aligned.  r[k] with k >= n_nets is ignored.  The y_j must not overlap each other
 * or any r_jk. */
#define CID_MAX_CONTROLNETS 4
typedef struct cid_accum_seg {
    cid_half* y;
    int64_t n;                              /* elements of y */
    int64_t nr;                             /* elements of every r[k] */
    const cid_half* r[CID_MAX_CONTROLNETS];
} cid_accum_seg;
int cid_residual_accum_f16(const cid_accum_seg* segs, int32_t n_segs, int32_t n_nets, const float* scales,
                           cid_stream_t stream);

/* The reference's  `for i, t in enumerate(timesteps):`  (pipline_StableDiffusion_ConsistentID.py:535, SDXL :611, CN :375)
 * turns every per-step host value -- t, the scheduler coefficients of step i, the embed set selected by
 * `i <= start_merge_step` (:542-549), SDXL's pooled embeds (:620-631), the time-embedding row -- into a kernel argument.
 * Here one row per step of all of them sits in a DEVICE table ([n_rows][row_bytes], built once per generation) and this
 * launch, the first node of the captured step, copies row *counter into the buffers the step's kernels read (segment k:
 * segs[k].nbytes bytes at table + row * row_bytes + segs[k].offset -> segs[k].dst; sizes and offsets multiples of 4
 * (16-byte aligned segments, rows and destinations move as 16-byte words: ops.StepTable pads its columns so),
 * n_segs <= 8), then increments *counter: a DDIM step is ONE graph replay with no host-side copy around it.
 * row = min(*counter, n_rows - 1). */
typedef struct cid_step_seg {
    void* dst;
    int64_t offset;
    int64_t nbytes;
} cid_step_seg;
int cid_step_select(const void* table, int64_t row_bytes, int32_t n_rows, int32_t* counter, const cid_step_seg* segs,
                    int32_t n_segs, cid_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

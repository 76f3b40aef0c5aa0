// The planner of cid_gemm_f16 (host code only: no kernel lives here, so a rule change recompiles no kernel).  cidg::plan turns
// a cid_gemm_desc into a GemmPlan (gemm_args.h): checked arguments, filled launch arguments, tile, kernel family and template
// instance.  cid_gemm_f16 (gemm.hip) launches the plan; cid_gemm_plan and cid_gemm_stats_rows, below, report it.
//
// The steps run in this order; each takes the descriptor and the plan so far, and each one's opening comment names the fields
// of earlier steps that it overwrites:
//    1. check_args          argument checks (every mode)
//    2. fill_args           descriptor -> GemmArgs, plan defaults
//    3. tiles_mode3         mode 3 only: its checks and tiles (steps 4-9 are skipped)
//    4. choose_tiles        tile (and split-K) by family: tiles_geglu | tiles_160 | tiles_off_grid
//    5. plan_nloop          GEGLU N-loop
//    6. route_linear_h32    GEGLU on linear_h32.hip
//    7. plan_ring           ring depth of the gather kernels
//    8. route_halo          stride-1 3x3 convolutions on the halo kernel
//    9. route_conv3x3       ... on conv3x3.hip, nine taps or four phases
//   10. finish_launch       instance flags of the family; nbuf dropped for the families that fix their own staging
//   11. check_stats         statistics legality
// The environment switches of all of them are PlanSwitches, read once per process.
#include "gemm_args.h"
#include "../../include/cid.h"
#include <stdlib.h>

namespace {
using namespace cidg;

int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }

// Every environment switch of the planner (A/B and experiment switches) with its default and what its values mean; read once
// per process, when switches() builds the one instance.
struct PlanSwitches {
    int geglu_tile = env_int("CID_GEGLU_TILE", 0);          // 0 the rule | 1 = 256-token GEGLU tiles wherever legal | 2 = 128-token tiles
    int gemm_tile = env_int("CID_GEMM_TILE", 0);            // 0 the rule | 1 / 2 / 3 = 256 / 128 / 64-token tiles on the 160-wide grid
    int gemm_sk = env_int("CID_GEMM_SK", 0);                // 0 the rule | n = split-K n on the 160-wide grid (where a split is legal)
    int prefer128 = env_int("CID_GEMM_PREFER128", 1);       // 1 128-token tiles wherever they number >= 256 | 0 = the rule of rounds 3-5
    int geglu_nloop = env_int("CID_GEGLU_NLOOP", 0);        // 0 the rule | 1 = off | n = force
    int geglu_h32 = env_int("CID_GEGLU_H32", 1);            // 1 GEGLU on linear_h32.hip where it fits | 0 = off
    int nbuf = env_int("CID_GEMM_NBUF", 0);                 // 0 the rule | 2 = never three stages | 3 = whenever legal
    int no_halo = env_int("CID_GEMM_NOHALO", 0);            // 0 | 1 = no halo kernel
    int conv_h32 = env_int("CID_CONV_H32", 1);              // 1 conv3x3.hip where it fits | 0 = never | 2 = its 256-token tiles only
    int upconv_fold = env_int("CID_UPCONV_FOLD", 1);        // 1 the phase mode for w_up4 | 0 = never
    int xcd_2d = env_int("CID_XCD_2D", 1);                  // 1 2-D tile -> XCD partition (choose_xcd_pn) | 0 = linear runs, the old order
    int ablate = env_int("CID_GEMM_ABLATE", 0);             // 0 profiling knob (GemmArgs.ablate): the kernels read it in experiment builds
                                                            //   only (build.py --variant ... CID_GEMM_ABLATION), else it is ignored
};

const PlanSwitches& switches() { static const PlanSwitches s; return s; }

constexpr int BK = 64;          // channels per slab (gemm.hip)
constexpr long TARGET = 2048;   // tile choice: aim for >= 2 waves on each of the 1024 SIMDs

void set_tile(GemmPlan& p, TileCfg cfg) {
    static const int bm[] = { 256, 128, 64, 256, 128, 64, 128 }, bn[] = { 160, 160, 160, 128, 128, 64, 32 };
    p.cfg = cfg; p.bm = bm[cfg]; p.bn = bn[cfg];
}

// columns of the plain launch (mode 2: the Q and K thirds; the V third is a second launch)
int n_plain(const cid_gemm_desc* d) { return d->mode == 2 ? d->n_vt0 : d->N; }

// waves of a launch on bm x bn tiles with w waves per workgroup
long waves(const cid_gemm_desc* d, int bm, int bn, int w) { return (long)((d->M + bm - 1) / bm) * ((n_plain(d) + bn - 1) / bn) * w; }

// ---- 1. argument checks of every mode (mode 3 adds its own: tiles_mode3).  Keeps the three buffer ranges it has to compute
// for the 2-GiB check (p.a.bytes_x1 / bytes_x2 / bytes_w); overwrites nothing.
int check_args(const cid_gemm_desc* d, GemmPlan& p) {
    CID_CHECK_ARG(d && d->x1 && d->w && d->out, "cid_gemm_f16: null pointer");
    CID_CHECK_ARG(d->taps == 1 || d->taps == 9, "cid_gemm_f16: taps must be 1 or 9 (got %d)", d->taps);
    CID_CHECK_ARG(d->c1 > 0 && d->c1 % 32 == 0 && d->c2 >= 0 && d->c2 % 32 == 0 && (d->c1 + d->c2) % 64 == 0 &&
                  (d->c2 == 0 || d->c1 % 64 == 0),
                  "cid_gemm_f16: channel counts must be multiples of 64 (c1=%d c2=%d)", d->c1, d->c2);
    CID_CHECK_ARG(d->c2 == 0 || d->x2, "cid_gemm_f16: c2 > 0 needs x2");
    CID_CHECK_ARG(d->N > 0 && d->N % 32 == 0 && d->M > 0, "cid_gemm_f16: bad M/N (%d, %d)", d->M, d->N);
    CID_CHECK_ARG(d->mode >= 0 && d->mode <= 3, "cid_gemm_f16: bad mode %d", d->mode);
    CID_CHECK_ARG(d->ld1 % 8 == 0 && d->ldo % 8 == 0 && (d->c2 == 0 || d->ld2 % 8 == 0) && (!d->res || d->ldr % 8 == 0),
                  "cid_gemm_f16: row pitches (ld1, ld2, ldo, ldr) must keep 16-byte alignment");
    CID_CHECK_ARG((((uintptr_t)d->out | (uintptr_t)d->res | (uintptr_t)d->out2) & 15) == 0,
                  "cid_gemm_f16: out / out2 / res must be 16-byte aligned (rows are stored and the residual is read in 16-byte chunks)");
    CID_CHECK_ARG((d->ln_s == nullptr) == (d->ln_b == nullptr), "cid_gemm_f16: ln_s and ln_b come together");
    CID_CHECK_ARG(!d->ln_s || (d->taps == 1 && d->c2 == 0 && !d->bias && d->ln_eps > 0.f),
                  "cid_gemm_f16: the LayerNorm fold applies to one-source linears; the bias belongs in ln_b");
    CID_CHECK_ARG(!d->out2 || d->mode == 0, "cid_gemm_f16: out2 (a second destination) goes with the plain epilogue, mode 0");
    // rows addressable through x1 / x2: the input image for convs, M rows for linears
    const long rows_in = (d->taps == 9) ? (long)(d->M / (d->Ho * d->Wo)) * d->Hi * d->Wi : (long)d->M;
    const long b1 = ((rows_in - 1) * d->ld1 + d->c1) * 2, b2 = d->c2 ? ((rows_in - 1) * d->ld2 + d->c2) * 2 : 0;
    const long bw = (long)d->N * d->taps * (d->c1 + d->c2) * 2;
    CID_CHECK_ARG(b1 < 0x7fffffffL && b2 < 0x7fffffffL && bw < 0x7fffffffL, "cid_gemm_f16: tensor exceeds 2 GiB");
    p.a.bytes_x1 = (unsigned)b1; p.a.bytes_x2 = (unsigned)b2; p.a.bytes_w = (unsigned)bw;
    if (d->taps == 9) {
        CID_CHECK_ARG(d->Hi > 0 && d->Wi > 0 && d->Ho > 0 && d->Wo > 0 && (d->stride == 1 || d->stride == 2)
                      && (d->up == 0 || d->up == 1), "cid_gemm_f16: bad conv geometry");
        CID_CHECK_ARG(d->M % (d->Ho * d->Wo) == 0, "cid_gemm_f16: M is not batch * Ho * Wo");
    }
    // pad_mode 1: diffusers' Downsample2D(padding=0) = F.pad(x, (0, 1, 0, 1)) then a stride-2 3x3 conv without padding --
    // output (y, x) reads input (2y + dy, 2x + dx), dy, dx in {0, 1, 2}; row Hi and column Wi (the pad) read as zero.  Only the
    // tap offset of the gather changes (set_tap), so the igemm_kernel instances run it; the halo / conv3x3.hip kernels below
    // are stride-1 only and never see it.
    CID_CHECK_ARG(d->pad_mode == 0 || d->pad_mode == 1, "cid_gemm_f16: bad pad_mode %d", d->pad_mode);
    CID_CHECK_ARG(d->pad_mode == 0 || (d->mode == 0 && d->taps == 9 && d->stride == 2 && d->up == 0 && d->Hi % 2 == 0 &&
                                       d->Wi % 2 == 0 && d->Ho == d->Hi / 2 && d->Wo == d->Wi / 2),
                  "cid_gemm_f16: pad_mode 1 needs mode 0, taps 9, stride 2, up 0, even Hi / Wi, Ho = Hi / 2 and Wo = Wi / 2 "
                  "(got mode %d taps %d stride %d up %d, %d x %d -> %d x %d)", d->mode, d->taps, d->stride, d->up, d->Hi, d->Wi,
                  d->Ho, d->Wo);
    // w_up4 (since cid_version() 103): the folded weights of an Upsample2D convolution (cid_upconv_fold_f16).  The launch may
    // then run as four 2x2 phase convolutions at input resolution (conv3x3.hip, routed below); where it cannot, w serves.
    CID_CHECK_ARG(!d->w_up4 || (d->taps == 9 && d->up == 1 && d->stride == 1 && d->mode == 0 && !d->res),
                  "cid_gemm_f16: w_up4 needs taps 9, up 1, stride 1, mode 0 and no res (got taps %d up %d stride %d mode %d)",
                  d->taps, d->up, d->stride, d->mode);
    CID_CHECK_ARG(((uintptr_t)d->w_up4 & 15) == 0, "cid_gemm_f16: w_up4 must be 16-byte aligned");
    // act 1 (since cid_version() 102): ReLU in the plain epilogue.  Only the igemm_kernel instances carry it (launch_act);
    // split-K (ws), the GroupNorm statistics and the LayerNorm fold are refused with it, the halo / conv3x3.hip kernels skipped.
    CID_CHECK_ARG(d->act == 0 || d->act == 1, "cid_gemm_f16: bad act %d", d->act);
    CID_CHECK_ARG(d->act == 0 || (d->mode == 0 && !d->gn_stats && !d->ws && !d->ln_s),
                  "cid_gemm_f16: act 1 needs mode 0 and no gn_stats / ws / ln_s (got mode %d)", d->mode);
    return 0;
}

// ---- 2. descriptor -> GemmArgs (all but the buffer ranges of step 1) and the plan's defaults: one unsplit launch of the gather
// kernel, one n-tile per workgroup, two ring stages, no instance flag
void fill_args(const cid_gemm_desc* d, GemmPlan& p) {
    GemmArgs& a = p.a;
    a.x1 = (const half_t*)d->x1; a.x2 = (const half_t*)d->x2;
    a.c1 = d->c1; a.c2 = d->c2; a.ld1 = d->ld1; a.ld2 = d->ld2;
    a.w = (const half_t*)d->w; a.out = (half_t*)d->out; a.ldo = d->ldo;
    a.out2 = (half_t*)d->out2;
    a.bias = (const half_t*)d->bias;
    a.rowbias = (const half_t*)d->rowbias; a.ld_rowbias = d->ld_rowbias;
    a.rows_per_sample = d->rows_per_sample > 0 ? d->rows_per_sample : 1;
    a.res = (const half_t*)d->res; a.ldr = d->ldr;
    a.M = d->M; a.N = d->N; a.taps = d->taps;
    a.Hi = d->Hi; a.Wi = d->Wi; a.Ho = d->Ho; a.Wo = d->Wo; a.stride = d->stride; a.up = d->up;
    a.mode = d->mode;
    a.vt = (half_t*)d->vt; a.n_vt0 = d->n_vt0; a.heads = d->heads; a.dhead = d->dhead;
    a.dvp = d->dvp; a.ntok = d->ntok;
    a.cslabs = (d->c1 + d->c2) / BK;
    a.ktot = d->taps * (d->c1 + d->c2);
    a.nslab = a.ktot / BK;
    a.splitk = 1; a.nloop = 1; a.nbuf = 2; a.xcd_pn = 0;
    a.att_kp = (const half_t*)d->att_kp; a.att_vp = (const half_t*)d->att_vp; a.att_kvrow = (const int*)d->att_kvrow;
    a.att_n_txt = d->att_n_txt; a.att_n_ip = d->att_n_ip; a.att_scale = d->att_ip_scale;
    a.att_krow = a.att_vrow = 0;
    a.ws = (float*)d->ws;
    a.ln_s = d->ln_s; a.ln_b = d->ln_b; a.ln_eps = d->ln_eps;
    a.gn_stats = d->gn_stats; a.gn_unit = d->N / 32;
    a.ablate = switches().ablate;
    a.n_begin = 0; a.n_end = a.N;      // the whole width (what every launcher but launch() expects; that one narrows a copy)
    a.tap0 = d->pad_mode == 1 ? 0 : -1;
    a.w4 = nullptr;
    p.family = CID_GEMM_FAMILY_IGEMM;
    p.bm = p.bn = p.stats_rows = 0;
    p.ln = p.act = p.vmode = p.sk_epilogue = false;
}

// ---- 3. mode 3: query projection with the identity cross-attention as its epilogue: tiles of whole heads inside one sample.
// Sets the family, the tile and a.att_krow / a.att_vrow (zero since step 2).
int tiles_mode3(const cid_gemm_desc* d, GemmPlan& p) {
    CID_CHECK_ARG(d->att_kp && d->att_vp && d->att_kvrow, "cid_gemm_f16: mode 3 needs att_kp / att_vp / att_kvrow");
    CID_CHECK_ARG(d->taps == 1 && d->c2 == 0 && !d->bias && !d->rowbias && !d->res && !d->gn_stats,
                  "cid_gemm_f16: mode 3 is a plain projection (no bias / residual / statistics)");
    CID_CHECK_ARG(d->heads > 0 && d->dhead > 0 && d->N == d->heads * d->dhead && (d->dhead == 64 || d->dhead == 80 || d->dhead == 160),
                  "cid_gemm_f16: mode 3 needs N = heads * dhead with dhead in {64, 80, 160} (got %d x %d, N = %d)", d->heads, d->dhead, d->N);
    CID_CHECK_ARG(d->att_n_txt == 77 && d->att_n_ip == 4, "cid_gemm_f16: mode 3 is built for the reference's 77 + 4 context (got %d + %d)",
                  d->att_n_txt, d->att_n_ip);
    CID_CHECK_ARG(d->ntok > 0 && d->M % d->ntok == 0 && d->ntok % 64 == 0, "cid_gemm_f16: mode 3 needs ntok (tokens per sample, a multiple of 64)");
    const int qks = (d->dhead + 15) / 16, dvt = (d->dhead + 31) / 32;
    p.a.att_krow = (long)d->heads * 3 * qks * 512;
    p.a.att_vrow = (long)d->heads * dvt * 6 * 512;
    p.family = CID_GEMM_FAMILY_IGEMM_ATT;
    if (d->dhead == 64) { set_tile(p, G128x128); CID_CHECK_ARG(d->N % 128 == 0 && d->ntok % 128 == 0, "cid_gemm_f16: mode 3, dhead 64: N and ntok multiples of 128"); }
    else {
        // 160-wide tiles span whole heads (two of 80 channels, one of 160): N must be a whole number of them
        CID_CHECK_ARG(d->N % 160 == 0, "cid_gemm_f16: mode 3, dhead %d: N = %d is not a multiple of the 160-channel tile", d->dhead, d->N);
        set_tile(p, d->ntok % 128 == 0 && (long)(d->M / 128) * (d->N / 160) >= 256 ? B128x160 : C64x160);
    }
    return 0;
}

// ---- 4a. GEGLU tiles (mode 1).  Overwrites nothing.
int tiles_geglu(const cid_gemm_desc* d, GemmPlan& p) {
    // GEGLU with short K (few slabs): the erf epilogue and the pipeline prologue dominate a tile's
    // life, so prefer the tile that lets two workgroups share a CU and overlap them (measured:
    // 156 -> 115 us at M=32768, N=2560, K=320; plain epilogues do not benefit)
    // 256-token tiles only for deep K AND at least 1024 of them (in situ: SDXL's M = 4096, K = 1280 level +0.9 % end to end
    // with the big tile, SD1.5's M = 2048 level +0.3 % with the small one)
    bool small_tiles = p.a.nslab <= 10 || waves(d, 256, 128, 1) < 1024;
    if (switches().geglu_tile == 1) small_tiles = false;
    if (switches().geglu_tile == 2) small_tiles = true;
    if (d->N % 128 != 0) set_tile(p, O64x64);
    else if (waves(d, 256, 128, 8) >= TARGET && !small_tiles) set_tile(p, G256x128);
    else set_tile(p, G128x128);
    CID_CHECK_ARG(d->N % 64 == 0, "cid_gemm_f16: GEGLU needs N %% 64 == 0");
    return 0;
}

// ---- 4b. the 160-wide tiles (modes 0 and 2, columns on the 160 grid) and their split-K.  Overwrites a.splitk (1 since step 2).
void tiles_160(const cid_gemm_desc* d, GemmPlan& p) {
    // plain epilogue: the largest tile that still yields >= 256 workgroups, if necessary with the help
    // of split-K (small-M levels are weight-traffic bound: W is re-read once per token tile)
    GemmArgs& a = p.a;
    const bool can_split = (d->mode == 0) && a.ws != nullptr && !a.ln_s;
    auto tiles = [&](int bm_) { return (long)((a.M + bm_ - 1) / bm_) * (n_plain(d) / 160); };
    auto sk_for = [&](int bm_) {
        long t = tiles(bm_);
        int sk = (int)((256 + t - 1) / t);
        if (!can_split) sk = 1;
        if (sk > 16) sk = 16;
        while (sk > 1 && a.nslab / sk < 6) --sk;
        while (sk > 1 && (int64_t)sk * a.M * a.N * 4 > d->ws_bytes) --sk;
        return sk;
    };
    int pick = 0;
    bool nosplit = false;
    if (switches().gemm_tile) pick = switches().gemm_tile;
    else if (d->taps == 1 && tiles(256) >= 256) {
        // enough 256-token tiles without split-K; the fused QKV projection (no split possible, short K) prefers
        // twice as many half-size tiles when the big ones only just fill the chip (measured 63 -> 55 us at SDXL's
        // 32x32 level, 45 -> 42 us at SD1.5's 32x32 level)
        // (and 45 -> 41 us at SD1.5's 64x64 level, where the big tiles number exactly 512: CID_GEMM_TILE A/B, round 4)
        // Round 6 re-measured the rule for every linear (CID_GEMM_TILE A/B at SD1.5 CFG batch 8 / 16 and SDXL batch 4,
        // profiles/r06_tile_rule.txt): 128-token tiles win wherever they number >= 256 -- 320 -> 320 at 64 x 64 17.8 -> 14.9 us
        // (33.1 -> 26.9 at CFG batch 16), SDXL's 640 -> 640 24.4 -> 21.1, ff2 at 1280 channels 68.6 -> 63.2 (unsplit instead of
        // 256-token tiles + split-K 2).  One 256-token workgroup per CU loads, multiplies and stores in lock step with every
        // other CU; two half-size workgroups per CU are out of phase.  CID_GEMM_PREFER128=0: the rule of rounds 3-5.
        pick = (switches().prefer128 || (d->mode == 2 && tiles(256) <= 512 && tiles(128) >= 512)) ? 2 : 1;
        nosplit = true;
    } else if (d->taps == 1 && tiles(128) >= 256 && (a.nslab <= 40 || switches().prefer128)) { pick = 2; nosplit = true; }   // no fp32 partials
    else if (d->taps == 1 && tiles(64) >= 256 && a.nslab <= 20) { pick = 3; nosplit = true; }      // beats 256-tiles + split-K
    else if (tiles(256) * sk_for(256) >= 256) pick = 1;                                             // (tools/sweep_tiles*.sh)
    else if (tiles(128) * sk_for(128) >= 256) pick = 2;
    else pick = 3;
    set_tile(p, pick == 1 ? A256x160 : pick == 2 ? B128x160 : C64x160);
    a.splitk = switches().gemm_sk ? switches().gemm_sk : (nosplit ? 1 : sk_for(p.bm));
    if (!can_split || (int64_t)a.splitk * a.M * a.N * 4 > d->ws_bytes || a.nslab < a.splitk) a.splitk = 1;
}

// ---- 4c. widths off the 160 grid (modes 0 and 2) and their split-K.  Overwrites a.splitk (1 since step 2).
void tiles_off_grid(const cid_gemm_desc* d, GemmPlan& p) {
    GemmArgs& a = p.a;
    int nw = 4;      // waves per workgroup
    if (d->mode == 0 && n_plain(d) % 128 == 0) {
        // widths off the 160 grid (VAE decoder: 128 / 256 / 512 channels, attention score / value GEMMs)
        set_tile(p, waves(d, 256, 128, 8) >= TARGET ? G256x128 : G128x128);
        nw = 8;
    } else if (n_plain(d) % 64 == 0) set_tile(p, O64x64);
    else set_tile(p, O128x32);
    // split-K for small-M / deep-K problems (plain epilogue only)
    if (d->mode == 0 && a.ws && !a.ln_s && a.nslab >= 16) {
        const long w = waves(d, p.bm, p.bn, nw);
        if (w < TARGET) {
            int sk = (int)((TARGET + w - 1) / w);
            if (sk > 8) sk = 8;
            while (sk > 1 && a.nslab / sk < 8) --sk;
            while (sk > 1 && (int64_t)sk * a.M * a.N * 4 > d->ws_bytes) --sk;
            a.splitk = sk;
        }
    }
}

// ---- 4. tile choice: aim for >= 2 waves on each of the 1024 SIMDs; one function per family.  Sets cfg / bm / bn.
int choose_tiles(const cid_gemm_desc* d, GemmPlan& p) {
    if (d->mode == 1) { if (int rc = tiles_geglu(d, p)) return rc; }
    else if (n_plain(d) % 160 == 0) tiles_160(d, p);
    else tiles_off_grid(d, p);
    CID_CHECK_ARG(d->mode != 2 || (d->vt && d->ntok % 16 == 0 && d->M % d->ntok == 0 && d->n_vt0 % p.bn == 0 && d->dhead > 0
                                   && d->heads > 0 && d->dvp >= d->dhead && (d->N - d->n_vt0) % 16 == 0),
                  "cid_gemm_f16: bad QKV/V^T description");
    return 0;
}

// ---- 5. N-loop of the GEGLU tiles.  Overwrites a.nloop (1 since step 2).
void plan_nloop(const cid_gemm_desc* d, GemmPlan& p) {
    if (d->mode == 1 && (p.cfg == G128x128 || p.cfg == G256x128) && d->taps == 1 && d->c2 == 0 && d->M % p.bm == 0) {
        // N-loop: one workgroup walks several n-tiles of its token tile (igemm_kernel, NLOOP) -- as many as leave one round of
        // resident workgroups; the count must divide the n-tiles (the flattened slab sequence has no ragged tail)
        const int f_nl = switches().geglu_nloop;      // A/B switch: 1 = off, n = force
        const int nt = d->N / p.bn;
        const long tiles = (long)(d->M / p.bm) * nt;
        int nl = f_nl > 0 ? f_nl : (int)(tiles / (p.cfg == G128x128 ? 512 : 256));      // (128-token tiles: two workgroups per CU)
        if (nl > nt) nl = nt;
        while (nl > 1 && nt % nl != 0) --nl;
        if (nl > 1 && (long)nl * p.bn * p.a.ktot * 2 < 0x7fffffffL) p.a.nloop = nl;
    }
}

// ---- 6. GEGLU on linear_h32.hip.  Overwrites the family (gather kernel since step 2), a.nloop (step 5) and bm (step 4; bn
// follows in step 10).
void route_linear_h32(const cid_gemm_desc* d, GemmPlan& p) {
    if (d->mode == 1 && d->taps == 1 && d->c2 == 0 && !d->ln_s && d->N % 160 == 0 && d->M % 256 == 0 && p.a.cslabs >= 16) {
        // linear_h32.hip: 256 x 160 tiles of 32 x 32 x 16 MFMAs, loader / compute wave roles, N-loop -- the 16 x 16 x 32 tiles
        // above are LDS-bandwidth-bound on this op (profiles/r06_gemm_ablation.txt).  Deep K only (>= 1024 channels): the erf
        // epilogue of that kernel is exposed once per n-tile (one compute wave per SIMD), which costs more than the leaner loop
        // gains at K = 320 (86 vs 73 us at SD1.5's 64 x 64 level), draws at K = 640 and wins at K = 1280 (64 vs 77 us).  One
        // round of 256 workgroups: every workgroup walks tiles / 256 n-tiles (a divisor of the n-tile count); launches that
        // cannot fill the chip stay above.
        const int nt = d->N / 160;
        const long tiles = (long)(d->M / 256) * nt;
        int nl = (int)(tiles / 256);
        if (nl > nt) nl = nt;
        while (nl > 1 && nt % nl != 0) --nl;
        if (switches().geglu_h32 && tiles >= 256 && nl >= 1 && (long)nl * 160 * p.a.ktot * 2 < 0x7fffffffL) {      // A/B switch: 0 = off
            p.family = CID_GEMM_FAMILY_GEGLU_H32;
            p.a.nloop = nl;
            p.bm = 256;
        }
    }
}

// ---- 7. ring depth of the gather kernels.  Overwrites a.nbuf (2 since step 2).
void plan_ring(const cid_gemm_desc* d, GemmPlan& p) {
    // three-stage ring: launches of the 128- / 64-token tiles that put at most one workgroup on a CU anyway (<= 256
    // workgroups) and walk enough slabs for the lookahead to matter
    const int f_nb = switches().nbuf;      // A/B switch: 2 = never, 3 = whenever legal
    const bool legal = (p.cfg == A256x160 || p.cfg == B128x160 || p.cfg == C64x160) && d->mode != 1 && !d->act;
    const long wgs = (long)((d->M + p.bm - 1) / p.bm) * ((n_plain(d) + p.bn - 1) / p.bn) * p.a.splitk;
    // (the 256-token tile holds one workgroup per CU whatever its ring: three stages whenever there are slabs to look ahead;
    //  the smaller tiles only where a third stage does not cost a co-resident workgroup)
    const bool want = p.cfg == A256x160 ? (p.a.nslab / p.a.splitk >= 4) : (wgs <= 256 && p.a.nslab / p.a.splitk >= 8);
    if (legal && (f_nb == 3 || (f_nb == 0 && want))) p.a.nbuf = 3;
}

// ---- 8. stride-1 3x3 convolutions on the halo kernel.  Overwrites the family (gather kernel since step 2) and clamps
// a.splitk (step 4).
void route_halo(const cid_gemm_desc* d, GemmPlan& p) {
    if (p.cfg == A256x160 && !switches().no_halo && !d->act && d->mode == 0 && d->taps == 9 && d->stride == 1 && d->up == 0 &&
        d->Wo == d->Wi && d->Ho == d->Hi) {
        // halo kernel: the 256-token tile must be whole image rows of one image, or whole images
        const int HW = d->Ho * d->Wo;
        const int seg = 256 < HW ? 256 : HW;
        const bool rows_ok = (seg % d->Wo == 0) && (HW % seg == 0) && (256 % seg == 0) && (d->M % 256 == 0);
        const int nh = (256 / seg) * (seg / d->Wo + 2) * (d->Wo + 2);
        if (rows_ok && nh <= 448) {
            p.family = CID_GEMM_FAMILY_IGEMM_HALO;
            if (p.a.splitk > p.a.cslabs) p.a.splitk = p.a.cslabs;     // split over whole channel slabs only
        }
    }
}

// ---- 9. stride-1 3x3 convolutions on conv3x3.hip, nine taps or four phases.  Overwrites the family (steps 2 and 8: a launch
// routed to the halo kernel moves here), bm (step 4), a.splitk (back to 1: steps 4 and 8) and a.w4 (nullptr since step 2).
void route_conv3x3(const cid_gemm_desc* d, GemmPlan& p) {
    GemmArgs& a = p.a;
    // conv3x3.hip (32 x 32 MFMA tiles, loader / compute wave roles) for the stride-1 3x3 convolutions on the 160-channel
    // grid, unsplit: 256-token tiles where they fill the chip; 128-token tiles where those do and K is short (they are
    // LDS-bound: measured faster than 256-token tiles + split-K up to 10 channel slabs -- the 32 x 32 level's 640 -> 640,
    // the first resnet of the CFG-deduplicated level 0 -- and slower beyond).  Three weight stages next to two halo buffers
    // need a halo of <= 400 rows.  Everything else stays on the halo kernel above (+ splitk_epilogue_kernel).
    const bool only256 = switches().conv_h32 == 2;
    const int HW = d->taps == 9 ? d->Ho * d->Wo : 0;
    // (Upsample2D's convolution, up == 1: the halo holds input pixels; a tile must be an even number of whole output rows of
    //  one image, starting on an even row)
    const bool shape_ok = switches().conv_h32 != 0 && !d->act && d->mode == 0 && d->taps == 9 && d->stride == 1 && (d->up == 0 || d->up == 1) &&
                          d->Wo == (d->Wi << d->up) && d->Ho == (d->Hi << d->up) && d->N % 160 == 0 && HW >= 64 &&
                          (!d->rowbias || (a.rows_per_sample >= 64 && a.rows_per_sample % 64 == 0));
    // Upsample2D with folded weights (w_up4): the phase mode -- a tile is bm_try INPUT pixels of one output parity, whole
    // input rows of one image; same tile-count rules.  One source, no time row (the UNets' Upsample2D has neither); the
    // nine-tap path below serves everything else.  CID_UPCONV_FOLD=0: never (A/B switch).
    const bool fold_ok = shape_ok && switches().upconv_fold && d->w_up4 && d->up == 1 && d->c2 == 0 && !d->rowbias && !d->res &&
                         (long)d->N * d->c1 * 32 < 0x7fffffffL;
    for (int bm_try = 256; shape_ok && bm_try >= (only256 ? 256 : 128); bm_try >>= 1) {
        const long tiles = (long)(d->M / bm_try) * (d->N / 160);
        if (tiles < 256 || (bm_try == 128 && a.cslabs > 10) || d->M % bm_try != 0) continue;
        if (fold_ok && (d->Hi * d->Wi) % bm_try == 0 && bm_try % d->Wi == 0 && (bm_try / d->Wi + 2) * (d->Wi + 2) <= 400)
            a.w4 = (const half_t*)d->w_up4;
        else {
            const int seg = bm_try < HW ? bm_try : HW;
            if (seg % d->Wo != 0 || HW % seg != 0 || bm_try % seg != 0) continue;
            if (d->up && (seg != bm_try || (seg / d->Wo) % 2 != 0)) continue;
            const int nh = (bm_try / seg) * (((seg / d->Wo) >> d->up) + 2) * ((d->Wo >> d->up) + 2);
            if (nh > 400) continue;
        }
        p.family = a.w4 ? CID_GEMM_FAMILY_CONV_H32_PHASE : CID_GEMM_FAMILY_CONV_H32;
        p.bm = bm_try;
        a.splitk = 1;
        return;
    }
}

// ---- 10. the template instance of the family.  Overwrites bn (step 4) for linear_h32.hip's 160-wide tiles and drops a.nbuf
// (steps 2 and 7) for the families that fix their own staging.
void finish_launch(const cid_gemm_desc* d, GemmPlan& p) {
    const int f = p.family;
    const bool plain = f == CID_GEMM_FAMILY_IGEMM && !d->act;      // the plain family of the gather kernel (launch, not launch_act)
    if (f == CID_GEMM_FAMILY_GEGLU_H32) p.bn = 160;
    p.act = f == CID_GEMM_FAMILY_IGEMM && d->act;
    p.ln = (plain || f == CID_GEMM_FAMILY_IGEMM_ATT) && p.a.ln_s != nullptr;
    p.vmode = plain && p.a.mode == 2 && p.a.N > p.a.n_vt0;
    p.sk_epilogue = (plain || f == CID_GEMM_FAMILY_IGEMM_HALO) && p.a.splitk > 1;
    // the ring depth is a launch parameter of the gather kernels only (launch_one reads it); the other kernels fix their staging
    if (f != CID_GEMM_FAMILY_IGEMM && f != CID_GEMM_FAMILY_IGEMM_ATT) p.a.nbuf = 0;
}

// ---- 11. token rows per GroupNorm statistics block of the planned launch (its tile height), 0 where it cannot emit them: the
// plain, unsplit, ReLU-free epilogue of the 160-wide tiles, whole tiles only.  A launch asked for statistics it cannot emit is
// refused.
int check_stats(const cid_gemm_desc* d, GemmPlan& p) {
    const int unit = d->N / 32;
    const bool ok = d->mode == 0 && d->act == 0 && p.a.splitk == 1 && (p.cfg == A256x160 || p.cfg == B128x160 || p.cfg == C64x160) &&
                    d->N % 32 == 0 && unit > 0 && 80 % unit == 0 && p.bm > 0 && d->M % p.bm == 0;
    p.stats_rows = ok ? p.bm : 0;
    // GroupNorm statistics come out of the plain, unsplit epilogue of the 160-wide tiles, whole tiles only
    CID_CHECK_ARG(!p.a.gn_stats || p.stats_rows > 0,
                  "cid_gemm_f16: gn_stats requested for a launch that cannot emit them (ask cid_gemm_stats_rows first)");
    return 0;
}

}  // namespace

int cidg::plan(const cid_gemm_desc* d, GemmPlan& p) {
    if (int rc = check_args(d, p)) return rc;
    fill_args(d, p);
    if (d->mode == 3) {
        if (int rc = tiles_mode3(d, p)) return rc;
    } else {
        if (int rc = choose_tiles(d, p)) return rc;
        plan_nloop(d, p);
        route_linear_h32(d, p);
        plan_ring(d, p);
        route_halo(d, p);
        route_conv3x3(d, p);
    }
    finish_launch(d, p);
    return check_stats(d, p);
}

int cidg::choose_xcd_pn(int gx, int gy, double w_bytes, double x_bytes) {
    if (!switches().xcd_2d || ((long)gx * gy) % 8 != 0) return 0;
    int best = 0;
    double cost = 0.0;
    for (int pn = 1; pn <= 8; pn *= 2) {
        const int pm = 8 / pn;
        if (gx % pn != 0 || gy % pm != 0) continue;
        const double c = pm * w_bytes + pn * x_bytes;
        if (best == 0 || c < cost) { best = pn; cost = c; }      // (ties keep the smaller pn: the order of rounds 2-5)
    }
    return best;
}

extern "C" int cid_gemm_plan(const cid_gemm_desc* d, cid_gemm_plan_info* out) {
    CID_CHECK_ARG(out, "cid_gemm_plan: null output");
    cidg::GemmPlan p;
    int rc = cidg::plan(d, p);
    if (rc) return rc;
    out->family = p.family; out->bm = p.bm; out->bn = p.bn;
    out->splitk = p.a.splitk; out->nloop = p.a.nloop; out->nbuf = p.a.nbuf;
    out->ln = p.ln; out->act = p.act; out->vmode = p.vmode;
    out->splitk_epilogue = p.sk_epilogue; out->stats_rows = p.stats_rows;
    return 0;
}

extern "C" int cid_gemm_stats_rows(const cid_gemm_desc* d) {
    if (!d) return 0;
    cid_gemm_desc q = *d;
    q.gn_stats = nullptr;
    cidg::GemmPlan p;
    return cidg::plan(&q, p) == 0 ? p.stats_rows : 0;
}

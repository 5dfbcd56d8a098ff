// amp_bamp_trials.hip — BAMP over E independent single-trial detections that share one channel
// (amp_bamp_trials_run): the launch engine's parameter block (BampK with B = E rows), f32 tiles and
// epilogues (amp_bamp.h) with per-row records.
//
// Restates, for every trial e alone, BAMP.forward at B = 1 (bamp.py:116-143) with its Tracker
// (bamp.py:12-25), BAMPLayer.forward (bamp.py:48-64), the per-element-tau block denoiser
// (bamp.py:66-77, the max|xi| shift of bamp.py:70 over the trial's own logits) and the allclose
// exit on the trial's own var (bamp.py:140) — the way the reference's drivers run it (batch = 1,
// res epochs per channel: bamp_model.py:89, 96).
// Per iteration: four GEMM launches over row tiles of 32 trials, each kernel the entry guard (a
// tile whose rows have all stopped returns at once), the launch engine's gemm_tile call and its
// epilogue under the LiveRows guard (a stopped row is never stored to); the denoiser runs row by
// row with one partial per (tile, row); then tbamp_r, a grid over the trials: workgroup e reduces
// trial e's partials, settles its exact float64 fix-up (fixup_sections, against the trial's own
// max|xi|) and its allclose exit.  Every kernel returns at once when the stop counter has reached E.
// amp_bamp_trials_ch_run: the same over G channels, trial e on channel e / per_channel.  One kernel
// family serves both entries: the four GEMM kernels are templates over the channel mapping
// (amp_trials.h: OneChannel where the call has one channel, TrialChannels for several), one host
// function runs either, and the operators of all channels are packed in a number of launches that
// does not depend on G; tbamp_r is per trial.
// amp_bamp_random_trials_run: the same run for generator_mode 'random' (one channel or several): the
// element-wise Bayes denoiser (BAMPLayer.random_denoiser, bamp.py:79-88) in tbamp_kb2, row by row,
// through the device function the launch engine's bamp_kb2 calls (amp_bamp.h bamp_bayes_rows); no
// max|xi| shift, so tbamp_r only reduces and settles the exit; decided by Loss.random_decision per
// trial (amp_trials_decide.hip).  The two entries above refuse that denoiser and that rule.
#include <algorithm>
#include <mutex>

#include "amp_bamp.h"

namespace amp {

constexpr int TBRWG = 1024;

struct alignas(16) TBampIter {
    int32_t stopped, T, fixed, fixed_all;
};

// what the trial engine keeps beside BampK: trial e's record, advanced in place by tbamp_r, and the
// count of trials whose allclose exit has fired
struct BampTrials {
    TBampIter* iters;      // [E]
    unsigned* nstop;
};

struct TBampWs {
    float *Wabs2, *WH, *Wabs2T, *WHH, *v, *z, *invu, *s, *cov, *var1, *secmax, *secabs;
    Partial* parts;
    TBampIter* iters;
    int* band[4];
    unsigned* nstop;
    void* dec;
    size_t bytes;
};

// G: channels whose packed operators and band ranges the workspace holds (one channel keeps the dense
// band ranges: the bytes amp_bamp_trials_workspace_bytes answers)
static TBampWs tbamp_carve(const amp_dims* d, int E, void* base, int G = 1) {
    BampK P;
    bamp_geometry(d, E, P);
    Carve cv(base);
    TBampWs w;
    w.Wabs2 = cv.take<float>((size_t)G * P.ncpA1 * P.kapA1);
    w.WH = cv.take<float>((size_t)G * P.ncpA2 * P.kapA2);
    w.Wabs2T = cv.take<float>((size_t)G * P.ncpB1 * P.kapB1);
    w.WHH = cv.take<float>((size_t)G * P.ncpB2 * P.kapB2);
    w.v = cv.take<float>((size_t)E * d->n);
    w.z = cv.take<float>((size_t)E * 2 * d->n);
    w.invu = cv.take<float>((size_t)E * P.ild);
    w.s = cv.take<float>((size_t)E * P.sld);
    w.cov = cv.take<float>((size_t)E * d->N);
    w.var1 = cv.take<float>((size_t)E * d->N);
    w.secmax = cv.take<float>((size_t)E * d->L);
    w.secabs = cv.take<float>((size_t)E * d->L);
    w.parts = cv.take<Partial>((size_t)E * (P.ncpB2 / P.bn));
    w.iters = cv.take<TBampIter>((size_t)E);
    const int nts[4] = {P.ncpA1 / 128, P.ncpA2 / 128, P.ncpB1 / 128, P.ncpB2 / P.bn};
    for (int i = 0; i < 4; ++i) w.band[i] = cv.take<int>(G == 1 ? (size_t)2 * nts[i] : (size_t)G * band_stride(nts[i]));
    w.nstop = cv.take<unsigned>(16);
    w.dec = cv.take<char>(trials_decide_ws_bytes(d, E));
    w.bytes = cv.off;
    return w;
}

// The entry of every GEMM kernel.  false (workgroup-uniform) when every trial has stopped or no row
// of the tile is live (rows up to the channel's limit; s_stop then holds the tile's row flags for
// LiveRows); else P holds channel ct.g's operator w and band ranges.  The stop counter is compared
// with E (P.B) whatever the channels.
template <class CH>
__device__ __forceinline__ bool tbamp_enter(BampK& P, const BampTrials& R, const CH& ch, const ChannelTile& ct, int w,
                                            const float*& wt, int* s_stop) {
    if (*R.nstop >= (unsigned)P.B) return false;
    if (!tile_rows_live(R.iters, ct.row0, ct.lim, s_stop)) return false;
    wt += ch.woff(ct.g, w);
    if (P.band[w]) P.band[w] += ch.boff(ct.g, w);
    return true;
}

// The four GEMM kernels, each written once over the channel mapping CH (amp_trials.h): row tile rb
// is channel ct.g's, its rows staged and guarded up to ct.lim, then the launch engine's gemm_tile
// call and epilogue: a row has the bits of its own B = 1 forward with that channel, wherever in a
// tile it lies (a first row that is no multiple of 32, or odd, changes no alignment: every row
// stride is even, lda of ALoadPair's 8-byte loads included).
// KC: the A chunk of the f32 tile, as amp_bamp.hip launches it (256 at the narrow column tile);
// the chunking does not change the MFMA order: the same bits.
// bamp_ka1.  AL: var's loader (ALoadPair where N % 4 == 2)
template <class AL, class CH>
__global__ __launch_bounds__(AMP_WG) void tbamp_ka1(BampK P, BampTrials R, CH ch, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_stop[GBM];
    const GemmTile tile = xcd_tile();
    const ChannelTile ct = ch.tile(tile.rb, P.B);
    const int row0 = ct.row0, col0 = tile.cb * 128;
    if (!tbamp_enter(P, R, ch, ct, 0, P.Wabs2, s_stop)) return;
    gemm_tile<128, AL, 256>(AL{bvar(P, t + 1), P.N, ct.lim, P.N}, P.Wabs2, P.kapA1, row0, col0, lds,
                            bkb(P, 0, tile.cb), bke(P, 0, tile.cb));
    bamp_store_v(P, LiveRows{s_stop}, lds, row0, col0);
}

// bamp_ka2
template <class CH>
__global__ __launch_bounds__(AMP_WG) void tbamp_ka2(BampK P, BampTrials R, CH ch, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_stop[GBM];
    const GemmTile tile = xcd_tile();
    const ChannelTile ct = ch.tile(tile.rb, P.B);
    const int row0 = ct.row0, col0 = tile.cb * 128;
    if (!tbamp_enter(P, R, ch, ct, 1, P.WH, s_stop)) return;
    const int twoN = 2 * P.N;
    gemm_tile<128, ALoadPlain, 256>(ALoadPlain{P.xm, twoN, ct.lim, twoN}, P.WH, P.kapA2, row0, col0, lds,
                                    bkb(P, 1, tile.cb), bke(P, 1, tile.cb));
    bamp_residual(P, LiveRows{s_stop}, lds, row0, col0);
}

// bamp_kb1
template <class CH>
__global__ __launch_bounds__(AMP_WG) void tbamp_kb1(BampK P, BampTrials R, CH ch, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_stop[GBM];
    const GemmTile tile = xcd_tile();
    const ChannelTile ct = ch.tile(tile.rb, P.B);
    const int row0 = ct.row0, col0 = tile.cb * 128;
    if (!tbamp_enter(P, R, ch, ct, 2, P.Wabs2T, s_stop)) return;
    gemm_tile<128, ALoadPlain, 256>(ALoadPlain{P.invu, P.ild, ct.lim, P.ild}, P.Wabs2T, P.kapB1, row0, col0, lds,
                                    bkb(P, 2, tile.cb), bke(P, 2, tile.cb));
    bamp_store_cov(P, LiveRows{s_stop}, lds, row0, col0);
}

// bamp_kb2, the denoiser row by row: each live row's own partial, in the slot its B = 1 forward
// stores it to, from scratch past the C tile (later rows still read the tile and the 1 / tau tile).
// P.elementwise (amp_bamp_random_trials_run): the row's element-wise denoiser, bamp_kb2's call
// (bamp_bayes_rows) on that one row, its BN / 2 columns on the threads of the row's B = 1 forward.
template <int BN, int KK, int KC, class CH>
__global__ __launch_bounds__(AMP_WG) void tbamp_kb2(BampK P, BampTrials R, CH ch, Const64 c64, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_stop[GBM];
    using C = GemmCfg<BN, KC>;
    const GemmTile tile = xcd_tile();
    const ChannelTile ct = ch.tile(tile.rb, P.B);
    const int row0 = ct.row0, col0 = tile.cb * BN;
    if (!tbamp_enter(P, R, ch, ct, 3, P.WHH, s_stop)) return;
    gemm_tile<BN, ALoadPlain, KC>(ALoadPlain{P.s, P.sld, ct.lim, P.sld}, P.WHH, P.kapB2, row0, col0, lds,
                                  bkb(P, 3, tile.cb), bke(P, 3, tile.cb));
    const int nrows = min(GBM, ct.lim - row0), ncols = min(BN, 2 * P.N - col0);
    const float* sit = bamp_xmap<BN, KC>(P, LiveRows{s_stop}, lds, row0, col0, nrows, ncols);
    const int nct = P.ncpB2 / BN, slot = seq_part_slot(tile.cb, nct);
    for (int rho = 0; rho < nrows; ++rho) {
        if (s_stop[rho]) continue;   // workgroup-uniform
        PartAcc pa;
        if (P.elementwise) {
            bamp_bayes_rows<BN, KC, KK>(P, c64, t, lds, row0, col0, rho, 1, ncols, pa);
        } else {
            const BampDenoisePolicy pol = bamp_policy<BN, KC>(P, t, lds, sit, row0, col0, ncols, rho);
            denoise_sections<true, KK>(pol, pol.spr, P.M, P.c, pa);
        }
        part_block_store(pa, P.parts + (size_t)(row0 + rho) * nct + slot, lds + C::CTILE_FLOATS);
    }
}

// Workgroup e: trial e's reduction, exact float64 fix-up against its own max|xi| and allclose
// decision (bamp.py:140) — bamp_r + bamp_fixall of amp_bamp.hip on the trial's rows, every trial in
// parallel.  The element-wise denoiser has no max|xi| shift and leaves the section statistics of its
// partials neutral (maxabs 0, minsecmax +inf): neither the all-NaN fill nor the fix-up is entered, the
// workgroup reduces the partials and settles stopped, T, the status record and the stop counter.
__global__ __launch_bounds__(TBRWG) void tbamp_r(BampK P, BampTrials R, Const64 c64, int t) {
    __shared__ __attribute__((aligned(16))) float lds[512];
    __shared__ double s_fix[TBRWG / 64];
    __shared__ int s_nc[TBRWG / 64];
    if (*R.nstop >= (unsigned)P.B) return;
    const int e = blockIdx.x, nct = P.ncpB2 / P.bn;
    const TBampIter cur = R.iters[e];
    if (cur.stopped) return;
    PartAcc pa = part_reduce_all(P.parts + (size_t)e * nct, nct, lds);
    uint32_t notclose = pa.notclose;
    int fixed = 0;
    if (P.elementwise) {
        // nothing to settle but the allclose count
    } else if (part_allnan(pa)) {
        if (!cur.fixed_all) nan_fill(P.xm + (size_t)e * 2 * P.N, bvar(P, t) + (size_t)e * P.N, (size_t)P.N);
        notclose = 1u;
        fixed = -1;
    } else if (part_danger(pa)) {
        const size_t o0 = (size_t)e * P.N;
        const int M = P.M;
        int dnc = 0;
        auto ldf = [&](int s) { return bamp_section_load(P, o0 + (size_t)s * M); };
        auto stf = [&](int s) { return bamp_section_store(P, t, o0 + (size_t)s * M, &dnc); };
        double G;
        fixed = fixup_sections<true>(P.L, M, P.secmax + (size_t)e * P.L, P.secabs + (size_t)e * P.L, pa.maxabs, c64,
                                     ldf, stf, &G, s_fix);
        notclose = (uint32_t)((int)notclose + block_sum(dnc, s_nc));
    }
    if (threadIdx.x == 0) {
        TBampIter nx;
        nx.stopped = notclose == 0 ? 1 : 0;
        nx.T = t + 1;
        nx.fixed = fixed;
        nx.fixed_all = (fixed < 0) ? 1 : 0;
        R.iters[e] = nx;
        if (nx.stopped || t + 1 == P.max_iter) P.status[e] = bamp_status(P, t, fixed, nx.stopped);
        if (nx.stopped) __hip_atomic_fetch_add(R.nstop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Tracker (bamp.py:13-25) for every trial, its record and the stop counter
__global__ void tbamp_init_kernel(BampK P, BampTrials R) {
    bamp_init_state(P);
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < P.B; e += gridDim.x * blockDim.x)
        R.iters[e] = TBampIter{0, 0, 0, 0};
    if (blockIdx.x == 0 && threadIdx.x == 0) *R.nstop = 0u;
}

// Trial e's last executed iteration wrote var into buffer (T_e - 1) & 1; buffer 0 is the caller's.
__global__ __launch_bounds__(256) void tbamp_output_kernel(BampK P) {
    const int e = blockIdx.x;
    const int T = P.status[e].T;
    if (((T - 1) & 1) == 0) return;
    for (int i = threadIdx.x; i < P.N; i += blockDim.x) P.var0[(size_t)e * P.N + i] = P.var1[(size_t)e * P.N + i];
}

constexpr size_t TB_LDS_S = GemmCfg<128, 256>::LDS_BYTES;   // within the default 64 KB
constexpr size_t TB_LDS_W = GemmCfg<256>::LDS_BYTES;

static std::once_flag g_tbamp_once;
static int g_tbamp_rc = 0;
static int tbamp_attrs() {
    std::call_once(g_tbamp_once, [] {
        for (int K : {1, 2, 4, 8, 16, 64})
            dispatch_K(K, [](auto kk) {
                constexpr int KK = decltype(kk)::value;
                if (!g_tbamp_rc) g_tbamp_rc = set_lds_attr<256>((const void*)tbamp_kb2<256, KK, GKC, OneChannel>);
                if (!g_tbamp_rc) g_tbamp_rc = set_lds_attr<256>((const void*)tbamp_kb2<256, KK, GKC, TrialChannels>);
            });
    });
    return g_tbamp_rc;
}

template <int KK, class CH>
static void tbamp_launch_kb2(const BampK& P, const BampTrials& R, const CH& ch, const Const64& c64, int gr, int t,
                             hipStream_t st) {
    if (P.bn == 128)
        hipLaunchKernelGGL((tbamp_kb2<128, KK, 256, CH>), dim3(gr, P.ncpB2 / 128), dim3(AMP_WG), TB_LDS_S, st, P, R, ch,
                           c64, t);
    else
        hipLaunchKernelGGL((tbamp_kb2<256, KK, GKC, CH>), dim3(gr, P.ncpB2 / 256), dim3(AMP_WG), TB_LDS_W, st, P, R, ch,
                           c64, t);
}

// iteration t's four GEMM launches over gr row tiles
template <class CH>
static void tbamp_launch_gemms(const BampK& P, const BampTrials& R, const CH& ch, const Const64& c64, int gr, int t,
                               hipStream_t st) {
    if (P.N % 4 != 0)
        hipLaunchKernelGGL((tbamp_ka1<ALoadPair, CH>), dim3(gr, P.ncpA1 / 128), dim3(AMP_WG), TB_LDS_S, st, P, R, ch, t);
    else
        hipLaunchKernelGGL((tbamp_ka1<ALoadPlain, CH>), dim3(gr, P.ncpA1 / 128), dim3(AMP_WG), TB_LDS_S, st, P, R, ch, t);
    hipLaunchKernelGGL(tbamp_ka2<CH>, dim3(gr, P.ncpA2 / 128), dim3(AMP_WG), TB_LDS_S, st, P, R, ch, t);
    hipLaunchKernelGGL(tbamp_kb1<CH>, dim3(gr, P.ncpB1 / 128), dim3(AMP_WG), TB_LDS_S, st, P, R, ch, t);
    dispatch_K(P.c.K, [&](auto kk) { tbamp_launch_kb2<decltype(kk)::value>(P, R, ch, c64, gr, t, st); });
}

// The operators of G channels (H: c64 [G][n][N]) and their band ranges, each channel's own, in a
// number of launches that does not depend on G: 4 builds + 4 x 3 for the ranges
static int tbamp_pack_ch(const BampK& P, const TrialChannels& CH, const float2* H, int G, hipStream_t st) {
    int rc;
    const size_t sg = (size_t)P.n * P.N;
    if ((rc = build_abs2_weight_ch(H, sg, P.N, 1, P.n, P.N, (float*)P.Wabs2, CH.wstride[0], P.kapA1, P.ncpA1, G, st))) return rc;
    if ((rc = build_cweight_ch(H, sg, P.N, 1, 0, P.n, P.N, (float*)P.WH, CH.wstride[1], P.kapA2, P.ncpA2, G, st))) return rc;
    if ((rc = build_abs2_weight_ch(H, sg, 1, P.N, P.N, P.n, (float*)P.Wabs2T, CH.wstride[2], P.kapB1, P.ncpB1, G, st))) return rc;
    if ((rc = build_cweight_ch(H, sg, 1, P.N, 1, P.N, P.n, (float*)P.WHH, CH.wstride[3], P.kapB2, P.ncpB2, G, st))) return rc;
    if (!P.band[0]) return AMP_OK;
    const float* wts[4] = {P.Wabs2, P.WH, P.Wabs2T, P.WHH};
    const int kaps[4] = {P.kapA1, P.kapA2, P.kapB1, P.kapB2}, ncps[4] = {P.ncpA1, P.ncpA2, P.ncpB1, P.ncpB2};
    const int bns[4] = {128, 128, 128, P.bn};
    for (int i = 0; i < 4; ++i)
        if ((rc = weight_kband_ch(wts[i], CH.wstride[i], kaps[i], ncps[i], bns[i], const_cast<int*>(P.band[i]),
                                  CH.bstride[i], G, st)))
            return rc;
    return AMP_OK;
}

// Every entry.  fn: the entry that was called (amp_bamp_trials_run passes per_channel = trials: one
// channel); a->H holds the G = ceil(trials / per_channel) channels in order.  random
// (amp_bamp_random_trials_run): the element-wise denoiser (a->denoiser == 1, the prior a->P0 / a->Ps)
// and the 'random' decision rule; the other entries refuse both.
static int tbamp_run(const amp_dims* d, const amp_constellation* c, const amp_bamp_args* a,
                     const amp_trials_decide_args* dec, int trials, int per_channel, const char* fn, hipStream_t st,
                     bool random = false) {
    int rc = check_dims(d, c, true, true);   // any n, any even N, a partial last column tile (amp_bamp_run)
    if (rc) return rc;
    AMP_REQUIRE(d->B == 1, "%s: dims describe ONE trial (B = %d, must be 1)", fn, d->B);
    AMP_REQUIRE(trials >= 1, "%s: trials = %d", fn, trials);
    AMP_REQUIRE(per_channel >= 1, "%s: per_channel = %d", fn, per_channel);
    AMP_REQUIRE(bamp_index_ok(d, trials), "%s: %d trials of max(2N, 2n) = %d columns need more than 32-bit offsets "
                "(or more than 65535 column tiles)", fn, trials, 2 * std::max(d->N, d->n));
    AMP_REQUIRE(a && a->H && a->y && a->xmap && a->xmmse && a->var && a->status && a->ws, "%s: null pointer argument",
                fn);
    AMP_REQUIRE(a->max_iter > 0, "%s: max_iter must be positive", fn);
    if (random)
        AMP_REQUIRE(a->denoiser == 1, "%s: denoiser %d (this entry runs the element-wise denoiser, 1)", fn, a->denoiser);
    else
        AMP_REQUIRE(a->denoiser == 0, "%s: the element-wise denoiser ('random' mode) has no independent-trial form", fn);
    AMP_REQUIRE(a->gemm == AMP_GEMM_AUTO || a->gemm == AMP_GEMM_F32, "%s: f32 GEMMs only (gemm %d)", fn, a->gemm);
    const int E = trials;
    int per = per_channel;
    const int G = trial_channels(E, per);
    AMP_REQUIRE(G <= WCH_MAX, "%s: %d channels (at most %d per call: a grid axis)", fn, G, WCH_MAX);
    TrialsDecide td{};
    // the 'random' rule's own limits (Na <= 64) before the workspace is looked at
    if (random && dec && (rc = trials_decide_args(d, dec, a->xmap, a->xmmse, td, true))) return rc;
    const TBampWs w = tbamp_carve(d, E, a->ws, G);
    AMP_REQUIRE(a->ws_bytes >= w.bytes, "%s: workspace %zu < %zu bytes", fn, a->ws_bytes, w.bytes);
    if (!random && dec && (rc = trials_decide_args(d, dec, a->xmap, a->xmmse, td))) return rc;
    if ((rc = tbamp_attrs())) return rc;
    BampK P{};             // f32 tiles (h2 = x3 = 0); the block denoiser unless `random`
    bamp_geometry(d, E, P);
    P.max_iter = a->max_iter;
    P.sigma2 = (float)a->noise_var;
    P.elementwise = random ? 1 : 0;
    P.P0 = a->P0;
    P.Ps = a->Ps;
    P.Wabs2 = w.Wabs2; P.WH = w.WH; P.Wabs2T = w.Wabs2T; P.WHH = w.WHH;   // channel 0's; the GEMM kernels step to theirs
    P.y = (const float*)a->y; P.v = w.v; P.z = w.z; P.invu = w.invu; P.s = w.s; P.cov = w.cov;
    P.xmap = (float*)a->xmap; P.xm = (float*)a->xmmse; P.var0 = (float*)a->var; P.var1 = w.var1;
    P.secmax = w.secmax; P.secabs = w.secabs; P.parts = w.parts;
    P.status = (amp_status*)a->status;
    const bool band = d->Lin > 1 || d->Lout > 1;   // block-banded H (channel.py:75-95)
    for (int i = 0; i < 4; ++i) P.band[i] = band ? w.band[i] : nullptr;
    P.c = to_const(c);
    TrialChannels CH{};
    CH.per = per; CH.tpg = cdiv(per, GBM);
    const int kaps[4] = {P.kapA1, P.kapA2, P.kapB1, P.kapB2}, ncps[4] = {P.ncpA1, P.ncpA2, P.ncpB1, P.ncpB2};
    const int bns[4] = {128, 128, 128, P.bn};
    for (int i = 0; i < 4; ++i) {
        CH.wstride[i] = (size_t)ncps[i] * kaps[i];
        CH.bstride[i] = G == 1 ? 2 * (ncps[i] / bns[i]) : band_stride(ncps[i] / bns[i]);
    }
    const BampTrials R{w.iters, w.nstop};
    const Const64 c64 = to_const64(c);
    if ((rc = tbamp_pack_ch(P, CH, (const float2*)a->H, G, st))) return rc;   // every channel's operators, once per call
    const size_t tot = std::max((size_t)E * P.N, (size_t)E * P.n);
    hipLaunchKernelGGL(tbamp_init_kernel, dim3((int)std::min<size_t>((tot + 255) / 256, 2048)), dim3(256), 0, st, P, R);
    AMP_LAUNCH_CHECK("tbamp_init");
    const int gr = G * CH.tpg;                     // <= E row tiles; one channel: cdiv(E, 32)
    for (int t = 0; t < P.max_iter; ++t) {
        if (G == 1)
            tbamp_launch_gemms(P, R, OneChannel{}, c64, gr, t, st);
        else
            tbamp_launch_gemms(P, R, CH, c64, gr, t, st);
        hipLaunchKernelGGL(tbamp_r, dim3(E), dim3(TBRWG), 0, st, P, R, c64, t);
        AMP_LAUNCH_CHECK("tbamp iteration");
    }
    hipLaunchKernelGGL(tbamp_output_kernel, dim3(E), dim3(256), 0, st, P);
    AMP_LAUNCH_CHECK("tbamp_output");
    return dec ? trials_decide_launch(d, c, td, E, w.dec, st) : AMP_OK;
}

}  // namespace amp

using namespace amp;

extern "C" {

size_t amp_bamp_trials_workspace_bytes(const amp_dims* d, int32_t max_iter, int32_t trials) {
    if (!d || max_iter <= 0 || trials <= 0 || d->B != 1) return 0;
    return tbamp_carve(d, trials, nullptr).bytes;
}

int amp_bamp_trials_run(const amp_dims* d, const amp_constellation* c, const amp_bamp_args* a,
                        const amp_trials_decide_args* dec, int32_t trials, void* stream) {
    return tbamp_run(d, c, a, dec, trials, trials, "amp_bamp_trials_run", (hipStream_t)stream);
}

size_t amp_bamp_trials_ch_workspace_bytes(const amp_dims* d, int32_t max_iter, int32_t trials, int32_t per_channel) {
    if (!d || max_iter <= 0 || trials <= 0 || per_channel < 1 || d->B != 1) return 0;
    if (d->N <= 0 || d->n <= 0 || d->M <= 0 || d->N % 2 != 0 || !bamp_index_ok(d, trials)) return 0;
    int per = per_channel;
    const int G = trial_channels(trials, per);
    if (G > WCH_MAX) return 0;
    return tbamp_carve(d, trials, nullptr, G).bytes;
}

int amp_bamp_trials_ch_run(const amp_dims* d, const amp_constellation* c, const amp_bamp_args* a,
                           const amp_trials_decide_args* dec, int32_t trials, int32_t per_channel, void* stream) {
    return tbamp_run(d, c, a, dec, trials, per_channel, "amp_bamp_trials_ch_run", (hipStream_t)stream);
}

// the carve is amp_bamp_trials_ch_run's (the decision's workspace holds either rule's partials)
size_t amp_bamp_random_trials_workspace_bytes(const amp_dims* d, int32_t max_iter, int32_t trials, int32_t per_channel) {
    return amp_bamp_trials_ch_workspace_bytes(d, max_iter, trials, per_channel);
}

int amp_bamp_random_trials_run(const amp_dims* d, const amp_constellation* c, const amp_bamp_args* a,
                               const amp_trials_decide_args* dec, int32_t trials, int32_t per_channel, void* stream) {
    return tbamp_run(d, c, a, dec, trials, per_channel, "amp_bamp_random_trials_run", (hipStream_t)stream, true);
}

}  // extern "C"

// amp_scamp_trials.hip — SCAMP over E independent single-trial detections that share one channel
// (amp_scamp_trials_run): the launch engine's parameter block (ScampK with B = E rows, iters one
// record per trial), f32 tiles and epilogues (amp_scamp.h) with per-row records.
//
// Restates, for every trial e alone, SCAMP.forward at B = 1 (scamp.py:77-107) with its Tracker
// (scamp.py:8-25), SCAMPLayer.forward (scamp.py:43-59), the mean-only block denoiser (scamp.py:61-68,
// the max|xi| shift of scamp.py:65 over the trial's own logits) and the allclose exit on the
// trial's own psi (scamp.py:105) — the way the reference's driver runs it (batch = 1, res epochs
// per channel: scamp_model.py:88, 95).
// Per iteration: two GEMM launches over row tiles of 32 trials, each kernel the entry guard (a tile
// whose rows have all stopped returns at once), the launch engine's gemm_tile call and its epilogue
// under the LiveRows guard (a stopped row is never stored to); the denoiser and the in-tile psi run
// row by row with one partial per (tile, row); tscamp_psi where a tile holds part of a coupling
// block; then tscamp_r, a grid over the trials: workgroup e reduces trial e's partials and either
// settles its exit or leaves a pending exact float64 fix-up in the trial's record, which
// tscamp_fix_sec and tscamp_fix_psi_fin (also grids over the trials) carry out against the trial's
// own max|xi|.  Every kernel returns at once when the stop counter has reached E.
// amp_scamp_trials_ch_run: the same over G channels, trial e on channel e / per_channel.  One kernel
// family serves both entries: the two GEMM kernels are templates over the channel mapping
// (amp_trials.h: OneChannel where the call has one channel, TrialChannels for several), one host
// function runs either, and the operators of all channels are packed in a number of launches that
// does not depend on G; every other kernel is per trial.
#include <algorithm>
#include <mutex>

#include "amp_scamp.h"

namespace amp {

// what the trial engine keeps beside ScampK (whose iters holds trial e's record, advanced in place)
struct ScampTrials {
    unsigned* nstop;       // trials whose allclose exit has fired
    int* fixcnt;           // [E] sections recomputed by tscamp_fix_sec
    unsigned* psi_nc;      // [E][Lin] allclose flags of tscamp_psi (split tiles only)
};

struct TScampWs {
    float *WA, *WAH, *z, *s, *phi, *tau, *psi1, *secmax, *secabs;
    Partial* parts;
    unsigned* psi_nc;
    int* fixcnt;
    ScampIter* iters;
    int *bandA, *bandB;
    unsigned* nstop;
    void* dec;
    size_t bytes;
};

// G: channels whose packed operators and band ranges the workspace holds (one channel keeps the dense
// band ranges: the bytes amp_scamp_trials_workspace_bytes answers)
static TScampWs tscamp_carve(const amp_dims* d, int E, void* base, int G = 1) {
    ScampK P;
    scamp_geometry(d, E, P);
    Carve cv(base);
    TScampWs w;
    w.WA = cv.take<float>((size_t)G * P.ncpA * P.kapA);
    w.WAH = cv.take<float>((size_t)G * P.ncpB * P.kapB);
    w.z = cv.take<float>((size_t)E * 2 * d->n);
    w.s = cv.take<float>((size_t)E * scamp_sld(d->n));
    w.phi = cv.take<float>((size_t)2 * E * d->Lout);
    w.tau = cv.take<float>((size_t)E * d->Lin);
    w.psi1 = cv.take<float>((size_t)E * d->Lin);
    w.secmax = cv.take<float>((size_t)E * d->L);
    w.secabs = cv.take<float>((size_t)E * d->L);
    w.parts = cv.take<Partial>((size_t)E * (P.ncpB / P.bn));
    w.psi_nc = cv.take<unsigned>((size_t)E * d->Lin);
    w.fixcnt = cv.take<int>((size_t)E);
    w.iters = cv.take<ScampIter>((size_t)E);
    w.bandA = cv.take<int>(G == 1 ? (size_t)2 * (P.ncpA / 128) : (size_t)G * band_stride(P.ncpA / 128));
    w.bandB = cv.take<int>(G == 1 ? (size_t)2 * (P.ncpB / P.bn) : (size_t)G * band_stride(P.ncpB / P.bn));
    w.nstop = cv.take<unsigned>(16);
    w.dec = cv.take<char>(trials_decide_ws_bytes(d, E));
    w.bytes = cv.off;
    return w;
}

// The entry of both GEMM kernels.  false (workgroup-uniform) when every trial has stopped or no row
// of the tile is live (rows up to the channel's limit; s_stop then holds the tile's row flags for
// LiveRows); else operator w (0: A, 1: A^H) and its band ranges are channel ct.g's.  The stop
// counter is compared with E (P.B) whatever the channels.
template <class CH>
__device__ __forceinline__ bool tscamp_enter(const ScampK& P, const ScampTrials& R, const CH& ch, const ChannelTile& ct,
                                             int w, const float*& wt, const int*& band, int* s_stop) {
    if (*R.nstop >= (unsigned)P.B) return false;
    if (!tile_rows_live(P.iters, ct.row0, ct.lim, s_stop)) return false;
    wt += ch.woff(ct.g, w);
    if (band) band += ch.boff(ct.g, w);
    return true;
}

// The two GEMM kernels, each written once over the channel mapping CH (amp_trials.h): row tile rb is
// channel ct.g's, its rows staged and guarded up to ct.lim, then the launch engine's gemm_tile call
// and epilogue: a row has the bits of its own B = 1 forward with that channel, wherever in a tile it
// lies.
// scamp_ka, every row on its own psi and phi.  KC = 256: the A chunk amp_scamp.hip launches for a
// block-banded A; the chunking does not change the MFMA order: the same bits.
template <class CH>
__global__ __launch_bounds__(AMP_WG) void tscamp_ka(ScampK P, ScampTrials R, CH ch, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_stop[GBM];
    const GemmTile tile = xcd_tile();
    const ChannelTile ct = ch.tile(tile.rb, P.B);
    const int row0 = ct.row0, col0 = tile.cb * 128;
    if (!tscamp_enter(P, R, ch, ct, 0, P.WA, P.bandA, s_stop)) return;
    const int twoN = 2 * P.N;
    const int kb = P.bandA ? P.bandA[2 * tile.cb] : 0, ke = P.bandA ? P.bandA[2 * tile.cb + 1] : -1;
    gemm_tile<128, ALoadPlain, 256>(ALoadPlain{P.xm, twoN, ct.lim, twoN}, P.WA, P.kapA, row0, col0, lds, kb, ke);
    scamp_residual<256>(P, LiveRows{s_stop}, t, lds, row0, col0);
}

// scamp_kb, the denoiser and the in-tile psi row by row: each live row's own partial, in the slot
// its B = 1 forward stores it to, from scratch past the C tile (LiveRows::PSCR: later rows still
// read the tile and the tau tile)
template <int BN, int KK, int KC, class CH>
__global__ __launch_bounds__(AMP_WG) void tscamp_kb(ScampK P, ScampTrials R, CH ch, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_stop[GBM];
    using C = GemmCfg<BN, KC>;
    const GemmTile tile = xcd_tile();
    const ChannelTile ct = ch.tile(tile.rb, P.B);
    const int row0 = ct.row0, col0 = tile.cb * BN;
    if (!tscamp_enter(P, R, ch, ct, 1, P.WAH, P.bandB, s_stop)) return;
    const int sld = scamp_sld(P.n);
    const int kb = P.bandB ? P.bandB[2 * tile.cb] : 0, ke = P.bandB ? P.bandB[2 * tile.cb + 1] : -1;
    gemm_tile<BN, ALoadPlain, KC>(ALoadPlain{P.s, sld, ct.lim, sld}, P.WAH, P.kapB, row0, col0, lds, kb, ke);
    const int nrows = min(GBM, ct.lim - row0), ncols = min(BN, 2 * P.N - col0);
    const ScampTileBlocks tb = scamp_tile_blocks(P, col0, ncols);
    const float* tau_t = scamp_xmap<BN, KC>(P, LiveRows{s_stop}, t, lds, row0, col0, nrows, ncols, tb);
    const int nct = P.ncpB / BN, slot = seq_part_slot(tile.cb, nct);
    for (int rho = 0; rho < nrows; ++rho) {
        if (s_stop[rho]) continue;   // workgroup-uniform
        const ScampDenoisePolicy pol = scamp_policy<BN, KC>(P, lds, tau_t, row0, col0, ncols, tb, rho);
        PartAcc pa;
        denoise_sections<false, KK>(pol, pol.spr, P.M, P.c, pa);
        __syncthreads();
        if (!P.psi_split && (int)threadIdx.x < tb.nlc)
            pa.notclose += scamp_psi_in_tile(P, t, row0 + rho, tb.lc0 + threadIdx.x);
        part_block_store(pa, P.parts + (size_t)(row0 + rho) * nct + slot, lds + C::CTILE_FLOATS);
    }
}

// psi (scamp.py:59) and its allclose flag (scamp.py:105) when the A^H tile holds only part of a
// coupling block (scamp_psi of amp_scamp.hip): one wavefront per (trial, coupling block), after
// every tile of the iteration is written; the flags are kept per trial.
__global__ __launch_bounds__(AMP_WG) void tscamp_psi(ScampK P, ScampTrials R, int t) {
    if (*R.nstop >= (unsigned)P.B) return;
    const int nwave = gridDim.x * (AMP_WG / 64);
    for (int blk = blockIdx.x * (AMP_WG / 64) + (threadIdx.x >> 6); blk < P.B * P.Lin; blk += nwave) {
        if (P.iters[blk / P.Lin].stopped) continue;   // wavefront-uniform
        const double ssum = scamp_block_energy(reinterpret_cast<const float2*>(P.xm) + (size_t)blk * P.Nt, P.Nt);
        if ((threadIdx.x & 63) == 0) R.psi_nc[blk] = (unsigned)scamp_psi_store(P, t, blk, ssum);
    }
}

constexpr int TSRWG = 256;

// scamp_finish of amp_scamp.hip for trial e: its record, its status and the stop counter
__device__ __forceinline__ void tscamp_finish(const ScampK& P, const ScampTrials& R, int e, int t, uint32_t notclose,
                                              int fixed, int fixed_all) {
    if (scamp_record(P, &P.iters[e], P.status + e, t, notclose, fixed, fixed_all))
        __hip_atomic_fetch_add(R.nstop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Workgroup e: trial e's reduction (scamp_r of amp_scamp.hip on the trial's rows): the all-NaN
// rule over the trial's own rows, the exit decision, or — when a section of the trial may leave the
// float64 range — the trial's exact float64 max |xi| into a pending record.
__global__ __launch_bounds__(TSRWG) void tscamp_r(ScampK P, ScampTrials R, Const64 c64, int t) {
    __shared__ __attribute__((aligned(16))) float lds[512];
    __shared__ double s_d[TSRWG / 64];
    __shared__ int s_i[TSRWG / 64];
    if (*R.nstop >= (unsigned)P.B) return;
    const int e = blockIdx.x, nct = P.ncpB / P.bn;
    const ScampIter cur = P.iters[e];
    if (cur.stopped) return;
    PartAcc pa = part_reduce_all(P.parts + (size_t)e * nct, nct, lds);
    if (P.psi_split) {
        int nc = 0;
        for (int i = threadIdx.x; i < P.Lin; i += blockDim.x) nc += (int)R.psi_nc[(size_t)e * P.Lin + i];
        pa.notclose += (uint32_t)block_sum(nc, s_i);
    }
    if (part_allnan(pa)) {
        if (!cur.fixed_all) {
            nan_fill(P.xm + (size_t)e * 2 * P.N, nullptr, (size_t)P.N);
            float* psi_new = spsi(P, t) + (size_t)e * P.Lin;
            for (int i = threadIdx.x; i < P.Lin; i += blockDim.x) psi_new[i] = __int_as_float(0x7fc00000);
        }
        if (threadIdx.x == 0) tscamp_finish(P, R, e, t, 1u, -1, 1);
    } else if (part_danger(pa)) {
        // exact float64 max |xi| of the trial over its candidate sections (those within the float32
        // estimate's slack of its float32 max)
        const double slack = logit_slack(pa.maxabs);
        const float* secabs = P.secabs + (size_t)e * P.L;
        double gm = 0.0;
        for (int sct = threadIdx.x; sct < P.L; sct += blockDim.x) {
            if ((double)secabs[sct] < pa.maxabs - slack) continue;
            gm = fmax(gm, section_absmax_f64(scamp_section_load(P, (size_t)e * P.N + (size_t)sct * P.M), P.M, c64));
        }
        gm = group_max(gm, 64);
        if ((threadIdx.x & 63) == 0) s_d[threadIdx.x >> 6] = gm;
        __syncthreads();
        if (threadIdx.x == 0) {
            double G = 0.0;
            for (int w = 0; w < TSRWG / 64; ++w) G = fmax(G, s_d[w]);
            P.iters[e] = scamp_pending(t, G, slack, pa.notclose);
        }
    } else if (threadIdx.x == 0) {
        tscamp_finish(P, R, e, t, pa.notclose, 0, 0);
    }
}

// Workgroup e: the sections of trial e that leave the float64 range against the trial's own G,
// recomputed with the reference's exact arithmetic (scamp_fix_sec).  Returns at once unless
// tscamp_r left the trial a pending record.
__global__ __launch_bounds__(TSRWG) void tscamp_fix_sec(ScampK P, ScampTrials R, Const64 c64, int t) {
    __shared__ int s_i[TSRWG / 64];
    if (*R.nstop >= (unsigned)P.B) return;
    const int e = blockIdx.x;
    const ScampIter pend = P.iters[e];
    if (!pend.active || pend.stopped) return;
    const float* secmax = P.secmax + (size_t)e * P.L;
    int cnt = 0;
    for (int sct = threadIdx.x; sct < P.L; sct += blockDim.x) {
        if (!((double)secmax[sct] - pend.G < AMP_DANGER + pend.slack)) continue;
        const size_t o0 = (size_t)e * P.N + (size_t)sct * P.M;
        exact_section_f64<false>(scamp_section_load(P, o0), scamp_section_store(P, o0), P.M, c64, pend.G);
        ++cnt;
    }
    cnt = block_sum(cnt, s_i);
    if (threadIdx.x == 0) R.fixcnt[e] = cnt;
}

// Workgroup e: psi of the coupling blocks of trial e that hold a recomputed section, the allclose
// delta, then the trial's exit, stop record and status (scamp_fix_psi_fin).
__global__ __launch_bounds__(TSRWG) void tscamp_fix_psi_fin(ScampK P, ScampTrials R, int t) {
    __shared__ int s_i[TSRWG / 64];
    if (*R.nstop >= (unsigned)P.B) return;
    const int e = blockIdx.x;
    const ScampIter pend = P.iters[e];
    if (!pend.active || pend.stopped) return;
    const size_t blk0 = (size_t)e * P.Lin;
    int dnc = 0;
    if (P.Nt > SFIX_SERIAL_NT) {
        for (int blk = threadIdx.x >> 6; blk < P.Lin; blk += blockDim.x >> 6)
            dnc += scamp_fix_psi_wave(P, t, blk0 + blk, pend);
    } else {
        for (int blk = threadIdx.x; blk < P.Lin; blk += blockDim.x) dnc += scamp_fix_psi_serial(P, t, blk0 + blk, pend);
    }
    dnc = block_sum(dnc, s_i);
    if (threadIdx.x == 0) tscamp_finish(P, R, e, t, (uint32_t)((int)pend.notclose + dnc), R.fixcnt[e], 0);
}

// Tracker (scamp.py:9-25) for every trial, its record and the stop counter
__global__ void tscamp_init_kernel(ScampK P, ScampTrials R) {
    scamp_init_state(P);
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < P.B; e += gridDim.x * blockDim.x)
        P.iters[e] = scamp_iter(0, 0, 0, 0, 0);
    if (blockIdx.x == 0 && threadIdx.x == 0) *R.nstop = 0u;
}

// Trial e's last executed iteration wrote psi into buffer (T_e - 1) & 1; buffer 0 is the caller's.
__global__ __launch_bounds__(64) void tscamp_output_kernel(ScampK P) {
    const int e = blockIdx.x;
    const int T = P.status[e].T;
    if (((T - 1) & 1) == 0) return;
    for (int i = threadIdx.x; i < P.Lin; i += blockDim.x) P.psi0[(size_t)e * P.Lin + i] = P.psi1[(size_t)e * P.Lin + i];
}

constexpr size_t TS_LDS_S = GemmCfg<128, 256>::LDS_BYTES;   // within the default 64 KB
constexpr size_t TS_LDS_W = GemmCfg<256>::LDS_BYTES;

static std::once_flag g_tscamp_once;
static int g_tscamp_rc = 0;
static int tscamp_attrs() {
    std::call_once(g_tscamp_once, [] {
        for (int K : {1, 2, 4, 8, 16, 64})
            dispatch_K(K, [](auto kk) {
                constexpr int KK = decltype(kk)::value;
                if (!g_tscamp_rc) g_tscamp_rc = set_lds_attr<256>((const void*)tscamp_kb<256, KK, GKC, OneChannel>);
                if (!g_tscamp_rc) g_tscamp_rc = set_lds_attr<256>((const void*)tscamp_kb<256, KK, GKC, TrialChannels>);
            });
    });
    return g_tscamp_rc;
}

template <int KK, class CH>
static void tscamp_launch_kb(const ScampK& P, const ScampTrials& R, const CH& ch, int gr, int t, hipStream_t st) {
    if (P.bn == 128)
        hipLaunchKernelGGL((tscamp_kb<128, KK, 256, CH>), dim3(gr, P.ncpB / 128), dim3(AMP_WG), TS_LDS_S, st, P, R, ch, t);
    else
        hipLaunchKernelGGL((tscamp_kb<256, KK, GKC, CH>), dim3(gr, P.ncpB / 256), dim3(AMP_WG), TS_LDS_W, st, P, R, ch, t);
}

// iteration t's two GEMM launches over gr row tiles
template <class CH>
static void tscamp_launch_gemms(const ScampK& P, const ScampTrials& R, const CH& ch, int gr, int t, hipStream_t st) {
    hipLaunchKernelGGL(tscamp_ka<CH>, dim3(gr, P.ncpA / 128), dim3(AMP_WG), TS_LDS_S, st, P, R, ch, t);
    dispatch_K(P.c.K, [&](auto kk) { tscamp_launch_kb<decltype(kk)::value>(P, R, ch, gr, t, st); });
}

// The operators of G channels (A: c64 [G][n][N]) and their band ranges, each channel's own, in a
// number of launches that does not depend on G: 2 builds + 2 x 3 for the ranges
static int tscamp_pack_ch(const ScampK& P, const TrialChannels& CH, const float2* A, int G, hipStream_t st) {
    int rc;
    const size_t sg = (size_t)P.n * P.N;
    if ((rc = build_cweight_ch(A, sg, P.N, 1, 0, P.n, P.N, (float*)P.WA, CH.wstride[0], P.kapA, P.ncpA, G, st))) return rc;
    if ((rc = build_cweight_ch(A, sg, 1, P.N, 1, P.N, P.n, (float*)P.WAH, CH.wstride[1], P.kapB, P.ncpB, G, st))) return rc;
    if (!P.bandA) return AMP_OK;
    if ((rc = weight_kband_ch(P.WA, CH.wstride[0], P.kapA, P.ncpA, 128, const_cast<int*>(P.bandA), CH.bstride[0], G, st)))
        return rc;
    return weight_kband_ch(P.WAH, CH.wstride[1], P.kapB, P.ncpB, P.bn, const_cast<int*>(P.bandB), CH.bstride[1], G, st);
}

// any Nt (amp_scamp_run's shapes); the byte query answers 0 for dims the run would refuse
static bool tscamp_shape_ok(const amp_dims* d, int E) {
    return d->Nt > 0 && d->Na > 0 && d->Nr > 0 && d->Lin > 0 && d->Lout > 0 && d->Lin <= SMAXLIN &&
           d->N == d->Nt * d->Lin && d->n == d->Nr * d->Lout && scamp_index_ok(d, E);
}

// Both entries.  fn: the entry that was called (amp_scamp_trials_run passes per_channel = trials:
// one channel); a->A holds the G = ceil(trials / per_channel) channels in order.
static int tscamp_run(const amp_dims* d, const amp_constellation* c, const amp_scamp_args* a,
                      const amp_trials_decide_args* dec, int trials, int per_channel, const char* fn, hipStream_t st) {
    int rc = check_dims(d, c, true, true);   // any Nt, a partial last column tile (amp_scamp_run)
    if (rc) return rc;
    AMP_REQUIRE(d->B == 1, "%s: dims describe ONE trial (B = %d, must be 1)", fn, d->B);
    AMP_REQUIRE(trials >= 1, "%s: trials = %d", fn, trials);
    AMP_REQUIRE(per_channel >= 1, "%s: per_channel = %d", fn, per_channel);
    AMP_REQUIRE(a && a->W && a->A && a->y && a->xmap && a->xmmse && a->psi && a->status && a->ws,
                "%s: null pointer argument", fn);
    AMP_REQUIRE(a->max_iter > 0, "%s: max_iter must be positive", fn);
    AMP_REQUIRE(d->Lin <= SMAXLIN, "%s: Lin = %d > %d", fn, d->Lin, SMAXLIN);
    AMP_REQUIRE(scamp_index_ok(d, trials), "%s: %d trials of max(2N, 2n) = %d columns need more than 32-bit offsets "
                "(or more than 65535 column tiles)", fn, trials, 2 * std::max(d->N, d->n));
    AMP_REQUIRE(a->engine == AMP_ENGINE_AUTO || a->engine == AMP_ENGINE_LAUNCHES, "%s: launch engine only (engine %d)",
                fn, a->engine);
    AMP_REQUIRE(a->gemm == AMP_GEMM_AUTO || a->gemm == AMP_GEMM_F32, "%s: f32 GEMMs only (gemm %d)", fn, a->gemm);
    const int E = trials;
    int per = per_channel;
    const int G = trial_channels(E, per);
    AMP_REQUIRE(G <= WCH_MAX, "%s: %d channels (at most %d per call: a grid axis)", fn, G, WCH_MAX);
    const TScampWs w = tscamp_carve(d, E, a->ws, G);
    AMP_REQUIRE(a->ws_bytes >= w.bytes, "%s: workspace %zu < %zu bytes", fn, a->ws_bytes, w.bytes);
    TrialsDecide td{};
    if (dec && (rc = trials_decide_args(d, dec, a->xmap, a->xmmse, td))) return rc;
    if ((rc = tscamp_attrs())) return rc;
    ScampK P{};            // f32 tiles (lx3 = 0); the persistent engine's fields stay null
    scamp_geometry(d, E, P);
    P.max_iter = a->max_iter;
    P.sigma2 = (float)a->noise_var;
    P.W = (const float*)a->W;          // ONE W: channel.py:80-83 builds it from the config alone
    P.WA = w.WA; P.WAH = w.WAH;        // channel 0's; the GEMM kernels step to their channel's
    P.y = (const float*)a->y; P.z = w.z; P.s = w.s; P.phi = w.phi; P.tau = w.tau;
    P.xmap = (float*)a->xmap; P.xm = (float*)a->xmmse; P.psi0 = (float*)a->psi; P.psi1 = w.psi1;
    P.secmax = w.secmax; P.secabs = w.secabs; P.parts = w.parts;
    P.iters = w.iters;
    P.status = (amp_status*)a->status;
    const bool band = d->Lin > 1 || d->Lout > 1;   // block-banded A (channel.py:75-95)
    P.bandA = band ? w.bandA : nullptr;
    P.bandB = band ? w.bandB : nullptr;
    P.c = to_const(c);
    TrialChannels CH{};
    CH.per = per; CH.tpg = cdiv(per, GBM);
    CH.wstride[0] = (size_t)P.ncpA * P.kapA; CH.wstride[1] = (size_t)P.ncpB * P.kapB;
    CH.bstride[0] = G == 1 ? 2 * (P.ncpA / 128) : band_stride(P.ncpA / 128);
    CH.bstride[1] = G == 1 ? 2 * (P.ncpB / P.bn) : band_stride(P.ncpB / P.bn);
    const ScampTrials R{w.nstop, w.fixcnt, w.psi_nc};
    const Const64 c64 = to_const64(c);
    if ((rc = tscamp_pack_ch(P, CH, (const float2*)a->A, G, st))) return rc;   // every channel's operators, once per call
    const size_t tot = std::max(std::max((size_t)E * P.N, (size_t)E * P.n), (size_t)E * std::max(P.Lout, P.Lin));
    hipLaunchKernelGGL(tscamp_init_kernel, dim3((int)std::min<size_t>((tot + 255) / 256, 2048)), dim3(256), 0, st, P, R);
    AMP_LAUNCH_CHECK("tscamp_init");
    const int gr = G * CH.tpg;                     // <= E row tiles; one channel: cdiv(E, 32)
    const int npsi = std::max(1, std::min(cdiv(E * P.Lin, AMP_WG / 64), 2048));
    for (int t = 0; t < P.max_iter; ++t) {
        if (G == 1)
            tscamp_launch_gemms(P, R, OneChannel{}, gr, t, st);
        else
            tscamp_launch_gemms(P, R, CH, gr, t, st);
        if (P.psi_split) hipLaunchKernelGGL(tscamp_psi, dim3(npsi), dim3(AMP_WG), 0, st, P, R, t);
        hipLaunchKernelGGL(tscamp_r, dim3(E), dim3(TSRWG), 0, st, P, R, c64, t);
        hipLaunchKernelGGL(tscamp_fix_sec, dim3(E), dim3(TSRWG), 0, st, P, R, c64, t);
        hipLaunchKernelGGL(tscamp_fix_psi_fin, dim3(E), dim3(TSRWG), 0, st, P, R, t);
        AMP_LAUNCH_CHECK("tscamp iteration");
    }
    hipLaunchKernelGGL(tscamp_output_kernel, dim3(E), dim3(64), 0, st, P);
    AMP_LAUNCH_CHECK("tscamp_output");
    return dec ? trials_decide_launch(d, c, td, E, w.dec, st) : AMP_OK;
}

}  // namespace amp

using namespace amp;

extern "C" {

size_t amp_scamp_trials_workspace_bytes(const amp_dims* d, int32_t max_iter, int32_t trials) {
    if (!d || max_iter <= 0 || trials <= 0 || d->B != 1 || !tscamp_shape_ok(d, trials)) return 0;
    return tscamp_carve(d, trials, nullptr).bytes;
}

int amp_scamp_trials_run(const amp_dims* d, const amp_constellation* c, const amp_scamp_args* a,
                         const amp_trials_decide_args* dec, int32_t trials, void* stream) {
    return tscamp_run(d, c, a, dec, trials, trials, "amp_scamp_trials_run", (hipStream_t)stream);
}

size_t amp_scamp_trials_ch_workspace_bytes(const amp_dims* d, int32_t max_iter, int32_t trials, int32_t per_channel) {
    if (!d || max_iter <= 0 || trials <= 0 || per_channel < 1 || d->B != 1 || !tscamp_shape_ok(d, trials)) return 0;
    int per = per_channel;
    const int G = trial_channels(trials, per);
    if (G > WCH_MAX) return 0;
    return tscamp_carve(d, trials, nullptr, G).bytes;
}

int amp_scamp_trials_ch_run(const amp_dims* d, const amp_constellation* c, const amp_scamp_args* a,
                            const amp_trials_decide_args* dec, int32_t trials, int32_t per_channel, void* stream) {
    return tscamp_run(d, c, a, dec, trials, per_channel, "amp_scamp_trials_ch_run", (hipStream_t)stream);
}

}  // extern "C"

// amp_vamp_trials.hip — VAMP over E independent single-trial detections that share one channel
// (amp_vamp_trials_run): the launch engine (amp_vamp.hip) with per-row records.
//
// Every trial e alone is VAMP.forward at B = 1 (vamp.py:159-187) on the trial's own var — the way
// the reference's drivers run it (batch = 1, res epochs per channel: vamp_model.py:91, 98).  The
// bodies are the launch engine's own, written once in amp_vamp_launch.h; the kernels here call them
// with the tile's records in LDS (VampLiveRows) where amp_vamp.hip passes the one record of
// iteration t.
//
// Per iteration t, three launches on one stream, no host synchronisation:
//   tvamp_k1  GEMM1 over row tiles of 32 trials, each row's r~ and LMMSE epilogue with its own record.
//   tvamp_k2  GEMM2 and its epilogue with the row's record, then the section denoiser row by row:
//             one partial per (tile, row).
//   tvamp_r   a grid over the trials: workgroup e is vamp_r on trial e as a batch of one (its own
//             partials, max|xi| shift, fix-up, allclose count and next record).
// A stopped trial's rows are frozen: no kernel stores to them again.  A tile whose rows have all
// stopped returns at once, and every kernel returns at once when the stop counter has reached E.
// A row's GEMM result does not depend on the other rows of its tile (each MFMA output row reduces
// its own A row only), so a trial's values are those of its own B = 1 forward on the launch engine.
// amp_vamp_trials_ch_run: the same over G channels, trial e on channel e / per_channel
// (vamp_model.py:45-61 redraws the channel every `res` epochs).  One kernel family serves both
// entries: tvamp_k1 / tvamp_k2 / tvamp_r are templates over the channel mapping (amp_trials.h:
// OneChannel where the call has one channel, TrialChannels for several) and take the channel's view
// of the parameter block at their entry (Wt1, Wt2, s, s2 and the channel's last row as the row
// limit); one host function runs either; y~ is gemm_store_ch with each channel's Wt0, the
// iteration-0 record is one per channel, and the operators of all channels are packed in three
// launches.
#include <algorithm>
#include <mutex>

#include "amp_vamp_launch.h"

namespace amp {

struct TVampWs {
    float *Wt0, *Wt1, *Wt2, *s2, *ytil, *w, *var1, *secmax, *secabs;
    Partial* parts;     // [E][nct]: trial e's partial of column tile slot j (rewritten every iteration)
    VampIter* iters;    // [E]: trial e's record, advanced in place by tvamp_r
    unsigned* nstop;    // trials whose allclose exit has fired
    void* dec;          // per-trial decision workspace
    size_t bytes;
};

// floats between two channels' s2 in a workspace of G channels: whole 256-byte granules, so G
// channels cost exactly G times one channel's bytes (one channel: the dense k)
inline size_t tvamp_s2_stride(int k, int G) { return G == 1 ? (size_t)k : (size_t)round_up(k, 64); }

// G: channels whose packed operators and s2 the workspace holds (one channel: the bytes
// amp_vamp_trials_workspace_bytes answers)
static TVampWs tvamp_carve(const amp_dims* d, int k, int E, void* base, int G = 1) {
    VampK P;
    vamp_geometry(d, k, P);
    Carve cv(base);
    TVampWs w;
    w.Wt0 = cv.take<float>((size_t)G * P.ncp0 * P.kap0);
    w.Wt1 = cv.take<float>((size_t)G * P.ncp1 * P.kap1);
    w.Wt2 = cv.take<float>((size_t)G * P.ncp2 * P.kap2);
    w.s2 = cv.take<float>((size_t)G * tvamp_s2_stride(k, G));
    w.ytil = cv.take<float>((size_t)E * 2 * k);
    w.w = cv.take<float>((size_t)E * P.wld);
    w.var1 = cv.take<float>((size_t)E * d->N);
    w.secmax = cv.take<float>((size_t)E * d->L);
    w.secabs = cv.take<float>((size_t)E * d->L);
    w.parts = cv.take<Partial>((size_t)E * (P.ncp2 / P.bn2));
    w.iters = cv.take<VampIter>((size_t)E);
    w.nstop = cv.take<unsigned>(16);
    w.dec = cv.take<char>(trials_decide_ws_bytes(d, E));
    w.bytes = cv.off;
    return w;
}

// The channel mapping CH (amp_trials.h) of the kernels below.  CH.wstride: floats between two
// channels' Wt0 / Wt1 / Wt2 / s2; the singular values lie dense, k apart.  A kernel takes the
// channel's view of its by-value P at the entry and calls the launch engine's bodies: a row has the
// bits of its own B = 1 forward with that channel, wherever in a tile it lies (every row stride is
// even: no alignment changes with a first row that is no multiple of 32, or odd).

// Tracker (vamp.py:22-26) for every trial, every channel's s2 and its own iteration-0 record
// (vamp_first_iter sums 1 / (s_i^2 + vr) over the channel's singular values: it depends on the
// channel and the SNR only), written to the channel's trials; the channels go grid-strided over the
// workgroups.  Once per call, so one runtime form for any G.
__global__ __launch_bounds__(256) void tvamp_init_kernel(VampK P, TrialChannels CH, int G, unsigned* nstop) {
    __shared__ __attribute__((aligned(16))) float lds[64];
    vamp_init_state(P);   // and channel 0's s2
    const size_t rest = (size_t)(G - 1) * P.k;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < rest; i += (size_t)gridDim.x * blockDim.x) {
        const size_t g = 1 + i / P.k, o = i % P.k;
        const float sv = P.s[g * P.k + o];
        P.s2[g * CH.wstride[3] + o] = sv * sv;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *nstop = 0u;
    for (int g = blockIdx.x; g < G; g += gridDim.x) {   // workgroup-uniform
        VampK Pg = P;
        Pg.s = P.s + (size_t)g * P.k;
        const VampIter it = vamp_first_iter(Pg, lds);
        const int lim = min((g + 1) * CH.per, P.B);
        for (int e = g * CH.per + threadIdx.x; e < lim; e += blockDim.x) P.iters[e] = it;
    }
}

// The entry of both GEMM kernels.  false (workgroup-uniform) when every trial has stopped or no row
// of the tile is live; else s_it holds the tile's records (rows of the next channel as stopped) and
// P is channel ct.g's: its operators, s and s2, and its last row + 1 as the row limit of the loaders
// and epilogues (P.B).  The stop counter is compared with E whatever the channels.
template <class CH>
__device__ __forceinline__ bool tvamp_enter(VampK& P, const CH& ch, const ChannelTile& ct, const unsigned* nstop,
                                            VampIter* s_it) {
    if (*nstop >= (unsigned)P.B) return false;
    if (!vamp_tile_records(P.iters, ct.row0, ct.lim, s_it)) return false;
    P.Wt1 += ch.woff(ct.g, 1);
    P.Wt2 += ch.woff(ct.g, 2);
    P.s2 += ch.woff(ct.g, 3);
    P.s += (size_t)ct.g * P.k;
    P.B = ct.lim;
    return true;
}

// GEMM1 over row tiles of 32 trials, each row's r~ and LMMSE epilogue with its own record
template <class CH>
__global__ __launch_bounds__(AMP_WG) void tvamp_k1(VampK P, CH ch, const unsigned* nstop) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ VampIter s_it[GBM];
    const GemmTile tile = xcd_tile();
    const ChannelTile ct = ch.tile(tile.rb, P.B);
    const int row0 = ct.row0, col0 = tile.cb * 128;
    if (!tvamp_enter(P, ch, ct, nstop, s_it)) return;
    const VampLiveRows g{s_it};
    gemm_tile<128>(vamp_aload_rt(P, g, row0), P.Wt1, P.kap1, row0, col0, lds);
    vamp_lmmse_epilogue(P, g, lds, row0, col0);
}

template <int BN, int KK, class CH>
__global__ __launch_bounds__(AMP_WG) void tvamp_k2(VampK P, CH ch, int t, const unsigned* nstop) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ VampIter s_it[GBM];
    const GemmTile tile = xcd_tile();
    const ChannelTile ct = ch.tile(tile.rb, P.B);
    const int row0 = ct.row0, col0 = tile.cb * BN;
    if (!tvamp_enter(P, ch, ct, nstop, s_it)) return;
    const VampLiveRows g{s_it};
    gemm_tile<BN, ALoadPlain, GKC, VAMP_SEG2>(ALoadPlain{P.w, P.wld, ct.lim, P.wld}, P.Wt2, P.kap2, row0, col0, lds);
    const int nrows = min(GBM, ct.lim - row0), ncols = min(BN, 2 * P.N - col0);
    vamp_r_epilogue<BN>(P, g, lds, row0, col0, nrows, ncols);
    // the denoiser row by row, the row's own partial in the slot its B = 1 forward stores it to
    // (s_it is workgroup-uniform: no divergent barrier)
    const int nct = P.ncp2 / BN, slot = seq_part_slot(tile.cb, nct);
    for (int rho = 0; rho < nrows; ++rho) {
        if (!g.live(rho)) continue;
        const VampDenoisePolicy pol = vamp_policy<BN>(P, g, t, lds, row0, col0, ncols, rho);
        PartAcc pa;
        denoise_sections<true, KK>(pol, pol.spr, P.M, P.c, pa);
        part_block_store(pa, P.parts + (size_t)(row0 + rho) * nct + slot, lds + GemmCfg<BN>::CTILE_FLOATS);
    }
}
template <class CH>
struct TVampK2 {
    template <int BN, int KK>
    static constexpr auto fn() { return &tvamp_k2<BN, KK, CH>; }
};

// Workgroup e after K2(t): vamp_r (amp_vamp.hip) on trial e's rows, every trial in parallel, with
// P.s at the singular values of trial e's channel (vamp_lmmse_scalars' mean(scale), vamp.py:68-71).
template <class CH>
__global__ __launch_bounds__(RWG) void tvamp_r(VampK PE, CH ch, Const64 c64, int t, unsigned* nstop) {
    __shared__ __attribute__((aligned(16))) float lds[512];
    if (*nstop >= (unsigned)PE.B) return;
    const int e = blockIdx.x;
    const VampIter cur = PE.iters[e];
    if (cur.stopped) return;
    // the trial as a batch of one
    VampK P = PE;
    const int nct = PE.ncp2 / PE.bn2;
    P.B = 1; P.Bmean = 1;
    P.s = PE.s + (size_t)ch.of(e) * PE.k;
    P.r = PE.r + (size_t)e * 2 * PE.N; P.xm = PE.xm + (size_t)e * 2 * PE.N;
    P.var0 = PE.var0 + (size_t)e * PE.N; P.var1 = PE.var1 + (size_t)e * PE.N;
    P.secmax = PE.secmax + (size_t)e * PE.L; P.secabs = PE.secabs + (size_t)e * PE.L;
    P.parts = PE.parts + (size_t)e * nct;
    const VampIter nx = vamp_reduce(P, c64, cur, P.parts, nct, &PE.iters[e], &PE.status[e], t, lds);
    if (threadIdx.x == 0 && nx.stopped) __hip_atomic_fetch_add(nstop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Trial e's last executed iteration wrote var into buffer (T_e - 1) & 1; buffer 0 is the caller's.
__global__ __launch_bounds__(256) void tvamp_output_kernel(VampK P) {
    const int e = blockIdx.x;
    const int T = P.status[e].T;
    if (((T - 1) & 1) == 0) return;
    for (int i = threadIdx.x; i < P.N; i += blockDim.x) P.var0[(size_t)e * P.N + i] = P.var1[(size_t)e * P.N + i];
}

static std::once_flag g_tvamp_attr_once;
static int g_tvamp_attr_rc = 0;

static int tvamp_attrs() {
    std::call_once(g_tvamp_attr_once, [] {
        int rc = set_lds_attr<128>((const void*)tvamp_k1<OneChannel>);
        if (!rc) rc = set_lds_attr<128>((const void*)tvamp_k1<TrialChannels>);
        if (!rc) rc = vamp_k2_attrs<TVampK2<OneChannel>>();
        g_tvamp_attr_rc = rc ? rc : vamp_k2_attrs<TVampK2<TrialChannels>>();
    });
    return g_tvamp_attr_rc;
}

// iteration t's three launches: K1 and K2 over gr row tiles, tvamp_r over the E trials
template <class CH>
static int tvamp_launch_iter(const VampK& P, const CH& ch, const Const64& c64, int gr, int t, unsigned* nstop,
                             hipStream_t st) {
    const dim3 g1(gr, P.ncp1 / 128), g2(gr, P.ncp2 / P.bn2);
    hipLaunchKernelGGL(tvamp_k1<CH>, g1, dim3(AMP_WG), GemmCfg<128>::LDS_BYTES, st, P, ch, (const unsigned*)nstop);
    AMP_LAUNCH_CHECK("tvamp_k1");
    dispatch_K(P.c.K, [&](auto kk) {
        constexpr int KK = decltype(kk)::value;
        if (P.bn2 == 128)
            hipLaunchKernelGGL((tvamp_k2<128, KK, CH>), g2, dim3(AMP_WG), GemmCfg<128>::LDS_BYTES, st, P, ch, t,
                               (const unsigned*)nstop);
        else
            hipLaunchKernelGGL((tvamp_k2<256, KK, CH>), g2, dim3(AMP_WG), GemmCfg<256>::LDS_BYTES, st, P, ch, t,
                               (const unsigned*)nstop);
    });
    AMP_LAUNCH_CHECK("tvamp_k2");
    hipLaunchKernelGGL(tvamp_r<CH>, dim3(P.B), dim3(RWG), 0, st, P, ch, c64, t, nstop);
    AMP_LAUNCH_CHECK("tvamp_r");
    return AMP_OK;
}

// vamp_pack_f32 for G channels (a->U c64 [G][n][k], a->s f32 [G][k], a->Vh c64 [G][k][N]), each
// channel's Wt0 scaled by its own singular values: three launches, whatever G
static int vamp_pack_f32_ch(const VampK& P, const TrialChannels& CH, const amp_vamp_args* a, int G, hipStream_t st) {
    int rc;
    const size_t su = (size_t)P.n * P.k, sv = (size_t)P.k * P.N;
    if ((rc = build_cweight_ch((const float2*)a->U, su, 1, P.k, 1, P.k, P.n, (float*)P.Wt0, CH.wstride[0], P.kap0,
                               P.ncp0, G, st, P.s, (size_t)P.k)))
        return rc;
    if ((rc = build_cweight_ch((const float2*)a->Vh, sv, P.N, 1, 0, P.k, P.N, (float*)P.Wt1, CH.wstride[1], P.kap1,
                               P.ncp1, G, st)))
        return rc;
    return build_cweight_ch((const float2*)a->Vh, sv, 1, P.N, 1, P.N, P.k, (float*)P.Wt2, CH.wstride[2], P.kap2, P.ncp2,
                            G, st);
}

// Both entries.  fn: the entry that was called (amp_vamp_trials_run passes per_channel = trials: one
// channel); a->U / a->s / a->Vh hold the G = ceil(trials / per_channel) channels in order.
static int tvamp_run(const amp_dims* d, const amp_constellation* c, const amp_vamp_args* a,
                     const amp_trials_decide_args* dec, int trials, int per_channel, const char* fn, hipStream_t st) {
    int rc = check_dims(d, c, true, true);   // any n, any k, any even N, a partial last column tile (amp_vamp_run)
    if (rc) return rc;
    AMP_REQUIRE(d->B == 1, "%s: dims describe ONE trial (B = %d, must be 1)", fn, d->B);
    AMP_REQUIRE(trials >= 1, "%s: trials = %d", fn, trials);
    AMP_REQUIRE(per_channel >= 1, "%s: per_channel = %d", fn, per_channel);
    AMP_REQUIRE(vamp_index_ok(d, trials), "%s: %d trials of max(2N, 2n) = %d columns need more than 32-bit offsets "
                "(or more than 65535 column tiles)", fn, trials, 2 * std::max(d->N, d->n));
    const int E = trials;
    int per = per_channel;
    const int G = trial_channels(E, per);
    AMP_REQUIRE(G <= WCH_MAX, "%s: %d channels (at most %d per call: a grid axis)", fn, G, WCH_MAX);
    AMP_REQUIRE(a && a->U && a->s && a->Vh && a->y && a->r && a->xmmse && a->var && a->status && a->ws,
                "%s: null pointer argument", fn);
    AMP_REQUIRE(a->k > 0 && a->k <= d->N && a->k <= d->n, "%s: k = %d must be min(n, N)", fn, a->k);
    AMP_REQUIRE(a->max_iter > 0, "%s: max_iter must be positive", fn);
    AMP_REQUIRE(a->engine == AMP_ENGINE_AUTO || a->engine == AMP_ENGINE_LAUNCHES,
                "%s: the persistent engine has no independent-trial form", fn);
    AMP_REQUIRE(a->gemm == AMP_GEMM_AUTO || a->gemm == AMP_GEMM_F32, "%s: f32 GEMMs only (gemm %d)", fn, a->gemm);
    const TVampWs w = tvamp_carve(d, a->k, E, a->ws, G);
    AMP_REQUIRE(a->ws_bytes >= w.bytes, "%s: workspace %zu < %zu bytes", fn, a->ws_bytes, w.bytes);
    TrialsDecide td{};
    if (dec && (rc = trials_decide_args(d, dec, a->r, a->xmmse, td))) return rc;
    VampK P{};
    vamp_geometry(d, a->k, P);
    P.B = E;            // rows; every per-trial quantity is formed over one row (tvamp_r: Bmean = 1)
    P.Bmean = 1;
    P.max_iter = a->max_iter;
    P.noise_var = a->noise_var;
    P.sparsity = a->sparsity;
    P.Wt0 = w.Wt0; P.Wt1 = w.Wt1; P.Wt2 = w.Wt2;   // channel 0's, as s and s2; the kernels step to theirs
    P.s = (const float*)a->s; P.s2 = w.s2; P.ytil = w.ytil; P.w = w.w;
    P.r = (float*)a->r; P.xm = (float*)a->xmmse;
    P.var0 = (float*)a->var; P.var1 = w.var1;
    P.secmax = w.secmax; P.secabs = w.secabs; P.parts = w.parts; P.iters = w.iters;
    P.status = (amp_status*)a->status;
    P.y = (const float*)a->y;
    P.x3 = 0;           // amp_status.gemm = AMP_ARITH_F32
    P.c = to_const(c);
    TrialChannels CH{};
    CH.per = per; CH.tpg = cdiv(per, GBM);
    CH.wstride[0] = (size_t)P.ncp0 * P.kap0; CH.wstride[1] = (size_t)P.ncp1 * P.kap1;
    CH.wstride[2] = (size_t)P.ncp2 * P.kap2; CH.wstride[3] = tvamp_s2_stride(P.k, G);
    const Const64 c64 = to_const64(c);
    if ((rc = tvamp_attrs())) return rc;
    if ((rc = vamp_pack_f32_ch(P, CH, a, G, st))) return rc;   // every channel's operators, once per call
    const int gi = (int)std::min<size_t>(((size_t)E * P.N + 255) / 256, 2048);
    hipLaunchKernelGGL(tvamp_init_kernel, dim3(gi), dim3(256), 0, st, P, CH, G, w.nstop);
    AMP_LAUNCH_CHECK("tvamp_init");
    rc = gemm_store_ch((const float*)a->y, 2 * P.n, E, 2 * P.n, P.Wt0, CH.wstride[0], P.kap0, P.ncp0, P.ytil, 2 * P.k,
                       2 * P.k, per, CH.tpg, G, st);
    if (rc) return rc;
    const int gr = G * CH.tpg;                     // <= E row tiles; one channel: cdiv(E, 32)
    for (int t = 0; t < P.max_iter; ++t) {
        rc = G == 1 ? tvamp_launch_iter(P, OneChannel{}, c64, gr, t, w.nstop, st)
                    : tvamp_launch_iter(P, CH, c64, gr, t, w.nstop, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(tvamp_output_kernel, dim3(E), dim3(256), 0, st, P);
    AMP_LAUNCH_CHECK("tvamp_output");
    return dec ? trials_decide_launch(d, c, td, E, w.dec, st) : AMP_OK;
}

}  // namespace amp

using namespace amp;

extern "C" {

size_t amp_vamp_trials_workspace_bytes(const amp_dims* d, int32_t k, int32_t max_iter, int32_t trials) {
    if (!d || k <= 0 || max_iter <= 0 || trials <= 0 || d->B != 1) return 0;
    return tvamp_carve(d, k, trials, nullptr).bytes;
}

int amp_vamp_trials_run(const amp_dims* d, const amp_constellation* c, const amp_vamp_args* a,
                        const amp_trials_decide_args* dec, int32_t trials, void* stream) {
    return tvamp_run(d, c, a, dec, trials, trials, "amp_vamp_trials_run", (hipStream_t)stream);
}

size_t amp_vamp_trials_ch_workspace_bytes(const amp_dims* d, int32_t k, int32_t max_iter, int32_t trials,
                                          int32_t per_channel) {
    if (!d || k <= 0 || max_iter <= 0 || trials <= 0 || per_channel < 1 || d->B != 1) return 0;
    if (d->N <= 0 || d->n <= 0 || d->M <= 0 || d->N % 2 != 0 || k > d->N || k > d->n || !vamp_index_ok(d, trials))
        return 0;
    int per = per_channel;
    const int G = trial_channels(trials, per);
    if (G > WCH_MAX) return 0;
    return tvamp_carve(d, k, trials, nullptr, G).bytes;
}

int amp_vamp_trials_ch_run(const amp_dims* d, const amp_constellation* c, const amp_vamp_args* a,
                           const amp_trials_decide_args* dec, int32_t trials, int32_t per_channel, void* stream) {
    return tvamp_run(d, c, a, dec, trials, per_channel, "amp_vamp_trials_ch_run", (hipStream_t)stream);
}

}  // extern "C"

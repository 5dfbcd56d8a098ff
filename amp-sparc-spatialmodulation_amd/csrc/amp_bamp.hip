// amp_bamp.hip — BAMP detector, device-resident iteration loop.
//
// Restates BAMP.forward (bamp.py:116-143) with its Tracker (bamp.py:12-25) and
// BAMPLayer.forward (bamp.py:48-64):
//   v = |H|^2 var ; z = H xmmse - v (y - z) / u ; u = v + sigma2 ;
//   cov = 1 / (|H|^2^T (1/u)) ; xmap = xmmse + cov (H^H ((y - z)/u)) ;
//   xmmse, var = denoiser(xmap, tau = cov/2)  (bamp.py:66-77)
// and the allclose(var) early exit (bamp.py:140).
// Per iteration: four fp32-MFMA GEMM launches with fused epilogues + one reduction /
// exact-float64 fix-up workgroup (same scheme as amp_vamp.hip).  The parameter block and the
// epilogues are amp_bamp.h's, shared with the independent-trial engine (amp_bamp_trials.hip): a
// GEMM kernel here is its entry guard, the tile of its arithmetic and one epilogue call.
#include <algorithm>
#include <mutex>

#include "amp_bamp.h"
#include "amp_gemm_h2.h"
#include "amp_gemm_x3.h"
#include <vector>
#include <cstdio>
#include "amp_host.h"

namespace amp {

constexpr int BRWG = 1024;

// BAMP's fp16x2 operator scale exponent (the opt-in AMP_GEMM_H2 form): every operator piece is
// scaled by 2^10, so |H|^2 must stay below 64 (|H| < 8; the channel's entries are ~CN(0, 1/Nr));
// larger entries overflow their fp16 piece, the result is then non-finite (NaN detections,
// counted as errors), never silently wrong
constexpr int BH2_EX = 10;

// the fp16x2 GEMMs need whole 64-wide reduction groups and output tiles (a block-banded H reduces
// over each tile's h2_kband range)
static inline bool bamp_h2_shape(const amp_dims* d) {
    return d->N % 64 == 0 && d->n % 64 == 0;
}

struct BampWs {
    float *Wabs2, *WH, *Wabs2T, *WHH, *v, *z, *invu, *s, *cov, *var1;
    unsigned short* ap;
    int* rexp;
    int* band[4];
    XState* xs;
    float *secmax, *secabs;
    Partial* parts;
    BampIter* iters;
    unsigned* rcnt;
    size_t bytes;
};

static BampWs bamp_carve(const amp_dims* d, int max_iter, void* base) {
    BampK P;
    bamp_geometry(d, d->B, P);
    Carve cv(base);
    BampWs w;
    // the split forms' shapes also hold the bf16x3 real operators: three 16-bit planes, 1.5x the
    // f32 weight, over the padded outputs the last column tile streams
    const bool x3 = bamp_h2_shape(d);
    w.Wabs2 = cv.take<float>((size_t)P.ncpA1 * P.kapA1 * (x3 ? 3 : 2) / 2);
    w.WH = cv.take<float>((size_t)P.ncpA2 * P.kapA2);
    w.Wabs2T = cv.take<float>((size_t)P.ncpB1 * P.kapB1 * (x3 ? 3 : 2) / 2);
    w.WHH = cv.take<float>((size_t)P.ncpB2 * P.kapB2);
    w.v = cv.take<float>((size_t)d->B * d->n);
    w.z = cv.take<float>((size_t)d->B * 2 * d->n);
    w.invu = cv.take<float>((size_t)d->B * P.ild);
    w.s = cv.take<float>((size_t)d->B * P.sld);
    w.cov = cv.take<float>((size_t)d->B * d->N);
    w.var1 = cv.take<float>((size_t)d->B * d->N);
    w.secmax = cv.take<float>((size_t)d->B * d->L);
    w.secabs = cv.take<float>((size_t)d->B * d->L);
    w.parts = cv.take<Partial>((size_t)max_iter * P.nblk);
    w.iters = cv.take<BampIter>((size_t)max_iter + 1);
    w.band[0] = cv.take<int>((size_t)2 * (P.ncpA1 / 128));
    w.band[1] = cv.take<int>((size_t)2 * (P.ncpA2 / 128));
    w.band[2] = cv.take<int>((size_t)2 * (P.ncpB1 / 128));
    w.band[3] = cv.take<int>((size_t)2 * (P.ncpB2 / P.bn));
    w.xs = cv.take<XState>(1);
    w.rcnt = cv.take<unsigned>(16);
    w.ap = nullptr;
    w.rexp = nullptr;
    if (bamp_h2_shape(d)) {
        // the A planes of either split form (fp16x2: four, bf16x3: six)
        const size_t rp = (size_t)round_up(d->B, GBM);
        w.ap = cv.take<unsigned short>(6 * rp * std::max(d->N, d->n));
        w.rexp = cv.take<int>(rp);
    }
    w.bytes = cv.off;
    return w;
}

// KC: the A chunk of the f32 tile (GKC; 256 for the block-banded H, whose short reduction ranges
// need no longer chunks: 33 KB of LDS, four tiles per CU instead of two; the fp16x2 tile only in
// the GKC instantiations).  The chunking does not change the MFMA order: the same bits.
// v = |H|^2 var (bamp.py:59).  AL: var's loader (ALoadPair where N % 4 == 2: the caller's rows are
// then only 8-byte aligned)
template <int KC = GKC, bool X3 = false, class AL = ALoadPlain>
__global__ __launch_bounds__(AMP_WG) void bamp_ka1(BampK P, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (P.iters[t].stopped) return;
    const GemmTile tile = (KC == GKC && P.tile_rows) ? xcd_tile_rows() : xcd_tile();
    const int row0 = tile.rb * GBM, col0 = tile.cb * 128;
    if constexpr (X3)
        gemm_tile_x3<128, false>(P.ap, P.rows_pad, P.N, P.Wabs2, row0, col0, lds, bkb(P, 0, tile.cb), bke(P, 0, tile.cb));
    else if (KC == GKC && P.h2)
        gemm_tile_h2<128, false>(P.ap, P.rows_pad, P.rexp, P.N, P.Wabs2, BH2_EX, row0, col0, lds, bkb(P, 0, tile.cb),
                                       bke(P, 0, tile.cb));
    else
        gemm_tile<128, AL, KC>(AL{bvar(P, t + 1), P.N, P.B, P.N}, P.Wabs2, P.kapA1, row0, col0, lds,
                               bkb(P, 0, tile.cb), bke(P, 0, tile.cb));
    bamp_store_v(P, AllRows{}, lds, row0, col0);
}

// z = H xmmse - v (y - z) / u ; u = v + sigma2 ; s = (y - z) / u   (bamp.py:60-63)
template <int KC = GKC, bool X3 = false>
__global__ __launch_bounds__(AMP_WG) void bamp_ka2(BampK P, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (P.iters[t].stopped) return;
    const GemmTile tile = (KC == GKC && P.tile_rows) ? xcd_tile_rows() : xcd_tile();
    const int row0 = tile.rb * GBM, col0 = tile.cb * 128;
    const int twoN = 2 * P.N;
    if constexpr (X3)
        gemm_tile_x3<128, true>(P.ap, P.rows_pad, P.N, P.WH, row0, col0, lds, bkb(P, 1, tile.cb), bke(P, 1, tile.cb));
    else if (KC == GKC && P.h2)
        gemm_tile_h2<128, true>(P.ap, P.rows_pad, P.rexp, P.N, P.WH, BH2_EX, row0, col0, lds, bkb(P, 1, tile.cb),
                                       bke(P, 1, tile.cb));
    else
        gemm_tile<128, ALoadPlain, KC>(ALoadPlain{P.xm, twoN, P.B, twoN}, P.WH, P.kapA2, row0, col0, lds,
                                       bkb(P, 1, tile.cb), bke(P, 1, tile.cb));
    bamp_residual(P, AllRows{}, lds, row0, col0);
}

// cov = 1 / (|H|^2^T (1/u))   (bamp.py:62)
template <int KC = GKC, bool X3 = false>
__global__ __launch_bounds__(AMP_WG) void bamp_kb1(BampK P, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (P.iters[t].stopped) return;
    const GemmTile tile = (KC == GKC && P.tile_rows) ? xcd_tile_rows() : xcd_tile();
    const int row0 = tile.rb * GBM, col0 = tile.cb * 128;
    if constexpr (X3)
        gemm_tile_x3<128, false>(P.ap, P.rows_pad, P.n, P.Wabs2T, row0, col0, lds, bkb(P, 2, tile.cb), bke(P, 2, tile.cb));
    else if (KC == GKC && P.h2)
        gemm_tile_h2<128, false>(P.ap, P.rows_pad, P.rexp, P.n, P.Wabs2T, BH2_EX, row0, col0, lds, bkb(P, 2, tile.cb),
                                       bke(P, 2, tile.cb));
    else
        gemm_tile<128, ALoadPlain, KC>(ALoadPlain{P.invu, P.ild, P.B, P.ild}, P.Wabs2T, P.kapB1, row0, col0, lds,
                                       bkb(P, 2, tile.cb), bke(P, 2, tile.cb));
    bamp_store_cov(P, AllRows{}, lds, row0, col0);
}

// xmap = xmmse + cov (H^H s) ; xmmse, var = denoiser(xmap, cov/2)   (bamp.py:63-64)
template <int BN, int KK, int KC = GKC, bool X3 = false>
__global__ __launch_bounds__(AMP_WG) void bamp_kb2(BampK P, Const64 c64, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (P.iters[t].stopped) return;
    using C = GemmCfg<BN, KC>;
    const GemmTile tile = (KC == GKC && P.tile_rows) ? xcd_tile_rows() : xcd_tile();
    const int row0 = tile.rb * GBM, col0 = tile.cb * BN;
    const int twoN = 2 * P.N;
    if constexpr (X3)
        gemm_tile_x3<BN, true>(P.ap, P.rows_pad, P.n, P.WHH, row0, col0, lds, bkb(P, 3, tile.cb), bke(P, 3, tile.cb));
    else if (KC == GKC && P.h2)
        gemm_tile_h2<BN, true>(P.ap, P.rows_pad, P.rexp, P.n, P.WHH, BH2_EX, row0, col0, lds, bkb(P, 3, tile.cb),
                               bke(P, 3, tile.cb));
    else
        gemm_tile<BN, ALoadPlain, KC>(ALoadPlain{P.s, P.sld, P.B, P.sld}, P.WHH, P.kapB2, row0, col0, lds,
                                      bkb(P, 3, tile.cb), bke(P, 3, tile.cb));
    const int nrows = min(GBM, P.B - row0), ncols = min(BN, twoN - col0);
    const float* sit = bamp_xmap<BN, KC>(P, AllRows{}, lds, row0, col0, nrows, ncols);
    const BampDenoisePolicy pol = bamp_policy<BN, KC>(P, t, lds, sit, row0, col0, ncols, 0);
    PartAcc pa;
    if (P.elementwise) {
        bamp_bayes_rows<BN, KC, KK>(P, c64, t, lds, row0, col0, 0, nrows, ncols, pa);   // amp_bamp.h
    } else {
        denoise_sections<true, KK>(pol, nrows * pol.spr, P.M, P.c, pa);
    }
    part_block_store(pa, P.parts + (size_t)t * P.nblk + blockIdx.y * gridDim.x + blockIdx.x, lds + C::CTILE_FLOATS);
}

// Iteration record t+1 (bamp.py:140): early exit when no var moved beyond allclose.
__device__ __forceinline__ void bamp_finish(const BampK& P, int t, uint32_t notclose, int fixed) {
    BampIter nx{};
    nx.stopped = notclose == 0 ? 1 : 0;
    nx.T = t + 1;
    nx.fixed = fixed;
    nx.fixed_all = (fixed < 0) ? 1 : 0;
    P.iters[t + 1] = nx;
    if (nx.stopped || t + 1 == P.max_iter) *P.status = bamp_status(P, t, fixed, nx.stopped);
}

// Reduction and allclose decision (bamp.py:140).  The rare exact-float64 path (a section's
// normaliser out of the float64 range against the batch-global shift, amp_denoise.h) is spread
// over the grid as SCAMP's is: this workgroup only settles the exact batch max |xi| G over the
// candidate sections and leaves a pending record; bamp_fix_sec_body recomputes the out-of-range
// sections (a grid kernel: at 64-QAM on a failing detector most sections of the batch take this
// path every iteration, 314 ms per cfg5 detection when one workgroup recomputed them all), and
// bamp_fin adds the per-block counts and decides the early exit (both in one launch, bamp_fixall,
// in the whole-batch engine; the trial-sharded stages split this work, bamp_xr*).
__global__ __launch_bounds__(BRWG) void bamp_r(BampK P, Const64 c64, int t) {
    __shared__ __attribute__((aligned(16))) float lds[512];
    __shared__ double s_d[BRWG / 64];
    const BampIter cur = P.iters[t];
    if (cur.stopped) {
        if (threadIdx.x == 0) P.iters[t + 1] = cur;
        return;
    }
    PartAcc pa = part_reduce_all(P.parts + (size_t)t * P.nblk, P.nblk, lds);
    if (part_allnan(pa)) {
        if (!cur.fixed_all) nan_fill(P.xm, bvar(P, t), (size_t)P.B * P.N);
        if (threadIdx.x == 0) bamp_finish(P, t, 1u, -1);
    } else if (part_danger(pa)) {
        const double slack = logit_slack(pa.maxabs);
        double gm = 0.0;
        for (int sct = threadIdx.x; sct < P.B * P.L; sct += blockDim.x) {
            if ((double)P.secabs[sct] < pa.maxabs - slack) continue;
            gm = fmax(gm, section_absmax_f64(bamp_section_load(P, (size_t)sct * P.M), P.M, c64));
        }
        gm = group_max(gm, 64);
        if ((threadIdx.x & 63) == 0) s_d[threadIdx.x >> 6] = gm;
        __syncthreads();
        if (threadIdx.x == 0) {
            double G = 0.0;
            for (int w = 0; w < BRWG / 64; ++w) G = fmax(G, s_d[w]);
            BampIter nx{};
            nx.stopped = 0; nx.T = t + 1; nx.fixed = 0; nx.fixed_all = 0;
            nx.G = G; nx.slack = slack; nx.notclose = pa.notclose; nx.active = 1;
            P.iters[t + 1] = nx;
        }
    } else if (threadIdx.x == 0) {
        bamp_finish(P, t, pa.notclose, 0);
    }
}

// per-block counts of bamp_fix_sec_body, written over iteration t's partials (consumed by
// bamp_r):
// slot i = {sections fixed, allclose delta} of block i
__device__ __forceinline__ int2* bamp_fix_counts(const BampK& P, int t) {
    return reinterpret_cast<int2*>(P.parts + (size_t)t * P.nblk);
}

// the out-of-range sections of a pending record, recomputed with the reference's exact float64
// op sequence (exact_section_f64): xmmse, var and the allclose delta against the previous var
__device__ __forceinline__ void bamp_fix_sec_body(const BampK& P, const Const64& c64, int t, const BampIter& pend,
                                                  int* s_i) {
    int cnt = 0, dnc = 0;
    for (int sct = blockIdx.x * blockDim.x + threadIdx.x; sct < P.B * P.L; sct += gridDim.x * blockDim.x) {
        if (!((double)P.secmax[sct] - pend.G < AMP_DANGER + pend.slack)) continue;
        const size_t o0 = (size_t)sct * P.M;
        exact_section_f64<true>(bamp_section_load(P, o0), bamp_section_store(P, t, o0, &dnc), P.M, c64, pend.G);
        ++cnt;
    }
    cnt = block_sum(cnt, s_i);
    dnc = block_sum(dnc, s_i);
    if (threadIdx.x == 0) bamp_fix_counts(P, t)[blockIdx.x] = make_int2(cnt, dnc);
}

// bamp_fix_sec_body, then (last workgroup to arrive) bamp_fin's count and exit decision: one launch
__global__ __launch_bounds__(AMP_WG) void bamp_fixall(BampK P, Const64 c64, int t) {
    __shared__ int s_i[AMP_WG / 64];
    const BampIter pend = P.iters[t + 1];
    if (!pend.active || P.iters[t].stopped) return;
    bamp_fix_sec_body(P, c64, t, pend, s_i);
    if (last_arrival(P.rcnt + 1, gridDim.x)) {
        const int2* c = bamp_fix_counts(P, t);
        int fixed = 0, dnc = 0;
        for (int i = threadIdx.x; i < (int)gridDim.x; i += blockDim.x) { fixed += c[i].x; dnc += c[i].y; }
        fixed = block_sum(fixed, s_i);
        dnc = block_sum(dnc, s_i);
        if (threadIdx.x == 0) bamp_finish(P, t, (uint32_t)((int)pend.notclose + dnc), fixed);
    }
}

// ---- trial-sharded iteration (amp_bamp_run_sharded; SURVEY §8(e) exact-compat) ----
// bamp_r split at its batch-global values, as the VAMP stages (amp_vamp.hip vamp_xr*): the
// not-close count (bamp.py:140) and max|xi| / min section max (bamp.py:70) after xr1, the rare
// path's exact max|xi| after xr2 and its recomputed sections' deltas after xr3.
__global__ __launch_bounds__(BRWG) void bamp_xr1(BampK P, int t) {
    __shared__ __attribute__((aligned(16))) float lds[512];
    XState* xs = P.xs;
    if (P.iters[t].stopped) {
        if (threadIdx.x == 0) { xs->sum[0] = xs->sum[1] = 0.0; xs->mx[0] = xs->mx[1] = 0.0; }
        return;
    }
    const PartAcc pa = part_reduce_all(P.parts + (size_t)t * P.nblk, P.nblk, lds);
    if (threadIdx.x == 0) {
        xs->sum[0] = 0.0;
        xs->sum[1] = (double)pa.notclose;
        xs->mx[0] = (pa.maxabs <= 1.7976931348623157e308) ? pa.maxabs : INFINITY;   // NaN / inf wins
        xs->mx[1] = (pa.minsecmax == pa.minsecmax) ? -pa.minsecmax : INFINITY;
    }
}

__device__ inline PartAcc bamp_xs_global(const XState& x) {
    PartAcc pa;
    pa.sumvar = 0.0;
    pa.notclose = (uint32_t)x.sum[1];
    pa.maxabs = x.mx[0];
    pa.minsecmax = -x.mx[1];
    return pa;
}

__global__ __launch_bounds__(BRWG) void bamp_xr2(BampK P, Const64 c64, int t) {
    __shared__ double s_d[BRWG / 64];
    XState* xs = P.xs;
    const BampIter cur = P.iters[t];
    if (cur.stopped) {
        if (threadIdx.x == 0) { P.iters[t + 1] = cur; xs->mode = 0; xs->gmax[0] = 0.0; }
        return;
    }
    PartAcc pa = bamp_xs_global(*xs);
    if (!part_allnan(pa) && part_danger(pa)) {
        const double G32 = pa.maxabs, slack = logit_slack(G32);
        double gm = 0.0;
        for (int sct = threadIdx.x; sct < P.B * P.L; sct += blockDim.x) {
            if (!((double)P.secabs[sct] >= G32 - slack)) continue;
            gm = fmax(gm, section_absmax_f64(bamp_section_load(P, (size_t)sct * P.M), P.M, c64));
        }
        gm = group_max(gm, 64);
        if ((threadIdx.x & 63) == 0) s_d[threadIdx.x >> 6] = gm;
        __syncthreads();
        if (threadIdx.x == 0) {
            double G = 0.0;
            for (int w = 0; w < BRWG / 64; ++w) G = fmax(G, s_d[w]);
            xs->gmax[0] = G;
            xs->mode = 2;
        }
        return;
    }
    int fixed = 0;
    if (part_allnan(pa)) {
        if (!cur.fixed_all) nan_fill(P.xm, bvar(P, t), (size_t)P.B * P.N);
        pa.notclose = 1;
        fixed = -1;
    }
    if (threadIdx.x == 0) {
        bamp_finish(P, t, pa.notclose, fixed);
        xs->mode = 0;
        xs->gmax[0] = 0.0;
    }
}

__global__ __launch_bounds__(BRWG) void bamp_xr3(BampK P, Const64 c64, int t) {
    __shared__ double s_d[2][BRWG / 64];
    XState* xs = P.xs;
    if (xs->mode != 2) {
        if (threadIdx.x == 0) xs->fix[0] = xs->fix[1] = xs->fix[2] = 0.0;
        return;
    }
    const PartAcc pa = bamp_xs_global(*xs);
    const double G = xs->gmax[0], slack = logit_slack(pa.maxabs);
    int dnc = 0, cnt = 0;
    for (int sct = threadIdx.x; sct < P.B * P.L; sct += blockDim.x) {
        if (!((double)P.secmax[sct] - G < AMP_DANGER + slack)) continue;
        ++cnt;
        const size_t o0 = (size_t)sct * P.M;
        exact_section_f64<true>(bamp_section_load(P, o0), bamp_section_store(P, t, o0, &dnc), P.M, c64, G);
    }
    dnc = group_sum(dnc, 64);
    cnt = group_sum(cnt, 64);
    if ((threadIdx.x & 63) == 0) { s_d[0][threadIdx.x >> 6] = (double)dnc; s_d[1][threadIdx.x >> 6] = (double)cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double b = 0.0, c = 0.0;
        for (int w = 0; w < BRWG / 64; ++w) { b += s_d[0][w]; c += s_d[1][w]; }
        xs->fix[0] = 0.0; xs->fix[1] = b; xs->fix[2] = c;
    }
}

__global__ void bamp_xr4(BampK P, int t) {
    const XState* xs = P.xs;
    if (xs->mode != 2 || threadIdx.x != 0) return;
    const PartAcc pa = bamp_xs_global(*xs);
    const long long nc = (long long)pa.notclose + (long long)xs->fix[1];
    bamp_finish(P, t, nc == 0 ? 0u : 1u, (int)xs->fix[2]);
}

// Tracker (bamp.py:13-25) and the record of iteration 0
__global__ void bamp_init_kernel(BampK P) {
    bamp_init_state(P);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        P.rcnt[0] = 0u; P.rcnt[1] = 0u;
        BampIter it{};
        it.stopped = 0; it.T = 0; it.fixed = 0; it.fixed_all = 0;
        P.iters[0] = it;
    }
}

__global__ void bamp_output_kernel(BampK P) {
    const int T = P.status->T;
    if (((T - 1) & 1) == 0) return;
    const size_t BN_ = (size_t)P.B * P.N;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < BN_; e += (size_t)gridDim.x * blockDim.x)
        P.var0[e] = P.var1[e];
}

// dynamic LDS of every BAMP GEMM launch: the f32 tile's A block or the split tiles' staged planes,
// whichever is larger (every arithmetic runs from the same instantiation)
constexpr size_t cmax(size_t a, size_t b) { return a > b ? a : b; }
constexpr size_t BLDS = cmax(h2_tile_lds<256, true>(), GemmCfg<256>::LDS_BYTES);
// the bf16x3 launches' LDS: the staged planes or the C tile + the epilogue's scratch past it (the
// partial-store scratch; bamp_kb2: + the 1 / tau tile): 48 KB for the complex tiles, three per CU
constexpr size_t XLDS_R = x3_tile_lds<128, false>(2048);
constexpr size_t XLDS_C = x3_tile_lds<128, true>(2048);
template <int BN>
constexpr size_t xlds_kb2() { return x3_tile_lds<BN, true>(2048 + GBM * (BN / 2)); }
static_assert(xlds_kb2<256>() <= BLDS && XLDS_C <= BLDS, "bf16x3 tiles within the attribute");
static_assert(BLDS <= 80 * 1024, "two BAMP GEMM workgroups per CU");
static int bamp_lds_attr(const void* fn) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BLDS);
    if (e != hipSuccess) {
        set_error("hipFuncSetAttribute: %s", hipGetErrorString(e));
        return AMP_E_LAUNCH;
    }
    return AMP_OK;
}
template <int KK>
static int bamp_kb2_attrs() {
    int rc = bamp_lds_attr((const void*)bamp_kb2<128, KK>);
    if (!rc) rc = bamp_lds_attr((const void*)bamp_kb2<256, KK, GKC, true>);
    return rc ? rc : bamp_lds_attr((const void*)bamp_kb2<256, KK>);   // the KC = 256 forms fit the default 64 KB
}

// The f32 tiles stage 256-wide A chunks (33 KB of LDS: four tiles per CU instead of two, the
// chunk loaded one ahead); AMP_BAMP_KC=512 keeps 512 (A/B runs).  The chunking does not change
// the MFMA order: the same bits.
constexpr size_t BSKC_LDS = GemmCfg<128, 256>::LDS_BYTES;
static bool bamp_short_chunks(const BampK& P) {
    static const bool off = [] {
        const char* e = diag_env("AMP_BAMP_KC");
        return e && atoi(e) == 512;
    }();
    // N % 4 == 2: always (the pair loader is instantiated at the short chunk only)
    return !P.h2 && !P.x3 && (!off || P.N % 4 != 0);
}

template <int KK>
static void launch_kb2_kk(const BampK& P, const Const64& c64, int gr, int t, hipStream_t st) {
    if (P.bn == 128 && bamp_short_chunks(P)) {
        hipLaunchKernelGGL((bamp_kb2<128, KK, 256>), dim3(gr, P.ncpB2 / 128), dim3(AMP_WG), BSKC_LDS, st, P, c64, t);
        return;
    }
    if (P.bn == 128) {
        if (P.x3)
            hipLaunchKernelGGL((bamp_kb2<128, KK, GKC, true>), dim3(gr, P.ncpB2 / 128), dim3(AMP_WG), xlds_kb2<128>(), st,
                               P, c64, t);
        else
            hipLaunchKernelGGL((bamp_kb2<128, KK>), dim3(gr, P.ncpB2 / 128), dim3(AMP_WG), BLDS, st, P, c64, t);
    } else {
        if (P.x3)
            hipLaunchKernelGGL((bamp_kb2<256, KK, GKC, true>), dim3(gr, P.ncpB2 / 256), dim3(AMP_WG), xlds_kb2<256>(), st,
                               P, c64, t);
        else
            hipLaunchKernelGGL((bamp_kb2<256, KK>), dim3(gr, P.ncpB2 / 256), dim3(AMP_WG), BLDS, st, P, c64, t);
    }
}

static void launch_kb2(const BampK& P, const Const64& c64, int gr, int t, hipStream_t st) {
    dispatch_K(P.c.K, [&](auto kk) { launch_kb2_kk<decltype(kk)::value>(P, c64, gr, t, st); });
}

static std::once_flag g_bamp_once;
static int g_bamp_rc = 0;

static int bamp_attrs() {
    std::call_once(g_bamp_once, [] {
        g_bamp_rc = bamp_lds_attr((const void*)bamp_ka1<>);
        if (!g_bamp_rc) g_bamp_rc = bamp_lds_attr((const void*)bamp_ka2<>);
        if (!g_bamp_rc) g_bamp_rc = bamp_lds_attr((const void*)bamp_kb1<>);
        if (!g_bamp_rc) g_bamp_rc = bamp_kb2_attrs<1>();
        if (!g_bamp_rc) g_bamp_rc = bamp_kb2_attrs<2>();
        if (!g_bamp_rc) g_bamp_rc = bamp_kb2_attrs<4>();
        if (!g_bamp_rc) g_bamp_rc = bamp_kb2_attrs<8>();
        if (!g_bamp_rc) g_bamp_rc = bamp_kb2_attrs<16>();
        if (!g_bamp_rc) g_bamp_rc = bamp_kb2_attrs<64>();
    });
    return g_bamp_rc;
}

}  // namespace amp

using namespace amp;

extern "C" {

size_t amp_bamp_workspace_bytes(const amp_dims* d, int32_t max_iter) {
    if (!d || max_iter <= 0) return 0;
    return bamp_carve(d, max_iter, nullptr).bytes;
}

}  // extern "C"

namespace amp {

// The parameter block of one BAMP forward from the C-ABI arguments (validated).
static int bamp_setup(const amp_dims* d, const amp_constellation* c, const amp_bamp_args* a, BampK& P, Const64& c64) {
    // any n and any even N (check_dims: M = Nt / Na a power of two); the column tiles take a partial
    // last tile, invu and s padded row strides, var at N % 4 == 2 the pair loader
    int rc = check_dims(d, c, true, true);
    if (rc) return rc;
    AMP_REQUIRE(bamp_index_ok(d, d->B), "amp_bamp_run: B = %d trials of max(2N, 2n) = %d columns need more than "
                "32-bit offsets (or more than 65535 column tiles)", d->B, 2 * std::max(d->N, d->n));
    AMP_REQUIRE(a && a->H && a->y && a->xmap && a->xmmse && a->var && a->status && a->ws,
                "amp_bamp_run: null pointer argument");
    AMP_REQUIRE(a->max_iter > 0, "amp_bamp_run: max_iter must be positive");
    // every argument check before the workspace is carved (the arithmetic's comment: below)
    AMP_REQUIRE(a->denoiser == 0 || a->denoiser == 1, "amp_bamp_run: denoiser %d", a->denoiser);
    AMP_REQUIRE(a->gemm == AMP_GEMM_AUTO || a->gemm == AMP_GEMM_F32 || a->gemm == AMP_GEMM_H2 || a->gemm == AMP_GEMM_X3,
                "amp_bamp_run: gemm %d (AUTO, F32, X3 or H2)", a->gemm);
    const bool h2ok = bamp_h2_shape(d);
    AMP_REQUIRE((a->gemm != AMP_GEMM_H2 && a->gemm != AMP_GEMM_X3) || h2ok,
                "amp_bamp_run: the split-precision GEMMs need N %% 64 == 0 and n %% 64 == 0 (N = %d, n = %d)", d->N, d->n);
    const BampWs w = bamp_carve(d, a->max_iter, a->ws);
    AMP_REQUIRE(a->ws_bytes >= w.bytes, "amp_bamp_run: workspace %zu < %zu bytes", a->ws_bytes, w.bytes);
    rc = bamp_attrs();
    if (rc) return rc;
    bamp_geometry(d, d->B, P);
    P.max_iter = a->max_iter;
    P.sigma2 = (float)a->noise_var;
    P.Wabs2 = w.Wabs2; P.WH = w.WH; P.Wabs2T = w.Wabs2T; P.WHH = w.WHH;
    P.y = (const float*)a->y; P.v = w.v; P.z = w.z; P.invu = w.invu; P.s = w.s; P.cov = w.cov;
    P.xmap = (float*)a->xmap; P.xm = (float*)a->xmmse; P.var0 = (float*)a->var; P.var1 = w.var1;
    P.secmax = w.secmax; P.secabs = w.secabs; P.parts = w.parts; P.iters = w.iters; P.status = (amp_status*)a->status;
    P.c = to_const(c);
    P.xs = w.xs;
    P.rcnt = w.rcnt;
    {
        // block-banded H: the ranges are formed by the prepare launch sequence (AMP_BAND_GEMM=0: off)
        const char* e = diag_env("AMP_BAND_GEMM");
        const bool band = (d->Lin > 1 || d->Lout > 1) && !(e && e[0] == '0');
        for (int i = 0; i < 4; ++i) P.band[i] = band ? w.band[i] : nullptr;
    }
    P.elementwise = a->denoiser;
    P.P0 = a->P0;
    P.Ps = a->Ps;
    // GEMM arithmetic, all at the reference's c64 operand precision (bamp.py:59-64) unless fp16x2 is
    // asked for: AMP_GEMM_F32 (f32 MFMA), AMP_GEMM_X3 (bf16x3 tiles, 24-bit operands) or, only when
    // asked for (AMP_GEMM_H2, or AUTO with AMP_BAMP_GEMM=h2), the fp16x2 tile (22-bit operands:
    // narrower than the reference).  AUTO: f32 MFMA (AMP_BAMP_GEMM=x3: bf16x3 where the shape tiles).
    static const char gemm_env = [] {
        const char* e = diag_env("AMP_BAMP_GEMM");
        return e ? e[0] : '\0';
    }();
    P.h2 = (a->gemm == AMP_GEMM_H2 || (a->gemm == AMP_GEMM_AUTO && h2ok && gemm_env == 'h')) ? 1 : 0;
    P.x3 = (a->gemm == AMP_GEMM_X3 || (a->gemm == AMP_GEMM_AUTO && h2ok && gemm_env == 'x')) ? 1 : 0;
    // tile order: the fp16x2 tiles walk row blocks (each XCD serves the whole 4 MB operator from its
    // L2); the bf16x3 operator (6 MB at cfg5) does not fit, so its tiles walk column blocks (each
    // XCD keeps its share of the operator resident).  AMP_BAMP_X3_ROWS=1: row-major (A/B runs).
    static const bool x3_rows = [] {
        const char* e = diag_env("AMP_BAMP_X3_ROWS");
        return e && e[0] == '1';
    }();
    P.tile_rows = P.h2 || (P.x3 && x3_rows) ? 1 : 0;
    P.rows_pad = round_up(d->B, GBM);
    P.ap = w.ap;
    P.rexp = w.rexp;
    c64 = to_const64(c);
    return AMP_OK;
}

// Tracker (bamp.py:13-25): the four weights and the initial state.
static int bamp_prepare_impl(const BampK& P, const amp_bamp_args* a, hipStream_t st) {
    int rc;
    const float2* H = (const float2*)a->H;
    if (P.x3) {
        // the four operators as bf16x3 planes in ONE launch: |H|^2 (O = n, J = N), H (O = n, J = N),
        // |H|^2^T (O = N, J = n), H^H (O = N, J = n)
        CWeightJob j[4];
        j[0] = CWeightJob{H, P.N, 1, 0, nullptr, P.n, P.N, (float*)P.Wabs2, P.N, P.n, WPACKX3_ABS2, 0};
        j[1] = CWeightJob{H, P.N, 1, 0, nullptr, P.n, P.N, (float*)P.WH, P.N, P.n, WPACKX3, 0};
        j[2] = CWeightJob{H, 1, P.N, 0, nullptr, P.N, P.n, (float*)P.Wabs2T, P.n, P.N, WPACKX3_ABS2, 0};
        j[3] = CWeightJob{H, 1, P.N, 1, nullptr, P.N, P.n, (float*)P.WHH, P.n, P.N, WPACKX3, 0};
        if ((rc = build_cweights(j, 4, nullptr, 0, st))) return rc;
    } else if (P.h2) {
        // the four operators as fp16x2 planes (exponent BH2_EX) in ONE launch: |H|^2 (O = n, J = N),
        // H (O = n, J = N), |H|^2^T (O = N, J = n), H^H (O = N, J = n)
        CWeightJob j[4];
        j[0] = CWeightJob{H, P.N, 1, 0, nullptr, P.n, P.N, (float*)P.Wabs2, P.N, P.n, WPACKH2_ABS2, BH2_EX};
        j[1] = CWeightJob{H, P.N, 1, 0, nullptr, P.n, P.N, (float*)P.WH, P.N, P.n, WPACKH2, BH2_EX};
        j[2] = CWeightJob{H, 1, P.N, 0, nullptr, P.N, P.n, (float*)P.Wabs2T, P.n, P.N, WPACKH2_ABS2, BH2_EX};
        j[3] = CWeightJob{H, 1, P.N, 1, nullptr, P.N, P.n, (float*)P.WHH, P.n, P.N, WPACKH2, BH2_EX};
        if ((rc = build_cweights(j, 4, nullptr, 0, st))) return rc;
    } else if ((rc = bamp_pack_f32(P, H, st))) {   // the f32 weights and their band ranges, once per forward
        return rc;
    }
    if (P.band[0] && (P.h2 || P.x3)) {
        // per column tile: real |H|^2 (fp16x2 two planes, bf16x3 three; 8 16-tiles per 128
        // outputs), complex H (four / six planes, 4)
        const int pr = P.x3 ? 3 : 2, pc = P.x3 ? 6 : 4;
        if ((rc = h2_kband(P.Wabs2, pr, P.N / 32, 8, P.ncpA1 / 128, P.n / 16, const_cast<int*>(P.band[0]), st))) return rc;
        if ((rc = h2_kband(P.WH, pc, P.N / 32, 4, P.ncpA2 / 128, P.n / 16, const_cast<int*>(P.band[1]), st))) return rc;
        if ((rc = h2_kband(P.Wabs2T, pr, P.n / 32, 8, P.ncpB1 / 128, P.N / 16, const_cast<int*>(P.band[2]), st))) return rc;
        if ((rc = h2_kband(P.WHH, pc, P.n / 32, P.bn / 32, P.ncpB2 / P.bn, P.N / 16, const_cast<int*>(P.band[3]), st))) return rc;
    }
    const size_t tot = std::max((size_t)P.B * P.N, (size_t)P.B * P.n);
    const int g = (int)std::min<size_t>((tot + 255) / 256, 2048);
    hipLaunchKernelGGL(bamp_init_kernel, dim3(g), dim3(256), 0, st, P);
    AMP_LAUNCH_CHECK("bamp_init");
    return AMP_OK;
}

// the four GEMM launches of one BAMPLayer.forward (bamp.py:59-64), each preceded on the fp16x2
// path by the split of its A rows (var, xmmse, 1/u, s) into the plane buffer
static void bamp_split(const BampK& P, const float* a, int lda, int K, bool cpx, int t, hipStream_t st) {
    const int* stop = &P.iters[t].stopped;
    // a workgroup per row when four rows per workgroup would leave CUs idle on long rows
    const int wpr = (P.rows_pad / 4 < 2 * device_cu_count() && K >= 1024) ? 4 : 1;
    const dim3 grid(P.rows_pad * wpr / 4);
    if (P.x3) {
        if (cpx)
            hipLaunchKernelGGL(x3_split_rows_kernel<true>, grid, dim3(256), 0, st, a, lda, P.B, P.rows_pad, K, P.ap,
                               stop, wpr);
        else
            hipLaunchKernelGGL(x3_split_rows_kernel<false>, grid, dim3(256), 0, st, a, lda, P.B, P.rows_pad, K, P.ap,
                               stop, wpr);
        return;
    }
    if (cpx)
        hipLaunchKernelGGL(h2_split_rows_kernel<true>, grid, dim3(256), 0, st, a, lda, P.B, P.rows_pad, K, P.ap,
                           P.rexp, stop, wpr);
    else
        hipLaunchKernelGGL(h2_split_rows_kernel<false>, grid, dim3(256), 0, st, a, lda, P.B, P.rows_pad, K, P.ap,
                           P.rexp, stop, wpr);
}

static void bamp_gemms(const BampK& P, const Const64& c64, int t, hipStream_t st) {
    const int gr = cdiv(P.B, GBM);
    // the host reads bvar(P, t + 1) as the device does: (t + 1) & 1 picks var1, else var0
    if (P.h2 || P.x3) bamp_split(P, ((t + 1) & 1) ? P.var1 : P.var0, P.N, P.N, false, t, st);
    const bool skc = bamp_short_chunks(P);
    if (skc && P.N % 4 != 0)
        hipLaunchKernelGGL((bamp_ka1<256, false, ALoadPair>), dim3(gr, P.ncpA1 / 128), dim3(AMP_WG), BSKC_LDS, st, P, t);
    else if (skc) hipLaunchKernelGGL((bamp_ka1<256>), dim3(gr, P.ncpA1 / 128), dim3(AMP_WG), BSKC_LDS, st, P, t);
    else if (P.x3) hipLaunchKernelGGL((bamp_ka1<GKC, true>), dim3(gr, P.ncpA1 / 128), dim3(AMP_WG), XLDS_R, st, P, t);
    else hipLaunchKernelGGL((bamp_ka1<>), dim3(gr, P.ncpA1 / 128), dim3(AMP_WG), BLDS, st, P, t);
    if (P.h2 || P.x3) bamp_split(P, P.xm, 2 * P.N, P.N, true, t, st);
    if (skc) hipLaunchKernelGGL((bamp_ka2<256>), dim3(gr, P.ncpA2 / 128), dim3(AMP_WG), BSKC_LDS, st, P, t);
    else if (P.x3) hipLaunchKernelGGL((bamp_ka2<GKC, true>), dim3(gr, P.ncpA2 / 128), dim3(AMP_WG), XLDS_C, st, P, t);
    else hipLaunchKernelGGL((bamp_ka2<>), dim3(gr, P.ncpA2 / 128), dim3(AMP_WG), BLDS, st, P, t);
    if (P.h2 || P.x3) bamp_split(P, P.invu, P.ild, P.n, false, t, st);
    if (skc) hipLaunchKernelGGL((bamp_kb1<256>), dim3(gr, P.ncpB1 / 128), dim3(AMP_WG), BSKC_LDS, st, P, t);
    else if (P.x3) hipLaunchKernelGGL((bamp_kb1<GKC, true>), dim3(gr, P.ncpB1 / 128), dim3(AMP_WG), XLDS_R, st, P, t);
    else hipLaunchKernelGGL((bamp_kb1<>), dim3(gr, P.ncpB1 / 128), dim3(AMP_WG), BLDS, st, P, t);
    if (P.h2 || P.x3) bamp_split(P, P.s, P.sld, P.n, true, t, st);
    launch_kb2(P, c64, gr, t, st);
}

// One BAMPLayer.forward (bamp.py:48-64) + the allclose test of bamp.py:140 (no-op once stopped).
// bamp_fixall is a no-op unless bamp_r left a pending record (nfix blocks' counts fit the
// iteration's nblk partial slots).
static int bamp_iterate_impl(const BampK& P, const Const64& c64, int t, hipStream_t st) {
    bamp_gemms(P, c64, t, st);
    hipLaunchKernelGGL(bamp_r, dim3(1), dim3(BRWG), 0, st, P, c64, t);
    const int nfix = fix_grid(P.nblk, P.B * P.L);
    hipLaunchKernelGGL(bamp_fixall, dim3(nfix), dim3(AMP_WG), 0, st, P, c64, t);
    AMP_LAUNCH_CHECK("bamp iteration");
    return AMP_OK;
}

static int bamp_iterate_sharded(const BampK& P, const Const64& c64, int t, hipStream_t st, bool& hook_failed) {
    bamp_gemms(P, c64, t, st);
    hipLaunchKernelGGL(bamp_xr1, dim3(1), dim3(BRWG), 0, st, P, t);
    AMP_LAUNCH_CHECK("bamp_xr1");
    // every hook call is made on every rank even after one failed: the ranks' collectives stay
    // matched and a failed rank's poisoned words reach the others (amp_sparc.h)
    hook_failed |= call_allreduce_hook(P.xs->sum, 2, AMP_ALLREDUCE_SUM, st) != AMP_OK;
    hook_failed |= call_allreduce_hook(P.xs->mx, 2, AMP_ALLREDUCE_MAX, st) != AMP_OK;
    hipLaunchKernelGGL(bamp_xr2, dim3(1), dim3(BRWG), 0, st, P, c64, t);
    AMP_LAUNCH_CHECK("bamp_xr2");
    hook_failed |= call_allreduce_hook(P.xs->gmax, 1, AMP_ALLREDUCE_MAX, st) != AMP_OK;
    hipLaunchKernelGGL(bamp_xr3, dim3(1), dim3(BRWG), 0, st, P, c64, t);
    AMP_LAUNCH_CHECK("bamp_xr3");
    hook_failed |= call_allreduce_hook(P.xs->fix, 3, AMP_ALLREDUCE_SUM, st) != AMP_OK;
    hipLaunchKernelGGL(bamp_xr4, dim3(1), dim3(64), 0, st, P, t);
    AMP_LAUNCH_CHECK("bamp_xr4");
    return AMP_OK;
}

// the caller's var holds the last executed iteration's (ping-pong buffers)
static int bamp_finalize_impl(const BampK& P, hipStream_t st) {
    hipLaunchKernelGGL(bamp_output_kernel, dim3((int)std::min<size_t>(((size_t)P.B * P.N + 255) / 256, 2048)),
                       dim3(256), 0, st, P);
    AMP_LAUNCH_CHECK("bamp_output");
    return AMP_OK;
}

}  // namespace amp

extern "C" {

int amp_bamp_run_sharded(const amp_dims* d, const amp_constellation* c, const amp_bamp_args* a, int32_t B_global,
                         void* stream) {
    BampK P;
    Const64 c64;
    int rc = bamp_setup(d, c, a, P, c64);
    if (rc) return rc;
    AMP_REQUIRE(allreduce_hook_set(), "amp_bamp_run_sharded: no all-reduce hook registered (amp_set_allreduce_hook)");
    AMP_REQUIRE(B_global >= d->B, "amp_bamp_run_sharded: B_global = %d < this rank's B = %d", B_global, d->B);
    AMP_REQUIRE(a->denoiser == 0, "amp_bamp_run_sharded: the element-wise denoiser (mode 'random', B = 1) has no "
                "batch-global values to share");
    hipStream_t st = (hipStream_t)stream;
    rc = bamp_prepare_impl(P, a, st);
    bool hook_failed = false;
    for (int t = 0; t < P.max_iter && !rc; ++t) rc = bamp_iterate_sharded(P, c64, t, st, hook_failed);
    if (!rc && hook_failed) rc = hook_failure("bamp");
    return rc ? rc : bamp_finalize_impl(P, st);
}

int amp_bamp_run(const amp_dims* d, const amp_constellation* c, const amp_bamp_args* a, void* stream) {
    BampK P;
    Const64 c64;
    int rc = bamp_setup(d, c, a, P, c64);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = bamp_prepare_impl(P, a, st))) return rc;
    for (int t = 0; t < P.max_iter; ++t)
        if ((rc = bamp_iterate_impl(P, c64, t, st))) return rc;
    return bamp_finalize_impl(P, st);
}

int amp_bamp_prepare(const amp_dims* d, const amp_constellation* c, const amp_bamp_args* a, void* stream) {
    BampK P;
    Const64 c64;
    int rc = bamp_setup(d, c, a, P, c64);
    return rc ? rc : bamp_prepare_impl(P, a, (hipStream_t)stream);
}

int amp_bamp_iterate(const amp_dims* d, const amp_constellation* c, const amp_bamp_args* a, int32_t t, void* stream) {
    BampK P;
    Const64 c64;
    int rc = bamp_setup(d, c, a, P, c64);
    if (rc) return rc;
    AMP_REQUIRE(t >= 0 && t < a->max_iter, "amp_bamp_iterate: t = %d outside [0, %d)", t, a->max_iter);
    return bamp_iterate_impl(P, c64, t, (hipStream_t)stream);
}

int amp_bamp_finalize(const amp_dims* d, const amp_constellation* c, const amp_bamp_args* a, void* stream) {
    BampK P;
    Const64 c64;
    int rc = bamp_setup(d, c, a, P, c64);
    return rc ? rc : bamp_finalize_impl(P, (hipStream_t)stream);
}

// BAMPLayer.random_denoiser (bamp.py:79-88) as a standalone element-wise op (layer-level API).
__global__ __launch_bounds__(AMP_WG) void bamp_random_denoise_kernel(BampK P, Const64 c64, long long count,
                                                                     const float2* r, const float* cov, float2* xm,
                                                                     float* var) {
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < count;
         e += (long long)gridDim.x * blockDim.x) {
        float xr, xi, v;
        bamp_bayes_elem<AMP_MAX_K>(P, c64, r[e].x, r[e].y, cov[e], xr, xi, v);
        xm[e] = make_float2(xr, xi);
        var[e] = v;
    }
}

int amp_bamp_random_denoise(const amp_constellation* c, int64_t count, const void* r, const void* cov, float P0,
                            float Ps, void* xmmse, void* var, void* stream) {
    AMP_REQUIRE(c && c->K >= 1 && c->K <= AMP_MAX_K, "amp_bamp_random_denoise: bad constellation size %d",
                c ? c->K : 0);
    AMP_REQUIRE(count >= 0, "amp_bamp_random_denoise: count < 0");
    if (count == 0) return AMP_OK;
    AMP_REQUIRE(r && cov && xmmse && var, "amp_bamp_random_denoise: null pointer argument");
    BampK P{};
    P.c = to_const(c);
    P.P0 = P0;
    P.Ps = Ps;
    const Const64 c64 = to_const64(c);
    const int g = (int)std::max(1LL, std::min(((long long)count + AMP_WG - 1) / AMP_WG, 8192LL));
    hipLaunchKernelGGL(bamp_random_denoise_kernel, dim3(g), dim3(AMP_WG), 0, (hipStream_t)stream, P, c64, (long long)count,
                       (const float2*)r, (const float*)cov, (float2*)xmmse, (float*)var);
    AMP_LAUNCH_CHECK("bamp_random_denoise");
    return AMP_OK;
}

}  // extern "C"

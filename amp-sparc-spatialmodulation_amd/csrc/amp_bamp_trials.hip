// amp_bamp_trials.hip — BAMP over E independent single-trial detections that share one channel
// (amp_bamp_trials_run): the iteration kernels of the launch engine (amp_bamp.hip, f32 tiles) with
// per-row records.
//
// Restates, for every trial e alone, BAMP.forward at B = 1 (bamp.py:116-143) with its Tracker
// (bamp.py:12-25), BAMPLayer.forward (bamp.py:48-64), the per-element-tau block denoiser
// (bamp.py:66-77, the max|xi| shift of bamp.py:70 over the trial's own logits) and the allclose
// exit on the trial's own var (bamp.py:140) — the way the reference's drivers run it (batch = 1,
// res epochs per channel: bamp_model.py:89, 96).
// Per iteration: the four GEMM launches of amp_bamp.hip over row tiles of 32 trials (a stopped
// row is never stored to; a tile whose rows have all stopped returns at once), the denoiser row by
// row with one partial per (tile, row), then tbamp_r, a grid over the trials: workgroup e reduces
// trial e's partials, settles its exact float64 fix-up (fixup_sections, against the trial's own
// max|xi|) and its allclose exit.  Every kernel returns at once when the stop counter has reached E.
#include <algorithm>
#include <mutex>

#include "amp_trials.h"

namespace amp {

constexpr int TBRWG = 1024;

struct alignas(16) TBampIter {
    int32_t stopped, T, fixed, fixed_all;
};

struct TBampK {
    int E, N, n, L, M, bn;
    int kapA1, ncpA1, kapA2, ncpA2, kapB1, ncpB1, kapB2, ncpB2;
    int nct, max_iter;
    int ild, sld;          // row strides of invu and s (bamp_ild / bamp_sld: n, 2n rounded up to 4)
    float sigma2;          // f32(noise_var): u = v + sigma2 (bamp.py:61)
    const float* Wabs2;    // [ncpA1][kapA1]   v = |H|^2 var
    const float* WH;       // [ncpA2][kapA2]   H xmmse
    const float* Wabs2T;   // [ncpB1][kapB1]   |H|^2^T (1/u)
    const float* WHH;      // [ncpB2][kapB2]   H^H s
    const float* y;        // [E][2n]
    float* v;              // [E][n]
    float* z;              // [E][2n]
    float* invu;           // [E][ild]
    float* s;              // [E][sld]  (y - z)/u
    float* cov;            // [E][N]
    float* xmap;           // [E][2N]  caller
    float* xm;             // [E][2N]  caller
    float* var0;           // caller's var (even iterations)
    float* var1;           // workspace  (odd iterations)
    float* secmax;         // [E][L]
    float* secabs;         // [E][L]
    Partial* parts;        // [E][nct]
    TBampIter* iters;      // [E], advanced in place by tbamp_r
    amp_status* status;    // [E]
    unsigned* nstop;       // trials whose allclose exit has fired
    const int* band[4];    // block-banded H: per column tile reduction ranges (weight_kband), else null
    Const c;
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

static void tbamp_geometry(const amp_dims* d, int E, TBampK& P) {
    P.E = E; P.N = d->N; P.n = d->n; P.L = d->L; P.M = d->M;
    P.bn = section_bn(d);
    P.kapA1 = round_up(d->N, GBK); P.ncpA1 = round_up(d->n, 128);
    P.kapA2 = round_up(2 * d->N, GBK); P.ncpA2 = round_up(2 * d->n, 128);
    P.kapB1 = round_up(d->n, GBK); P.ncpB1 = round_up(d->N, 128);
    P.kapB2 = round_up(2 * d->n, GBK); P.ncpB2 = round_up(2 * d->N, P.bn);
    P.nct = P.ncpB2 / P.bn;
    P.ild = bamp_ild(d->n); P.sld = bamp_sld(d->n);
}

static TBampWs tbamp_carve(const amp_dims* d, int E, void* base) {
    TBampK P;
    tbamp_geometry(d, E, P);
    Carve cv(base);
    TBampWs w;
    w.Wabs2 = cv.take<float>((size_t)P.ncpA1 * P.kapA1);
    w.WH = cv.take<float>((size_t)P.ncpA2 * P.kapA2);
    w.Wabs2T = cv.take<float>((size_t)P.ncpB1 * P.kapB1);
    w.WHH = cv.take<float>((size_t)P.ncpB2 * P.kapB2);
    w.v = cv.take<float>((size_t)E * d->n);
    w.z = cv.take<float>((size_t)E * 2 * d->n);
    w.invu = cv.take<float>((size_t)E * P.ild);
    w.s = cv.take<float>((size_t)E * P.sld);
    w.cov = cv.take<float>((size_t)E * d->N);
    w.var1 = cv.take<float>((size_t)E * d->N);
    w.secmax = cv.take<float>((size_t)E * d->L);
    w.secabs = cv.take<float>((size_t)E * d->L);
    w.parts = cv.take<Partial>((size_t)E * P.nct);
    w.iters = cv.take<TBampIter>((size_t)E);
    w.band[0] = cv.take<int>((size_t)2 * (P.ncpA1 / 128));
    w.band[1] = cv.take<int>((size_t)2 * (P.ncpA2 / 128));
    w.band[2] = cv.take<int>((size_t)2 * (P.ncpB1 / 128));
    w.band[3] = cv.take<int>((size_t)2 * (P.ncpB2 / P.bn));
    w.nstop = cv.take<unsigned>(16);
    w.dec = cv.take<char>(trials_decide_ws_bytes(d, E));
    w.bytes = cv.off;
    return w;
}

__device__ __forceinline__ float* tbvar(const TBampK& P, int t) { return (t & 1) ? P.var1 : P.var0; }
__device__ __forceinline__ int tbkb(const TBampK& P, int w, int cb) { return P.band[w] ? P.band[w][2 * cb] : 0; }
__device__ __forceinline__ int tbke(const TBampK& P, int w, int cb) { return P.band[w] ? P.band[w][2 * cb + 1] : -1; }

// KC: the A chunk of the f32 tile, as amp_bamp.hip launches it (256 at the narrow column tile);
// the chunking does not change the MFMA order: the same bits.
// v = |H|^2 var (bamp.py:59).  AL: var's loader (ALoadPair where N % 4 == 2, as bamp_ka1)
template <class AL>
__global__ __launch_bounds__(AMP_WG) void tbamp_ka1(TBampK P, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_stop[GBM];
    if (*P.nstop >= (unsigned)P.E) return;
    const GemmTile tile = xcd_tile();
    const int row0 = tile.rb * GBM, col0 = tile.cb * 128;
    if (!tile_rows_live(P.iters, row0, P.E, s_stop)) return;
    gemm_tile<128, AL, 256>(AL{tbvar(P, t + 1), P.N, P.E, P.N}, P.Wabs2, P.kapA1, row0, col0, lds,
                            tbkb(P, 0, tile.cb), tbke(P, 0, tile.cb));
    using C = GemmCfg<128, 256>;
    for (int e = threadIdx.x; e < GBM * 128; e += AMP_WG) {
        const int rho = e >> 7, cc = e & 127;
        const int row = row0 + rho, col = col0 + cc;
        if (row < P.E && col < P.n && !s_stop[rho]) P.v[(size_t)row * P.n + col] = lds[rho * C::LDC + cc];
    }
}

// z = H xmmse - v (y - z) / u ; u = v + sigma2 ; s = (y - z) / u   (bamp.py:60-63)
__global__ __launch_bounds__(AMP_WG) void tbamp_ka2(TBampK P, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_stop[GBM];
    if (*P.nstop >= (unsigned)P.E) return;
    const GemmTile tile = xcd_tile();
    const int row0 = tile.rb * GBM, col0 = tile.cb * 128;
    if (!tile_rows_live(P.iters, row0, P.E, s_stop)) return;
    const int twoN = 2 * P.N, twon = 2 * P.n;
    gemm_tile<128, ALoadPlain, 256>(ALoadPlain{P.xm, twoN, P.E, twoN}, P.WH, P.kapA2, row0, col0, lds,
                                    tbkb(P, 1, tile.cb), tbke(P, 1, tile.cb));
    using C = GemmCfg<128, 256>;
    constexpr int IT = GBM * 64 / AMP_WG;
    float2 yv[IT], zv[IT];
    float vv[IT], iuo[IT];
#pragma unroll
    for (int u = 0; u < IT; ++u) {
        // unconditional loads at a clamped index (amp_bamp.hip bamp_ka2); out-of-range elements are never stored
        const int e = threadIdx.x + u * AMP_WG;
        const int rho = e >> 6, cp = e & 63;
        const int row = min(row0 + rho, P.E - 1), i = min((col0 >> 1) + cp, P.n - 1);
        const size_t oc = (size_t)row * twon + 2 * i, o = (size_t)row * P.n + i;
        yv[u] = *reinterpret_cast<const float2*>(P.y + oc);
        zv[u] = *reinterpret_cast<const float2*>(P.z + oc);
        vv[u] = P.v[o];
        iuo[u] = P.invu[(size_t)row * P.ild + i];
    }
#pragma unroll
    for (int u = 0; u < IT; ++u) {
        const int e = threadIdx.x + u * AMP_WG;
        const int rho = e >> 6, cp = e & 63;
        const int row = row0 + rho, i = (col0 >> 1) + cp;
        if (row < P.E && i < P.n && !s_stop[rho]) {
            const size_t oc = (size_t)row * twon + 2 * i;
            const float hr = lds[rho * C::LDC + 2 * cp], hi = lds[rho * C::LDC + 2 * cp + 1];
            const float yr = yv[u].x, yi = yv[u].y;
            const float vi = vv[u], iu_old = iuo[u];
            const float zr = hr - (vi * (yr - zv[u].x)) * iu_old;
            const float zi = hi - (vi * (yi - zv[u].y)) * iu_old;
            const float uu = vi + P.sigma2;
            const float iu = 1.0f / uu;
            *reinterpret_cast<float2*>(P.z + oc) = make_float2(zr, zi);
            P.invu[(size_t)row * P.ild + i] = iu;
            *reinterpret_cast<float2*>(P.s + (size_t)row * P.sld + 2 * i) = make_float2((yr - zr) * iu, (yi - zi) * iu);
        }
    }
}

// cov = 1 / (|H|^2^T (1/u))   (bamp.py:62)
__global__ __launch_bounds__(AMP_WG) void tbamp_kb1(TBampK P, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_stop[GBM];
    if (*P.nstop >= (unsigned)P.E) return;
    const GemmTile tile = xcd_tile();
    const int row0 = tile.rb * GBM, col0 = tile.cb * 128;
    if (!tile_rows_live(P.iters, row0, P.E, s_stop)) return;
    gemm_tile<128, ALoadPlain, 256>(ALoadPlain{P.invu, P.ild, P.E, P.ild}, P.Wabs2T, P.kapB1, row0, col0, lds,
                                    tbkb(P, 2, tile.cb), tbke(P, 2, tile.cb));
    using C = GemmCfg<128, 256>;
    for (int e = threadIdx.x; e < GBM * 128; e += AMP_WG) {
        const int rho = e >> 7, cc = e & 127;
        const int row = row0 + rho, col = col0 + cc;
        if (row < P.E && col < P.N && !s_stop[rho]) P.cov[(size_t)row * P.N + col] = 1.0f / lds[rho * C::LDC + cc];
    }
}

// One row of the tile for the section denoiser (BampDenoisePolicy of amp_bamp.hip at B = 1).
struct TBampDenoisePolicy {
    const float* tile;    // the row's C-tile row (xmap)
    const float* itile;   // the row's 1 / (cov / 2)
    int M;
    size_t o0, s0;        // row * N + first position, row * L + first section of the tile
    float* xm;
    float* var_new;
    const float* var_prev;
    float* secmax;
    float* secabs;
    __device__ __forceinline__ void load(int sec, int m, float& rr, float& ri, float& it) const {
        const float2 v = *reinterpret_cast<const float2*>(tile + 2 * (sec * M + m));
        rr = v.x; ri = v.y;
        it = itile[sec * M + m];   // 1 / tau, tau = cov / 2 (bamp.py:68)
    }
    __device__ __forceinline__ void store(int sec, int m, float xr, float xi, float var, PartAcc& pa) const {
        const size_t o = o0 + sec * M + m;
        *reinterpret_cast<float2*>(xm + 2 * o) = make_float2(xr, xi);
        var_new[o] = var;
        pa.sumvar += (double)var;
        pa.notclose += torch_close(var, var_prev[o]) ? 0u : 1u;     // bamp.py:140
    }
    __device__ __forceinline__ void section(int sec, float smax, float sabs) const {
        secmax[s0 + sec] = smax;
        secabs[s0 + sec] = sabs;
    }
};

// xmap = xmmse + cov (H^H s) ; xmmse, var = denoiser(xmap, cov/2)   (bamp.py:63-64)
template <int BN, int KK, int KC>
__global__ __launch_bounds__(AMP_WG) void tbamp_kb2(TBampK P, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_stop[GBM];
    if (*P.nstop >= (unsigned)P.E) return;
    using C = GemmCfg<BN, KC>;
    const GemmTile tile = xcd_tile();
    const int row0 = tile.rb * GBM, col0 = tile.cb * BN;
    if (!tile_rows_live(P.iters, row0, P.E, s_stop)) return;
    const int twoN = 2 * P.N;
    gemm_tile<BN, ALoadPlain, KC>(ALoadPlain{P.s, P.sld, P.E, P.sld}, P.WHH, P.kapB2, row0, col0, lds,
                                  tbkb(P, 3, tile.cb), tbke(P, 3, tile.cb));
    const int nrows = min(GBM, P.E - row0), ncols = min(BN, twoN - col0);
    float* sit = lds + C::CTILE_FLOATS + 2048;   // past the partial-store scratch
    {
        constexpr int IT = GBM * BN / AMP_WG;
        static_assert(C::CTILE_FLOATS + 2048 + GBM * (BN / 2) <= C::A_FLOATS, "1 / tau tile");
        float xv[IT], cvv[IT];
#pragma unroll
        for (int u = 0; u < IT; ++u) {
            const int e = threadIdx.x + u * AMP_WG, rho = min(e / BN, nrows - 1), cc = min(e % BN, ncols - 1);
            xv[u] = P.xm[(size_t)(row0 + rho) * twoN + col0 + cc];
            cvv[u] = P.cov[(size_t)(row0 + rho) * P.N + ((col0 + cc) >> 1)];
        }
#pragma unroll
        for (int u = 0; u < IT; ++u) {
            const int e = threadIdx.x + u * AMP_WG, rho = e / BN, cc = e % BN;
            if (rho < nrows && cc < ncols && !s_stop[rho]) {
                const size_t o = (size_t)(row0 + rho) * twoN + col0 + cc;
                const float xp = xv[u] + cvv[u] * lds[rho * C::LDC + cc];
                P.xmap[o] = xp;
                lds[rho * C::LDC + cc] = xp;
                if ((cc & 1) == 0) sit[rho * (BN / 2) + (cc >> 1)] = 1.0f / (cvv[u] * 0.5f);
            }
        }
    }
    __syncthreads();
    // the denoiser row by row: the row's own partial, in the slot its B = 1 forward stores it to
    const int slot = seq_part_slot(tile.cb, P.nct), spr = (ncols / 2) / P.M;
    for (int rho = 0; rho < nrows; ++rho) {
        if (s_stop[rho]) continue;   // workgroup-uniform
        const int row = row0 + rho;
        TBampDenoisePolicy pol;
        pol.tile = lds + rho * C::LDC; pol.itile = sit + rho * (BN / 2); pol.M = P.M;
        pol.o0 = (size_t)row * P.N + col0 / 2;
        pol.s0 = (size_t)row * P.L + (col0 / 2) / P.M;
        pol.xm = P.xm; pol.var_new = tbvar(P, t); pol.var_prev = tbvar(P, t + 1);
        pol.secmax = P.secmax; pol.secabs = P.secabs;
        PartAcc pa;
        denoise_sections<true, KK>(pol, spr, P.M, P.c, pa);
        part_block_store(pa, P.parts + (size_t)row * P.nct + slot, lds + C::CTILE_FLOATS);
    }
}

// Workgroup e: trial e's reduction, exact float64 fix-up against its own max|xi| and allclose
// decision (bamp.py:140) — bamp_r + bamp_fixall of amp_bamp.hip on the trial's rows, every trial in
// parallel.
__global__ __launch_bounds__(TBRWG) void tbamp_r(TBampK P, Const64 c64, int t) {
    __shared__ __attribute__((aligned(16))) float lds[512];
    __shared__ double s_fix[TBRWG / 64];
    __shared__ int s_nc[TBRWG / 64];
    if (*P.nstop >= (unsigned)P.E) return;
    const int e = blockIdx.x;
    const TBampIter cur = P.iters[e];
    if (cur.stopped) return;
    float* xm = P.xm + (size_t)e * 2 * P.N;
    float* vn = tbvar(P, t) + (size_t)e * P.N;
    const float* vp = tbvar(P, t + 1) + (size_t)e * P.N;
    PartAcc pa = part_reduce_all(P.parts + (size_t)e * P.nct, P.nct, lds);
    uint32_t notclose = pa.notclose;
    int fixed = 0;
    if (part_allnan(pa)) {
        if (!cur.fixed_all) nan_fill(xm, vn, (size_t)P.N);
        notclose = 1u;
        fixed = -1;
    } else if (part_danger(pa)) {
        const float2* xp2 = reinterpret_cast<const float2*>(P.xmap + (size_t)e * 2 * P.N);
        float2* x2 = reinterpret_cast<float2*>(xm);
        const float* cov = P.cov + (size_t)e * P.N;
        const int M = P.M;
        int dnc = 0;
        auto ldf = [=](int s) {
            const size_t o0 = (size_t)s * M;
            return [=](int m, float& rr, float& ri, float& it) {
                const float2 v = xp2[o0 + m];
                rr = v.x; ri = v.y; it = 1.0f / (cov[o0 + m] * 0.5f);
            };
        };
        auto stf = [&](int s) {
            const size_t o0 = (size_t)s * M;
            return [&, o0](int m, float xr, float xi, float var) {
                const size_t o = o0 + m;
                dnc += (torch_close(var, vp[o]) ? 0 : 1) - (torch_close(vn[o], vp[o]) ? 0 : 1);
                x2[o] = make_float2(xr, xi);
                vn[o] = var;
            };
        };
        double G;
        fixed = fixup_sections<true>(P.L, M, P.secmax + (size_t)e * P.L, P.secabs + (size_t)e * P.L, pa.maxabs, c64,
                                     ldf, stf, &G, s_fix);
        dnc = group_sum(dnc, 64);
        if ((threadIdx.x & 63) == 0) s_nc[threadIdx.x >> 6] = dnc;
        __syncthreads();
        int tot = 0;
        for (int w = 0; w < TBRWG / 64; ++w) tot += s_nc[w];
        notclose = (uint32_t)((int)notclose + tot);
    }
    if (threadIdx.x == 0) {
        TBampIter nx;
        nx.stopped = notclose == 0 ? 1 : 0;
        nx.T = t + 1;
        nx.fixed = fixed;
        nx.fixed_all = (fixed < 0) ? 1 : 0;
        P.iters[e] = nx;
        if (nx.stopped || t + 1 == P.max_iter) {
            amp_status s;
            s.T = t + 1; s.nan_state = fixed != 0 ? 1 : 0; s.stopped = nx.stopped;
            s.gemm = AMP_ARITH_F32;
            s.last_scalar[0] = s.last_scalar[1] = s.last_scalar[2] = s.last_scalar[3] = 0.f;
            P.status[e] = s;
        }
        if (nx.stopped) __hip_atomic_fetch_add(P.nstop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Tracker (bamp.py:13-25) for every trial: xmmse = 0, var(prev) = 1, z = y, u = 0 + sigma2 -> 1/u.
__global__ void tbamp_init_kernel(TBampK P) {
    const size_t EN = (size_t)P.E * P.N, En = (size_t)P.E * P.n;
    const size_t tot = EN > En ? EN : En;
    const float iu = 1.0f / P.sigma2;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
        if (e < EN) {
            reinterpret_cast<float2*>(P.xm)[e] = make_float2(0.f, 0.f);
            P.var1[e] = 1.0f;
        }
        if (e < En) {
            reinterpret_cast<float2*>(P.z)[e] = reinterpret_cast<const float2*>(P.y)[e];
            P.invu[P.ild == P.n ? e : (e / P.n) * P.ild + e % P.n] = iu;
        }
        if (e < (size_t)P.E) {
            P.iters[e] = TBampIter{0, 0, 0, 0};
            // the pads of the invu and s rows (bamp_ild / bamp_sld), zeroed once
            for (int k = P.n; k < P.ild; ++k) P.invu[e * P.ild + k] = 0.f;
            for (int k = 2 * P.n; k < P.sld; ++k) P.s[e * P.sld + k] = 0.f;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *P.nstop = 0u;
}

// Trial e's last executed iteration wrote var into buffer (T_e - 1) & 1; buffer 0 is the caller's.
__global__ __launch_bounds__(256) void tbamp_output_kernel(TBampK P) {
    const int e = blockIdx.x;
    const int T = P.status[e].T;
    if (((T - 1) & 1) == 0) return;
    for (int i = threadIdx.x; i < P.N; i += blockDim.x) P.var0[(size_t)e * P.N + i] = P.var1[(size_t)e * P.N + i];
}

constexpr size_t TB_LDS_S = GemmCfg<128, 256>::LDS_BYTES;   // within the default 64 KB
constexpr size_t TB_LDS_W = GemmCfg<256>::LDS_BYTES;

template <int KK>
static int tbamp_kb2_attr() { return set_lds_attr<256>((const void*)tbamp_kb2<256, KK, GKC>); }

static std::once_flag g_tbamp_once;
static int g_tbamp_rc = 0;
static int tbamp_attrs() {
    std::call_once(g_tbamp_once, [] {
        int rc = tbamp_kb2_attr<1>();
        if (!rc) rc = tbamp_kb2_attr<2>();
        if (!rc) rc = tbamp_kb2_attr<4>();
        if (!rc) rc = tbamp_kb2_attr<8>();
        if (!rc) rc = tbamp_kb2_attr<16>();
        if (!rc) rc = tbamp_kb2_attr<64>();
        g_tbamp_rc = rc;
    });
    return g_tbamp_rc;
}

template <int KK>
static void tbamp_launch_kb2_kk(const TBampK& P, int gr, int t, hipStream_t st) {
    if (P.bn == 128)
        hipLaunchKernelGGL((tbamp_kb2<128, KK, 256>), dim3(gr, P.ncpB2 / 128), dim3(AMP_WG), TB_LDS_S, st, P, t);
    else
        hipLaunchKernelGGL((tbamp_kb2<256, KK, GKC>), dim3(gr, P.ncpB2 / 256), dim3(AMP_WG), TB_LDS_W, st, P, t);
}

static void tbamp_launch_kb2(const TBampK& P, int gr, int t, hipStream_t st) {
    switch (P.c.K) {
    case 1: tbamp_launch_kb2_kk<1>(P, gr, t, st); break;
    case 2: tbamp_launch_kb2_kk<2>(P, gr, t, st); break;
    case 4: tbamp_launch_kb2_kk<4>(P, gr, t, st); break;
    case 8: tbamp_launch_kb2_kk<8>(P, gr, t, st); break;
    case 16: tbamp_launch_kb2_kk<16>(P, gr, t, st); break;
    default: tbamp_launch_kb2_kk<64>(P, gr, t, st); break;
    }
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
    int rc = check_dims(d, c, true, true);   // any n, any even N, a partial last column tile (amp_bamp_run)
    if (rc) return rc;
    AMP_REQUIRE(d->B == 1, "amp_bamp_trials_run: dims describe ONE trial (B = %d, must be 1)", d->B);
    AMP_REQUIRE(trials >= 1, "amp_bamp_trials_run: trials = %d", trials);
    AMP_REQUIRE(bamp_index_ok(d, trials), "amp_bamp_trials_run: %d trials of max(2N, 2n) = %d columns need more "
                "than 32-bit offsets (or more than 65535 column tiles)", trials, 2 * std::max(d->N, d->n));
    AMP_REQUIRE(a && a->H && a->y && a->xmap && a->xmmse && a->var && a->status && a->ws,
                "amp_bamp_trials_run: null pointer argument");
    AMP_REQUIRE(a->max_iter > 0, "amp_bamp_trials_run: max_iter must be positive");
    AMP_REQUIRE(a->denoiser == 0, "amp_bamp_trials_run: the element-wise denoiser ('random' mode) has no "
                "independent-trial form");
    AMP_REQUIRE(a->gemm == AMP_GEMM_AUTO || a->gemm == AMP_GEMM_F32, "amp_bamp_trials_run: f32 GEMMs only (gemm %d)",
                a->gemm);
    const int E = trials;
    const TBampWs w = tbamp_carve(d, E, a->ws);
    AMP_REQUIRE(a->ws_bytes >= w.bytes, "amp_bamp_trials_run: workspace %zu < %zu bytes", a->ws_bytes, w.bytes);
    TrialsDecide td{};
    if (dec && (rc = trials_decide_args(d, dec, a->xmap, a->xmmse, td))) return rc;
    if ((rc = tbamp_attrs())) return rc;
    TBampK P{};
    tbamp_geometry(d, E, P);
    P.max_iter = a->max_iter;
    P.sigma2 = (float)a->noise_var;
    P.Wabs2 = w.Wabs2; P.WH = w.WH; P.Wabs2T = w.Wabs2T; P.WHH = w.WHH;
    P.y = (const float*)a->y; P.v = w.v; P.z = w.z; P.invu = w.invu; P.s = w.s; P.cov = w.cov;
    P.xmap = (float*)a->xmap; P.xm = (float*)a->xmmse; P.var0 = (float*)a->var; P.var1 = w.var1;
    P.secmax = w.secmax; P.secabs = w.secabs; P.parts = w.parts; P.iters = w.iters;
    P.status = (amp_status*)a->status;
    P.nstop = w.nstop;
    const bool band = d->Lin > 1 || d->Lout > 1;   // block-banded H (channel.py:75-95)
    for (int i = 0; i < 4; ++i) P.band[i] = band ? w.band[i] : nullptr;
    P.c = to_const(c);
    const Const64 c64 = to_const64(c);
    hipStream_t st = (hipStream_t)stream;
    // the operators, packed once per call (Tracker: adj, abs2, abs2T, bamp.py:17-19)
    const float2* H = (const float2*)a->H;
    if ((rc = build_abs2_weight(H, P.N, 1, P.n, P.N, (float*)P.Wabs2, P.kapA1, P.ncpA1, st))) return rc;
    if ((rc = build_cweight(H, P.N, 1, 0, nullptr, P.n, P.N, (float*)P.WH, P.kapA2, P.ncpA2, st))) return rc;
    if ((rc = build_abs2_weight(H, 1, P.N, P.N, P.n, (float*)P.Wabs2T, P.kapB1, P.ncpB1, st))) return rc;
    if ((rc = build_cweight(H, 1, P.N, 1, nullptr, P.N, P.n, (float*)P.WHH, P.kapB2, P.ncpB2, st))) return rc;
    if (band) {
        const float* wts[4] = {P.Wabs2, P.WH, P.Wabs2T, P.WHH};
        const int kaps[4] = {P.kapA1, P.kapA2, P.kapB1, P.kapB2}, ncps[4] = {P.ncpA1, P.ncpA2, P.ncpB1, P.ncpB2};
        const int bns[4] = {128, 128, 128, P.bn};
        for (int i = 0; i < 4; ++i)
            if ((rc = weight_kband(wts[i], kaps[i], ncps[i], bns[i], w.band[i], st))) return rc;
    }
    const size_t tot = std::max((size_t)E * P.N, (size_t)E * P.n);
    hipLaunchKernelGGL(tbamp_init_kernel, dim3((int)std::min<size_t>((tot + 255) / 256, 2048)), dim3(256), 0, st, P);
    AMP_LAUNCH_CHECK("tbamp_init");
    const int gr = cdiv(E, GBM);
    for (int t = 0; t < P.max_iter; ++t) {
        if (P.N % 4 != 0)
            hipLaunchKernelGGL(tbamp_ka1<ALoadPair>, dim3(gr, P.ncpA1 / 128), dim3(AMP_WG), TB_LDS_S, st, P, t);
        else
            hipLaunchKernelGGL(tbamp_ka1<ALoadPlain>, dim3(gr, P.ncpA1 / 128), dim3(AMP_WG), TB_LDS_S, st, P, t);
        hipLaunchKernelGGL(tbamp_ka2, dim3(gr, P.ncpA2 / 128), dim3(AMP_WG), TB_LDS_S, st, P, t);
        hipLaunchKernelGGL(tbamp_kb1, dim3(gr, P.ncpB1 / 128), dim3(AMP_WG), TB_LDS_S, st, P, t);
        tbamp_launch_kb2(P, gr, t, st);
        hipLaunchKernelGGL(tbamp_r, dim3(E), dim3(TBRWG), 0, st, P, c64, t);
        AMP_LAUNCH_CHECK("tbamp iteration");
    }
    hipLaunchKernelGGL(tbamp_output_kernel, dim3(E), dim3(256), 0, st, P);
    AMP_LAUNCH_CHECK("tbamp_output");
    return dec ? trials_decide_launch(d, c, td, E, w.dec, st) : AMP_OK;
}

}  // extern "C"

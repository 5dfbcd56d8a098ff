// amp_scamp_trials.hip — SCAMP over E independent single-trial detections that share one channel
// (amp_scamp_trials_run): the iteration kernels of the launch engine (amp_scamp.hip, f32 tiles)
// with per-row records.
//
// Restates, for every trial e alone, SCAMP.forward at B = 1 (scamp.py:77-107) with its Tracker
// (scamp.py:8-25), SCAMPLayer.forward (scamp.py:43-59), the mean-only block denoiser (scamp.py:61-68,
// the max|xi| shift of scamp.py:65 over the trial's own logits) and the allclose exit on the
// trial's own psi (scamp.py:105) — the way the reference's driver runs it (batch = 1, res epochs
// per channel: scamp_model.py:88, 95).
// Per iteration: the two GEMM launches of amp_scamp.hip over row tiles of 32 trials (a stopped row
// is never stored to; a tile whose rows have all stopped returns at once), the denoiser row by row
// with one partial per (tile, row), tscamp_psi where a tile holds part of a coupling block, then
// tscamp_r, a grid over the trials: workgroup e reduces trial e's partials and either settles its
// exit or leaves a pending exact float64 fix-up in the trial's record, which tscamp_fix_sec and
// tscamp_fix_psi_fin (also grids over the trials) carry out against the trial's own max|xi|.
// Every kernel returns at once when the stop counter has reached E.
#include <algorithm>
#include <mutex>

#include "amp_scamp.h"
#include "amp_trials.h"

namespace amp {

// Trial e's record, advanced in place (ScampK::iters is one record per iteration of the batch).
struct alignas(16) TScampIter {
    int32_t stopped, T, fixed, fixed_all;
    // exact float64 fix-up of iteration T-1 pending (set by tscamp_r, done by tscamp_fix_sec and
    // tscamp_fix_psi_fin, settled by the latter): the trial's exact max |xi| G, the float32
    // estimate's slack and the allclose count before the fix-up
    double G, slack;
    uint32_t notclose;
    int32_t active, pad[2];
};

struct TScampK {
    int E, N, n, L, M, Nt, Nr, Na, Lin, Lout, bn;
    int kapA, ncpA, kapB, ncpB;
    int nct, max_iter, psi_split;
    float sigma2;          // f32(noise_var) (scamp.py:51)
    const float* W;        // [Lout][Lin]
    const float* WA;       // [ncpA][kapA]  A xmmse
    const float* WAH;      // [ncpB][kapB]  A^H (z/phi)
    const float* y;        // [E][2n]
    float* z;              // [E][2n]
    float* s;              // [E][scamp_sld(n)] z / phi_use
    float* phi;            // [2][E][Lout] ping-pong
    float* tau;            // [E][Lin] (per iteration)
    float* xmap;           // caller [E][2N]
    float* xm;             // caller [E][2N]
    float* psi0;           // caller's psi [E][Lin] (even iterations)
    float* psi1;           // workspace     (odd iterations)
    float* secmax;         // [E][L]
    float* secabs;         // [E][L]
    Partial* parts;        // [E][nct]
    unsigned* psi_nc;      // [E][Lin] allclose flags of tscamp_psi (split tiles only)
    int* fixcnt;           // [E] sections recomputed by tscamp_fix_sec
    TScampIter* iters;     // [E]
    amp_status* status;    // [E]
    unsigned* nstop;       // trials whose allclose exit has fired
    const int* bandA;      // block-banded A: per column tile reduction ranges (weight_kband), else null
    const int* bandB;
    Const c;
};

struct TScampWs {
    float *WA, *WAH, *z, *s, *phi, *tau, *psi1, *secmax, *secabs;
    Partial* parts;
    unsigned* psi_nc;
    int* fixcnt;
    TScampIter* iters;
    int *bandA, *bandB;
    unsigned* nstop;
    void* dec;
    size_t bytes;
};

static void tscamp_geometry(const amp_dims* d, int E, TScampK& P) {
    P.E = E; P.N = d->N; P.n = d->n; P.L = d->L; P.M = d->M;
    P.Nt = d->Nt; P.Nr = d->Nr; P.Na = d->Na; P.Lin = d->Lin; P.Lout = d->Lout;
    P.bn = scamp_bn(d);
    P.kapA = round_up(2 * d->N, GBK); P.ncpA = round_up(2 * d->n, 128);
    P.kapB = round_up(2 * d->n, GBK); P.ncpB = round_up(2 * d->N, P.bn);
    P.nct = P.ncpB / P.bn;
    P.psi_split = scamp_psi_split(P.bn, P.Nt);
}

static TScampWs tscamp_carve(const amp_dims* d, int E, void* base) {
    TScampK P;
    tscamp_geometry(d, E, P);
    Carve cv(base);
    TScampWs w;
    w.WA = cv.take<float>((size_t)P.ncpA * P.kapA);
    w.WAH = cv.take<float>((size_t)P.ncpB * P.kapB);
    w.z = cv.take<float>((size_t)E * 2 * d->n);
    w.s = cv.take<float>((size_t)E * scamp_sld(d->n));
    w.phi = cv.take<float>((size_t)2 * E * d->Lout);
    w.tau = cv.take<float>((size_t)E * d->Lin);
    w.psi1 = cv.take<float>((size_t)E * d->Lin);
    w.secmax = cv.take<float>((size_t)E * d->L);
    w.secabs = cv.take<float>((size_t)E * d->L);
    w.parts = cv.take<Partial>((size_t)E * P.nct);
    w.psi_nc = cv.take<unsigned>((size_t)E * d->Lin);
    w.fixcnt = cv.take<int>((size_t)E);
    w.iters = cv.take<TScampIter>((size_t)E);
    w.bandA = cv.take<int>((size_t)2 * (P.ncpA / 128));
    w.bandB = cv.take<int>((size_t)2 * (P.ncpB / P.bn));
    w.nstop = cv.take<unsigned>(16);
    w.dec = cv.take<char>(trials_decide_ws_bytes(d, E));
    w.bytes = cv.off;
    return w;
}

__device__ __forceinline__ float* tspsi(const TScampK& P, int t) { return (t & 1) ? P.psi1 : P.psi0; }
__device__ __forceinline__ float* tsphi(const TScampK& P, int t) { return P.phi + (size_t)(t & 1) * P.E * P.Lout; }

// gamma[lo] = (W psi)[lo] / Lc (scamp.py:45): scamp_gamma of amp_scamp.h on the trial's own psi
__device__ __forceinline__ float tscamp_gamma(const TScampK& P, const float* psi_row, int lo) {
    float g = 0.f;
    for (int lc = 0; lc < P.Lin; ++lc) g += P.W[lo * P.Lin + lc] * psi_row[lc];
    return g / (float)P.Lin;
}

// z = y - A xmmse + b z ; phi = sigma2 + gamma ; s = z / phi   (scamp.py:45-51, 57), scamp_ka of
// amp_scamp.hip with every row on its own psi and phi.  KC: the A chunk of the f32 tile; the
// chunking does not change the MFMA order: the same bits.
__global__ __launch_bounds__(AMP_WG) void tscamp_ka(TScampK P, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_stop[GBM];
    if (*P.nstop >= (unsigned)P.E) return;
    const GemmTile tile = xcd_tile();
    const int row0 = tile.rb * GBM, col0 = tile.cb * 128;
    if (!tile_rows_live(P.iters, row0, P.E, s_stop)) return;
    const int twoN = 2 * P.N, twon = 2 * P.n, sld = scamp_sld(P.n);
    const int kb = P.bandA ? P.bandA[2 * tile.cb] : 0, ke = P.bandA ? P.bandA[2 * tile.cb + 1] : -1;
    gemm_tile<128, ALoadPlain, 256>(ALoadPlain{P.xm, twoN, P.E, twoN}, P.WA, P.kapA, row0, col0, lds, kb, ke);
    using C = GemmCfg<128, 256>;
    const float* psi = tspsi(P, t + 1);               // psi of iteration t-1 (ones at t = 0)
    const float* phi_old = tsphi(P, t + 1);           // +inf at t = 0 (scamp.py:19)
    float* phi_new = tsphi(P, t);
    // gamma of each (trial, output block) the tile touches, formed once from LDS copies of the
    // rows' psi and the W rows (scamp_ka): the same float32 sum as tscamp_gamma, in its order
    const int lo0 = (col0 >> 1) / P.Nr, nlo = (min((col0 >> 1) + 63, P.n - 1)) / P.Nr - lo0 + 1;
    const int Lin = P.Lin;
    float* sg = lds + C::CTILE_FLOATS;                 // [GBM][nlo] gamma
    float* sp = sg + GBM * nlo;                        // [GBM][Lin] psi rows
    float* sw = sp + GBM * Lin;                        // [nlo][Lin] W rows lo0 ..
    const bool per_block = C::CTILE_FLOATS + GBM * nlo + GBM * Lin + nlo * Lin <= C::A_FLOATS;
    if (per_block) {
        for (int e = threadIdx.x; e < GBM * Lin; e += AMP_WG) {
            const int row = row0 + e / Lin;
            sp[e] = row < P.E ? psi[(size_t)row0 * Lin + e] : 0.f;
        }
        for (int e = threadIdx.x; e < nlo * Lin; e += AMP_WG) sw[e] = P.W[(size_t)lo0 * Lin + e];
        __syncthreads();
        for (int e = threadIdx.x; e < GBM * nlo; e += AMP_WG) {
            const int rho = e / nlo, j = e - rho * nlo;
            float g = 0.f;
            for (int lc = 0; lc < Lin; ++lc) g += sw[j * Lin + lc] * sp[rho * Lin + lc];
            sg[e] = g / (float)Lin;
        }
        __syncthreads();
    }
    // every global load of this thread's elements before any store (scamp_ka)
    constexpr int IT = GBM * 64 / AMP_WG;
    float2 yv[IT], zv[IT];
    float po[IT];
#pragma unroll
    for (int u = 0; u < IT; ++u) {
        // unconditional loads at a clamped index; out-of-range elements are never stored
        const int e = threadIdx.x + u * AMP_WG;
        const int rho = e >> 6, cp = e & 63;
        const int row = min(row0 + rho, P.E - 1), i = min((col0 >> 1) + cp, P.n - 1);
        const size_t oc = (size_t)row * twon + 2 * i;
        yv[u] = *reinterpret_cast<const float2*>(P.y + oc);
        zv[u] = *reinterpret_cast<const float2*>(P.z + oc);
        po[u] = phi_old[(size_t)row * P.Lout + i / P.Nr];
    }
#pragma unroll
    for (int u = 0; u < IT; ++u) {
        const int e = threadIdx.x + u * AMP_WG;
        const int rho = e >> 6, cp = e & 63;
        const int row = row0 + rho, i = (col0 >> 1) + cp;
        if (row < P.E && i < P.n && !s_stop[rho]) {
            const int lo = i / P.Nr;
            const float gma = per_block ? sg[rho * nlo + lo - lo0] : tscamp_gamma(P, psi + (size_t)row * P.Lin, lo);
            const float b = gma / po[u];
            const size_t oc = (size_t)row * twon + 2 * i;
            const float ar = lds[rho * C::LDC + 2 * cp], ai = lds[rho * C::LDC + 2 * cp + 1];
            const float zr = (yv[u].x - ar) + b * zv[u].x;
            const float zi = (yv[u].y - ai) + b * zv[u].y;
            const float ph = P.sigma2 + gma;
            const float iph = 1.0f / ph;
            *reinterpret_cast<float2*>(P.z + oc) = make_float2(zr, zi);
            *reinterpret_cast<float2*>(P.s + (size_t)row * sld + 2 * i) = make_float2(zr * iph, zi * iph);
            if (i % P.Nr == 0) phi_new[(size_t)row * P.Lout + lo] = ph;
        }
    }
}

// One row of the tile for the section denoiser (ScampDenoisePolicy of amp_scamp.hip at B = 1).
struct TScampDenoisePolicy {
    const float* tile;       // the row's C-tile row (xmap)
    const float* tau_row;    // LDS: tau of the row's blocks lc0 .. lc0 + ntc - 1
    int M, Nt, colc0, lc0;
    size_t o0, s0;           // row * N + first position, row * L + first section of the tile
    float* xm;
    float* secmax;
    float* secabs;
    __device__ __forceinline__ void load(int sec, int m, float& rr, float& ri, float& it) const {
        const int cc = sec * M + m;
        const float2 v = *reinterpret_cast<const float2*>(tile + 2 * cc);
        rr = v.x; ri = v.y;
        it = 1.0f / (tau_row[(colc0 + cc) / Nt - lc0] * 0.5f);   // tau_use / 2 (scamp.py:63)
    }
    __device__ __forceinline__ void store(int sec, int m, float xr, float xi, float, PartAcc&) const {
        *reinterpret_cast<float2*>(xm + 2 * (o0 + sec * M + m)) = make_float2(xr, xi);
    }
    __device__ __forceinline__ void section(int sec, float smax, float sabs) const {
        secmax[s0 + sec] = smax;
        secabs[s0 + sec] = sabs;
    }
};

// tau = L / (W^T (1/phi)) / Mr ; xmap = xmmse + tau (A^H s) ; xmmse = denoiser ; psi   (scamp.py:53-59),
// scamp_kb of amp_scamp.hip with the denoiser, psi and the partial row by row
template <int BN, int KK, int KC>
__global__ __launch_bounds__(AMP_WG) void tscamp_kb(TScampK P, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_stop[GBM];
    if (*P.nstop >= (unsigned)P.E) return;
    using C = GemmCfg<BN, KC>;
    const GemmTile tile = xcd_tile();
    const int row0 = tile.rb * GBM, col0 = tile.cb * BN;
    if (!tile_rows_live(P.iters, row0, P.E, s_stop)) return;
    const int twoN = 2 * P.N, sld = scamp_sld(P.n);
    const int kb = P.bandB ? P.bandB[2 * tile.cb] : 0, ke = P.bandB ? P.bandB[2 * tile.cb + 1] : -1;
    gemm_tile<BN, ALoadPlain, KC>(ALoadPlain{P.s, sld, P.E, sld}, P.WAH, P.kapB, row0, col0, lds, kb, ke);
    const int nrows = min(GBM, P.E - row0), ncols = min(BN, twoN - col0);
    const int lc0 = (col0 / 2) / P.Nt, nlc = max(1, (ncols / 2) / P.Nt);   // coupling blocks in this tile
    // tau of the blocks this tile covers only (blocks lc0 .. lc0 + ntc - 1): each is written to
    // P.tau by the tile that holds its first column
    const int ntc = (col0 / 2 + ncols / 2 - 1) / P.Nt - lc0 + 1;
    constexpr int PSCR = 64;                                                 // the partial store's scratch
    float* tau_t = lds + C::CTILE_FLOATS + PSCR;                             // [32][ntc]
    const float* phi = tsphi(P, t);
    const int Lout = P.Lout;
    float* siph = tau_t + GBM * ntc;                                         // [32][Lout] 1 / phi
    float* swc = siph + GBM * Lout;                                          // [ntc][Lout] W columns
    const bool staged = C::CTILE_FLOATS + PSCR + GBM * ntc + GBM * Lout + ntc * Lout <= C::A_FLOATS;
    if (staged) {
        for (int e = threadIdx.x; e < GBM * Lout; e += AMP_WG)
            siph[e] = e / Lout < nrows ? 1.0f / phi[(size_t)row0 * Lout + e] : 0.f;
        for (int e = threadIdx.x; e < ntc * Lout; e += AMP_WG) {
            const int j = e / Lout, lo = e - j * Lout;
            swc[e] = P.W[lo * P.Lin + lc0 + j];
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < GBM * ntc; e += AMP_WG) {
        const int rho = e / ntc, lc = lc0 + e - rho * ntc;
        float tv = 0.f;
        if (rho < nrows) {
            float acc = 0.f;   // (W^T (1/phi))[lc] in float32
            if (staged)
                for (int lo = 0; lo < Lout; ++lo) acc += swc[(lc - lc0) * Lout + lo] * siph[rho * Lout + lo];
            else
                for (int lo = 0; lo < P.Lout; ++lo)
                    acc += P.W[lo * P.Lin + lc] * (1.0f / phi[(size_t)(row0 + rho) * P.Lout + lo]);
            tv = ((1.0f / acc) * (float)P.L) / (float)P.Nr;          // L / x = recip(x) * L ; / Mr
            if (lc * P.Nt >= col0 / 2 && !s_stop[rho]) P.tau[(size_t)(row0 + rho) * P.Lin + lc] = tv;
        }
        tau_t[e] = tv;
    }
    __syncthreads();
    {
        // xmmse of every element of this thread before the xmap stores (scamp_kb)
        constexpr int IT = GBM * BN / AMP_WG;
        float xv[IT];
#pragma unroll
        for (int u = 0; u < IT; ++u) {
            const int e = threadIdx.x + u * AMP_WG, rho = min(e / BN, nrows - 1), cc = min(e % BN, ncols - 1);
            xv[u] = P.xm[(size_t)(row0 + rho) * twoN + col0 + cc];
        }
#pragma unroll
        for (int u = 0; u < IT; ++u) {
            const int e = threadIdx.x + u * AMP_WG, rho = e / BN, cc = e % BN;
            if (rho < nrows && cc < ncols && !s_stop[rho]) {
                const size_t o = (size_t)(row0 + rho) * twoN + col0 + cc;
                const float tv = tau_t[rho * ntc + ((col0 + cc) >> 1) / P.Nt - lc0];
                const float xp = xv[u] + tv * lds[rho * C::LDC + cc];
                P.xmap[o] = xp;
                lds[rho * C::LDC + cc] = xp;
            }
        }
    }
    __syncthreads();
    // the denoiser row by row: the row's own partial, in the slot its B = 1 forward stores it to
    const int slot = seq_part_slot(tile.cb, P.nct), spr = (ncols / 2) / P.M;
    const float* psi_prev = tspsi(P, t + 1);
    float* psi_new = tspsi(P, t);
    for (int rho = 0; rho < nrows; ++rho) {
        if (s_stop[rho]) continue;   // workgroup-uniform
        const int row = row0 + rho;
        TScampDenoisePolicy pol;
        pol.tile = lds + rho * C::LDC; pol.tau_row = tau_t + rho * ntc;
        pol.M = P.M; pol.Nt = P.Nt; pol.colc0 = col0 / 2; pol.lc0 = lc0;
        pol.o0 = (size_t)row * P.N + col0 / 2;
        pol.s0 = (size_t)row * P.L + (col0 / 2) / P.M;
        pol.xm = P.xm; pol.secmax = P.secmax; pol.secabs = P.secabs;
        PartAcc pa;
        denoise_sections<false, KK>(pol, spr, P.M, P.c, pa);
        __syncthreads();
        // psi = 1 - sum_block |xmmse|^2 / Na (scamp.py:59) from the freshly written row
        if (!P.psi_split && (int)threadIdx.x < nlc) {
            const int lc = lc0 + threadIdx.x;
            const float2* xr = reinterpret_cast<const float2*>(P.xm) + (size_t)row * P.N + (size_t)lc * P.Nt;
            double ssum = 0.0;
            for (int m = 0; m < P.Nt; ++m) {
                const float2 v = xr[m];
                const float a = (float)sqrt((double)v.x * v.x + (double)v.y * v.y);   // torch abs (hypot)
                ssum += (double)(a * a);
            }
            const float ps = 1.0f - (float)ssum / (float)P.Na;
            const size_t o = (size_t)row * P.Lin + lc;
            pa.notclose += torch_close(ps, psi_prev[o]) ? 0u : 1u;                // scamp.py:105
            psi_new[o] = ps;
        }
        part_block_store(pa, P.parts + (size_t)row * P.nct + slot, lds + C::CTILE_FLOATS);
    }
}

// psi (scamp.py:59) and its allclose flag (scamp.py:105) when the A^H tile holds only part of a
// coupling block (scamp_psi of amp_scamp.hip): one wavefront per (trial, coupling block), after
// every tile of the iteration is written; the flags are kept per trial.
__global__ __launch_bounds__(AMP_WG) void tscamp_psi(TScampK P, int t) {
    if (*P.nstop >= (unsigned)P.E) return;
    const float* psi_prev = tspsi(P, t + 1);
    float* psi_new = tspsi(P, t);
    const int lane = threadIdx.x & 63;
    const int nwave = gridDim.x * (AMP_WG / 64);
    for (int blk = blockIdx.x * (AMP_WG / 64) + (threadIdx.x >> 6); blk < P.E * P.Lin; blk += nwave) {
        if (P.iters[blk / P.Lin].stopped) continue;   // wavefront-uniform
        const double ssum = scamp_block_energy(reinterpret_cast<const float2*>(P.xm) + (size_t)blk * P.Nt, P.Nt);
        if (lane == 0) {
            const float ps = 1.0f - (float)ssum / (float)P.Na;
            P.psi_nc[blk] = torch_close(ps, psi_prev[blk]) ? 0u : 1u;
            psi_new[blk] = ps;
        }
    }
}

constexpr int TSRWG = 256;

__device__ __forceinline__ int tscamp_block_sum(int v, int* s_i) {
    v = group_sum(v, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_i[threadIdx.x >> 6] = v;
    __syncthreads();
    int tot = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += s_i[w];
    return tot;
}

// scamp_finish of amp_scamp.hip for trial e: its record, its status and the stop counter
__device__ __forceinline__ void tscamp_finish(const TScampK& P, int e, int t, uint32_t notclose, int fixed,
                                              int fixed_all) {
    TScampIter nx;
    nx.stopped = notclose == 0 ? 1 : 0;
    nx.T = t + 1;
    nx.fixed = fixed;
    nx.fixed_all = fixed_all;
    nx.G = 0.0; nx.slack = 0.0; nx.notclose = notclose; nx.active = 0; nx.pad[0] = nx.pad[1] = 0;
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

// Workgroup e: trial e's reduction (scamp_r of amp_scamp.hip on the trial's rows): the all-NaN
// rule over the trial's own rows, the exit decision, or — when a section of the trial may leave the
// float64 range — the trial's exact float64 max |xi| into a pending record.
__global__ __launch_bounds__(TSRWG) void tscamp_r(TScampK P, Const64 c64, int t) {
    __shared__ __attribute__((aligned(16))) float lds[512];
    __shared__ double s_d[TSRWG / 64];
    __shared__ int s_i[TSRWG / 64];
    if (*P.nstop >= (unsigned)P.E) return;
    const int e = blockIdx.x;
    const TScampIter cur = P.iters[e];
    if (cur.stopped) return;
    PartAcc pa = part_reduce_all(P.parts + (size_t)e * P.nct, P.nct, lds);
    if (P.psi_split) {
        int nc = 0;
        for (int i = threadIdx.x; i < P.Lin; i += blockDim.x) nc += (int)P.psi_nc[(size_t)e * P.Lin + i];
        pa.notclose += (uint32_t)tscamp_block_sum(nc, s_i);
    }
    if (part_allnan(pa)) {
        if (!cur.fixed_all) {
            nan_fill(P.xm + (size_t)e * 2 * P.N, nullptr, (size_t)P.N);
            float* psi_new = tspsi(P, t) + (size_t)e * P.Lin;
            for (int i = threadIdx.x; i < P.Lin; i += blockDim.x) psi_new[i] = __int_as_float(0x7fc00000);
        }
        if (threadIdx.x == 0) tscamp_finish(P, e, t, 1u, -1, 1);
    } else if (part_danger(pa)) {
        // exact float64 max |xi| of the trial over its candidate sections (those within the float32
        // estimate's slack of its float32 max)
        const double slack = logit_slack(pa.maxabs);
        const float2* xp2 = reinterpret_cast<const float2*>(P.xmap) + (size_t)e * P.N;
        const float* tau = P.tau + (size_t)e * P.Lin;
        const float* secabs = P.secabs + (size_t)e * P.L;
        const int M = P.M, Nt = P.Nt;
        double gm = 0.0;
        for (int sct = threadIdx.x; sct < P.L; sct += blockDim.x) {
            if ((double)secabs[sct] < pa.maxabs - slack) continue;
            const size_t o0 = (size_t)sct * M;
            const float tv = tau[(int)(o0 / Nt)];
            auto ld = [=](int m, float& rr, float& ri, float& it) {
                const float2 v = xp2[o0 + m];
                rr = v.x; ri = v.y; it = 1.0f / (tv * 0.5f);
            };
            gm = fmax(gm, section_absmax_f64(ld, M, c64));
        }
        gm = group_max(gm, 64);
        if ((threadIdx.x & 63) == 0) s_d[threadIdx.x >> 6] = gm;
        __syncthreads();
        if (threadIdx.x == 0) {
            double G = 0.0;
            for (int w = 0; w < TSRWG / 64; ++w) G = fmax(G, s_d[w]);
            TScampIter nx;
            nx.stopped = 0; nx.T = t + 1; nx.fixed = 0; nx.fixed_all = 0;
            nx.G = G; nx.slack = slack; nx.notclose = pa.notclose; nx.active = 1; nx.pad[0] = nx.pad[1] = 0;
            P.iters[e] = nx;
        }
    } else if (threadIdx.x == 0) {
        tscamp_finish(P, e, t, pa.notclose, 0, 0);
    }
}

// Workgroup e: the sections of trial e that leave the float64 range against the trial's own G,
// recomputed with the reference's exact arithmetic (scamp_fix_sec).  Returns at once unless
// tscamp_r left the trial a pending record.
__global__ __launch_bounds__(TSRWG) void tscamp_fix_sec(TScampK P, Const64 c64, int t) {
    __shared__ int s_i[TSRWG / 64];
    if (*P.nstop >= (unsigned)P.E) return;
    const int e = blockIdx.x;
    const TScampIter pend = P.iters[e];
    if (!pend.active || pend.stopped) return;
    const float2* xp2 = reinterpret_cast<const float2*>(P.xmap) + (size_t)e * P.N;
    float2* x2 = reinterpret_cast<float2*>(P.xm) + (size_t)e * P.N;
    const float* tau = P.tau + (size_t)e * P.Lin;
    const float* secmax = P.secmax + (size_t)e * P.L;
    const int M = P.M, Nt = P.Nt;
    int cnt = 0;
    for (int sct = threadIdx.x; sct < P.L; sct += blockDim.x) {
        if (!((double)secmax[sct] - pend.G < AMP_DANGER + pend.slack)) continue;
        const size_t o0 = (size_t)sct * M;
        const float tv = tau[(int)(o0 / Nt)];
        auto ld = [=](int m, float& rr, float& ri, float& it) {
            const float2 v = xp2[o0 + m];
            rr = v.x; ri = v.y; it = 1.0f / (tv * 0.5f);
        };
        auto st = [=](int m, float xr, float xi, float) { x2[o0 + m] = make_float2(xr, xi); };
        exact_section_f64<false>(ld, st, M, c64, pend.G);
        ++cnt;
    }
    cnt = tscamp_block_sum(cnt, s_i);
    if (threadIdx.x == 0) P.fixcnt[e] = cnt;
}

// Workgroup e: psi of the coupling blocks of trial e that hold a recomputed section, the allclose
// delta, then the trial's exit, stop record and status (scamp_fix_psi_fin).
__global__ __launch_bounds__(TSRWG) void tscamp_fix_psi_fin(TScampK P, int t) {
    __shared__ int s_i[TSRWG / 64];
    if (*P.nstop >= (unsigned)P.E) return;
    const int e = blockIdx.x;
    const TScampIter pend = P.iters[e];
    if (!pend.active || pend.stopped) return;
    const float* psi_prev = tspsi(P, t + 1) + (size_t)e * P.Lin;
    float* psi_new = tspsi(P, t) + (size_t)e * P.Lin;
    const float* secmax = P.secmax + (size_t)e * P.L;
    const int spb = P.Nt / P.M;   // sections per coupling block
    int dnc = 0;
    if (P.Nt > SFIX_SERIAL_NT) {
        // wide blocks: one wavefront per block, in tscamp_psi's summation order (scamp_fix_psi_body)
        for (int blk = threadIdx.x >> 6; blk < P.Lin; blk += blockDim.x >> 6) {
            if (!scamp_block_hit_wave(secmax + (size_t)blk * spb, spb, pend.G, pend.slack)) continue;
            const double ssum = scamp_block_energy(
                reinterpret_cast<const float2*>(P.xm) + (size_t)e * P.N + (size_t)blk * P.Nt, P.Nt);
            if ((threadIdx.x & 63) == 0) {
                const float ps = 1.0f - (float)ssum / (float)P.Na;
                dnc += (torch_close(ps, psi_prev[blk]) ? 0 : 1) - (torch_close(psi_new[blk], psi_prev[blk]) ? 0 : 1);
                psi_new[blk] = ps;
            }
        }
    } else
    for (int blk = threadIdx.x; blk < P.Lin; blk += blockDim.x) {
        bool hit = false;
        for (int j = 0; j < spb && !hit; ++j)
            hit = (double)secmax[(size_t)blk * spb + j] - pend.G < AMP_DANGER + pend.slack;
        if (!hit) continue;
        const float2* xr = reinterpret_cast<const float2*>(P.xm) + (size_t)e * P.N + (size_t)blk * P.Nt;
        double ssum = 0.0;
        for (int m = 0; m < P.Nt; ++m) {
            const float a = (float)sqrt((double)xr[m].x * xr[m].x + (double)xr[m].y * xr[m].y);
            ssum += (double)(a * a);
        }
        const float ps = 1.0f - (float)ssum / (float)P.Na;
        dnc += (torch_close(ps, psi_prev[blk]) ? 0 : 1) - (torch_close(psi_new[blk], psi_prev[blk]) ? 0 : 1);
        psi_new[blk] = ps;
    }
    dnc = tscamp_block_sum(dnc, s_i);
    if (threadIdx.x == 0) tscamp_finish(P, e, t, (uint32_t)((int)pend.notclose + dnc), P.fixcnt[e], 0);
}

// Tracker (scamp.py:9-25) for every trial: z = y, psi = 1, phi = inf, xmmse = 0
__global__ void tscamp_init_kernel(TScampK P) {
    const size_t EN = (size_t)P.E * P.N, En = (size_t)P.E * P.n, EL = (size_t)P.E * P.Lout;
    const size_t tot = std::max(std::max(EN, En), std::max(EL, (size_t)P.E * P.Lin));
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
        if (e < EN) reinterpret_cast<float2*>(P.xm)[e] = make_float2(0.f, 0.f);
        if (e < En) reinterpret_cast<float2*>(P.z)[e] = reinterpret_cast<const float2*>(P.y)[e];
        if (e < (size_t)P.E * P.Lin) P.psi1[e] = 1.0f;
        if (e < EL) P.phi[EL + e] = INFINITY;        // phi buffer of "iteration -1"
        if (e < (size_t)P.E)                         // the pad of an odd n's s rows (scamp_sld)
            for (int k = 2 * P.n; k < scamp_sld(P.n); ++k) P.s[e * scamp_sld(P.n) + k] = 0.f;
        if (e < (size_t)P.E) {
            TScampIter it;
            it.stopped = 0; it.T = 0; it.fixed = 0; it.fixed_all = 0;
            it.G = 0.0; it.slack = 0.0; it.notclose = 0; it.active = 0; it.pad[0] = it.pad[1] = 0;
            P.iters[e] = it;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *P.nstop = 0u;
}

// Trial e's last executed iteration wrote psi into buffer (T_e - 1) & 1; buffer 0 is the caller's.
__global__ __launch_bounds__(64) void tscamp_output_kernel(TScampK P) {
    const int e = blockIdx.x;
    const int T = P.status[e].T;
    if (((T - 1) & 1) == 0) return;
    for (int i = threadIdx.x; i < P.Lin; i += blockDim.x) P.psi0[(size_t)e * P.Lin + i] = P.psi1[(size_t)e * P.Lin + i];
}

constexpr size_t TS_LDS_S = GemmCfg<128, 256>::LDS_BYTES;   // within the default 64 KB
constexpr size_t TS_LDS_W = GemmCfg<256>::LDS_BYTES;

template <int KK>
static int tscamp_kb_attr() { return set_lds_attr<256>((const void*)tscamp_kb<256, KK, GKC>); }

static std::once_flag g_tscamp_once;
static int g_tscamp_rc = 0;
static int tscamp_attrs() {
    std::call_once(g_tscamp_once, [] {
        int rc = tscamp_kb_attr<1>();
        if (!rc) rc = tscamp_kb_attr<2>();
        if (!rc) rc = tscamp_kb_attr<4>();
        if (!rc) rc = tscamp_kb_attr<8>();
        if (!rc) rc = tscamp_kb_attr<16>();
        if (!rc) rc = tscamp_kb_attr<64>();
        g_tscamp_rc = rc;
    });
    return g_tscamp_rc;
}

template <int KK>
static void tscamp_launch_kb_kk(const TScampK& P, int gr, int t, hipStream_t st) {
    if (P.bn == 128)
        hipLaunchKernelGGL((tscamp_kb<128, KK, 256>), dim3(gr, P.ncpB / 128), dim3(AMP_WG), TS_LDS_S, st, P, t);
    else
        hipLaunchKernelGGL((tscamp_kb<256, KK, GKC>), dim3(gr, P.ncpB / 256), dim3(AMP_WG), TS_LDS_W, st, P, t);
}

static void tscamp_launch_kb(const TScampK& P, int gr, int t, hipStream_t st) {
    switch (P.c.K) {
    case 1: tscamp_launch_kb_kk<1>(P, gr, t, st); break;
    case 2: tscamp_launch_kb_kk<2>(P, gr, t, st); break;
    case 4: tscamp_launch_kb_kk<4>(P, gr, t, st); break;
    case 8: tscamp_launch_kb_kk<8>(P, gr, t, st); break;
    case 16: tscamp_launch_kb_kk<16>(P, gr, t, st); break;
    default: tscamp_launch_kb_kk<64>(P, gr, t, st); break;
    }
}

// any Nt (amp_scamp_run's shapes); the byte query answers 0 for dims the run would refuse
static bool tscamp_shape_ok(const amp_dims* d, int E) {
    return d->Nt > 0 && d->Na > 0 && d->Nr > 0 && d->Lin > 0 && d->Lout > 0 && d->Lin <= SMAXLIN &&
           d->N == d->Nt * d->Lin && d->n == d->Nr * d->Lout && scamp_index_ok(d, E);
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
    int rc = check_dims(d, c, true, true);   // any Nt, a partial last column tile (amp_scamp_run)
    if (rc) return rc;
    AMP_REQUIRE(d->B == 1, "amp_scamp_trials_run: dims describe ONE trial (B = %d, must be 1)", d->B);
    AMP_REQUIRE(trials >= 1, "amp_scamp_trials_run: trials = %d", trials);
    AMP_REQUIRE(a && a->W && a->A && a->y && a->xmap && a->xmmse && a->psi && a->status && a->ws,
                "amp_scamp_trials_run: null pointer argument");
    AMP_REQUIRE(a->max_iter > 0, "amp_scamp_trials_run: max_iter must be positive");
    AMP_REQUIRE(d->Lin <= SMAXLIN, "amp_scamp_trials_run: Lin = %d > %d", d->Lin, SMAXLIN);
    AMP_REQUIRE(scamp_index_ok(d, trials), "amp_scamp_trials_run: %d trials of max(2N, 2n) = %d columns need more "
                "than 32-bit offsets (or more than 65535 column tiles)", trials, 2 * std::max(d->N, d->n));
    AMP_REQUIRE(a->engine == AMP_ENGINE_AUTO || a->engine == AMP_ENGINE_LAUNCHES,
                "amp_scamp_trials_run: launch engine only (engine %d)", a->engine);
    AMP_REQUIRE(a->gemm == AMP_GEMM_AUTO || a->gemm == AMP_GEMM_F32, "amp_scamp_trials_run: f32 GEMMs only (gemm %d)",
                a->gemm);
    const int E = trials;
    const TScampWs w = tscamp_carve(d, E, a->ws);
    AMP_REQUIRE(a->ws_bytes >= w.bytes, "amp_scamp_trials_run: workspace %zu < %zu bytes", a->ws_bytes, w.bytes);
    TrialsDecide td{};
    if (dec && (rc = trials_decide_args(d, dec, a->xmap, a->xmmse, td))) return rc;
    if ((rc = tscamp_attrs())) return rc;
    TScampK P{};
    tscamp_geometry(d, E, P);
    P.max_iter = a->max_iter;
    P.sigma2 = (float)a->noise_var;
    P.W = (const float*)a->W;
    P.WA = w.WA; P.WAH = w.WAH;
    P.y = (const float*)a->y; P.z = w.z; P.s = w.s; P.phi = w.phi; P.tau = w.tau;
    P.xmap = (float*)a->xmap; P.xm = (float*)a->xmmse; P.psi0 = (float*)a->psi; P.psi1 = w.psi1;
    P.secmax = w.secmax; P.secabs = w.secabs; P.parts = w.parts; P.psi_nc = w.psi_nc; P.fixcnt = w.fixcnt;
    P.iters = w.iters;
    P.status = (amp_status*)a->status;
    P.nstop = w.nstop;
    const bool band = d->Lin > 1 || d->Lout > 1;   // block-banded A (channel.py:75-95)
    P.bandA = band ? w.bandA : nullptr;
    P.bandB = band ? w.bandB : nullptr;
    P.c = to_const(c);
    const Const64 c64 = to_const64(c);
    hipStream_t st = (hipStream_t)stream;
    // the operators and their band ranges, packed once per call (Tracker: A, A^H, scamp.py:12-13)
    const float2* A = (const float2*)a->A;
    if ((rc = build_cweight(A, P.N, 1, 0, nullptr, P.n, P.N, (float*)P.WA, P.kapA, P.ncpA, st))) return rc;
    if ((rc = build_cweight(A, 1, P.N, 1, nullptr, P.N, P.n, (float*)P.WAH, P.kapB, P.ncpB, st))) return rc;
    if (band) {
        if ((rc = weight_kband(P.WA, P.kapA, P.ncpA, 128, w.bandA, st))) return rc;
        if ((rc = weight_kband(P.WAH, P.kapB, P.ncpB, P.bn, w.bandB, st))) return rc;
    }
    const size_t tot = std::max(std::max((size_t)E * P.N, (size_t)E * P.n), (size_t)E * std::max(P.Lout, P.Lin));
    hipLaunchKernelGGL(tscamp_init_kernel, dim3((int)std::min<size_t>((tot + 255) / 256, 2048)), dim3(256), 0, st, P);
    AMP_LAUNCH_CHECK("tscamp_init");
    const int gr = cdiv(E, GBM);
    const int npsi = std::max(1, std::min(cdiv(E * P.Lin, AMP_WG / 64), 2048));
    for (int t = 0; t < P.max_iter; ++t) {
        hipLaunchKernelGGL(tscamp_ka, dim3(gr, P.ncpA / 128), dim3(AMP_WG), TS_LDS_S, st, P, t);
        tscamp_launch_kb(P, gr, t, st);
        if (P.psi_split) hipLaunchKernelGGL(tscamp_psi, dim3(npsi), dim3(AMP_WG), 0, st, P, t);
        hipLaunchKernelGGL(tscamp_r, dim3(E), dim3(TSRWG), 0, st, P, c64, t);
        hipLaunchKernelGGL(tscamp_fix_sec, dim3(E), dim3(TSRWG), 0, st, P, c64, t);
        hipLaunchKernelGGL(tscamp_fix_psi_fin, dim3(E), dim3(TSRWG), 0, st, P, t);
        AMP_LAUNCH_CHECK("tscamp iteration");
    }
    hipLaunchKernelGGL(tscamp_output_kernel, dim3(E), dim3(64), 0, st, P);
    AMP_LAUNCH_CHECK("tscamp_output");
    return dec ? trials_decide_launch(d, c, td, E, w.dec, st) : AMP_OK;
}

}  // extern "C"

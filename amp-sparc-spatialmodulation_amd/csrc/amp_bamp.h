// amp_bamp.h — BAMP state and GEMM epilogues shared by the launch engine (amp_bamp.hip) and the
// independent-trial engine (amp_bamp_trials.hip): the parameter block, its geometry, and every
// epilogue of BAMPLayer.forward (bamp.py:59-64) written once.  A kernel of either engine is its
// entry guard, its gemm_tile call and one call in here, with the row guard of its engine
// (amp_trials.h AllRows / LiveRows): a trial has the bits of its own B = 1 forward by construction.
#pragma once

#include <algorithm>

#include "amp_trials.h"

namespace amp {

struct alignas(16) BampIter {
    int32_t stopped, T, fixed, fixed_all;
    // exact float64 fix-up of iteration T-1 pending (set by bamp_r, done and settled by
    // bamp_fixall): the exact batch max |xi| G, the float32 estimate's slack, the allclose count
    // before the fix-up
    double G, slack;
    uint32_t notclose;
    int32_t active, pad[2];
};

// B: the rows of the GEMM tiles (the batch; the trials of amp_bamp_trials_run, whose per-trial
// records, BampTrials, travel beside this block)
struct BampK {
    int B, N, n, L, M, bn;
    int kapA1, ncpA1, kapA2, ncpA2, kapB1, ncpB1, kapB2, ncpB2;
    int nblk, max_iter;
    int ild, sld;       // row strides of invu and s (bamp_ild / bamp_sld: n, 2n rounded up to 4)
    float sigma2;       // f32(noise_var): u = v + sigma2 (bamp.py:61)
    const float* Wabs2;    // [ncpA1][kapA1]   v = |H|^2 var
    const float* WH;       // [ncpA2][kapA2]   H xmmse
    const float* Wabs2T;   // [ncpB1][kapB1]   |H|^2^T (1/u)
    const float* WHH;      // [ncpB2][kapB2]   H^H s
    const float* y;        // [B][2n]
    float* v;              // [B][n]
    float* z;              // [B][2n]
    float* invu;           // [B][ild]
    float* s;              // [B][sld]  (y - z)/u
    float* cov;            // [B][N]
    float* xmap;           // [B][2N]  caller
    float* xm;             // [B][2N]  caller
    float* var0;           // caller's var (even iterations)
    float* var1;           // workspace  (odd iterations)
    float* secmax;         // [B*L] per-section max logit (fast path)
    float* secabs;         // [B*L] per-section max |logit|
    Partial* parts;        // launch engine [max_iter][nblk]; trial engine [B][column tiles]
    BampIter* iters;       // launch engine [max_iter + 1]
    amp_status* status;    // launch engine: one; trial engine [B]
    // block-banded H (Lin > 1 or Lout > 1): per column tile of Wabs2 / WH / Wabs2T / WHH the
    // reduction range holding its nonzero blocks (weight_kband), else null (whole range)
    const int* band[4];
    XState* xs;            // trial-sharded exchange words (amp_bamp_run_sharded)
    Const c;
    int elementwise;                       // random_denoiser (bamp.py:79-88) instead of the block one
    float P0, Ps;
    // fp16x2 GEMMs (amp_gemm_h2.h): the four operators h2-packed into the weight buffers above
    // (real |H|^2 two planes, complex H / H^H four), each GEMM's A rows split into `ap` first
    // bf16x3 GEMMs (amp_gemm_x3.h, x3 = 1): the same scheme with three bf16 pieces per value (real
    // |H|^2 three planes, complex H / H^H six; no exponents)
    int h2, x3, rows_pad;
    int tile_rows;         // row-block-major tile order (xcd_tile_rows: the fp16x2 tiles), else xcd_tile
    unsigned short* ap;    // [4 planes][rows_pad][max(N, n)] fp16, or [6 planes][...] bf16
    int* rexp;             // [rows_pad] row exponents
    // launch engine: rcnt[1] is bamp_fixall's arrival counter (zeroed by bamp_init_kernel)
    unsigned* rcnt;
};

// tile geometry of `rows` rows sharing the operators of `d`
inline void bamp_geometry(const amp_dims* d, int rows, BampK& P) {
    P.B = rows; P.N = d->N; P.n = d->n; P.L = d->L; P.M = d->M;
    P.bn = section_bn(d);
    P.kapA1 = round_up(d->N, GBK); P.ncpA1 = round_up(d->n, 128);
    P.kapA2 = round_up(2 * d->N, GBK); P.ncpA2 = round_up(2 * d->n, 128);
    P.kapB1 = round_up(d->n, GBK); P.ncpB1 = round_up(d->N, 128);
    P.kapB2 = round_up(2 * d->n, GBK); P.ncpB2 = round_up(2 * d->N, P.bn);
    P.nblk = cdiv(rows, GBM) * (P.ncpB2 / P.bn);
    P.ild = bamp_ild(d->n); P.sld = bamp_sld(d->n);
}

__device__ __forceinline__ float* bvar(const BampK& P, int t) { return (t & 1) ? P.var1 : P.var0; }
// reduction range of column tile cb of GEMM weight w (0..3: Wabs2, WH, Wabs2T, WHH); whole range
// when the channel is not block-banded
__device__ __forceinline__ int bkb(const BampK& P, int w, int cb) { return P.band[w] ? P.band[w][2 * cb] : 0; }
__device__ __forceinline__ int bke(const BampK& P, int w, int cb) { return P.band[w] ? P.band[w][2 * cb + 1] : -1; }

// The f32 operators, MFMA-packed, and their band ranges (Tracker: adj, abs2, abs2T, bamp.py:17-19)
inline int bamp_pack_f32(const BampK& P, const float2* H, hipStream_t st) {
    int rc;
    if ((rc = build_abs2_weight(H, P.N, 1, P.n, P.N, (float*)P.Wabs2, P.kapA1, P.ncpA1, st))) return rc;
    if ((rc = build_cweight(H, P.N, 1, 0, nullptr, P.n, P.N, (float*)P.WH, P.kapA2, P.ncpA2, st))) return rc;
    if ((rc = build_abs2_weight(H, 1, P.N, P.N, P.n, (float*)P.Wabs2T, P.kapB1, P.ncpB1, st))) return rc;
    if ((rc = build_cweight(H, 1, P.N, 1, nullptr, P.N, P.n, (float*)P.WHH, P.kapB2, P.ncpB2, st))) return rc;
    if (!P.band[0]) return AMP_OK;
    const float* wts[4] = {P.Wabs2, P.WH, P.Wabs2T, P.WHH};
    const int kaps[4] = {P.kapA1, P.kapA2, P.kapB1, P.kapB2}, ncps[4] = {P.ncpA1, P.ncpA2, P.ncpB1, P.ncpB2};
    const int bns[4] = {128, 128, 128, P.bn};
    for (int i = 0; i < 4; ++i)
        if ((rc = weight_kband(wts[i], kaps[i], ncps[i], bns[i], const_cast<int*>(P.band[i]), st))) return rc;
    return AMP_OK;
}

// Tracker (bamp.py:13-25) of every row: xmmse = 0, var(prev) = 1, z = y, u = 0 + sigma2 -> 1/u;
// a grid-stride body (the engines' init kernels add their records)
__device__ __forceinline__ void bamp_init_state(const BampK& P) {
    const size_t BN_ = (size_t)P.B * P.N, Bn = (size_t)P.B * P.n;
    const size_t tot = BN_ > Bn ? BN_ : Bn;
    const float iu = 1.0f / P.sigma2;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
        if (e < BN_) {
            reinterpret_cast<float2*>(P.xm)[e] = make_float2(0.f, 0.f);
            P.var1[e] = 1.0f;
        }
        if (e < Bn) {
            reinterpret_cast<float2*>(P.z)[e] = reinterpret_cast<const float2*>(P.y)[e];
            P.invu[P.ild == P.n ? e : (e / P.n) * P.ild + e % P.n] = iu;
        }
        if (e < (size_t)P.B) {   // the pads of the invu and s rows (bamp_ild / bamp_sld), zeroed once
            for (int k = P.n; k < P.ild; ++k) P.invu[e * P.ild + k] = 0.f;
            for (int k = 2 * P.n; k < P.sld; ++k) P.s[e * P.sld + k] = 0.f;
        }
    }
}

// The status record of a forward that ends after iteration t (bamp.py:140)
__device__ __forceinline__ amp_status bamp_status(const BampK& P, int t, int fixed, int stopped) {
    amp_status s;
    s.T = t + 1; s.nan_state = fixed != 0 ? 1 : 0; s.stopped = stopped;
    s.gemm = P.h2 ? AMP_ARITH_FP16X2 : P.x3 ? AMP_ARITH_BF16X3 : AMP_ARITH_F32;
    s.last_scalar[0] = s.last_scalar[1] = s.last_scalar[2] = s.last_scalar[3] = 0.f;
    return s;
}

// ---- the GEMM epilogues: `lds` holds the C tile (row stride GemmCfg<BN>::LDC), g the row guard ----

// v = |H|^2 var (bamp.py:59)
template <class G>
__device__ __forceinline__ void bamp_store_v(const BampK& P, const G& g, const float* lds, int row0, int col0) {
    using C = GemmCfg<128>;
    for (int e = threadIdx.x; e < GBM * 128; e += AMP_WG) {
        const int rho = e >> 7, cc = e & 127;
        const int row = row0 + rho, col = col0 + cc;
        if (row < P.B && col < P.n && g.live(rho)) P.v[(size_t)row * P.n + col] = lds[rho * C::LDC + cc];
    }
}

// z = H xmmse - v (y - z) / u ; u = v + sigma2 ; s = (y - z) / u   (bamp.py:60-63)
template <class G>
__device__ __forceinline__ void bamp_residual(const BampK& P, const G& g, const float* lds, int row0, int col0) {
    using C = GemmCfg<128>;
    const int twon = 2 * P.n;
    // every global load of this thread's epilogue elements before any store (the z / invu / s
    // stores may alias the next element's loads as far as the compiler knows: one memory latency
    // per element otherwise); each element reads and writes only its own z and invu.  (The loads
    // issued before the GEMM measured slower: cfg5 64-QAM 18.24 -> 18.52 ms, ISI BAMP 0.1330 ->
    // 0.1345 ms per iteration; the 48 registers they hold across the reduction cost more than the
    // overlap gains.)
    constexpr int IT = GBM * 64 / AMP_WG;
    float2 yv[IT], zv[IT];
    float vv[IT], iuo[IT];
#pragma unroll
    for (int u = 0; u < IT; ++u) {
        // unconditional loads at a clamped index (a lane-divergent branch around them
        // serialises their latencies, amp_gemm.h ALoadPlain); out-of-range elements are never stored
        const int e = threadIdx.x + u * AMP_WG;
        const int rho = e >> 6, cp = e & 63;           // complex column pair
        const int row = min(row0 + rho, P.B - 1), i = min((col0 >> 1) + cp, P.n - 1);
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
        if (row < P.B && i < P.n && g.live(rho)) {
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
template <class G>
__device__ __forceinline__ void bamp_store_cov(const BampK& P, const G& g, const float* lds, int row0, int col0) {
    using C = GemmCfg<128>;
    for (int e = threadIdx.x; e < GBM * 128; e += AMP_WG) {
        const int rho = e >> 7, cc = e & 127;
        const int row = row0 + rho, col = col0 + cc;
        if (row < P.B && col < P.N && g.live(rho)) P.cov[(size_t)row * P.N + col] = 1.0f / lds[rho * C::LDC + cc];
    }
}

// xmap = xmmse + cov (H^H s)  (bamp.py:63), stored and left in the C tile for the denoiser, with the
// denoiser's 1 / tau = 1 / (cov / 2) of every position beside it in LDS (returned: [GBM][BN / 2],
// past the partial-store scratch): read there instead of a global load per position inside the
// denoiser's loop (the same float32 operations).  Ends with a barrier.
template <int BN, int KC, class G>
__device__ __forceinline__ float* bamp_xmap(const BampK& P, const G& g, float* lds, int row0, int col0, int nrows,
                                            int ncols) {
    using C = GemmCfg<BN, KC>;
    const int twoN = 2 * P.N;
    float* sit = lds + C::CTILE_FLOATS + 2048;
    // the loads of this thread's elements before the xmap stores (which may alias them as far as
    // the compiler knows)
    constexpr int IT = GBM * BN / AMP_WG;
    static_assert(C::CTILE_FLOATS + 2048 + GBM * (BN / 2) <= C::A_FLOATS, "1 / tau tile");
    float xv[IT], cvv[IT];
#pragma unroll
    for (int u = 0; u < IT; ++u) {
        // unconditional loads at a clamped index (see bamp_residual); out-of-range elements unused
        const int e = threadIdx.x + u * AMP_WG, rho = min(e / BN, nrows - 1), cc = min(e % BN, ncols - 1);
        xv[u] = P.xm[(size_t)(row0 + rho) * twoN + col0 + cc];
        cvv[u] = P.cov[(size_t)(row0 + rho) * P.N + ((col0 + cc) >> 1)];
    }
#pragma unroll
    for (int u = 0; u < IT; ++u) {
        const int e = threadIdx.x + u * AMP_WG, rho = e / BN, cc = e % BN;
        if (rho < nrows && cc < ncols && g.live(rho)) {
            const size_t o = (size_t)(row0 + rho) * twoN + col0 + cc;
            const float xp = xv[u] + cvv[u] * lds[rho * C::LDC + cc];
            P.xmap[o] = xp;
            lds[rho * C::LDC + cc] = xp;
            if ((cc & 1) == 0) sit[rho * (BN / 2) + (cc >> 1)] = 1.0f / (cvv[u] * 0.5f);
        }
    }
    __syncthreads();
    return sit;
}

struct BampDenoisePolicy {
    const float* tile;
    const float* itile;   // LDS [rows][ldi]: 1 / (cov / 2) of the tile's positions (bamp_xmap)
    int ldc, ldi, spr, M, N, row0, colc0;
    float* xm;
    float* var_new;
    const float* var_prev;
    float* secmax;
    float* secabs;
    int L;
    __device__ __forceinline__ void load(int sec, int m, float& rr, float& ri, float& it) const {
        const int rho = sec / spr, sj = sec - rho * spr;
        const float2 v = *reinterpret_cast<const float2*>(tile + rho * ldc + 2 * (sj * M + m));
        rr = v.x; ri = v.y;
        it = itile[rho * ldi + sj * M + m];   // 1 / tau, tau = cov / 2 (bamp.py:68)
    }
    __device__ __forceinline__ void store(int sec, int m, float xr, float xi, float var, PartAcc& pa) const {
        const int rho = sec / spr, sj = sec - rho * spr;
        const size_t o = (size_t)(row0 + rho) * N + colc0 + sj * M + m;
        *reinterpret_cast<float2*>(xm + 2 * o) = make_float2(xr, xi);
        var_new[o] = var;
        pa.sumvar += (double)var;
        pa.notclose += torch_close(var, var_prev[o]) ? 0u : 1u;     // bamp.py:140
    }
    __device__ __forceinline__ void section(int sec, float smax, float sabs) const {
        const int rho = sec / spr, sj = sec - rho * spr;
        const size_t o = (size_t)(row0 + rho) * L + (colc0 / M) + sj;
        secmax[o] = smax;
        secabs[o] = sabs;
    }
};

// The denoiser's view of the tile rows from rho on (bamp_xmap's C tile and 1 / tau tile): the whole
// tile at rho = 0 (the launch engine: nrows * spr sections), one row when only spr sections are
// denoised (the trial engine: sec / spr is then 0 and every address the same integer as the
// B = 1 forward's, whose tile has that one row)
template <int BN, int KC>
__device__ __forceinline__ BampDenoisePolicy bamp_policy(const BampK& P, int t, const float* lds, const float* sit,
                                                         int row0, int col0, int ncols, int rho) {
    using C = GemmCfg<BN, KC>;
    BampDenoisePolicy pol;
    pol.tile = lds + rho * C::LDC; pol.itile = sit + rho * (BN / 2); pol.ldi = BN / 2; pol.ldc = C::LDC;
    pol.M = P.M; pol.N = P.N; pol.L = P.L;
    pol.spr = (ncols / 2) / P.M; pol.row0 = row0 + rho; pol.colc0 = col0 / 2;
    pol.xm = P.xm; pol.var_new = bvar(P, t); pol.var_prev = bvar(P, t + 1); pol.secmax = P.secmax; pol.secabs = P.secabs;
    return pol;
}

// BAMPLayer.random_denoiser (bamp.py:79-88) for one entry, in the reference's dtypes: G(0) in
// float32 (r - 0 stays complex64), G(a_k) in float64 (complex64 - complex128), norm / exp / var
// in float64 (the float32 prior scalars promoted), complex128 / float64 as a reciprocal multiply.
// c64: torch.tensor(config.symbols), complex128 (bamp.py:37).
// KK: the table size as a compile-time bound (points k >= c64.K skipped): the loop is unrolled so
// the by-value kernel-argument table is only read at constant offsets (a runtime-indexed loop made
// the compiler copy the whole table into scratch memory at every kernel entry: ~900 B per lane).
template <int KK>
__device__ __forceinline__ void bamp_bayes_elem(const BampK& P, const Const64& c64, float rr, float ri, float cov,
                                                float& xr, float& xi, float& var) {
    const float a0 = hypotf(rr, ri);
    const float g0 = expf(-(a0 * a0) / cov);
    const double cd = (double)cov;
    double gs = 0.0, sr = 0.0, si = 0.0, s2 = 0.0;
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        if (k >= c64.K) break;
        const double a = hypot((double)rr - c64.re[k], (double)ri - c64.im[k]);
        const double g = exp(-(a * a) / cd);
        const double ak = hypot(c64.re[k], c64.im[k]);
        gs += g;
        sr += c64.re[k] * g;
        si += c64.im[k] * g;
        s2 += (ak * ak) * g;
    }
    double norm = (double)(P.P0 * g0) + (double)P.Ps * gs;
    if (norm == 0.0) norm = 1e-9;                                       // regularize_zero (bamp.py:90-92)
    const double rn = 1.0 / norm;
    const double er = ((double)P.Ps * sr) * rn, ei = ((double)P.Ps * si) * rn;
    const double ae = hypot(er, ei);
    xr = (float)er;
    xi = (float)ei;
    var = (float)(((double)P.Ps * s2) / norm - ae * ae);
}

// The element-wise denoiser (generator_mode 'random') over rows [rho0, rho0 + nrho) of the C tile
// bamp_xmap left in `lds`: xmmse, this iteration's var, and into pa the sum of var and the allclose
// count against the previous var (bamp.py:140).  There is no batch-global shift in random_denoiser:
// the section statistics of pa stay neutral.  Element e = threadIdx.x + i AMP_WG of the
// nrho x BN / 2 block: the launch engine calls it once for the tile's rows, the trial engine row by
// row (a row's BN / 2 columns then go to the threads its own B = 1 forward gives them, so the row's
// partial is folded in that forward's order).
template <int BN, int KC, int KK>
__device__ __forceinline__ void bamp_bayes_rows(const BampK& P, const Const64& c64, int t, const float* lds, int row0,
                                                int col0, int rho0, int nrho, int ncols, PartAcc& pa) {
    using C = GemmCfg<BN, KC>;
    float* vn = bvar(P, t);
    const float* vp = bvar(P, t + 1);
    for (int e = threadIdx.x; e < nrho * (BN / 2); e += AMP_WG) {
        const int rho = rho0 + e / (BN / 2), cc = e % (BN / 2);
        if (2 * cc < ncols) {
            const size_t o = (size_t)(row0 + rho) * P.N + col0 / 2 + cc;
            const float2 v = *reinterpret_cast<const float2*>(lds + rho * C::LDC + 2 * cc);
            float xr, xi, var;
            bamp_bayes_elem<KK>(P, c64, v.x, v.y, P.cov[o], xr, xi, var);
            *reinterpret_cast<float2*>(P.xm + 2 * o) = make_float2(xr, xi);
            vn[o] = var;
            pa.sumvar += (double)var;
            pa.notclose += torch_close(var, vp[o]) ? 0u : 1u;     // bamp.py:140
        }
    }
}

// One section for the exact float64 fix-up (section_absmax_f64 / exact_section_f64), o0 its first
// position in [B][N]: the loader (xmap and 1 / tau, tau = cov / 2) and the store (xmmse, var and the
// allclose delta against the previous var, added to *dnc)
struct BampSectionLoad {
    const float2* xp2;
    const float* cov;
    __device__ __forceinline__ void operator()(int m, float& rr, float& ri, float& it) const {
        const float2 v = xp2[m];
        rr = v.x; ri = v.y; it = 1.0f / (cov[m] * 0.5f);
    }
};
struct BampSectionStore {
    float2* x2;
    float* vn;
    const float* vp;
    int* dnc;
    __device__ __forceinline__ void operator()(int m, float xr, float xi, float var) const {
        *dnc += (torch_close(var, vp[m]) ? 0 : 1) - (torch_close(vn[m], vp[m]) ? 0 : 1);
        x2[m] = make_float2(xr, xi);
        vn[m] = var;
    }
};
__device__ __forceinline__ BampSectionLoad bamp_section_load(const BampK& P, size_t o0) {
    return BampSectionLoad{reinterpret_cast<const float2*>(P.xmap) + o0, P.cov + o0};
}
__device__ __forceinline__ BampSectionStore bamp_section_store(const BampK& P, int t, size_t o0, int* dnc) {
    return BampSectionStore{reinterpret_cast<float2*>(P.xm) + o0, bvar(P, t) + o0, bvar(P, t + 1) + o0, dnc};
}

}  // namespace amp

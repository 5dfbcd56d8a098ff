// amp_vamp_launch.h — the VAMP launch engine's bodies, shared by the batch engine (amp_vamp.hip)
// and the independent-trial engine (amp_vamp_trials.hip): the A-operand prologue and both GEMM
// epilogues of VAMPLayer.forward (vamp.py:56-94), the denoiser's view of the C tile, the Tracker
// (vamp.py:22-26), and the reduction step (all-NaN rule, exact float64 fix-up, next record and
// status), each written once.  A kernel of either engine is its entry guard, its gemm_tile call and
// calls in here with the record guard of its engine: a trial has the bits of its own B = 1 forward
// by construction.  (Not part of amp_vamp.h: the persistent engines include that, and none of this
// is theirs.)
#pragma once

#include <algorithm>
#include <initializer_list>

#include "amp_trials.h"
#include "amp_vamp.h"

namespace amp {

// GEMM2 of both engines (vamp_k2, tvamp_k2): a reduction over more than one 512-float chunk (k > 256,
// launch-engine shapes only) is summed per chunk (amp_gemm.h gemm_tile SEG)
constexpr int VAMP_SEG2 = 1;

// ---- record guards: AllRows / LiveRows (amp_trials.h) that also hand out row rho's scalars ----
// (PSCR is theirs, kept for the interface: VAMP's epilogues stage nothing past the C tile.)
// The batch engine: the one record of iteration t, by value, for every row.  live() is a constant
// (the test folds away) and the scalars stay wave-uniform.
struct VampAllRows {
    static constexpr int PSCR = AllRows::PSCR;
    VampIter it;
    __device__ __forceinline__ bool live(int) const { return true; }
    __device__ __forceinline__ const VampIter& rec(int) const { return it; }
};
// The trial engine: the tile's records in LDS (vamp_tile_records); a stopped row is never stored to.
struct VampLiveRows {
    static constexpr int PSCR = LiveRows::PSCR;
    const VampIter* s_it;   // LDS [GBM]
    __device__ __forceinline__ bool live(int rho) const { return !s_it[rho].stopped; }
    __device__ __forceinline__ const VampIter& rec(int rho) const { return s_it[rho]; }
};

// tile_rows_live (amp_trials.h) that stages the rows' whole records: the tile's records into LDS, a
// row past the last as stopped; false (workgroup-uniform) when none of its rows is live
__device__ __forceinline__ bool vamp_tile_records(const VampIter* recs, int row0, int rows, VampIter* s_it) {
    if (threadIdx.x < GBM) {
        const int row = row0 + threadIdx.x;
        VampIter it = recs[min(row, rows - 1)];
        if (row >= rows) it.stopped = 1;
        s_it[threadIdx.x] = it;
    }
    __syncthreads();
    int live = 0;
#pragma unroll
    for (int i = 0; i < GBM; ++i) live |= s_it[i].stopped ^ 1;
    return live != 0;
}

// r~ = (xmmse - dxdr * r) * normScalar (vamp.py:85-91) with the row's dxdr and normScalar, formed
// while loading GEMM1's A tile.  Staged in two steps like ALoadPlain (amp_gemm.h): both loads at a
// clamped address, the formula and the zeroing of out-of-range elements at the LDS store.
template <class G>
struct ALoadRt {
    const float* __restrict__ xm;
    const float* __restrict__ r;
    int lda, rows, ka, row0;
    G g;
    struct Raw {
        float4 x, q;
    };
    __device__ __forceinline__ Raw raw(int row, int k) const {
        const size_t o = (size_t)min(row, rows - 1) * lda + min(k, ka - 4);
        return Raw{*reinterpret_cast<const float4*>(xm + o), *reinterpret_cast<const float4*>(r + o)};
    }
    __device__ __forceinline__ float4 fin(const Raw& v, int row, int k) const {
        const bool ok = row < rows && k < ka;
        const float dxdr = g.rec(row - row0).dxdr_prev, ns = g.rec(row - row0).ns_prev;
        const float4 x = v.x, q = v.q;
        const float4 f = make_float4((x.x - dxdr * q.x) * ns, (x.y - dxdr * q.y) * ns, (x.z - dxdr * q.z) * ns,
                                     (x.w - dxdr * q.w) * ns);
        return ok ? f : make_float4(0.f, 0.f, 0.f, 0.f);
    }
};
template <class G>
__device__ __forceinline__ ALoadRt<G> vamp_aload_rt(const VampK& P, const G& g, int row0) {
    return ALoadRt<G>{P.xm, P.r, 2 * P.N, P.B, 2 * P.N, row0, g};
}

// ---- the GEMM epilogues: `lds` holds the C tile (row stride GemmCfg<BN>::LDC), g the record guard ----

// GEMM1: w = scale * (y~ + vr * q) - q   (vamp.py:68-72; `x_tilde - q` is what V @ consumes).  Every
// load of this thread's elements first, unconditional at a clamped index (the w stores may alias
// them as far as the compiler knows, and a branch around a load serialises the loads' latencies:
// amp_gemm.h ALoadPlain); out-of-range elements are never stored
template <class G>
__device__ __forceinline__ void vamp_lmmse_epilogue(const VampK& P, const G& g, const float* lds, int row0, int col0) {
    using C = GemmCfg<128>;
    const int twok = 2 * P.k;
    constexpr int IT = GBM * 128 / AMP_WG;
    float yv[IT], s2v[IT];
#pragma unroll
    for (int u = 0; u < IT; ++u) {
        const int e = threadIdx.x + u * AMP_WG;
        const int row = min(row0 + (e >> 7), P.B - 1), col = min(col0 + (e & 127), twok - 1);
        yv[u] = P.ytil[(size_t)row * twok + col];
        s2v[u] = P.s2[col >> 1];
    }
#pragma unroll
    for (int u = 0; u < IT; ++u) {
        const int e = threadIdx.x + u * AMP_WG;
        const int rho = e >> 7, cc = e & 127;
        const int row = row0 + rho, col = col0 + cc;
        if (row < P.B && col < twok && g.live(rho)) {
            const float vr = g.rec(rho).vr;
            const float q = lds[rho * C::LDC + cc];
            const float sc = 1.0f / (s2v[u] + vr);
            P.w[(size_t)row * P.wld + col] = sc * (yv[u] + vr * q) - q;
        }
    }
}

// GEMM2: x~ = V w + r~ ; r = (x~ - alpha r~) / (1 - alpha)   (vamp.py:72, 79), stored and left in the
// C tile for the denoiser.  The loads first, as in vamp_lmmse_epilogue.  Ends with a barrier.
template <int BN, class G>
__device__ __forceinline__ void vamp_r_epilogue(const VampK& P, const G& g, float* lds, int row0, int col0, int nrows,
                                                int ncols) {
    using C = GemmCfg<BN>;
    const int twoN = 2 * P.N;
    constexpr int IT = GBM * BN / AMP_WG;
    float xv[IT], rv[IT];
#pragma unroll
    for (int u = 0; u < IT; ++u) {
        const int e = threadIdx.x + u * AMP_WG;
        const size_t o = (size_t)(row0 + min(e / BN, nrows - 1)) * twoN + col0 + min(e % BN, ncols - 1);
        xv[u] = P.xm[o];
        rv[u] = P.r[o];
    }
#pragma unroll
    for (int u = 0; u < IT; ++u) {
        const int e = threadIdx.x + u * AMP_WG;
        const int rho = e / BN, cc = e % BN;
        if (rho < nrows && cc < ncols && g.live(rho)) {
            const VampIter& it = g.rec(rho);
            const size_t o = (size_t)(row0 + rho) * twoN + col0 + cc;
            const float rt = (xv[u] - it.dxdr_prev * rv[u]) * it.ns_prev;
            const float xt = lds[rho * C::LDC + cc] + rt;
            const float rn = (xt - it.alpha * rt) * it.inv1ma;
            P.r[o] = rn;
            lds[rho * C::LDC + cc] = rn;
        }
    }
    __syncthreads();
}

struct VampDenoisePolicy {
    const float* tile;
    int ldc, spr, M, N, L, row0, colc0;
    float inv_sigma2;
    float* xm;
    float* var_new;
    const float* var_prev;
    float* secmax;
    float* secabs;
    __device__ __forceinline__ void load(int sec, int m, float& rr, float& ri, float& it) const {
        const int rho = sec / spr, sj = sec - rho * spr;
        const float2 v = *reinterpret_cast<const float2*>(tile + rho * ldc + 2 * (sj * M + m));
        rr = v.x; ri = v.y; it = inv_sigma2;
    }
    __device__ __forceinline__ void store(int sec, int m, float xr, float xi, float var, PartAcc& pa) const {
        const int rho = sec / spr, sj = sec - rho * spr;
        const size_t o = (size_t)(row0 + rho) * N + colc0 + sj * M + m;
        *reinterpret_cast<float2*>(xm + 2 * o) = make_float2(xr, xi);
        var_new[o] = var;
        pa.sumvar += (double)var;
        pa.notclose += torch_close(var, var_prev[o]) ? 0u : 1u;     // vamp.py:185
    }
    __device__ __forceinline__ void section(int sec, float smax, float sabs) const {
        const int rho = sec / spr, sj = sec - rho * spr;
        const size_t o = (size_t)(row0 + rho) * L + (colc0 / M) + sj;
        secmax[o] = smax;
        secabs[o] = sabs;
    }
};

// The denoiser's view of the tile rows from rho on (vamp_r_epilogue's C tile), with row rho's
// 1 / sigma2 (vamp.py:84, 111): the whole tile at rho = 0 (the batch engine: nrows * spr sections),
// one row when only spr sections are denoised (the trial engine: sec / spr is then 0 and every
// address the same integer as the B = 1 forward's, whose tile has that one row)
template <int BN, class G>
__device__ __forceinline__ VampDenoisePolicy vamp_policy(const VampK& P, const G& g, int t, const float* lds, int row0,
                                                         int col0, int ncols, int rho) {
    using C = GemmCfg<BN>;
    VampDenoisePolicy pol;
    pol.tile = lds + rho * C::LDC; pol.ldc = C::LDC; pol.M = P.M; pol.N = P.N; pol.L = P.L;
    pol.spr = (ncols / 2) / P.M; pol.row0 = row0 + rho; pol.colc0 = col0 / 2;
    pol.inv_sigma2 = g.rec(rho).inv_sigma2;
    pol.xm = P.xm; pol.var_new = var_buf(P, t); pol.var_prev = var_buf(P, t + 1);
    pol.secmax = P.secmax; pol.secabs = P.secabs;
    return pol;
}

// Tracker (vamp.py:22-26) of every row in the form the fused kernels consume, a grid-stride body
// (the engines' init kernels add their records):
//   xmmse = p, r = 0 so that r~ = (xmmse - 0*r)*1 = p   (vamp.py:25)
//   var buffer 1 = ones: the `prev` of iteration 0      (vamp.py:24, 182)
__device__ __forceinline__ void vamp_init_state(const VampK& P) {
    const float p = (float)P.sparsity;
    const size_t BN_ = (size_t)P.B * P.N;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < BN_; e += (size_t)gridDim.x * blockDim.x) {
        reinterpret_cast<float2*>(P.xm)[e] = make_float2(p, 0.f);
        reinterpret_cast<float2*>(P.r)[e] = make_float2(0.f, 0.f);
        P.var1[e] = 1.0f;
        if (e < (size_t)P.B)   // the pad of w's rows (vamp_wld), zeroed once: GEMM1's epilogue stores columns < 2k only
            for (int j = 2 * P.k; j < P.wld; ++j) P.w[e * P.wld + j] = 0.f;
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < P.k; i += gridDim.x * blockDim.x) P.s2[i] = P.s[i] * P.s[i];
}

// ---- the reduction step after GEMM2 (one workgroup per batch, or per trial) ----

// One section for the exact float64 fix-up (section_absmax_f64 / exact_section_f64), o0 its first
// position in [B][N]: the loader (r and the record's 1 / sigma2) and the store (xmmse, var, and the
// recomputed value's deltas against the fast path's: var into *dsum, allclose into *dnc)
struct VampSectionLoad {
    const float2* r2;
    float inv;
    __device__ __forceinline__ void operator()(int m, float& rr, float& ri, float& it) const {
        const float2 v = r2[m];
        rr = v.x; ri = v.y; it = inv;
    }
};
struct VampSectionStore {
    float2* x2;
    float* vn;
    const float* vp;
    double* dsum;
    int* dnc;
    __device__ __forceinline__ void operator()(int m, float xr, float xi, float var) const {
        const float old = vn[m];
        *dsum += (double)var - (double)old;
        *dnc += (torch_close(var, vp[m]) ? 0 : 1) - (torch_close(old, vp[m]) ? 0 : 1);
        x2[m] = make_float2(xr, xi);
        vn[m] = var;
    }
};
__device__ __forceinline__ VampSectionLoad vamp_section_load(const VampK& P, const VampIter& cur, size_t o0) {
    return VampSectionLoad{reinterpret_cast<const float2*>(P.r) + o0, cur.inv_sigma2};
}
__device__ __forceinline__ VampSectionStore vamp_section_store(const VampK& P, int t, size_t o0, double* dsum, int* dnc) {
    return VampSectionStore{reinterpret_cast<float2*>(P.xm) + o0, var_buf(P, t) + o0, var_buf(P, t + 1) + o0, dsum, dnc};
}

// The reference's G is NaN / inf: every section of this iteration is NaN (`rows` rows).  Returns `fixed`.
__device__ __forceinline__ int vamp_allnan(const VampK& P, const VampIter& cur, PartAcc& pa, int t, int rows) {
    if (!cur.fixed_all) nan_fill(P.xm, var_buf(P, t), (size_t)rows * P.N);
    pa.sumvar = __longlong_as_double(0x7ff8000000000000LL);
    pa.notclose = 1;
    return -1;
}

// Exact float64 G, then exact float64 recompute of every one of the `nsec` sections below the
// danger line (rare); the recomputed values replace the fast-path ones in the reductions:
// (sum - old) + new, in float64.  Called by every thread of the workgroup; returns `fixed`.
__device__ __forceinline__ int vamp_fixup(const VampK& P, const VampIter& cur, PartAcc& pa, const Const64& c64, int t,
                                          int nsec) {
    __shared__ double s_fix[RWG / 64];
    __shared__ int s_nc[RWG / 64];
    double dsum = 0.0, G;
    int dnc = 0;
    const auto ldf = [&](int s) { return vamp_section_load(P, cur, (size_t)s * P.M); };
    const auto stf = [&](int s) { return vamp_section_store(P, t, (size_t)s * P.M, &dsum, &dnc); };
    const int fixed = fixup_sections<true>(nsec, P.M, P.secmax, P.secabs, pa.maxabs, c64, ldf, stf, &G, s_fix);
    pa.maxabs = G;
    pa.sumvar += block_sum(dsum, s_fix);
    pa.notclose += (unsigned)block_sum(dnc, s_nc);
    return fixed;
}

// The record that drives the next iteration into *slot; the status when the loop ends here
__device__ __forceinline__ void vamp_commit(const VampK& P, VampIter* slot, amp_status* status_slot, const VampIter& cur,
                                            const VampIter& nx, int fixed, int t) {
    if (threadIdx.x == 0) {
        *slot = nx;
        if (nx.stopped || t + 1 == P.max_iter) *status_slot = vamp_make_status(P, cur, nx, fixed);
    }
}

// vamp_r / tvamp_r past their entry guards, on the P.B rows of P: partial reduction, all-NaN rule or
// exact float64 fix-up of out-of-range sections, allclose decision and the scalars of the next
// iteration (vamp.py:85-94, 66-82) or the stop record (vamp.py:185-186).  Returns the next record.
__device__ __forceinline__ VampIter vamp_reduce(const VampK& P, const Const64& c64, const VampIter& cur,
                                                const Partial* parts, int nparts, VampIter* slot, amp_status* status_slot,
                                                int t, float* lds) {
    PartAcc pa = part_reduce_all(parts, nparts, lds);
    int fixed = 0;
    if (part_allnan(pa))
        fixed = vamp_allnan(P, cur, pa, t, P.B);
    else if (part_danger(pa))
        fixed = vamp_fixup(P, cur, pa, c64, t, P.B * P.L);
    const VampIter nx = vamp_advance(P, cur, pa, fixed, t, lds);
    vamp_commit(P, slot, status_slot, cur, nx, fixed, t);
    return nx;
}

// ---- host side ----

// The f32 operators, MFMA-packed (Tracker, vamp.py:17-22)
inline int vamp_pack_f32(const VampK& P, const amp_vamp_args* a, hipStream_t st) {
    int rc;
    // Wt0: y~ = (s * U^H) y        (vamp.py:22)    X[o][j] = s_o conj(U[j][o]),  o < k, j < n
    if ((rc = build_cweight((const float2*)a->U, 1, P.k, 1, P.s, P.k, P.n, (float*)P.Wt0, P.kap0, P.ncp0, st))) return rc;
    // Wt1: q = Vh r~               (vamp.py:67)    X[o][j] = Vh[o][j],           o < k, j < N
    if ((rc = build_cweight((const float2*)a->Vh, P.N, 1, 0, nullptr, P.k, P.N, (float*)P.Wt1, P.kap1, P.ncp1, st))) return rc;
    // Wt2: V (x~ - q), V = Vh^H    (vamp.py:19,72) X[o][j] = conj(Vh[j][o]),     o < N, j < k
    return build_cweight((const float2*)a->Vh, 1, P.N, 1, nullptr, P.N, P.k, (float*)P.Wt2, P.kap2, P.ncp2, st);
}

// GEMM2 + denoiser of either engine, instantiated per column-tile width and constellation size (K
// is validated by check_dims).  K2: a struct whose K2::fn<BN, KK>() is the kernel's address;
// args: the kernel's arguments after P.
template <class K2>
inline int vamp_k2_attrs() {
    int rc = 0;
    for (int K : {1, 2, 4, 8, 16, 64})
        dispatch_K(K, [&](auto kk) {
            constexpr int KK = decltype(kk)::value;
            if (!rc) rc = set_lds_attr<128>((const void*)K2::template fn<128, KK>());
            if (!rc) rc = set_lds_attr<256>((const void*)K2::template fn<256, KK>());
        });
    return rc;
}
template <class K2, class... A>
inline void vamp_k2_launch(const VampK& P, hipStream_t st, A... args) {
    const dim3 g2(cdiv(P.B, GBM), P.ncp2 / P.bn2);
    dispatch_K(P.c.K, [&](auto kk) {
        constexpr int KK = decltype(kk)::value;
        if (P.bn2 == 128)
            hipLaunchKernelGGL((K2::template fn<128, KK>()), g2, dim3(AMP_WG), GemmCfg<128>::LDS_BYTES, st, P, args...);
        else
            hipLaunchKernelGGL((K2::template fn<256, KK>()), g2, dim3(AMP_WG), GemmCfg<256>::LDS_BYTES, st, P, args...);
    });
}

}  // namespace amp

// amp_vamp_trials.hip — VAMP over E independent single-trial detections that share one channel
// (amp_vamp_trials_run): the iteration kernels of the launch engine (amp_vamp.hip) with per-row
// records.
//
// Restates, for every trial e alone, VAMP.forward at B = 1 (vamp.py:159-187): Tracker
// (vamp.py:12-28), T_e x VAMPLayer.forward (vamp.py:56-94) and the allclose early exit
// (vamp.py:185) on the trial's own var — the way the reference's drivers run it (batch = 1,
// res epochs per channel: vamp_model.py:91, 98).
//
// Per iteration t, three launches on one stream, no host synchronisation:
//   tvamp_k1  GEMM1 over row tiles of 32 trials; row e's r~ = (xmmse - dxdr_e r) ns_e formed in the
//             A-operand prologue (vamp.py:89-91, 67), LMMSE epilogue with the row's var_ratio
//             (vamp.py:68-72).
//   tvamp_k2  GEMM2, epilogue with the row's alpha (vamp.py:72-79), then the section denoiser row
//             by row with the row's 1 / sigma2 (vamp.py:84, 96-119): one partial per (tile, row).
//   tvamp_r   a grid over the trials: workgroup e reduces trial e's partials (sum var over its N
//             values, its own max|xi|, its own allclose count), recomputes in exact float64 the
//             sections that leave the normal range against the trial's own shift (fixup_sections),
//             and forms the trial's next record (vamp_advance) or its stop record.
// A stopped trial's rows are frozen: no kernel stores to them again.  A tile whose rows have all
// stopped returns at once, and every kernel returns at once when the stop counter has reached E.
// A row's GEMM result does not depend on the other rows of its tile (each MFMA output row reduces
// its own A row only), so a trial's values are those of its own B = 1 forward on the launch engine.
#include <algorithm>
#include <mutex>

#include "amp_trials.h"
#include "amp_vamp.h"

namespace amp {

struct TVampWs {
    float *Wt0, *Wt1, *Wt2, *s2, *ytil, *w, *var1, *secmax, *secabs;
    Partial* parts;     // [E][nct]: trial e's partial of column tile slot j (rewritten every iteration)
    VampIter* iters;    // [E]: trial e's record, advanced in place by tvamp_r
    unsigned* nstop;    // trials whose allclose exit has fired
    void* dec;          // per-trial decision workspace
    size_t bytes;
};

static TVampWs tvamp_carve(const amp_dims* d, int k, int E, void* base) {
    VampK P;
    vamp_geometry(d, k, P);
    Carve cv(base);
    TVampWs w;
    w.Wt0 = cv.take<float>((size_t)P.ncp0 * P.kap0);
    w.Wt1 = cv.take<float>((size_t)P.ncp1 * P.kap1);
    w.Wt2 = cv.take<float>((size_t)P.ncp2 * P.kap2);
    w.s2 = cv.take<float>((size_t)k);
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

// Tracker (vamp.py:22-26) for every trial, and every trial's iteration-0 record (the same: it
// depends on the channel and the SNR only).
__global__ __launch_bounds__(256) void tvamp_init_kernel(VampK P, unsigned* nstop) {
    __shared__ __attribute__((aligned(16))) float lds[64];
    const float p = (float)P.sparsity;
    const size_t EN = (size_t)P.B * P.N;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < EN; e += (size_t)gridDim.x * blockDim.x) {
        reinterpret_cast<float2*>(P.xm)[e] = make_float2(p, 0.f);
        reinterpret_cast<float2*>(P.r)[e] = make_float2(0.f, 0.f);
        P.var1[e] = 1.0f;
        if (e < (size_t)P.B)   // the pad of w's rows (vamp_wld), zeroed once: tvamp_k1 stores columns < 2k only
            for (int j = 2 * P.k; j < P.wld; ++j) P.w[e * P.wld + j] = 0.f;
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < P.k; i += gridDim.x * blockDim.x) P.s2[i] = P.s[i] * P.s[i];
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) *nstop = 0u;
        const VampIter it = vamp_first_iter(P, lds);
        for (int e = threadIdx.x; e < P.B; e += blockDim.x) P.iters[e] = it;
    }
}

// ALoadRt (amp_vamp.hip) with the row's own dxdr and normScalar (vamp.py:85-91), read from the
// tile's records in LDS.
struct ALoadRtRows {
    const float* __restrict__ xm;
    const float* __restrict__ r;
    int lda, rows, ka, row0;
    const VampIter* rec;   // LDS [GBM]
    struct Raw {
        float4 x, q;
    };
    __device__ __forceinline__ Raw raw(int row, int k) const {
        const size_t o = (size_t)min(row, rows - 1) * lda + min(k, ka - 4);
        return Raw{*reinterpret_cast<const float4*>(xm + o), *reinterpret_cast<const float4*>(r + o)};
    }
    __device__ __forceinline__ float4 fin(const Raw& v, int row, int k) const {
        const bool ok = row < rows && k < ka;
        const float dxdr = rec[row - row0].dxdr_prev, ns = rec[row - row0].ns_prev;
        const float4 x = v.x, q = v.q;
        const float4 f = make_float4((x.x - dxdr * q.x) * ns, (x.y - dxdr * q.y) * ns, (x.z - dxdr * q.z) * ns,
                                     (x.w - dxdr * q.w) * ns);
        return ok ? f : make_float4(0.f, 0.f, 0.f, 0.f);
    }
};

// the tile's records into LDS; false (workgroup-uniform) when none of its rows is live
__device__ __forceinline__ bool tvamp_tile_records(const VampK& P, int row0, VampIter* s_it) {
    if (threadIdx.x < GBM) {
        const int row = row0 + threadIdx.x;
        VampIter it = P.iters[min(row, P.B - 1)];
        if (row >= P.B) it.stopped = 1;
        s_it[threadIdx.x] = it;
    }
    __syncthreads();
    int live = 0;
#pragma unroll
    for (int i = 0; i < GBM; ++i) live |= s_it[i].stopped ^ 1;
    return live != 0;
}

__global__ __launch_bounds__(AMP_WG) void tvamp_k1(VampK P, const unsigned* nstop) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ VampIter s_it[GBM];
    if (*nstop >= (unsigned)P.B) return;
    const GemmTile tile = xcd_tile();
    const int row0 = tile.rb * GBM, col0 = tile.cb * 128;
    if (!tvamp_tile_records(P, row0, s_it)) return;
    const int twoN = 2 * P.N, twok = 2 * P.k;
    gemm_tile<128>(ALoadRtRows{P.xm, P.r, twoN, P.B, twoN, row0, s_it}, P.Wt1, P.kap1, row0, col0, lds);
    using C = GemmCfg<128>;
    // w = scale * (y~ + vr_e * q) - q   (vamp.py:68-72), as vamp_k1 with the row's var_ratio
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
        if (row < P.B && col < twok && !s_it[rho].stopped) {
            const float vr = s_it[rho].vr;
            const float q = lds[rho * C::LDC + cc];
            const float sc = 1.0f / (s2v[u] + vr);
            P.w[(size_t)row * P.wld + col] = sc * (yv[u] + vr * q) - q;
        }
    }
}

// One row of the tile for the section denoiser (VampDenoisePolicy of amp_vamp.hip at B = 1: the
// section index is the section's position in the row's part of the tile).
struct TVampDenoisePolicy {
    const float* tile;    // the row's C-tile row
    int M;
    size_t o0;            // row * N + first position of the tile
    size_t s0;            // row * L + first section of the tile
    float inv_sigma2;
    float* xm;
    float* var_new;
    const float* var_prev;
    float* secmax;
    float* secabs;
    __device__ __forceinline__ void load(int sec, int m, float& rr, float& ri, float& it) const {
        const float2 v = *reinterpret_cast<const float2*>(tile + 2 * (sec * M + m));
        rr = v.x; ri = v.y; it = inv_sigma2;
    }
    __device__ __forceinline__ void store(int sec, int m, float xr, float xi, float var, PartAcc& pa) const {
        const size_t o = o0 + sec * M + m;
        *reinterpret_cast<float2*>(xm + 2 * o) = make_float2(xr, xi);
        var_new[o] = var;
        pa.sumvar += (double)var;
        pa.notclose += torch_close(var, var_prev[o]) ? 0u : 1u;     // vamp.py:185
    }
    __device__ __forceinline__ void section(int sec, float smax, float sabs) const {
        secmax[s0 + sec] = smax;
        secabs[s0 + sec] = sabs;
    }
};

template <int BN, int KK>
__global__ __launch_bounds__(AMP_WG) void tvamp_k2(VampK P, int t, const unsigned* nstop) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ VampIter s_it[GBM];
    if (*nstop >= (unsigned)P.B) return;
    using C = GemmCfg<BN>;
    const GemmTile tile = xcd_tile();
    const int row0 = tile.rb * GBM, col0 = tile.cb * BN;
    if (!tvamp_tile_records(P, row0, s_it)) return;
    const int twoN = 2 * P.N;
    gemm_tile<BN>(ALoadPlain{P.w, P.wld, P.B, P.wld}, P.Wt2, P.kap2, row0, col0, lds);
    // x~ = V w + r~ ; r = (x~ - alpha_e r~) / (1 - alpha_e)   (vamp.py:72, 79)
    const int nrows = min(GBM, P.B - row0), ncols = min(BN, twoN - col0);
    {
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
            if (rho < nrows && cc < ncols && !s_it[rho].stopped) {
                const size_t o = (size_t)(row0 + rho) * twoN + col0 + cc;
                const float rt = (xv[u] - s_it[rho].dxdr_prev * rv[u]) * s_it[rho].ns_prev;
                const float xt = lds[rho * C::LDC + cc] + rt;
                const float rn = (xt - s_it[rho].alpha * rt) * s_it[rho].inv1ma;
                P.r[o] = rn;
                lds[rho * C::LDC + cc] = rn;
            }
        }
    }
    __syncthreads();
    // the denoiser row by row: the row's own 1 / sigma2, and the row's own partial in the slot its
    // B = 1 forward stores it to (s_it is workgroup-uniform: no divergent barrier)
    const int nct = P.ncp2 / BN, slot = seq_part_slot(tile.cb, nct), spr = (ncols / 2) / P.M;
    for (int rho = 0; rho < nrows; ++rho) {
        if (s_it[rho].stopped) continue;
        const int row = row0 + rho;
        TVampDenoisePolicy pol;
        pol.tile = lds + rho * C::LDC; pol.M = P.M;
        pol.o0 = (size_t)row * P.N + col0 / 2;
        pol.s0 = (size_t)row * P.L + (col0 / 2) / P.M;
        pol.inv_sigma2 = s_it[rho].inv_sigma2;
        pol.xm = P.xm;
        pol.var_new = var_buf(P, t);
        pol.var_prev = var_buf(P, t + 1);
        pol.secmax = P.secmax;
        pol.secabs = P.secabs;
        PartAcc pa;
        denoise_sections<true, KK>(pol, spr, P.M, P.c, pa);
        part_block_store(pa, P.parts + (size_t)row * nct + slot, lds + C::CTILE_FLOATS);
    }
}

// Workgroup e after K2(t): trial e's partial reduction, exact float64 fix-up against the trial's
// own max|xi|, allclose decision and the trial's scalars of iteration t+1 (vamp_r of amp_vamp.hip
// on the trial's rows; every trial in parallel).
__global__ __launch_bounds__(RWG) void tvamp_r(VampK PE, Const64 c64, int t, unsigned* nstop) {
    __shared__ __attribute__((aligned(16))) float lds[512];
    __shared__ double s_fix[RWG / 64];
    __shared__ unsigned s_nc[RWG / 64];
    if (*nstop >= (unsigned)PE.B) return;
    const int e = blockIdx.x;
    const VampIter cur = PE.iters[e];
    if (cur.stopped) return;
    // the trial as a batch of one
    VampK P = PE;
    const int nct = PE.ncp2 / PE.bn2;
    P.B = 1; P.Bmean = 1;
    P.r = PE.r + (size_t)e * 2 * PE.N; P.xm = PE.xm + (size_t)e * 2 * PE.N;
    P.var0 = PE.var0 + (size_t)e * PE.N; P.var1 = PE.var1 + (size_t)e * PE.N;
    P.secmax = PE.secmax + (size_t)e * PE.L; P.secabs = PE.secabs + (size_t)e * PE.L;
    P.parts = PE.parts + (size_t)e * nct;
    PartAcc pa = part_reduce_all(P.parts, nct, lds);
    int fixed = 0;
    if (part_allnan(pa)) {
        // the reference's G is NaN / inf: every section of this trial's iteration is NaN
        if (!cur.fixed_all) nan_fill(P.xm, var_buf(P, t), (size_t)P.N);
        pa.sumvar = __longlong_as_double(0x7ff8000000000000LL);
        pa.notclose = 1;
        fixed = -1;
    } else if (part_danger(pa)) {
        float* vn = var_buf(P, t);
        const float* vp = var_buf(P, t + 1);
        const float inv = cur.inv_sigma2;
        const float2* r2 = reinterpret_cast<const float2*>(P.r);
        float2* x2 = reinterpret_cast<float2*>(P.xm);
        const int M = P.M;
        double dsum = 0.0;
        int dnc = 0;
        auto ldf = [=](int s) {
            const size_t o0 = (size_t)s * M;
            return [=](int m, float& rr, float& ri, float& it) {
                const float2 v = r2[o0 + m];
                rr = v.x; ri = v.y; it = inv;
            };
        };
        auto stf = [&](int s) {
            const size_t o0 = (size_t)s * M;
            return [&, o0](int m, float xr, float xi, float var) {
                const size_t o = o0 + m;
                const float old = vn[o];
                dsum += (double)var - (double)old;
                dnc += (torch_close(var, vp[o]) ? 0 : 1) - (torch_close(old, vp[o]) ? 0 : 1);
                x2[o] = make_float2(xr, xi);
                vn[o] = var;
            };
        };
        double G;
        fixed = fixup_sections<true>(P.L, P.M, P.secmax, P.secabs, pa.maxabs, c64, ldf, stf, &G, s_fix);
        pa.maxabs = G;
        dsum = group_sum(dsum, 64);
        dnc = group_sum(dnc, 64);
        if ((threadIdx.x & 63) == 0) {
            s_fix[threadIdx.x >> 6] = dsum;
            s_nc[threadIdx.x >> 6] = (unsigned)dnc;
        }
        __syncthreads();
        double d = 0.0;
        unsigned nc = 0;
        for (int w = 0; w < RWG / 64; ++w) { d += s_fix[w]; nc += s_nc[w]; }
        pa.sumvar += d;
        pa.notclose += nc;
        __syncthreads();
    }
    const VampIter nx = vamp_advance(P, cur, pa, fixed, t, lds);
    if (threadIdx.x == 0) {
        PE.iters[e] = nx;
        if (nx.stopped || t + 1 == P.max_iter) PE.status[e] = vamp_make_status(P, cur, nx, fixed);
        if (nx.stopped) __hip_atomic_fetch_add(nstop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
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

template <int KK>
static int tvamp_k2_attrs() {
    int rc = set_lds_attr<128>((const void*)tvamp_k2<128, KK>);
    return rc ? rc : set_lds_attr<256>((const void*)tvamp_k2<256, KK>);
}

static int tvamp_attrs() {
    std::call_once(g_tvamp_attr_once, [] {
        int rc = set_lds_attr<128>((const void*)tvamp_k1);
        if (!rc) rc = tvamp_k2_attrs<1>();
        if (!rc) rc = tvamp_k2_attrs<2>();
        if (!rc) rc = tvamp_k2_attrs<4>();
        if (!rc) rc = tvamp_k2_attrs<8>();
        if (!rc) rc = tvamp_k2_attrs<16>();
        if (!rc) rc = tvamp_k2_attrs<64>();
        g_tvamp_attr_rc = rc;
    });
    return g_tvamp_attr_rc;
}

template <int KK>
static void tvamp_launch_k2_kk(const VampK& P, int t, const unsigned* nstop, hipStream_t st) {
    dim3 g2(cdiv(P.B, GBM), P.ncp2 / P.bn2);
    if (P.bn2 == 128)
        hipLaunchKernelGGL((tvamp_k2<128, KK>), g2, dim3(AMP_WG), GemmCfg<128>::LDS_BYTES, st, P, t, nstop);
    else
        hipLaunchKernelGGL((tvamp_k2<256, KK>), g2, dim3(AMP_WG), GemmCfg<256>::LDS_BYTES, st, P, t, nstop);
}

static void tvamp_launch_k2(const VampK& P, int t, const unsigned* nstop, hipStream_t st) {
    switch (P.c.K) {
    case 1: tvamp_launch_k2_kk<1>(P, t, nstop, st); break;
    case 2: tvamp_launch_k2_kk<2>(P, t, nstop, st); break;
    case 4: tvamp_launch_k2_kk<4>(P, t, nstop, st); break;
    case 8: tvamp_launch_k2_kk<8>(P, t, nstop, st); break;
    case 16: tvamp_launch_k2_kk<16>(P, t, nstop, st); break;
    default: tvamp_launch_k2_kk<64>(P, t, nstop, st); break;
    }
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
    int rc = check_dims(d, c, true, true);   // any n, any k, any even N, a partial last column tile (amp_vamp_run)
    if (rc) return rc;
    AMP_REQUIRE(d->B == 1, "amp_vamp_trials_run: dims describe ONE trial (B = %d, must be 1)", d->B);
    AMP_REQUIRE(trials >= 1, "amp_vamp_trials_run: trials = %d", trials);
    AMP_REQUIRE(vamp_index_ok(d, trials), "amp_vamp_trials_run: %d trials of max(2N, 2n) = %d columns need more "
                "than 32-bit offsets (or more than 65535 column tiles)", trials, 2 * std::max(d->N, d->n));
    AMP_REQUIRE(a && a->U && a->s && a->Vh && a->y && a->r && a->xmmse && a->var && a->status && a->ws,
                "amp_vamp_trials_run: null pointer argument");
    AMP_REQUIRE(a->k > 0 && a->k <= d->N && a->k <= d->n, "amp_vamp_trials_run: k = %d must be min(n, N)", a->k);
    AMP_REQUIRE(a->max_iter > 0, "amp_vamp_trials_run: max_iter must be positive");
    AMP_REQUIRE(a->engine == AMP_ENGINE_AUTO || a->engine == AMP_ENGINE_LAUNCHES,
                "amp_vamp_trials_run: the persistent engine has no independent-trial form");
    AMP_REQUIRE(a->gemm == AMP_GEMM_AUTO || a->gemm == AMP_GEMM_F32, "amp_vamp_trials_run: f32 GEMMs only (gemm %d)",
                a->gemm);
    const int E = trials;
    const TVampWs w = tvamp_carve(d, a->k, E, a->ws);
    AMP_REQUIRE(a->ws_bytes >= w.bytes, "amp_vamp_trials_run: workspace %zu < %zu bytes", a->ws_bytes, w.bytes);
    TrialsDecide td{};
    if (dec && (rc = trials_decide_args(d, dec, a->r, a->xmmse, td))) return rc;
    VampK P{};
    vamp_geometry(d, a->k, P);
    P.B = E;            // rows; every per-trial quantity is formed over one row (tvamp_r: Bmean = 1)
    P.Bmean = 1;
    P.max_iter = a->max_iter;
    P.noise_var = a->noise_var;
    P.sparsity = a->sparsity;
    P.Wt0 = w.Wt0; P.Wt1 = w.Wt1; P.Wt2 = w.Wt2;
    P.s = (const float*)a->s; P.s2 = w.s2; P.ytil = w.ytil; P.w = w.w;
    P.r = (float*)a->r; P.xm = (float*)a->xmmse;
    P.var0 = (float*)a->var; P.var1 = w.var1;
    P.secmax = w.secmax; P.secabs = w.secabs; P.parts = w.parts; P.iters = w.iters;
    P.status = (amp_status*)a->status;
    P.y = (const float*)a->y;
    P.x3 = 0;           // amp_status.gemm = AMP_ARITH_F32
    P.c = to_const(c);
    const Const64 c64 = to_const64(c);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = tvamp_attrs())) return rc;
    // the operators, packed once per call (vamp_prepare_impl)
    //   y~ = (s U^H) y   (vamp.py:22)    X[o][j] = s_o conj(U[j][o]),  o < k, j < n
    rc = build_cweight((const float2*)a->U, 1, P.k, 1, P.s, P.k, P.n, (float*)P.Wt0, P.kap0, P.ncp0, st);
    if (rc) return rc;
    //   q = Vh r~        (vamp.py:67)    X[o][j] = Vh[o][j],           o < k, j < N
    rc = build_cweight((const float2*)a->Vh, P.N, 1, 0, nullptr, P.k, P.N, (float*)P.Wt1, P.kap1, P.ncp1, st);
    if (rc) return rc;
    //   V (x~ - q)       (vamp.py:19,72) X[o][j] = conj(Vh[j][o]),     o < N, j < k
    rc = build_cweight((const float2*)a->Vh, 1, P.N, 1, nullptr, P.N, P.k, (float*)P.Wt2, P.kap2, P.ncp2, st);
    if (rc) return rc;
    const int g = (int)std::min<size_t>(((size_t)E * P.N + 255) / 256, 2048);
    hipLaunchKernelGGL(tvamp_init_kernel, dim3(g), dim3(256), 0, st, P, w.nstop);
    AMP_LAUNCH_CHECK("tvamp_init");
    rc = gemm_store((const float*)a->y, 2 * P.n, E, 2 * P.n, P.Wt0, P.kap0, P.ncp0, P.ytil, 2 * P.k, 2 * P.k, st);
    if (rc) return rc;
    const dim3 g1(cdiv(E, GBM), P.ncp1 / 128);
    for (int t = 0; t < P.max_iter; ++t) {
        hipLaunchKernelGGL(tvamp_k1, g1, dim3(AMP_WG), GemmCfg<128>::LDS_BYTES, st, P, (const unsigned*)w.nstop);
        AMP_LAUNCH_CHECK("tvamp_k1");
        tvamp_launch_k2(P, t, w.nstop, st);
        AMP_LAUNCH_CHECK("tvamp_k2");
        hipLaunchKernelGGL(tvamp_r, dim3(E), dim3(RWG), 0, st, P, c64, t, w.nstop);
        AMP_LAUNCH_CHECK("tvamp_r");
    }
    hipLaunchKernelGGL(tvamp_output_kernel, dim3(E), dim3(256), 0, st, P);
    AMP_LAUNCH_CHECK("tvamp_output");
    return dec ? trials_decide_launch(d, c, td, E, w.dec, st) : AMP_OK;
}

}  // extern "C"

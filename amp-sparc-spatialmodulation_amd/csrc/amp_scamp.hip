// amp_scamp.hip — SCAMP (spatially coupled SPARC AMP), device-resident iteration loop.
//
// Restates SCAMP.forward (scamp.py:77-107), Tracker (scamp.py:8-25) and
// SCAMPLayer.forward (scamp.py:43-59):
//   gamma = W psi / Lc ; b = gamma / phi ; z = y - A xmmse + b z ; phi = sigma2 + gamma ;
//   tau = L / (W^T (1/phi)) / Mr ; xmap = xmmse + tau (A^H (z / phi)) ;
//   xmmse = denoiser(xmap, tau/2) (mean only, scamp.py:61-68) ;
//   psi = 1 - sum_{block} |xmmse|^2 / Na ; early exit on allclose(psi) (scamp.py:105).
// Per iteration: two fp32-MFMA GEMM launches with fused epilogues + one reduction /
// exact-float64 fix-up workgroup.  The second GEMM's column tile holds whole coupling
// blocks (2*Nt columns) so psi is formed in its epilogue.
#include <algorithm>
#include <atomic>
#include <mutex>

#include "amp_gemm_x3.h"
#include "amp_scamp.h"

namespace amp {

// The epilogues are amp_scamp.h's, shared with the independent-trial engine
// (amp_scamp_trials.hip): a GEMM kernel here is its entry guard, the tile of its arithmetic and the
// epilogue calls under the AllRows guard.

// scamp_residual.  X3: the bf16x3 tile (amp_gemm_x3.h) in an instantiation of its own, so the f32
// tiles keep their register budget (one instantiation holding both ran the f32 ISI shape 25 % slower)
template <int KC, bool X3 = false>
__global__ __launch_bounds__(AMP_WG) void scamp_ka(ScampK P, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (P.iters[t].stopped) return;
    const GemmTile tile = xcd_tile();
    const int row0 = tile.rb * GBM, col0 = tile.cb * 128;
    const int twoN = 2 * P.N;
    const int kb = P.bandA ? P.bandA[2 * tile.cb] : 0, ke = P.bandA ? P.bandA[2 * tile.cb + 1] : -1;
    if constexpr (X3)
        gemm_tile_x3<128, true>(P.lap, P.rows_pad, P.N, P.WA, row0, col0, lds, kb, ke);
    else
        gemm_tile<128, ALoadPlain, KC>(ALoadPlain{P.xm, twoN, P.B, twoN}, P.WA, P.kapA, row0, col0, lds, kb, ke);
    scamp_residual<KC>(P, AllRows{}, t, lds, row0, col0);
}

// scamp_xmap ; xmmse = denoiser ; psi where the tile holds whole coupling blocks   (scamp.py:53-59)
template <int BN, int KK, int KC = GKC, bool X3 = false>
__global__ __launch_bounds__(AMP_WG) void scamp_kb(ScampK P, int t) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (P.iters[t].stopped) return;
    const GemmTile tile = xcd_tile();
    const int row0 = tile.rb * GBM, col0 = tile.cb * BN;
    const int sld = scamp_sld(P.n);
    const int kb = P.bandB ? P.bandB[2 * tile.cb] : 0, ke = P.bandB ? P.bandB[2 * tile.cb + 1] : -1;
    if constexpr (X3)
        gemm_tile_x3<BN, true>(P.lap, P.rows_pad, P.n, P.WAH, row0, col0, lds, kb, ke);
    else
        gemm_tile<BN, ALoadPlain, KC>(ALoadPlain{P.s, sld, P.B, sld}, P.WAH, P.kapB, row0, col0, lds, kb, ke);
    const int nrows = min(GBM, P.B - row0), ncols = min(BN, 2 * P.N - col0);
    const ScampTileBlocks tb = scamp_tile_blocks(P, col0, ncols);
    const float* tau_t = scamp_xmap<BN, KC>(P, AllRows{}, t, lds, row0, col0, nrows, ncols, tb);
    const ScampDenoisePolicy pol = scamp_policy<BN, KC>(P, lds, tau_t, row0, col0, ncols, tb, 0);
    PartAcc pa;
    denoise_sections<false, KK>(pol, nrows * pol.spr, P.M, P.c, pa);
    __syncthreads();
    // psi from the freshly written tile: one thread per (row, whole coupling block)
    unsigned nc = 0;
    for (int e = threadIdx.x; e < (P.psi_split ? 0 : GBM * tb.nlc); e += AMP_WG) {
        const int rho = e / tb.nlc, b = e % tb.nlc;
        if (rho < nrows) nc += scamp_psi_in_tile(P, t, row0 + rho, tb.lc0 + b);
    }
    pa.notclose += nc;
    part_block_store(pa, P.parts + (size_t)t * P.nblk + blockIdx.y * gridDim.x + blockIdx.x, lds);
}

// psi (scamp.py:59) and its allclose count (scamp.py:105) when the A^H tile holds only part of
// a coupling block, after every tile of the iteration is written.

__global__ __launch_bounds__(AMP_WG) void scamp_psi(ScampK P, int t) {
    // one wavefront per (trial, coupling block): lanes stride the block's Nt entries
    __shared__ unsigned s_u[AMP_WG / 64];
    if (P.iters[t].stopped) return;
    const int lane = threadIdx.x & 63;
    const int nwave = gridDim.x * (AMP_WG / 64);
    unsigned nc = 0;
    for (int blk = blockIdx.x * (AMP_WG / 64) + (threadIdx.x >> 6); blk < P.B * P.Lin; blk += nwave) {
        const double ssum = scamp_block_energy(reinterpret_cast<const float2*>(P.xm) + (size_t)blk * P.Nt, P.Nt);
        if (lane == 0) nc += (unsigned)scamp_psi_store(P, t, blk, ssum);
    }
    nc = block_sum(nc, s_u);
    if (threadIdx.x == 0) P.psi_nc[(size_t)t * P.psi_nblk + blockIdx.x] = nc;
}

// Rare path (float64 fix-up) spread over the grid.  scamp_r reduces the partials and, when some
// section may leave the float64 range, settles the exact batch max |xi| G (one workgroup: few
// candidate sections); scamp_fix_sec recomputes the out-of-range sections with the reference's
// exact arithmetic, scamp_fix_psi_fin their coupling blocks' psi (and the allclose delta), each a
// grid kernel, and the last workgroup of the second adds the per-block counts and decides the
// early exit.  Without a pending fix-up both return at once.  The trial-sharded stages run
// scamp_fix_sec / scamp_fix_psi and settle the counts across ranks.  (Before: one
// workgroup recomputed every such section, 267 us per iteration at cfg3's NaN onset.)
__device__ __forceinline__ void scamp_finish(const ScampK& P, int t, uint32_t notclose, int fixed, int fixed_all) {
    scamp_record(P, &P.iters[t + 1], P.status, t, notclose, fixed, fixed_all);
}

__global__ __launch_bounds__(SRWG) void scamp_r(ScampK P, Const64 c64, int t) {
    __shared__ __attribute__((aligned(16))) float lds[512];
    __shared__ double s_d[SRWG / 64];
    const ScampIter cur = P.iters[t];
    if (cur.stopped) {
        if (threadIdx.x == 0) P.iters[t + 1] = cur;
        return;
    }
    PartAcc pa = part_reduce_all(P.parts + (size_t)t * P.nblk, P.nblk, lds);
    if (P.psi_split) {
        __shared__ unsigned s_u[SRWG / 64];
        unsigned nc = 0;
        for (int i = threadIdx.x; i < P.psi_nblk; i += blockDim.x) nc += P.psi_nc[(size_t)t * P.psi_nblk + i];
        pa.notclose += block_sum(nc, s_u);
    }
    if (part_allnan(pa)) {
        if (!cur.fixed_all) {
            nan_fill(P.xm, nullptr, (size_t)P.B * P.N);
            float* psi_new = spsi(P, t);
            for (int e = threadIdx.x; e < P.B * P.Lin; e += blockDim.x) psi_new[e] = __int_as_float(0x7fc00000);
        }
        if (threadIdx.x == 0) scamp_finish(P, t, 1u, -1, 1);
    } else if (part_danger(pa)) {
        // exact float64 batch max |xi| over the candidate sections (those within the float32
        // estimate's slack of the float32 batch max)
        const double slack = logit_slack(pa.maxabs);
        double gm = 0.0;
        for (int sct = threadIdx.x; sct < P.B * P.L; sct += blockDim.x) {
            if ((double)P.secabs[sct] < pa.maxabs - slack) continue;
            gm = fmax(gm, section_absmax_f64(scamp_section_load(P, (size_t)sct * P.M), P.M, c64));
        }
        gm = group_max(gm, 64);
        if ((threadIdx.x & 63) == 0) s_d[threadIdx.x >> 6] = gm;
        __syncthreads();
        if (threadIdx.x == 0) {
            double G = 0.0;
            for (int w = 0; w < SRWG / 64; ++w) G = fmax(G, s_d[w]);
            P.iters[t + 1] = scamp_pending(t, G, slack, pa.notclose);
        }
    } else if (threadIdx.x == 0) {
        scamp_finish(P, t, pa.notclose, 0, 0);
    }
}

// per-block integer counts of the fix-up kernels, written over iteration t's partials (already
// consumed by scamp_r): slot i = {sections fixed, allclose delta} of block i
__device__ __forceinline__ int2* scamp_fix_counts(const ScampK& P, int t) {
    return reinterpret_cast<int2*>(P.parts + (size_t)t * P.nblk);
}

__global__ __launch_bounds__(AMP_WG) void scamp_fix_sec(ScampK P, Const64 c64, int t) {
    __shared__ int s_i[AMP_WG / 64];
    const ScampIter pend = P.iters[t + 1];
    if (!pend.active || P.iters[t].stopped) return;
    int cnt = 0;
    for (int sct = blockIdx.x * blockDim.x + threadIdx.x; sct < P.B * P.L; sct += gridDim.x * blockDim.x) {
        if (!((double)P.secmax[sct] - pend.G < AMP_DANGER + pend.slack)) continue;
        const size_t o0 = (size_t)sct * P.M;
        exact_section_f64<false>(scamp_section_load(P, o0), scamp_section_store(P, o0), P.M, c64, pend.G);
        ++cnt;
    }
    cnt = block_sum(cnt, s_i);
    if (threadIdx.x == 0) scamp_fix_counts(P, t)[blockIdx.x].x = cnt;
}

__device__ __forceinline__ void scamp_fix_psi_body(const ScampK& P, int t, const ScampIter& pend, int* s_i) {
    int dnc = 0;
    if (P.Nt > SFIX_SERIAL_NT) {
        // wide blocks: one wavefront per block, in scamp_psi's summation order
        const int nwave = gridDim.x * (blockDim.x >> 6);
        for (int blk = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); blk < P.B * P.Lin; blk += nwave)
            dnc += scamp_fix_psi_wave(P, t, blk, pend);
    } else {
        for (int blk = blockIdx.x * blockDim.x + threadIdx.x; blk < P.B * P.Lin; blk += gridDim.x * blockDim.x)
            dnc += scamp_fix_psi_serial(P, t, blk, pend);
    }
    dnc = block_sum(dnc, s_i);
    if (threadIdx.x == 0) scamp_fix_counts(P, t)[blockIdx.x].y = dnc;
}

__global__ __launch_bounds__(AMP_WG) void scamp_fix_psi(ScampK P, int t) {
    __shared__ int s_i[AMP_WG / 64];
    const ScampIter pend = P.iters[t + 1];
    if (!pend.active || P.iters[t].stopped) return;
    scamp_fix_psi_body(P, t, pend, s_i);
}

// scamp_fix_psi, then (last workgroup to arrive) scamp_fin's count and exit decision over both
// fix-up launches' per-block counts: one launch fewer per iteration.  scamp_fix_sec stays a launch
// of its own (one thread per section: the exact float64 recompute is the rare path's cost).
__global__ __launch_bounds__(AMP_WG) void scamp_fix_psi_fin(ScampK P, int t) {
    __shared__ int s_i[AMP_WG / 64];
    const ScampIter pend = P.iters[t + 1];
    if (!pend.active || P.iters[t].stopped) return;
    scamp_fix_psi_body(P, t, pend, s_i);
    if (last_arrival(P.rcnt + 1, gridDim.x)) {
        const int2* c = scamp_fix_counts(P, t);
        int fixed = 0, d = 0;
        for (int i = threadIdx.x; i < (int)gridDim.x; i += blockDim.x) { fixed += c[i].x; d += c[i].y; }
        fixed = block_sum(fixed, s_i);
        d = block_sum(d, s_i);
        if (threadIdx.x == 0) scamp_finish(P, t, (uint32_t)((int)pend.notclose + d), fixed, 0);
    }
}

// ---- trial-sharded iteration (amp_scamp_run_sharded; SURVEY §8(e) exact-compat) ----
// scamp_r / scamp_fin split at their batch-global values, as the VAMP and BAMP stages: the
// denoiser's max|xi| / min section max (scamp.py:64) and the psi allclose count (scamp.py:105)
// after sxr1, the rare path's exact max|xi| after sxr2 (scamp_fix_sec / scamp_fix_psi then
// recompute this rank's sections and psi), the fix-up counts after sxr4.
__global__ __launch_bounds__(SRWG) void scamp_sxr1(ScampK P, int t) {
    __shared__ __attribute__((aligned(16))) float lds[512];
    __shared__ unsigned s_u[SRWG / 64];
    XState* xs = P.xs;
    if (P.iters[t].stopped) {
        if (threadIdx.x == 0) { xs->sum[0] = xs->sum[1] = 0.0; xs->mx[0] = xs->mx[1] = 0.0; }
        return;
    }
    PartAcc pa = part_reduce_all(P.parts + (size_t)t * P.nblk, P.nblk, lds);
    if (P.psi_split) {
        unsigned nc = 0;
        for (int i = threadIdx.x; i < P.psi_nblk; i += blockDim.x) nc += P.psi_nc[(size_t)t * P.psi_nblk + i];
        pa.notclose += block_sum(nc, s_u);
    }
    if (threadIdx.x == 0) {
        xs->sum[0] = 0.0;
        xs->sum[1] = (double)pa.notclose;
        xs->mx[0] = (pa.maxabs <= 1.7976931348623157e308) ? pa.maxabs : INFINITY;   // NaN / inf wins
        xs->mx[1] = (pa.minsecmax == pa.minsecmax) ? -pa.minsecmax : INFINITY;
    }
}

__global__ __launch_bounds__(SRWG) void scamp_sxr2(ScampK P, Const64 c64, int t) {
    __shared__ double s_d[SRWG / 64];
    XState* xs = P.xs;
    const ScampIter cur = P.iters[t];
    if (cur.stopped) {
        if (threadIdx.x == 0) { P.iters[t + 1] = cur; xs->mode = 0; xs->gmax[0] = 0.0; }
        return;
    }
    PartAcc pa;
    pa.notclose = (uint32_t)xs->sum[1];
    pa.maxabs = xs->mx[0];
    pa.minsecmax = -xs->mx[1];
    if (part_allnan(pa)) {
        if (!cur.fixed_all) {
            nan_fill(P.xm, nullptr, (size_t)P.B * P.N);
            float* psi_new = spsi(P, t);
            for (int e = threadIdx.x; e < P.B * P.Lin; e += blockDim.x) psi_new[e] = __int_as_float(0x7fc00000);
        }
        if (threadIdx.x == 0) { scamp_finish(P, t, 1u, -1, 1); xs->mode = 0; xs->gmax[0] = 0.0; }
    } else if (part_danger(pa)) {
        // this rank's exact float64 max |xi| over its candidate sections (scamp_r's first stage)
        const double slack = logit_slack(pa.maxabs);
        double gm = 0.0;
        for (int sct = threadIdx.x; sct < P.B * P.L; sct += blockDim.x) {
            if ((double)P.secabs[sct] < pa.maxabs - slack) continue;
            gm = fmax(gm, section_absmax_f64(scamp_section_load(P, (size_t)sct * P.M), P.M, c64));
        }
        gm = group_max(gm, 64);
        if ((threadIdx.x & 63) == 0) s_d[threadIdx.x >> 6] = gm;
        __syncthreads();
        if (threadIdx.x == 0) {
            double G = 0.0;
            for (int w = 0; w < SRWG / 64; ++w) G = fmax(G, s_d[w]);
            xs->gmax[0] = G;
            xs->mode = 2;
            P.iters[t + 1] = scamp_pending(t, G, slack, pa.notclose);   // G: set to the global value by scamp_sxr3
        }
    } else if (threadIdx.x == 0) {
        scamp_finish(P, t, pa.notclose, 0, 0);
        xs->mode = 0;
        xs->gmax[0] = 0.0;
    }
}

__global__ void scamp_sxr3(ScampK P, int t) {   // the global exact G into the pending record
    if (threadIdx.x == 0 && P.xs->mode == 2) P.iters[t + 1].G = P.xs->gmax[0];
}

__global__ __launch_bounds__(AMP_WG) void scamp_sxr4(ScampK P, int t, int nfix) {   // this rank's fix-up counts
    __shared__ int s_i[AMP_WG / 64];
    XState* xs = P.xs;
    if (xs->mode != 2) {
        if (threadIdx.x == 0) xs->fix[0] = xs->fix[1] = xs->fix[2] = 0.0;
        return;
    }
    const int2* c = scamp_fix_counts(P, t);
    int fixed = 0, dnc = 0;
    for (int i = threadIdx.x; i < nfix; i += blockDim.x) { fixed += c[i].x; dnc += c[i].y; }
    fixed = block_sum(fixed, s_i);
    dnc = block_sum(dnc, s_i);
    if (threadIdx.x == 0) { xs->fix[0] = 0.0; xs->fix[1] = (double)dnc; xs->fix[2] = (double)fixed; }
}

__global__ void scamp_sxr5(ScampK P, int t) {
    const XState* xs = P.xs;
    if (threadIdx.x != 0 || xs->mode != 2) return;
    const long long nc = (long long)xs->sum[1] + (long long)xs->fix[1];
    scamp_finish(P, t, (uint32_t)nc, (int)xs->fix[2], 0);
}

// Tracker (scamp.py:9-25) and the record of iteration 0
__global__ void scamp_init_kernel(ScampK P) {
    scamp_init_state(P);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        P.rcnt[0] = 0u; P.rcnt[1] = 0u;
        P.iters[0] = scamp_iter(0, 0, 0, 0, 0);
    }
}

__global__ void scamp_output_kernel(ScampK P) {
    const int T = P.status->T;
    if (((T - 1) & 1) == 0) return;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < (size_t)P.B * P.Lin;
         e += (size_t)gridDim.x * blockDim.x)
        P.psi0[e] = P.psi1[e];
}

static std::once_flag g_scamp_once;
static int g_scamp_rc = 0;

template <int KK>
static int scamp_kb_attrs() {
    int rc = set_lds_attr<128>((const void*)scamp_kb<128, KK>);
    if (!rc) rc = set_lds_attr<256>((const void*)scamp_kb<256, KK, GKC, true>);
    return rc ? rc : set_lds_attr<256>((const void*)scamp_kb<256, KK>);
}

// Block-banded A (the ISI operators): every tile reduces over a few coupling blocks only, so the
// 256-wide A chunk (half the LDS: four tiles per CU instead of two) costs no extra chunks there.
// AMP_SCAMP_KC=512 keeps the 512-wide chunk (A/B runs).
constexpr size_t SKC_LDS = GemmCfg<128, 256>::LDS_BYTES;   // the short-chunk tiles' LDS

static bool scamp_short_chunks(const ScampK& P) {
    static const bool off = [] {
        const char* e = diag_env("AMP_SCAMP_KC");
        return e && atoi(e) == 512;
    }();
    return P.bandA != nullptr && !off;
}

// the bf16x3 tiles run in the 128-wide short-chunk instantiations (their epilogues' LDS budget is
// the 256-chunk A block) with the staged planes' 48 KB, the 256-wide kb in its GKC instantiation
constexpr size_t SX3_LDS = x3_tile_lds<128, true>(GemmCfg<128, 256>::A_FLOATS - GemmCfg<128, 256>::CTILE_FLOATS);
static_assert(x3_tile_lds<256, true>(0) <= GemmCfg<256>::LDS_BYTES, "bf16x3 planes within the 256-wide tile's LDS");

// A rows -> six bf16 planes for the next bf16x3 GEMM (no-op launch once the loop has stopped)
static void scamp_split(const ScampK& P, const float* a, int lda, int K, int t, hipStream_t st) {
    const int wpr = (P.rows_pad / 4 < 2 * device_cu_count() && K >= 1024) ? 4 : 1;
    hipLaunchKernelGGL(x3_split_rows_kernel<true>, dim3(P.rows_pad * wpr / 4), dim3(256), 0, st, a, lda, P.B,
                       P.rows_pad, K, P.lap, &P.iters[t].stopped, wpr);
}

template <int KK>
static void launch_kb_kk(const ScampK& P, int gr, size_t ldsB, int t, hipStream_t st) {
    if (P.bn == 128 && P.lx3)
        hipLaunchKernelGGL((scamp_kb<128, KK, 256, true>), dim3(gr, P.ncpB / 128), dim3(AMP_WG), SX3_LDS, st, P, t);
    else if (P.lx3)
        hipLaunchKernelGGL((scamp_kb<256, KK, GKC, true>), dim3(gr, P.ncpB / 256), dim3(AMP_WG), ldsB, st, P, t);
    else if (P.bn == 128 && scamp_short_chunks(P))
        hipLaunchKernelGGL((scamp_kb<128, KK, 256>), dim3(gr, P.ncpB / 128), dim3(AMP_WG), SKC_LDS,
                           st, P, t);
    else if (P.bn == 128)
        hipLaunchKernelGGL((scamp_kb<128, KK>), dim3(gr, P.ncpB / 128), dim3(AMP_WG), ldsB, st, P, t);
    else
        hipLaunchKernelGGL((scamp_kb<256, KK>), dim3(gr, P.ncpB / 256), dim3(AMP_WG), ldsB, st, P, t);
}

static void launch_ka(const ScampK& P, int gr, int t, hipStream_t st) {
    if (P.lx3) {
        scamp_split(P, P.xm, 2 * P.N, P.N, t, st);
        hipLaunchKernelGGL((scamp_ka<256, true>), dim3(gr, P.ncpA / 128), dim3(AMP_WG), SX3_LDS, st, P, t);
    } else if (scamp_short_chunks(P))
        hipLaunchKernelGGL(scamp_ka<256>, dim3(gr, P.ncpA / 128), dim3(AMP_WG), SKC_LDS, st, P, t);
    else
        hipLaunchKernelGGL(scamp_ka<GKC>, dim3(gr, P.ncpA / 128), dim3(AMP_WG), GemmCfg<128>::LDS_BYTES, st, P, t);
}

static void launch_kb(const ScampK& P, int gr, size_t ldsB, int t, hipStream_t st) {
    if (P.lx3) scamp_split(P, P.s, 2 * P.n, P.n, t, st);
    dispatch_K(P.c.K, [&](auto kk) { launch_kb_kk<decltype(kk)::value>(P, gr, ldsB, t, st); });
}

static int scamp_attrs() {
    std::call_once(g_scamp_once, [] {
        g_scamp_rc = set_lds_attr<128>((const void*)scamp_ka<GKC>);
        if (!g_scamp_rc) g_scamp_rc = scamp_kb_attrs<1>();
        if (!g_scamp_rc) g_scamp_rc = scamp_kb_attrs<2>();
        if (!g_scamp_rc) g_scamp_rc = scamp_kb_attrs<4>();
        if (!g_scamp_rc) g_scamp_rc = scamp_kb_attrs<8>();
        if (!g_scamp_rc) g_scamp_rc = scamp_kb_attrs<16>();
        if (!g_scamp_rc) g_scamp_rc = scamp_kb_attrs<64>();
    });
    return g_scamp_rc;
}

}  // namespace amp

using namespace amp;

extern "C" {

size_t amp_scamp_workspace_bytes(const amp_dims* d, int32_t max_iter) {
    if (!d || max_iter <= 0) return 0;
    return scamp_carve(d, max_iter, nullptr).bytes;
}

}  // extern "C"

namespace amp {

// AMP_SCAMP_GEMM=f32: AMP_GEMM_AUTO keeps the f32-MFMA persistent GEMMs (A/B runs)
static bool scamp_gemm_f32_requested() {
    static const bool v = [] {
        const char* e = diag_env("AMP_SCAMP_GEMM");
        return e && e[0] == 'f';
    }();
    return v;
}

// AMP_SCAMP_GEMM=h2: AMP_GEMM_AUTO picks the fp16x2 persistent GEMMs instead of bf16x3 (A/B runs)
static bool scamp_gemm_h2_requested() {
    static const bool v = [] {
        const char* e = diag_env("AMP_SCAMP_GEMM");
        return e && e[0] == 'h';
    }();
    return v;
}

// Block-banded A (Lin > 1 or Lout > 1): the GEMMs skip the reduction blocks of each column tile
// that hold only zeros (weight_kband over the packed weights, once per forward).  Off with
// AMP_BAND_GEMM=0 (A/B runs).
static bool band_gemm_enabled() {
    static const bool on = [] {
        const char* e = diag_env("AMP_BAND_GEMM");
        return !(e && e[0] == '0');
    }();
    return on;
}

static int scamp_setup(const amp_dims* d, const amp_constellation* c, const amp_scamp_args* a, ScampK& P,
                       Const64& c64) {
    // any Nt whose section size M = Nt / Na is a power of two (check_dims); the A^H column tiles
    // take coupling blocks of any width and a partial last tile
    int rc = check_dims(d, c, true, true);
    if (rc) return rc;
    AMP_REQUIRE(a && a->W && a->A && a->y && a->xmap && a->xmmse && a->psi && a->status && a->ws,
                "amp_scamp_run: null pointer argument");
    AMP_REQUIRE(a->max_iter > 0, "amp_scamp_run: max_iter must be positive");
    AMP_REQUIRE(d->Lin <= SMAXLIN, "amp_scamp_run: Lin = %d > %d", d->Lin, SMAXLIN);
    AMP_REQUIRE(scamp_index_ok(d, d->B), "amp_scamp_run: B = %d trials of max(2N, 2n) = %d columns need more than "
                "32-bit offsets (or more than 65535 column tiles)", d->B, 2 * std::max(d->N, d->n));
    const ScampWs w = scamp_carve(d, a->max_iter, a->ws);
    AMP_REQUIRE(a->ws_bytes >= w.bytes, "amp_scamp_run: workspace %zu < %zu bytes", a->ws_bytes, w.bytes);
    rc = scamp_attrs();
    if (rc) return rc;
    scamp_geometry(d, d->B, P);
    P.max_iter = a->max_iter;
    P.sigma2 = (float)a->noise_var;
    P.W = (const float*)a->W;
    P.WA = w.WA; P.WAH = w.WAH;
    // block-banded A: the ranges are formed by the prepare launch sequence (every later call of
    // the layer-level API reads them from the workspace)
    const bool band = (d->Lin > 1 || d->Lout > 1) && band_gemm_enabled();
    P.bandA = band ? w.bandA : nullptr;
    P.bandB = band ? w.bandB : nullptr;
    P.xs = w.xs;
    P.y = (const float*)a->y; P.z = w.z; P.s = w.s; P.phi = w.phi; P.tau = w.tau;
    P.xmap = (float*)a->xmap; P.xm = (float*)a->xmmse; P.psi0 = (float*)a->psi; P.psi1 = w.psi1;
    P.secmax = w.secmax; P.secabs = w.secabs; P.parts = w.parts; P.iters = w.iters; P.status = (amp_status*)a->status;
    P.psi_nc = w.psi_nc; P.psi_nblk = scamp_psi_nblk(d);
    P.nwg = cdiv(d->B, 16);
    P.gen = 0;
    P.Wq1 = w.Wq1; P.Wq2 = w.Wq2; P.pparts = w.pparts; P.pxch = w.pxch; P.pbar = w.pbar;
    P.Wx1 = w.Wx1; P.Wx2 = w.Wx2;
    P.dec_on = 0; P.ibits = 0; P.xtrue = nullptr; P.sym = nullptr; P.idx = nullptr; P.counts = nullptr;
    P.host_rec = nullptr;
    P.fold_in = fold_in_kernel() ? 1 : 0;
    P.dwg = w.dwg;
    P.trace = nullptr;
    P.rcnt = w.pbar + 8;
    P.c = to_const(c);
    c64 = to_const64(c);
    AMP_REQUIRE(a->gemm >= AMP_GEMM_AUTO && a->gemm <= AMP_GEMM_H2, "amp_scamp: gemm %d", a->gemm);
    const bool fits = scamp_persist_x3_fits(d), lx3ok = scamp_lx3_shape(d);
    AMP_REQUIRE(a->gemm != AMP_GEMM_H2 || fits, "amp_scamp: the split-precision engine's LDS carve exceeds 160 KB");
    AMP_REQUIRE(a->gemm != AMP_GEMM_X3 || fits || lx3ok,
                "amp_scamp: bf16x3 needs the persistent engine's LDS carve within 160 KB or, on the launch engine, "
                "N %% 64 == 0 and n %% 64 == 0 (N = %d, n = %d)", d->N, d->n);
    // launch engine: bf16x3 tiles when asked for (AMP_GEMM_X3) or, under AUTO, with
    // AMP_SCAMP_LAUNCH_GEMM=x3; f32 MFMA tiles otherwise
    static const bool lx3_env = [] {
        const char* e = diag_env("AMP_SCAMP_LAUNCH_GEMM");
        return e && e[0] == 'x';
    }();
    P.lx3 = lx3ok && (a->gemm == AMP_GEMM_X3 || (a->gemm == AMP_GEMM_AUTO && lx3_env)) ? 1 : 0;
    P.rows_pad = round_up(d->B, GBM);
    P.lap = w.lap;
    // 0 f32 MFMA, 1 bf16x3, 2 fp16x2.  AUTO keeps bf16x3 for SCAMP: with fp16x2 one cfg3 golden
    // (QPSK, 7 dB, seed 1) never meets the psi allclose exit (T 20 vs the reference's 6, VER / SER
    // equal): at nMSE 1e-9 psi is ~1e-9 and torch.allclose's atol 1e-8 decides, which the
    // fp16x2 products' 2^-22 terms move.  AMP_SCAMP_GEMM=f32 / h2 for A/B runs.
    P.x3 = a->gemm == AMP_GEMM_H2 ? 2 : a->gemm == AMP_GEMM_X3 ? (fits ? 1 : 0) : a->gemm == AMP_GEMM_F32 || !fits ? 0
         : scamp_gemm_f32_requested() ? 0 : scamp_gemm_h2_requested() ? 2 : 1;
    return AMP_OK;
}

// The persistent engine's operators (16x16x4-packed A and A^H) and zeroed barrier words, in one
// launch; a fresh generation for the granule tags.
static int scamp_persist_prepare(ScampK& P, const amp_scamp_args* a, hipStream_t st) {
    static std::atomic<unsigned> gen{0};
    P.gen = ++gen;
    CWeightJob j[2];
    if (P.x3) {
        const int pk = P.x3 == 2 ? WPACKH2 : WPACKX3;
        //   A x     (scamp.py:47)   X[o][j] = A[o][j],        o < n, j < N   (bf16x3 / fp16x2 planes)
        j[0] = CWeightJob{(const float2*)a->A, P.N, 1, 0, nullptr, P.n, P.N, (float*)P.Wx1, P.N, P.n, pk, SH2_EX};
        //   A^H s   (scamp.py:57)   X[o][j] = conj(A[j][o]),  o < N, j < n
        j[1] = CWeightJob{(const float2*)a->A, 1, P.N, 1, nullptr, P.N, P.n, (float*)P.Wx2, P.n, P.N, pk, SH2_EX};
        return build_cweights(j, 2, P.pbar, 64, st);
    }
    //   A x       (scamp.py:47)   X[o][j] = A[o][j],        o < n, j < N
    j[0] = CWeightJob{(const float2*)a->A, P.N, 1, 0, nullptr, P.n, P.N, (float*)P.Wq1, 2 * P.N, 2 * P.n, WPACK16};
    //   A^H s     (scamp.py:57)   X[o][j] = conj(A[j][o]),  o < N, j < n
    j[1] = CWeightJob{(const float2*)a->A, 1, P.N, 1, nullptr, P.N, P.n, (float*)P.Wq2, 2 * P.n, 2 * P.N, WPACK16};
    return build_cweights(j, 2, P.pbar, 64, st);
}

// Tracker (scamp.py:9-25): the two weights and the initial state.
static int scamp_prepare_impl(const ScampK& P, const amp_scamp_args* a, hipStream_t st) {
    int rc;
    const float2* A = (const float2*)a->A;
    if (P.lx3) {
        // bf16x3 planes (x3_index) in the f32 weights' buffers (12 of their 16 bytes per entry):
        // A x (O = n, J = N), A^H s (O = N, J = n)
        CWeightJob j[2];
        j[0] = CWeightJob{A, P.N, 1, 0, nullptr, P.n, P.N, (float*)P.WA, P.N, P.n, WPACKX3, 0};
        j[1] = CWeightJob{A, 1, P.N, 1, nullptr, P.N, P.n, (float*)P.WAH, P.n, P.N, WPACKX3, 0};
        if ((rc = build_cweights(j, 2, nullptr, 0, st))) return rc;
        if (P.bandA) {
            if ((rc = h2_kband(P.WA, 6, P.N / 32, 4, P.ncpA / 128, P.n / 16, const_cast<int*>(P.bandA), st))) return rc;
            if ((rc = h2_kband(P.WAH, 6, P.n / 32, P.bn / 32, P.ncpB / P.bn, P.N / 16, const_cast<int*>(P.bandB), st)))
                return rc;
        }
    } else if ((rc = scamp_pack_f32(P, A, st))) {   // the f32 operators and their band ranges
        return rc;
    }
    const size_t tot = std::max(std::max((size_t)P.B * P.N, (size_t)P.B * P.n), (size_t)P.B * P.Lout);
    hipLaunchKernelGGL(scamp_init_kernel, dim3((int)std::min<size_t>((tot + 255) / 256, 2048)), dim3(256), 0, st, P);
    AMP_LAUNCH_CHECK("scamp_init");
    return AMP_OK;
}

// One SCAMPLayer.forward (scamp.py:43-59) + the allclose(psi) test of scamp.py:105: the two GEMM
// launches (+ scamp_psi when a tile holds part of a coupling block), the batch reduction and the
// rare path's fix-up with its exit decision (scamp_fix_sec, scamp_fix_psi_fin: they return at once
// unless scamp_r left a pending record).  The reduction keeps a launch of its own: folded into the last workgroup of
// the GEMM launch it needs an agent-scope release per workgroup (an L2 write-back on every XCD),
// which cost more than the launch (scamp_psi 6.9 -> 40 us at the ISI shape).
static int scamp_iterate_impl(const ScampK& P, const Const64& c64, int t, hipStream_t st) {
    const int gr = cdiv(P.B, GBM);
    const size_t ldsB = (P.bn == 128 ? GemmCfg<128>::LDS_BYTES : GemmCfg<256>::LDS_BYTES);
    // fix-up grid: one slot per block in iteration t's partials (consumed by then)
    const int nfix = fix_grid(P.nblk, P.B * P.L);
    launch_ka(P, gr, t, st);
    launch_kb(P, gr, ldsB, t, st);
    if (P.psi_split)
        hipLaunchKernelGGL(scamp_psi, dim3(P.psi_nblk), dim3(AMP_WG), 0, st, P, t);
    hipLaunchKernelGGL(scamp_r, dim3(1), dim3(SRWG), 0, st, P, c64, t);
    hipLaunchKernelGGL(scamp_fix_sec, dim3(nfix), dim3(AMP_WG), 0, st, P, c64, t);
    hipLaunchKernelGGL(scamp_fix_psi_fin, dim3(nfix), dim3(AMP_WG), 0, st, P, t);
    AMP_LAUNCH_CHECK("scamp iteration");
    return AMP_OK;
}

static int scamp_iterate_sharded(const ScampK& P, const Const64& c64, int t, hipStream_t st, bool& hook_failed) {
    const int gr = cdiv(P.B, GBM);
    const size_t ldsB = (P.bn == 128 ? GemmCfg<128>::LDS_BYTES : GemmCfg<256>::LDS_BYTES);
    const int nfix = fix_grid(P.nblk, P.B * P.L);
    launch_ka(P, gr, t, st);
    launch_kb(P, gr, ldsB, t, st);
    if (P.psi_split) hipLaunchKernelGGL(scamp_psi, dim3(P.psi_nblk), dim3(AMP_WG), 0, st, P, t);
    hipLaunchKernelGGL(scamp_sxr1, dim3(1), dim3(SRWG), 0, st, P, t);
    AMP_LAUNCH_CHECK("scamp_sxr1");
    // every hook call is made on every rank even after one failed: the ranks' collectives stay
    // matched and a failed rank's poisoned words reach the others (amp_sparc.h)
    hook_failed |= call_allreduce_hook(P.xs->sum, 2, AMP_ALLREDUCE_SUM, st) != AMP_OK;
    hook_failed |= call_allreduce_hook(P.xs->mx, 2, AMP_ALLREDUCE_MAX, st) != AMP_OK;
    hipLaunchKernelGGL(scamp_sxr2, dim3(1), dim3(SRWG), 0, st, P, c64, t);
    AMP_LAUNCH_CHECK("scamp_sxr2");
    hook_failed |= call_allreduce_hook(P.xs->gmax, 1, AMP_ALLREDUCE_MAX, st) != AMP_OK;
    hipLaunchKernelGGL(scamp_sxr3, dim3(1), dim3(64), 0, st, P, t);
    hipLaunchKernelGGL(scamp_fix_sec, dim3(nfix), dim3(AMP_WG), 0, st, P, c64, t);
    hipLaunchKernelGGL(scamp_fix_psi, dim3(nfix), dim3(AMP_WG), 0, st, P, t);
    hipLaunchKernelGGL(scamp_sxr4, dim3(1), dim3(AMP_WG), 0, st, P, t, nfix);
    AMP_LAUNCH_CHECK("scamp_sxr4");
    hook_failed |= call_allreduce_hook(P.xs->fix, 3, AMP_ALLREDUCE_SUM, st) != AMP_OK;
    hipLaunchKernelGGL(scamp_sxr5, dim3(1), dim3(64), 0, st, P, t);
    AMP_LAUNCH_CHECK("scamp_sxr5");
    return AMP_OK;
}

static int scamp_finalize_impl(const ScampK& P, hipStream_t st) {
    hipLaunchKernelGGL(scamp_output_kernel, dim3(64), dim3(256), 0, st, P);
    AMP_LAUNCH_CHECK("scamp_output");
    return AMP_OK;
}

__global__ __launch_bounds__(1024) void vamp_decide_fold(const DecWG* w, int n, amp_counts* out);   // amp_vamp_persist.hip

}  // namespace amp

extern "C" {

int amp_scamp_select_engine(const amp_dims* d, int32_t engine) {
    if (!d) return AMP_E_ARG;
    const bool elig = scamp_persist_eligible(d, device_cu_count());
    if (engine == AMP_ENGINE_PERSISTENT) return elig ? AMP_ENGINE_PERSISTENT : AMP_E_ARG;
    if (engine == AMP_ENGINE_AUTO && elig) return AMP_ENGINE_PERSISTENT;
    return engine == AMP_ENGINE_AUTO || engine == AMP_ENGINE_LAUNCHES ? AMP_ENGINE_LAUNCHES : AMP_E_ARG;
}

int amp_scamp_run_sharded(const amp_dims* d, const amp_constellation* c, const amp_scamp_args* a,
                          int32_t B_global, void* stream) {
    ScampK P;
    Const64 c64;
    int rc = scamp_setup(d, c, a, P, c64);
    if (rc) return rc;
    AMP_REQUIRE(allreduce_hook_set(), "amp_scamp_run_sharded: no all-reduce hook registered (amp_set_allreduce_hook)");
    AMP_REQUIRE(B_global >= d->B, "amp_scamp_run_sharded: B_global = %d < this rank's B = %d", B_global, d->B);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = scamp_prepare_impl(P, a, st))) return rc;
    bool hook_failed = false;
    for (int t = 0; t < P.max_iter && !rc; ++t) rc = scamp_iterate_sharded(P, c64, t, st, hook_failed);
    if (!rc && hook_failed) rc = hook_failure("scamp");
    return rc ? rc : scamp_finalize_impl(P, st);
}

int amp_scamp_run(const amp_dims* d, const amp_constellation* c, const amp_scamp_args* a, void* stream) {
    ScampK P;
    Const64 c64;
    int rc = scamp_setup(d, c, a, P, c64);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    AMP_REQUIRE(a->engine >= AMP_ENGINE_AUTO && a->engine <= AMP_ENGINE_PERSISTENT, "amp_scamp_run: engine %d",
                a->engine);
    const bool elig = scamp_persist_eligible(d, device_cu_count());
    AMP_REQUIRE(a->engine != AMP_ENGINE_PERSISTENT || elig,
                "amp_scamp_run: persistent engine needs (2N, 2n) in {(128, 256), (256, 512), (256, 256)}, M <= 64 "
                "and ceil(B/16) = %d <= %d CUs", cdiv(d->B, 16), device_cu_count());
    if (a->engine == AMP_ENGINE_PERSISTENT || (a->engine == AMP_ENGINE_AUTO && elig)) {
        AMP_REQUIRE(a->gemm != AMP_GEMM_X3 || scamp_persist_x3_fits(d),
                    "amp_scamp_run: the persistent bf16x3 engine's LDS carve exceeds 160 KB");
        if ((rc = scamp_persist_prepare(P, a, st))) return rc;
        DecConst dc;
        static_cast<Const64&>(dc) = c64;   // no decision in this launch: only the float64 table is read
        return scamp_persist_launch(P, dc, st);
    }
    if ((rc = scamp_prepare_impl(P, a, st))) return rc;
    for (int t = 0; t < P.max_iter; ++t)
        if ((rc = scamp_iterate_impl(P, c64, t, st))) return rc;
    return scamp_finalize_impl(P, st);
}

// Diagnostic: one persistent-engine forward whose workgroups stamp s_memtime at every phase
// boundary: trace[(wg * max_iter + t) * 10 + phase] (phases: amp_scamp_persist_kernel.h).
int amp_scamp_persist_trace(const amp_dims* d, const amp_constellation* c, const amp_scamp_args* a, void* trace,
                            void* stream) {
    ScampK P;
    Const64 c64;
    int rc = scamp_setup(d, c, a, P, c64);
    if (rc) return rc;
    AMP_REQUIRE(trace && scamp_persist_eligible(d, device_cu_count()), "amp_scamp_persist_trace: not eligible / null trace");
    hipStream_t st = (hipStream_t)stream;
    if ((rc = scamp_persist_prepare(P, a, st))) return rc;
    P.trace = (unsigned long long*)trace;
    DecConst dc;
    static_cast<Const64&>(dc) = c64;
    return scamp_persist_launch(P, dc, st);
}

int amp_scamp_detect_count(const amp_dims* d, const amp_constellation* c, const amp_scamp_args* a,
                           const amp_vamp_decide_args* dec, void* stream) {
    ScampK P;
    Const64 c64;
    int rc = scamp_setup(d, c, a, P, c64);
    if (rc) return rc;
    AMP_REQUIRE(dec && dec->x && dec->sym && dec->idx && dec->counts, "amp_scamp_detect_count: null pointer argument");
    AMP_REQUIRE(dec->ibits_trunc >= 0 && dec->ibits_trunc < 64, "amp_scamp_detect_count: ibits_trunc out of range");
    AMP_REQUIRE(d->Lin * d->Na * d->M == d->N, "amp_scamp_detect_count: inconsistent dims");
    AMP_REQUIRE(a->engine != AMP_ENGINE_LAUNCHES && scamp_persist_eligible(d, device_cu_count()),
                "amp_scamp_detect_count: needs the persistent engine ((2N, 2n) in {(128, 256), (256, 512), "
                "(256, 256)}, M <= 64, ceil(B/16) = %d <= %d CUs)", cdiv(d->B, 16), device_cu_count());
    hipStream_t st = (hipStream_t)stream;
    if ((rc = scamp_persist_prepare(P, a, st))) return rc;
    P.dec_on = 1;
    P.ibits = dec->ibits_trunc;
    P.xtrue = (const float2*)dec->x;
    P.sym = (const long long*)dec->sym;
    P.idx = (const long long*)dec->idx;
    P.counts = (amp_counts*)dec->counts;
    P.host_rec = P.fold_in ? (unsigned char*)dec->host_record : nullptr;
    DecConst dc = to_decconst(c);
    static_cast<Const64&>(dc) = c64;
    if ((rc = scamp_persist_launch(P, dc, st))) return rc;   // the counter records folded inside it ...
    if (P.fold_in) return AMP_OK;
    hipLaunchKernelGGL(vamp_decide_fold, dim3(1), dim3(256), 0, st, (const DecWG*)P.dwg, P.nwg, P.counts);   // ... or here
    AMP_LAUNCH_CHECK("vamp_decide_fold (scamp)");
    return AMP_OK;
}

int amp_scamp_prepare(const amp_dims* d, const amp_constellation* c, const amp_scamp_args* a, void* stream) {
    ScampK P;
    Const64 c64;
    int rc = scamp_setup(d, c, a, P, c64);
    return rc ? rc : scamp_prepare_impl(P, a, (hipStream_t)stream);
}

int amp_scamp_iterate(const amp_dims* d, const amp_constellation* c, const amp_scamp_args* a, int32_t t,
                      void* stream) {
    ScampK P;
    Const64 c64;
    int rc = scamp_setup(d, c, a, P, c64);
    if (rc) return rc;
    AMP_REQUIRE(t >= 0 && t < a->max_iter, "amp_scamp_iterate: t = %d outside [0, %d)", t, a->max_iter);
    return scamp_iterate_impl(P, c64, t, (hipStream_t)stream);
}

int amp_scamp_finalize(const amp_dims* d, const amp_constellation* c, const amp_scamp_args* a, void* stream) {
    ScampK P;
    Const64 c64;
    int rc = scamp_setup(d, c, a, P, c64);
    return rc ? rc : scamp_finalize_impl(P, (hipStream_t)stream);
}

}  // extern "C"

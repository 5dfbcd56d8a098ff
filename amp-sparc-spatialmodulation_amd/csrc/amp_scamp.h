// amp_scamp.h — SCAMP state shared by the launch engine (amp_scamp.hip), the independent-trial
// engine (amp_scamp_trials.hip) and the persistent engine (amp_scamp_persist.hip): parameter block,
// workspace carve, iteration record, and every GEMM epilogue of the launch and trial engines
// written once (a kernel of either is its entry guard, its gemm_tile call and the epilogue under
// its row guard, amp_trials.h AllRows / LiveRows).
#pragma once

#include <algorithm>

#include "amp_trials.h"

namespace amp {

// fp16x2 persistent GEMMs (amp_scamp_persist_kernel.h, H2): the operator A is packed as A 2^SH2_EX,
// so its entries must stay below 64 in magnitude (the channel's are ~CN(0, 1/Nr)).
constexpr int SH2_EX = 10;


constexpr int SRWG = 1024;
constexpr int SMAXLIN = 64;     // coupling blocks per trial handled in registers / LDS

struct alignas(16) ScampIter {
    int32_t stopped, T, fixed, fixed_all;
    // exact float64 fix-up of iteration T-1 pending (set by scamp_r, done by scamp_fix_sec and
    // scamp_fix_psi_fin, settled by the latter; scamp_fix_* and scamp_sxr* in the trial-sharded
    // stages): the exact batch max |xi| G, the float32 estimate's slack, and the
    // allclose count before the fix-up
    double G, slack;
    uint32_t notclose;
    int32_t active, pad[2];
};

struct ScampK {
    int B, N, n, L, M, Nt, Nr, Na, Lin, Lout, bn;
    int kapA, ncpA, kapB, ncpB;
    int nblk, max_iter;
    float sigma2;          // f32(noise_var) (scamp.py:51)
    const float* W;        // [Lout][Lin]
    const float* WA;       // [ncpA][kapA]  A xmmse
    const float* WAH;      // [ncpB][kapB]  A^H (z/phi)
    const float* y;        // [B][2n]
    float* z;              // [B][2n]
    float* s;              // [B][scamp_sld(n)] z / phi_use
    float* phi;            // [2][B][Lout] ping-pong
    float* tau;            // [B][Lin] (per iteration)
    float* xmap;           // caller [B][2N]
    float* xm;             // caller [B][2N]
    float* psi0;           // caller's psi [B][Lin] (even iterations)
    float* psi1;           // workspace     (odd iterations)
    float* secmax;         // [B*L] per-section max logit (fast path)
    float* secabs;         // [B*L] per-section max |logit|
    Partial* parts;
    ScampIter* iters;
    unsigned* psi_nc;      // [max_iter][psi_nblk] allclose counts of scamp_psi (split tiles only)
    int psi_nblk, psi_split;
    amp_status* status;
    // persistent engine (amp_scamp_persist.hip)
    int nwg;               // ceil(B / 16) workgroups
    unsigned gen;          // launch generation: granule tags are gen * (max_iter + 1) + t + 1
    const float* Wq1;      // A    16x16x4-packed [2n][2N]
    const float* Wq2;      // A^H  16x16x4-packed [2N][2n]
    Partial* pparts;       // [max_iter][nwg] 32-B granule pairs
    double* pxch;          // [max_iter][nwg][4] rare-path exchange
    unsigned* pbar;        // [0] arrivals, [1] abort flag (zeroed by the prepare launch)
    int x3;                // persistent GEMMs on the bf16x3 engine (Wx1 / Wx2)
    const void* Wx1;       // A    X3-packed (x3_index, O = n, J = N)
    const void* Wx2;       // A^H  X3-packed (O = N, J = n)
    // launch engine, block-banded A (Lin > 1 or Lout > 1: the ISI / coupled channel): per column
    // tile of WA (128 wide) / WAH (bn wide) the reduction range holding its nonzero blocks
    const int* bandA;
    const int* bandB;
    // launch engine, bf16x3 tiles (amp_gemm_x3.h, lx3 = 1): WA / WAH hold the x3-packed operators
    // (x3_index), each GEMM's A rows split first into `lap` (six bf16 planes)
    int lx3, rows_pad;
    unsigned short* lap;
    XState* xs;            // trial-sharded exchange words (amp_scamp_run_sharded)
    // fused decision (amp_scamp_detect_count: decide_epilogue at the end of scamp_persist)
    int dec_on, ibits;
    const float2* xtrue;   // [B][N] transmitted x
    const long long* sym;  // [B*L] gray labels
    const long long* idx;  // [B*L] flat nonzero indices
    DecWG* dwg;            // per-workgroup records: [nwg] x 256 B of tagged granules (folded in the
                           // persistent kernel, amp_decide_fused.h dec_fold_gather)
    amp_counts* counts;    // out
    unsigned char* host_rec;   // optional page-locked host record (amp_vamp_decide_args.host_record)
    int fold_in;               // the persistent kernel folds the records itself (else vamp_decide_fold)
    unsigned long long* trace;   // diagnostic phase stamps (amp_scamp_persist_trace), else null
    // launch engine: rcnt[1] is scamp_fix_psi_fin's arrival counter (zeroed by scamp_init_kernel)
    unsigned* rcnt;
    Const c;
};

struct ScampWs {
    float *WA, *WAH, *z, *s, *phi, *tau, *psi1;
    float *secmax, *secabs;
    Partial* parts;
    ScampIter* iters;
    unsigned* psi_nc;
    float *Wq1, *Wq2, *Wx1, *Wx2;
    unsigned* pbar;
    Partial* pparts;
    double* pxch;
    int *bandA, *bandB;
    unsigned short* lap;
    XState* xs;
    DecWG* dwg;
    size_t bytes;
};

// the launch engine's bf16x3 tiles need whole 64-wide reduction groups and output tiles
inline bool scamp_lx3_shape(const amp_dims* d) { return d->N % 64 == 0 && d->n % 64 == 0; }

// 128 columns whenever a section fits (2M <= 128): twice the workgroups of a whole-coupling-
// block tile (cfg3: 256 instead of 128).
inline int scamp_bn(const amp_dims* d) { return section_bn(d); }
// psi is formed in the A^H tile's epilogue only where every tile holds whole coupling blocks (Nt
// divides the tile's bn / 2 complex columns: a power of two up to it); scamp_psi / tscamp_psi form it
// after the tiles otherwise (blocks wider than a tile, or whose boundaries fall inside tiles).
inline int scamp_psi_split(int bn, int Nt) { return (bn / 2) % Nt != 0 ? 1 : 0; }
inline int scamp_psi_nblk(const amp_dims* d) { return std::max(1, std::min(cdiv(d->B * d->Lin, AMP_WG / 64), 2048)); }

// tile geometry of `rows` rows sharing the operators of `d`
inline void scamp_geometry(const amp_dims* d, int rows, ScampK& P) {
    P.B = rows; P.N = d->N; P.n = d->n; P.L = d->L; P.M = d->M;
    P.Nt = d->Nt; P.Nr = d->Nr; P.Na = d->Na; P.Lin = d->Lin; P.Lout = d->Lout;
    P.bn = scamp_bn(d);
    P.kapA = round_up(2 * d->N, GBK); P.ncpA = round_up(2 * d->n, 128);
    P.kapB = round_up(2 * d->n, GBK); P.ncpB = round_up(2 * d->N, P.bn);
    P.nblk = cdiv(rows, GBM) * (P.ncpB / P.bn);
    P.psi_split = scamp_psi_split(P.bn, P.Nt);
}

bool scamp_persist_shape(const amp_dims* d);
bool scamp_persist_eligible(const amp_dims* d, int ncu);
bool scamp_persist_x3_fits(const amp_dims* d);

// The kernels index trials x columns, sections and coupling blocks with 32-bit products and the
// GEMM grids put the column tiles on gridDim.y: shapes beyond either are refused, never wrapped.
// (The packed operators' offsets, ncp * kap floats, are 64-bit throughout.)
inline bool scamp_index_ok(const amp_dims* d, int rows) {
    const long long cols = 2LL * std::max(d->N, d->n);
    return cols <= 0x7fffffffLL / 2 && (long long)rows * cols <= 0x7fffffffLL && cols / 128 + 1 <= 65535;
}

// Row stride of s = z / phi, the A operand of the A^H GEMM: 2n floats rounded up to the tile's
// float4 loads (n odd: two pad floats per row, zeroed once by the init kernels; the operator's
// reduction rows beyond 2n are zero).  z and y keep the caller's stride 2n.
__host__ __device__ inline int scamp_sld(int n) { return (2 * n + 3) & ~3; }

inline ScampWs scamp_carve(const amp_dims* d, int max_iter, void* base) {
    ScampK P;
    scamp_geometry(d, d->B, P);
    // the persistent engines' operators and exchange buffers only where a persistent engine can run
    // (no device query: the byte count is a function of the shape alone)
    const bool persist = scamp_persist_shape(d) || scamp_persist_x3_fits(d);
    Carve cv(base);
    ScampWs w;
    w.WA = cv.take<float>((size_t)P.ncpA * P.kapA);
    w.WAH = cv.take<float>((size_t)P.ncpB * P.kapB);
    w.z = cv.take<float>((size_t)d->B * 2 * d->n);
    w.s = cv.take<float>((size_t)d->B * scamp_sld(d->n));
    w.phi = cv.take<float>((size_t)2 * d->B * d->Lout);
    w.tau = cv.take<float>((size_t)d->B * d->Lin);
    w.psi1 = cv.take<float>((size_t)d->B * d->Lin);
    w.secmax = cv.take<float>((size_t)d->B * d->L);
    w.secabs = cv.take<float>((size_t)d->B * d->L);
    w.parts = cv.take<Partial>((size_t)max_iter * P.nblk);
    w.iters = cv.take<ScampIter>((size_t)max_iter + 1);
    w.psi_nc = cv.take<unsigned>((size_t)max_iter * scamp_psi_nblk(d));
    const int nwg = cdiv(d->B, 16);
    w.Wq1 = persist ? cv.take<float>((size_t)2 * d->n * 2 * d->N) : nullptr;
    w.Wq2 = persist ? cv.take<float>((size_t)2 * d->N * 2 * d->n) : nullptr;
    w.Wx1 = persist ? cv.take<float>((size_t)3 * d->n * d->N) : nullptr;    // 6 bf16 per complex entry
    w.Wx2 = persist ? cv.take<float>((size_t)3 * d->N * d->n) : nullptr;
    w.pxch = persist ? cv.take<double>((size_t)max_iter * nwg * 4) : nullptr;
    w.pbar = cv.take<unsigned>(64);            // [8 ..]: the launch engine's arrival counters
    w.pparts = persist ? cv.take<Partial>((size_t)max_iter * nwg) : nullptr;
    w.bandA = cv.take<int>((size_t)2 * (P.ncpA / 128));
    w.bandB = cv.take<int>((size_t)2 * (P.ncpB / P.bn));
    w.xs = cv.take<XState>(1);
    w.dwg = persist ? cv.take<DecWG>((size_t)2 * nwg) : nullptr;   // 256 B of granules per workgroup
    w.lap = scamp_lx3_shape(d) ? cv.take<unsigned short>((size_t)6 * round_up(d->B, GBM) * std::max(d->N, d->n))
                               : nullptr;
    w.bytes = cv.off;
    return w;
}

__device__ __forceinline__ float* spsi(const ScampK& P, int t) { return (t & 1) ? P.psi1 : P.psi0; }
__device__ __forceinline__ float* sphi(const ScampK& P, int t) { return P.phi + (size_t)(t & 1) * P.B * P.Lout; }

// gamma[lo] = (W psi)[lo] / Lc (scamp.py:45), float32 as torch's [Lout x Lin] @ [Lin] product
__device__ __forceinline__ float scamp_gamma(const ScampK& P, const float* psi_row, int lo) {
    float g = 0.f;
    for (int lc = 0; lc < P.Lin; ++lc) g += P.W[lo * P.Lin + lc] * psi_row[lc];
    return g / (float)P.Lin;
}

// sum |xmmse|^2 over one coupling block (scamp.py:59; torch abs = the correctly rounded hypot, then
// an f32 square) by one wavefront: lane-strided float64 partials, then group_sum; every lane
// returns the sum.  scamp_psi, tscamp_psi and the wide-block form of the float64 fix-up (Nt >
// SFIX_SERIAL_NT) all go through it, so there a block's psi has the same bits whichever kernel
// formed it.
__device__ __forceinline__ double scamp_block_energy(const float2* xr, int Nt) {
    double ssum = 0.0;
    for (int m = threadIdx.x & 63; m < Nt; m += 64) {
        const float2 v = xr[m];
        const float a = (float)sqrt((double)v.x * v.x + (double)v.y * v.y);   // torch abs (hypot)
        ssum += (double)(a * a);
    }
    return group_sum(ssum, 64);
}

// The fix-up kernels recompute a coupling block's psi with one thread per block up to this Nt (a
// serial float64 sum over the block), with one wavefront per block (scamp_block_energy) beyond it.
constexpr int SFIX_SERIAL_NT = 128;

// Whether one of the block's `spb` sections was recomputed by the float64 fix-up (wavefront-uniform)
__device__ __forceinline__ bool scamp_block_hit_wave(const float* secmax, int spb, double G, double slack) {
    bool hit = false;
    for (int j = threadIdx.x & 63; j < spb; j += 64) hit |= (double)secmax[j] - G < AMP_DANGER + slack;
    return __any(hit) != 0;
}

// The same sum by one thread, serially over m = 0 .. Nt - 1: psi formed in the A^H tile's epilogue
// and the narrow-block form of the float64 fix-up (Nt <= SFIX_SERIAL_NT)
__device__ __forceinline__ double scamp_block_energy_serial(const float2* xr, int Nt) {
    double ssum = 0.0;
    for (int m = 0; m < Nt; ++m) {
        const float2 v = xr[m];
        const float a = (float)sqrt((double)v.x * v.x + (double)v.y * v.y);   // torch abs (hypot)
        ssum += (double)(a * a);
    }
    return ssum;
}

// psi = 1 - sum_block |xmmse|^2 / Na (scamp.py:59) of coupling block `blk` of [B][Lin] from its
// energy, stored; returns the change of the block's allclose flag (scamp.py:105) against the psi
// the buffer held (`had`: a fix-up recomputing a block whose flag is already counted), else the flag
__device__ __forceinline__ int scamp_psi_store(const ScampK& P, int t, size_t blk, double ssum, bool had = false) {
    const float* psi_prev = spsi(P, t + 1);
    float* psi_new = spsi(P, t);
    const float ps = 1.0f - (float)ssum / (float)P.Na;
    const int d = (torch_close(ps, psi_prev[blk]) ? 0 : 1) - (had && !torch_close(psi_new[blk], psi_prev[blk]) ? 1 : 0);
    psi_new[blk] = ps;
    return d;
}

// The float64 fix-up's psi of coupling block `blk` of [B][Lin], recomputed if one of its sections
// was; returns the allclose delta.  _wave: by one wavefront (blocks wider than SFIX_SERIAL_NT, in
// scamp_psi's summation order; lane 0 holds the delta), _serial: by one thread.
__device__ __forceinline__ int scamp_fix_psi_wave(const ScampK& P, int t, size_t blk, const ScampIter& pend) {
    const int spb = P.Nt / P.M;   // sections per coupling block
    if (!scamp_block_hit_wave(P.secmax + blk * spb, spb, pend.G, pend.slack)) return 0;
    const double ssum = scamp_block_energy(reinterpret_cast<const float2*>(P.xm) + blk * P.Nt, P.Nt);
    return (threadIdx.x & 63) == 0 ? scamp_psi_store(P, t, blk, ssum, true) : 0;
}
__device__ __forceinline__ int scamp_fix_psi_serial(const ScampK& P, int t, size_t blk, const ScampIter& pend) {
    const int spb = P.Nt / P.M;
    bool hit = false;
    for (int j = 0; j < spb && !hit; ++j) hit = (double)P.secmax[blk * spb + j] - pend.G < AMP_DANGER + pend.slack;
    if (!hit) return 0;
    const float2* xr = reinterpret_cast<const float2*>(P.xm) + blk * P.Nt;
    return scamp_psi_store(P, t, blk, scamp_block_energy_serial(xr, P.Nt), true);
}

// The f32 operators, MFMA-packed, and their band ranges (Tracker: A, A^H, scamp.py:12-13)
inline int scamp_pack_f32(const ScampK& P, const float2* A, hipStream_t st) {
    int rc;
    if ((rc = build_cweight(A, P.N, 1, 0, nullptr, P.n, P.N, (float*)P.WA, P.kapA, P.ncpA, st))) return rc;
    if ((rc = build_cweight(A, 1, P.N, 1, nullptr, P.N, P.n, (float*)P.WAH, P.kapB, P.ncpB, st))) return rc;
    if (!P.bandA) return AMP_OK;
    if ((rc = weight_kband(P.WA, P.kapA, P.ncpA, 128, const_cast<int*>(P.bandA), st))) return rc;
    return weight_kband(P.WAH, P.kapB, P.ncpB, P.bn, const_cast<int*>(P.bandB), st);
}

// Tracker (scamp.py:9-25) of every row: z = y, psi = 1, phi = inf, xmmse = 0; a grid-stride body
// (the engines' init kernels add their records)
__device__ __forceinline__ void scamp_init_state(const ScampK& P) {
    const size_t BN_ = (size_t)P.B * P.N, Bn = (size_t)P.B * P.n, BL = (size_t)P.B * P.Lout, Bl = (size_t)P.B * P.Lin;
    const size_t tot = std::max(std::max(BN_, Bn), std::max(BL, Bl));
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
        if (e < BN_) reinterpret_cast<float2*>(P.xm)[e] = make_float2(0.f, 0.f);
        if (e < Bn) reinterpret_cast<float2*>(P.z)[e] = reinterpret_cast<const float2*>(P.y)[e];
        if (e < Bl) P.psi1[e] = 1.0f;
        if (e < BL) P.phi[BL + e] = INFINITY;        // phi buffer of "iteration -1"
        if (e < (size_t)P.B)                         // the pad of an odd n's s rows (scamp_sld)
            for (int k = 2 * P.n; k < scamp_sld(P.n); ++k) P.s[e * scamp_sld(P.n) + k] = 0.f;
    }
}

// A record with no fix-up pending
__device__ __forceinline__ ScampIter scamp_iter(int stopped, int T, int fixed, int fixed_all, uint32_t notclose) {
    ScampIter it;
    it.stopped = stopped; it.T = T; it.fixed = fixed; it.fixed_all = fixed_all;
    it.G = 0.0; it.slack = 0.0; it.notclose = notclose; it.active = 0; it.pad[0] = it.pad[1] = 0;
    return it;
}

// A record with the exact float64 fix-up of iteration t pending
__device__ __forceinline__ ScampIter scamp_pending(int t, double G, double slack, uint32_t notclose) {
    ScampIter it = scamp_iter(0, t + 1, 0, 0, notclose);
    it.G = G; it.slack = slack; it.active = 1;
    return it;
}

// The record after iteration t (scamp.py:105: early exit when no psi moved beyond allclose) into
// *rec and, when the forward ends there, its status into *status; returns whether it stopped
__device__ __forceinline__ bool scamp_record(const ScampK& P, ScampIter* rec, amp_status* status, int t,
                                             uint32_t notclose, int fixed, int fixed_all) {
    const ScampIter nx = scamp_iter(notclose == 0 ? 1 : 0, t + 1, fixed, fixed_all, notclose);
    *rec = nx;
    if (nx.stopped || t + 1 == P.max_iter) {
        amp_status s;
        s.T = t + 1; s.nan_state = fixed != 0 ? 1 : 0; s.stopped = nx.stopped;
        s.gemm = P.lx3 ? AMP_ARITH_BF16X3 : AMP_ARITH_F32;
        s.last_scalar[0] = s.last_scalar[1] = s.last_scalar[2] = s.last_scalar[3] = 0.f;
        *status = s;
    }
    return nx.stopped != 0;
}

// One section for the exact float64 fix-up (section_absmax_f64 / exact_section_f64), o0 its first
// position in [B][N]: the loader (xmap and 1 / (tau / 2) of its coupling block) and the store (xmmse)
struct ScampSectionLoad {
    const float2* xp2;
    float tv;
    __device__ __forceinline__ void operator()(int m, float& rr, float& ri, float& it) const {
        const float2 v = xp2[m];
        rr = v.x; ri = v.y; it = 1.0f / (tv * 0.5f);
    }
};
struct ScampSectionStore {
    float2* x2;
    __device__ __forceinline__ void operator()(int m, float xr, float xi, float) const { x2[m] = make_float2(xr, xi); }
};
__device__ __forceinline__ ScampSectionLoad scamp_section_load(const ScampK& P, size_t o0) {
    const int b = (int)(o0 / (size_t)P.N), lc = (int)((o0 % (size_t)P.N) / P.Nt);
    return ScampSectionLoad{reinterpret_cast<const float2*>(P.xmap) + o0, P.tau[(size_t)b * P.Lin + lc]};
}
__device__ __forceinline__ ScampSectionStore scamp_section_store(const ScampK& P, size_t o0) {
    return ScampSectionStore{reinterpret_cast<float2*>(P.xm) + o0};
}

// ---- the GEMM epilogues of the launch engine (amp_scamp.hip) and the independent-trial engine
// (amp_scamp_trials.hip): `lds` holds the C tile, g is the engine's row guard (amp_trials.h) ----

// z = y - A xmmse + b z ; phi = sigma2 + gamma ; s = z / phi   (scamp.py:45-51, 57)
template <int KC, class G>
__device__ __forceinline__ void scamp_residual(const ScampK& P, const G& g, int t, float* lds, int row0, int col0) {
    using C = GemmCfg<128, KC>;
    const int twon = 2 * P.n, sld = scamp_sld(P.n);
    const float* psi = spsi(P, t + 1);               // psi of iteration t-1 (ones at t = 0)
    const float* phi_old = sphi(P, t + 1);           // +inf at t = 0 (scamp.py:19)
    float* phi_new = sphi(P, t);
    // gamma of each (trial, output block) the tile touches, formed once (the same float32 sum as
    // scamp_gamma) instead of once per element: Lin MACs of global loads per element had made the
    // epilogue, not the GEMM, the cost of a Lin > 1 tile
    // The rows' psi and the W rows come into LDS first (coalesced), so the serial float32 sums
    // read LDS, not a chain of dependent global loads.
    const int lo0 = (col0 >> 1) / P.Nr, nlo = (min((col0 >> 1) + 63, P.n - 1)) / P.Nr - lo0 + 1;
    const int Lin = P.Lin;
    float* sg = lds + C::CTILE_FLOATS;                 // [GBM][nlo] gamma
    float* sp = sg + GBM * nlo;                        // [GBM][Lin] psi rows
    float* sw = sp + GBM * Lin;                        // [nlo][Lin] W rows lo0 ..
    const bool per_block = C::CTILE_FLOATS + GBM * nlo + GBM * Lin + nlo * Lin <= C::A_FLOATS;
    if (per_block) {
        for (int e = threadIdx.x; e < GBM * Lin; e += AMP_WG) {
            const int row = row0 + e / Lin;
            sp[e] = row < P.B ? psi[(size_t)row0 * Lin + e] : 0.f;
        }
        for (int e = threadIdx.x; e < nlo * Lin; e += AMP_WG) sw[e] = P.W[(size_t)lo0 * Lin + e];
        __syncthreads();
        for (int e = threadIdx.x; e < GBM * nlo; e += AMP_WG) {
            const int rho = e / nlo, j = e - rho * nlo;
            float gm = 0.f;                            // scamp_gamma's sum, in its order
            for (int lc = 0; lc < Lin; ++lc) gm += sw[j * Lin + lc] * sp[rho * Lin + lc];
            sg[e] = gm / (float)Lin;
        }
        __syncthreads();
    }
    // Every global load of this thread's elements is issued before any store: the stores to z / s
    // may alias the next element's loads as far as the compiler knows, and a load-compute-store loop
    // waited a full memory latency per element (each element reads and writes only its own z).
    constexpr int IT = GBM * 64 / AMP_WG;
    float2 yv[IT], zv[IT];
    float po[IT];
#pragma unroll
    for (int u = 0; u < IT; ++u) {
        // unconditional loads at a clamped index (a lane-divergent branch around them serialises
        // their latencies, amp_gemm.h ALoadPlain); out-of-range elements are never stored
        const int e = threadIdx.x + u * AMP_WG;
        const int rho = e >> 6, cp = e & 63;
        const int row = min(row0 + rho, P.B - 1), i = min((col0 >> 1) + cp, P.n - 1);
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
        if (row < P.B && i < P.n && g.live(rho)) {
            const int lo = i / P.Nr;
            const float gma = per_block ? sg[rho * nlo + lo - lo0] : scamp_gamma(P, psi + (size_t)row * P.Lin, lo);
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

// The coupling blocks an A^H tile of ncols columns at col0 covers: lc0 .. lc0 + ntc - 1 (nlc whole
// blocks where psi is formed in the tile)
struct ScampTileBlocks {
    int lc0, nlc, ntc;
};
__device__ __forceinline__ ScampTileBlocks scamp_tile_blocks(const ScampK& P, int col0, int ncols) {
    ScampTileBlocks b;
    b.lc0 = (col0 / 2) / P.Nt;
    b.nlc = max(1, (ncols / 2) / P.Nt);
    b.ntc = (col0 / 2 + ncols / 2 - 1) / P.Nt - b.lc0 + 1;
    return b;
}

// tau = L / (W^T (1/phi)) / Mr of the tile's rows and blocks into LDS (returned: [GBM][ntc], past
// the guard's partial-store scratch; each tau is also written to P.tau by the tile that holds its
// block's first column), then xmap = xmmse + tau (A^H s)   (scamp.py:53-57), stored and left in the
// C tile for the denoiser.  Ends with a barrier.
template <int BN, int KC, class G>
__device__ __forceinline__ float* scamp_xmap(const ScampK& P, const G& g, int t, float* lds, int row0, int col0, int nrows,
                                             int ncols, const ScampTileBlocks& tb) {
    using C = GemmCfg<BN, KC>;
    const int twoN = 2 * P.N, lc0 = tb.lc0, ntc = tb.ntc;
    float* tau_t = lds + C::CTILE_FLOATS + G::PSCR;                          // [32][ntc]
    const float* phi = sphi(P, t);
    // the rows' 1 / phi and the W columns lc0 .. into LDS first (coalesced): the serial float32
    // sums then read LDS instead of a chain of dependent global loads
    const int Lout = P.Lout;
    float* siph = tau_t + GBM * ntc;                                         // [32][Lout] 1 / phi
    float* swc = siph + GBM * Lout;                                          // [ntc][Lout] W columns
    const bool staged = C::CTILE_FLOATS + G::PSCR + GBM * ntc + GBM * Lout + ntc * Lout <= C::A_FLOATS;
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
            if (lc * P.Nt >= col0 / 2 && g.live(rho)) P.tau[(size_t)(row0 + rho) * P.Lin + lc] = tv;
        }
        tau_t[e] = tv;
    }
    __syncthreads();
    // xmmse of every element of this thread first (the xmap stores may alias them as far as
    // the compiler knows: one load latency per element otherwise)
    constexpr int IT = GBM * BN / AMP_WG;
    float xv[IT];
#pragma unroll
    for (int u = 0; u < IT; ++u) {
        // unconditional loads at a clamped index (see scamp_residual); out-of-range elements unused
        const int e = threadIdx.x + u * AMP_WG, rho = min(e / BN, nrows - 1), cc = min(e % BN, ncols - 1);
        xv[u] = P.xm[(size_t)(row0 + rho) * twoN + col0 + cc];
    }
#pragma unroll
    for (int u = 0; u < IT; ++u) {
        const int e = threadIdx.x + u * AMP_WG, rho = e / BN, cc = e % BN;
        if (rho < nrows && cc < ncols && g.live(rho)) {
            const size_t o = (size_t)(row0 + rho) * twoN + col0 + cc;
            const float tv = tau_t[rho * ntc + ((col0 + cc) >> 1) / P.Nt - lc0];
            const float xp = xv[u] + tv * lds[rho * C::LDC + cc];
            P.xmap[o] = xp;
            lds[rho * C::LDC + cc] = xp;
        }
    }
    __syncthreads();
    return tau_t;
}

struct ScampDenoisePolicy {
    const float* tile;
    const float* tau_tile;   // LDS [rows][Lin] tau of the tile's rows and blocks lc0 .. lc0 + Lin - 1
    int ldc, spr, M, N, Nt, L, row0, colc0, Lin, lc0;
    float* xm;
    float* secmax;
    float* secabs;
    __device__ __forceinline__ void load(int sec, int m, float& rr, float& ri, float& it) const {
        const int rho = sec / spr, sj = sec - rho * spr;
        const int cc = sj * M + m;
        const float2 v = *reinterpret_cast<const float2*>(tile + rho * ldc + 2 * cc);
        rr = v.x; ri = v.y;
        it = 1.0f / (tau_tile[rho * Lin + (colc0 + cc) / Nt - lc0] * 0.5f);   // tau_use / 2 (scamp.py:63)
    }
    __device__ __forceinline__ void store(int sec, int m, float xr, float xi, float, PartAcc&) const {
        const int rho = sec / spr, sj = sec - rho * spr;
        const size_t o = (size_t)(row0 + rho) * N + colc0 + sj * M + m;
        *reinterpret_cast<float2*>(xm + 2 * o) = make_float2(xr, xi);
    }
    __device__ __forceinline__ void section(int sec, float smax, float sabs) const {
        const int rho = sec / spr, sj = sec - rho * spr;
        const size_t o = (size_t)(row0 + rho) * L + (colc0 / M) + sj;
        secmax[o] = smax;
        secabs[o] = sabs;
    }
};

// The denoiser's view of the tile rows from rho on (scamp_xmap's C tile and tau tile): the whole
// tile at rho = 0 (the launch engine: nrows * spr sections), one row when only spr sections are
// denoised (the trial engine: sec / spr is then 0 and every address the same integer as the
// B = 1 forward's, whose tile has that one row)
template <int BN, int KC>
__device__ __forceinline__ ScampDenoisePolicy scamp_policy(const ScampK& P, const float* lds, const float* tau_t,
                                                           int row0, int col0, int ncols, const ScampTileBlocks& tb,
                                                           int rho) {
    using C = GemmCfg<BN, KC>;
    ScampDenoisePolicy pol;
    pol.tile = lds + rho * C::LDC; pol.tau_tile = tau_t + rho * tb.ntc; pol.ldc = C::LDC;
    pol.M = P.M; pol.N = P.N; pol.Nt = P.Nt; pol.L = P.L;
    pol.spr = (ncols / 2) / P.M; pol.row0 = row0 + rho; pol.colc0 = col0 / 2; pol.Lin = tb.ntc; pol.lc0 = tb.lc0;
    pol.xm = P.xm; pol.secmax = P.secmax; pol.secabs = P.secabs;
    return pol;
}

// psi of coupling block lc of `row` from the freshly written xmmse of its tile, by one thread;
// returns its allclose flag
__device__ __forceinline__ unsigned scamp_psi_in_tile(const ScampK& P, int t, int row, int lc) {
    const float2* xr = reinterpret_cast<const float2*>(P.xm) + (size_t)row * P.N + (size_t)lc * P.Nt;
    return (unsigned)scamp_psi_store(P, t, (size_t)row * P.Lin + lc, scamp_block_energy_serial(xr, P.Nt));
}

int scamp_persist_launch(const ScampK& P, const DecConst& dc, hipStream_t st);

}  // namespace amp

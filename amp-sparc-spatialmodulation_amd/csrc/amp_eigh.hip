// amp_eigh.hip — batched Hermitian eigensolver for stacks of Gram matrices (amp_eigh_run): a cyclic
// one-sided (Hestenes) Jacobi iteration in float64.  It replaces torch.linalg.eigh inside
// model.svd_gram, which stands in for the reference's per-channel torch.linalg.svd
// (vamp_model.py:57-58); rocSOLVER runs the channels of a stack one after another, this runs them
// side by side.
//
// The columns g_c of G = V diag(w) V^H are rotated in pairs until they are mutually orthogonal: then
// G J = J diag(w) for the accumulated unitary J, so the columns ARE w_j J_j: eigenvalue = column
// norm, eigenvector = normalised column, and no separate J is kept.  Pair (p, q) with a = |g_p|^2,
// b = |g_q|^2, c = g_p^H g_q is rotated when |c| > tol sqrt(a b):
//     zeta = (b - a) / (2 |c|),  t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)),
//     cs = 1 / sqrt(1 + t^2),  sn = cs t,  ph = c / |c|,
//     g_p' = cs g_p - sn conj(ph) g_q,   g_q' = sn ph g_p + cs g_q.
// All arithmetic is float64, plain C++ (the Makefile's -ffp-contract=off holds here too).  Complex64
// arithmetic leaves the factors 20 to 50 times less orthogonal.
//
// Work matrix: X [batch][k][k] in the workspace, row c = column c of G (= conj of G's row c), so a
// column is one contiguous run of k complex128.  Columns are grouped in blocks of BW (a last block
// may be partial; with an odd block count a phantom block pads the round-robin: columns that do not
// exist are never rotated and never returned).  One sweep = one plain launch per round:
//   round W     grid (blocks) x batch: a workgroup holds ONE block in LDS and rotates every pair
//               inside it, BW - 1 inner rounds of BW / 2 disjoint pairs, one wave per pair;
//   rounds 0 .. nbe - 2 (nbe = block count made even)   grid (nbe / 2 block pairs of the round-robin)
//               x batch: a workgroup takes blocks (I, J); wave i keeps column I BW + i in registers
//               for the whole round, block J lies in LDS, and inner round t rotates the BW disjoint
//               pairs (I BW + i, J BW + (i + t) % BW), a workgroup barrier between inner rounds.
// Nothing waits on another workgroup: no persistent grid, no cooperative launch, no exchange buffer
// (DESIGN.md §3.8 tells what those cost).  A complex128 column in LDS is read and written as
// {re, im} double2, lane l at element l + 64 j: 16 contiguous bytes per lane, which the LDS serves
// in conflict-free groups of 8 lanes at any column stride.
//
// Convergence is per matrix: every wave adds its rotations to rot[sweep][matrix] (global atomicAdd);
// a workgroup of sweep s + 1 returns at once when its matrix's count of sweep s is 0, so a finished
// matrix costs nothing more and does not change whatever its neighbours do.
#include "amp_host.h"

#include <vector>

namespace amp {

constexpr int EIGH_MAX_K = AMP_EIGH_MAX_K;
constexpr int EIGH_MAX_SWEEPS = AMP_EIGH_MAX_SWEEPS;

struct EighK {
    int k, batch, sweep, round, nb, nbe;
    double tol;
    double2* X;     // [batch][k][k]
    int* rot;       // [EIGH_MAX_SWEEPS][batch]
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave, one pair: the columns lie in registers (lane l holds elements l + 64 j; elements past k
// are zeros).  Returns 1 when the pair was rotated.  Every lane computes the same scalars.
template <int NCH>
__device__ __forceinline__ int rotate_pair(double2 (&xp)[NCH], double2 (&xq)[NCH], double tol) {
    double a = 0.0, b = 0.0, cr = 0.0, ci = 0.0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        a += xp[j].x * xp[j].x + xp[j].y * xp[j].y;
        b += xq[j].x * xq[j].x + xq[j].y * xq[j].y;
        cr += xp[j].x * xq[j].x + xp[j].y * xq[j].y;     // c = conj(g_p) . g_q
        ci += xp[j].x * xq[j].y - xp[j].y * xq[j].x;
    }
    a = wave_sum(a); b = wave_sum(b); cr = wave_sum(cr); ci = wave_sum(ci);
    const double cabs = sqrt(cr * cr + ci * ci);
    if (!(cabs > tol * sqrt(a * b))) return 0;
    const double zeta = (b - a) / (2.0 * cabs);
    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
    const double sr = sn * (cr / cabs), si = sn * (ci / cabs);   // sn ph
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const double2 p = xp[j], q = xq[j];
        // g_p' = cs p - conj(sn ph) q;  g_q' = (sn ph) p + cs q
        xp[j] = make_double2(cs * p.x - (sr * q.x + si * q.y), cs * p.y - (sr * q.y - si * q.x));
        xq[j] = make_double2((sr * p.x - si * p.y) + cs * q.x, (sr * p.y + si * p.x) + cs * q.y);
    }
    return 1;
}

template <int NCH>
__device__ __forceinline__ void col_load(double2 (&x)[NCH], const double2* src, int lane, int k) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int e = lane + 64 * j;
        x[j] = e < k ? src[e] : make_double2(0.0, 0.0);
    }
}

template <int NCH>
__device__ __forceinline__ void col_store(const double2 (&x)[NCH], double2* dst, int lane, int k) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int e = lane + 64 * j;
        if (e < k) dst[e] = x[j];
    }
}

// Block pair g of round r in the round-robin over nbe (even) blocks: the circle method.
__device__ __forceinline__ void block_pair(int g, int r, int nbe, int& I, int& J) {
    const int m = nbe - 1;
    if (g == 0) { I = m; J = r; }
    else { I = (r + g) % m; J = (r - g + m) % m; }
    if (I > J) { const int s = I; I = J; J = s; }
}

// Rounds 0 .. nbe - 2: workgroup (g, matrix), BW waves.
template <int NCH, int BW>
__global__ __launch_bounds__(64 * BW) void eigh_cross_kernel(EighK P) {
    extern __shared__ double2 eigh_lds[];              // [BW][k]: block J
    const int mat = blockIdx.y;
    if (P.sweep > 0 && P.rot[(P.sweep - 1) * P.batch + mat] == 0) return;
    int I, J;
    block_pair(blockIdx.x, P.round, P.nbe, I, J);
    if (J >= P.nb) return;                              // the phantom block
    const int k = P.k, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double2* X = P.X + (size_t)mat * k * k;
    const int nq = min(BW, k - J * BW);                 // columns of block J that exist
    {
        const double2* src = X + (size_t)J * BW * k;
        for (int e = threadIdx.x; e < nq * k; e += 64 * BW) eigh_lds[e] = src[e];
    }
    const int p = I * BW + wv;                          // I < J: block I is never partial
    double2 xp[NCH], xq[NCH];
    col_load<NCH>(xp, X + (size_t)p * k, lane, k);
    __syncthreads();
    int cnt = 0;
    for (int t = 0; t < BW; ++t) {
        const int qs = (wv + t) % BW;
        if (qs < nq) {
            double2* q = eigh_lds + qs * k;
            col_load<NCH>(xq, q, lane, k);
            if (rotate_pair<NCH>(xp, xq, P.tol)) {
                col_store<NCH>(xq, q, lane, k);
                ++cnt;
            }
        }
        __syncthreads();
    }
    if (cnt) {
        col_store<NCH>(xp, X + (size_t)p * k, lane, k);
        if (lane == 0) atomicAdd(&P.rot[P.sweep * P.batch + mat], cnt);
    }
    if (__syncthreads_or(cnt)) {                        // block J goes back when any wave rotated
        double2* dst = X + (size_t)J * BW * k;
        for (int e = threadIdx.x; e < nq * k; e += 64 * BW) dst[e] = eigh_lds[e];
    }
}

// Round W: workgroup (block, matrix), BW / 2 waves, every pair inside the block.
template <int NCH, int BW>
__global__ __launch_bounds__(32 * BW) void eigh_within_kernel(EighK P) {
    extern __shared__ double2 eigh_lds[];              // [BW][k]
    const int mat = blockIdx.y;
    if (P.sweep > 0 && P.rot[(P.sweep - 1) * P.batch + mat] == 0) return;
    const int k = P.k, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c0 = blockIdx.x * BW, nc = min(BW, k - c0);
    if (nc < 2) return;
    double2* X = P.X + ((size_t)mat * k + c0) * k;
    for (int e = threadIdx.x; e < nc * k; e += 32 * BW) eigh_lds[e] = X[e];
    __syncthreads();
    double2 xp[NCH], xq[NCH];
    int cnt = 0;
    constexpr int m = BW - 1;
    for (int t = 0; t < m; ++t) {
        int ps, qs;
        if (wv == 0) { ps = m; qs = t; }
        else { ps = (t + wv) % m; qs = (t - wv + m) % m; }
        if (ps > qs) { const int s = ps; ps = qs; qs = s; }
        if (qs < nc) {
            double2* p = eigh_lds + ps * k;
            double2* q = eigh_lds + qs * k;
            col_load<NCH>(xp, p, lane, k);
            col_load<NCH>(xq, q, lane, k);
            if (rotate_pair<NCH>(xp, xq, P.tol)) {
                col_store<NCH>(xp, p, lane, k);
                col_store<NCH>(xq, q, lane, k);
                ++cnt;
            }
        }
        __syncthreads();
    }
    if (cnt && lane == 0) atomicAdd(&P.rot[P.sweep * P.batch + mat], cnt);
    if (__syncthreads_or(cnt))
        for (int e = threadIdx.x; e < nc * k; e += 32 * BW) X[e] = eigh_lds[e];
}

// X row c = column c of G = conj(G row c) (G is Hermitian: only its rows are read, along the fastest index)
__global__ __launch_bounds__(256) void eigh_init_kernel(const double2* __restrict__ G, double2* __restrict__ X, size_t count) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) {
        const double2 g = G[i];
        X[i] = make_double2(g.x, -g.y);
    }
}

struct EighCloseK {
    int k, batch, max_sweeps;
    const double2* X;
    const int* rot;
    double* w;        // [batch][k]
    int* info;        // [batch][2]
    int* src;         // [batch][k]: the column that has rank j
    double* inv;      // [batch][k]: 1 / its norm (0 for a zero column)
};

// Closing kernel, one workgroup per matrix: column norms -> w, ranks by counting (descending, ties by
// column index), info.  The normalised columns are written by eigh_write_kernel over a grid of tiles.
__global__ __launch_bounds__(256) void eigh_close_kernel(EighCloseK P) {
    __shared__ double nrm[EIGH_MAX_K];
    const int mat = blockIdx.x, k = P.k, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double2* X = P.X + (size_t)mat * k * k;
    for (int c = wv; c < k; c += 4) {
        const double2* x = X + (size_t)c * k;
        double a = 0.0;
        for (int e = lane; e < k; e += 64) a += x[e].x * x[e].x + x[e].y * x[e].y;
        a = wave_sum(a);
        if (lane == 0) nrm[c] = sqrt(a);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < k; c += 256) {
        const double v = nrm[c];
        int rank = 0;
        for (int o = 0; o < k; ++o) rank += (nrm[o] > v || (nrm[o] == v && o < c)) ? 1 : 0;
        P.w[(size_t)mat * k + rank] = v;
        P.src[(size_t)mat * k + rank] = c;
        P.inv[(size_t)mat * k + rank] = v > 0.0 ? 1.0 / v : 0.0;
    }
    if (threadIdx.x == 0) {
        int sweeps = P.max_sweeps, conv = 0;
        for (int s = 0; s < P.max_sweeps; ++s)
            if (P.rot[s * P.batch + mat] == 0) { sweeps = s + 1; conv = 1; break; }
        double lo = nrm[0], hi = nrm[0];
        for (int c = 1; c < k; ++c) { lo = fmin(lo, nrm[c]); hi = fmax(hi, nrm[c]); }
        if (!(lo > hi * 0x1p-40)) conv = 0;           // eigenvectors are not defined below 2^-40 w_max
        P.info[2 * mat] = sweeps;
        P.info[2 * mat + 1] = conv;
    }
}

// E[i][j] = X[src[j]][i] inv[j]: tile (32 i) x (32 j) of matrix z through LDS, reads along i, writes along j
__global__ __launch_bounds__(256) void eigh_write_kernel(EighCloseK P, double2* __restrict__ E) {
    __shared__ double2 tile[32][33];
    const int mat = blockIdx.z, k = P.k, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
    const double2* X = P.X + (size_t)mat * k * k;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = j0 + ty + 8 * q, i = i0 + tx;
        if (j < k && i < k) {
            const double s = P.inv[(size_t)mat * k + j];
            // clamped: with NaN norms the ranks are no permutation and a src entry may never have been written
            const int c = min(max(P.src[(size_t)mat * k + j], 0), k - 1);
            const double2 v = X[(size_t)c * k + i];
            tile[ty + 8 * q][tx] = make_double2(v.x * s, v.y * s);
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = i0 + ty + 8 * q, j = j0 + tx;
        if (i < k && j < k) E[((size_t)mat * k + i) * k + j] = tile[tx][ty + 8 * q];
    }
}

// Block width: 8 columns (eight waves per block pair, at most 80 KiB of LDS, so two workgroups fit a
// CU at any k).  Other widths are not measured in the committed records.
constexpr int EIGH_BW = 8;
static int eigh_readback = 1;       // amp_eigh_debug_readback

struct EighWs {
    double2* X;
    int* rot;
    int* src;
    double* inv;
    size_t bytes;
};

static EighWs eigh_carve(void* base, int k, int batch) {
    Carve cv(base);
    EighWs w;
    w.X = cv.take<double2>((size_t)batch * k * k);
    w.rot = cv.take<int>((size_t)EIGH_MAX_SWEEPS * batch);
    w.src = cv.take<int>((size_t)batch * k);
    w.inv = cv.take<double>((size_t)batch * k);
    w.bytes = align_up(cv.off, 256);
    return w;
}

// set_attr: the first launch of each kernel in a call asks for its dynamic LDS (above 64 KiB from
// k = 513 on); per call and not cached, so a process that runs the solver on several devices is served.
template <int NCH>
static hipError_t eigh_round(const EighK& P, bool within, bool set_attr, hipStream_t st) {
    constexpr int BW = EIGH_BW;
    const size_t lds = (size_t)BW * P.k * sizeof(double2);
    if (set_attr) {
        const void* fn = within ? (const void*)eigh_within_kernel<NCH, BW> : (const void*)eigh_cross_kernel<NCH, BW>;
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    if (within)
        hipLaunchKernelGGL((eigh_within_kernel<NCH, BW>), dim3(P.nb, P.batch), dim3(32 * BW), lds, st, P);
    else
        hipLaunchKernelGGL((eigh_cross_kernel<NCH, BW>), dim3(P.nbe / 2, P.batch), dim3(64 * BW), lds, st, P);
    return hipGetLastError();
}

static hipError_t eigh_round_k(const EighK& P, bool within, bool set_attr, hipStream_t st) {
    const int nch = cdiv(P.k, 64);
    if (nch <= 1) return eigh_round<1>(P, within, set_attr, st);
    if (nch <= 2) return eigh_round<2>(P, within, set_attr, st);
    if (nch <= 3) return eigh_round<3>(P, within, set_attr, st);
    if (nch <= 4) return eigh_round<4>(P, within, set_attr, st);
    if (nch <= 6) return eigh_round<6>(P, within, set_attr, st);
    if (nch <= 8) return eigh_round<8>(P, within, set_attr, st);
    if (nch <= 9) return eigh_round<9>(P, within, set_attr, st);
    return eigh_round<10>(P, within, set_attr, st);
}

static bool eigh_sizes_ok(int32_t k, int32_t batch) {
    return k >= 1 && k <= EIGH_MAX_K && batch >= 1 && batch <= 65535;
}

}  // namespace amp

using namespace amp;

extern "C" {

size_t amp_eigh_workspace_bytes(int32_t k, int32_t batch) {
    if (!eigh_sizes_ok(k, batch)) return 0;
    return eigh_carve(nullptr, k, batch).bytes;
}

int amp_eigh_debug_readback(int32_t on) {
    eigh_readback = on != 0;
    return AMP_OK;
}

int amp_eigh_run(const amp_eigh_args* a, int32_t k, int32_t batch, void* stream) {
    AMP_REQUIRE(a, "amp_eigh_run: null arguments");
    AMP_REQUIRE(k >= 1 && k <= EIGH_MAX_K, "amp_eigh_run: k = %d outside [1, %d]", k, EIGH_MAX_K);
    AMP_REQUIRE(batch >= 1 && batch <= 65535, "amp_eigh_run: batch = %d outside [1, 65535] (a grid axis)", batch);
    AMP_REQUIRE(a->G && a->E && a->w && a->info && a->workspace, "amp_eigh_run: null pointer argument");
    AMP_REQUIRE(a->tol >= 0.0, "amp_eigh_run: tol = %g must not be negative (0: 1e-9)", a->tol);   // NaN refused too
    AMP_REQUIRE(a->max_sweeps >= 0 && a->max_sweeps <= EIGH_MAX_SWEEPS, "amp_eigh_run: max_sweeps = %d outside [0, %d]",
                a->max_sweeps, EIGH_MAX_SWEEPS);
    const EighWs ws = eigh_carve(a->workspace, k, batch);
    AMP_REQUIRE(a->workspace_bytes >= ws.bytes, "amp_eigh_run: workspace of %zu bytes, %zu needed", a->workspace_bytes,
                ws.bytes);
    hipStream_t st = (hipStream_t)stream;
    const int max_sweeps = a->max_sweeps ? a->max_sweeps : EIGH_MAX_SWEEPS;
    const int bw = EIGH_BW;
    EighK P;
    P.k = k; P.batch = batch; P.sweep = 0; P.round = 0;
    P.nb = cdiv(k, bw);
    P.nbe = P.nb + (P.nb & 1);
    P.tol = a->tol > 0.0 ? a->tol : 1e-9;
    P.X = ws.X;
    P.rot = ws.rot;
    hipError_t e = hipMemsetAsync(ws.rot, 0, (size_t)EIGH_MAX_SWEEPS * batch * sizeof(int), st);
    if (e != hipSuccess) { set_error("amp_eigh_run: hipMemsetAsync: %s", hipGetErrorString(e)); return AMP_E_LAUNCH; }
    const size_t count = (size_t)batch * k * k;
    hipLaunchKernelGGL(eigh_init_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (const double2*)a->G,
                       ws.X, count);
    AMP_LAUNCH_CHECK("eigh_init");
    // the host may look at a sweep's counts to stop launching (never while the stream is captured)
    bool look = eigh_readback != 0;
    if (look) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); look = false; }
        else if (cs != hipStreamCaptureStatusNone) look = false;
    }
    std::vector<int> host;
    for (int s = 0; s < max_sweeps; ++s) {
        P.sweep = s;
        P.round = 0;
        e = eigh_round_k(P, true, s == 0, st);
        for (int r = 0; e == hipSuccess && P.nb > 1 && r < P.nbe - 1; ++r) {
            P.round = r;
            e = eigh_round_k(P, false, s == 0 && r == 0, st);
        }
        if (e != hipSuccess) { set_error("amp_eigh_run: sweep %d: %s", s, hipGetErrorString(e)); return AMP_E_LAUNCH; }
        if (look && s >= 8 && s + 1 < max_sweeps) {
            host.resize(batch);
            e = hipMemcpyAsync(host.data(), ws.rot + (size_t)s * batch, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) { set_error("amp_eigh_run: count read-back: %s", hipGetErrorString(e)); return AMP_E_LAUNCH; }
            bool done = true;
            for (int m = 0; m < batch; ++m) done = done && host[m] == 0;
            if (done) break;
        }
    }
    EighCloseK C;
    C.k = k; C.batch = batch; C.max_sweeps = max_sweeps;
    C.X = ws.X; C.rot = ws.rot; C.w = (double*)a->w; C.info = (int*)a->info; C.src = ws.src; C.inv = ws.inv;
    hipLaunchKernelGGL(eigh_close_kernel, dim3(batch), dim3(256), 0, st, C);
    AMP_LAUNCH_CHECK("eigh_close");
    hipLaunchKernelGGL(eigh_write_kernel, dim3(cdiv(k, 32), cdiv(k, 32), batch), dim3(256), 0, st, C, (double2*)a->E);
    AMP_LAUNCH_CHECK("eigh_write");
    return AMP_OK;
}

}  // extern "C"

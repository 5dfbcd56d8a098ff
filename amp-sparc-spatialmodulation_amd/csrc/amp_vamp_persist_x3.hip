// amp_vamp_persist_x3.hip — the persistent VAMP engine with both per-iteration GEMMs on the
// split-precision bf16x3 engine (amp_persist.h gemm_x3); its own translation unit so that the
// f32 and bf16x3 instantiations of vamp_persist compile in parallel.  One wave per SIMD.
#include "amp_vamp_persist_kernel.h"

namespace amp {

// N = 256: eight waves per workgroup (two per SIMD, 256 registers each, half the column tiles per
// wave) by default — the VALU phases (denoiser, plane builds) issue at twice the rate of one wave
// per SIMD, and the GEMMs' operator stream hides better (80.6k -> 70.2k cycles per
// cfg4 iteration).  AMP_VAMP_X3_WAVES=4 keeps the four-wave form (A/B runs).
static bool x3_waves8() {
    static const bool v = [] {
        const char* e = diag_env("AMP_VAMP_X3_WAVES");
        return !(e && atoi(e) == 4);
    }();
    return v;
}

int persist_dispatch_x3(const VampK& P, const DecConst& dc, hipStream_t st) {
    switch (P.N) {
    case 64:   // the two-per-CU build for every N = 64 launch, so that one epoch and side-by-side
               // epochs run the same arithmetic (bit-identical results, tests/test_gpu_epochs.py)
        return persist_wg2() ? persist_launch_nt<2, 4, true, 2>(P, dc, st) : AMP_DIAG_ONLY(persist_launch_nt<2, 4, true>(P, dc, st));
    case 128: return persist_launch_nt<4, 4, true>(P, dc, st);
    case 256:
        return x3_waves8() ? persist_launch_nt<4, 8, true>(P, dc, st) : AMP_DIAG_ONLY(persist_launch_nt<8, 4, true>(P, dc, st));
    default: break;
    }
    set_error("vamp_persist (bf16x3): N = %d not supported", P.N);
    return AMP_E_ARG;
}

}  // namespace amp

namespace amp {

// y~ = (s Uh) y (vamp.py:22) for the split-precision engines, as its own launch on the bf16x3
// GEMM (24-bit operands, as the engine's own GEMMs): one workgroup per 16 trials, the y rows
// split into six bf16 planes in LDS (n complex per row), the operator s Uh x3-packed (K = n,
// O = k), the result in the accumulator layout straight to ytil.  Replaces the f32-MFMA
// gemm_store launch (47.7 us per cfg4 step at 0.56 of the f32 peak, profiles/r04_cfg4_vamp_x3.txt).
// rows_per_op / wq_stride: side-by-side epochs with a channel each use the operator of their
// epoch, wq + (row / rows_per_op) * wq_stride bytes (rows_per_op a multiple of PBM).
// zero / nzero: words the launch's first workgroup clears (null: none) — vamp_persist's barrier
// words on a reuse forward, which has no operator-pack launch to clear them (amp_vamp.hip).
__device__ __forceinline__ void ytil_zero_words(unsigned* zero, int nzero) {
    if (zero && blockIdx.x == 0 && blockIdx.y == 0)
        for (int i = threadIdx.x; i < nzero; i += blockDim.x) zero[i] = 0u;
}

template <int NC, int G, int NWV = 4>
__global__ __launch_bounds__(64 * NWV, 1) void ytil_x3_kernel(const float* __restrict__ y, int rows, const void* wq,
                                                               float* __restrict__ ytil, int k, int rows_per_op,
                                                               long long wq_stride, unsigned* zero, int nzero) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    unsigned short* sP = reinterpret_cast<unsigned short*>(lds);
    constexpr int n = 32 * G;
    ytil_zero_words(zero, nzero);
    const int ldx = pl_ldx(n);
    const int row0 = blockIdx.x * PBM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < PBM * (n >> 3); e += 64 * NWV) {   // 8 complex values per item, rows fastest
        const int row = e % PBM, j0 = 8 * (e / PBM);
        float re[8], im[8];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            // unconditional load at a clamped row (a lane-divergent branch around it serialises the
            // loads' latencies, amp_gemm.h ALoadPlain); rows past `rows` are never stored
            const float4 v = *reinterpret_cast<const float4*>(y + (size_t)min(row0 + row, rows - 1) * 2 * n + 2 * j0 + 4 * h);
            re[2 * h] = v.x; im[2 * h] = v.y; re[2 * h + 1] = v.z; im[2 * h + 1] = v.w;
        }
        x3_store8(sP, ldx, row, j0, re, im);
    }
    __syncthreads();
    f32x4 cr[NC], ci[NC];
    const void* wop = (const char*)wq + (long long)(row0 / rows_per_op) * wq_stride;
    gemm_x3<NC, G, 1, false, true>(sP, ldx, wop, wave * NC, cr, ci);   // HL: the engines' accumulation
#pragma unroll
    for (int t = 0; t < NC; ++t) {
        const int o = 16 * (wave * NC + t) + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 4 * (lane >> 4) + r;
            if (row < rows) *reinterpret_cast<float2*>(ytil + (size_t)row * 2 * k + 2 * o) = make_float2(cr[t][r], ci[t][r]);
        }
    }
}

// The k = 256 form (cfg4: n = 512): a workgroup takes 32 trials (two 16-row A tiles) and half the
// outputs (eight 16-column tiles, one per wave), so each operator group a wave streams feeds 48
// MFMAs of two row tiles — half the operator bytes per CU of the 16-trial form (1.5 MB, the per-CU
// L2 rate was its wall).  The 32 rows' planes of all n = 512 columns would take 196 KB of LDS, so
// the reduction runs in NH stages of KS columns (96 KB of planes each), in order: every output
// sums the same products in the same order as gemm_x3 (bit-identical y~).
// D: operator groups in flight (the kernel has registers to spare: 94 VGPRs at D = 1).  hook():
// called once after the first group's MFMAs (the next stage's y loads go there, behind this
// stage's first operator loads in the in-order vmcnt).
// lr / li: the cross-piece sums, apart from the leading-piece sums cr / ci (gemm_x3's HL form; the
// caller adds them once after the last stage).
template <int GH, int D, class Hook>
__device__ __forceinline__ void x3_rows2(const unsigned short* sP0, const unsigned short* sP1, int ldx,
                                         __amdgpu_buffer_rsrc_t wr, int gbase, f32x4 (&cr)[2], f32x4 (&ci)[2],
                                         f32x4 (&lr)[2], f32x4 (&li)[2], Hook&& hook) {
    const int lane = threadIdx.x & 63;
    const int vo = lane * 16;
    u32x4 ring[D][6];
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
        for (int f = 0; f < 6; ++f) ring[d][f] = __builtin_amdgcn_raw_buffer_load_b128(wr, vo, ((gbase + d) * 6 + f) * 1024, 0);
    const int ln = pl_opaque(lane);
    const int sw = (ln & 15) & pl_mask(ldx);
    const int aoff = (ln & 15) * ldx + 8 * ((ln >> 4) ^ (sw & 3));
    const int s32 = 32 * (sw >> 2);
    const u32x4 sgn = {0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u};
    // A fragments one row tile ahead (read from LDS while the previous tile's MFMAs run)
    auto lda = [&](int g, int rt, u32x4 (&a)[6]) {
        const unsigned short* ap = (rt ? sP1 : sP0) + aoff + ((32 * g) ^ s32);
#pragma unroll
        for (int f = 0; f < 6; ++f) a[f] = *reinterpret_cast<const u32x4*>(ap + f * 16 * ldx);
    };
    u32x4 acur[6];
    lda(0, 0, acur);
#pragma unroll
    for (int g = 0; g < GH; ++g) {
        const u32x4* w = ring[g % D];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            u32x4 a[6], anx[6], na[3];
#pragma unroll
            for (int f = 0; f < 6; ++f) a[f] = acur[f];
            if (rt == 0) lda(g, 1, anx);
            else if (g + 1 < GH) lda(g + 1, 0, anx);
#pragma unroll
            for (int f = 0; f < 3; ++f) na[f] = a[3 + f] ^ sgn;
            f32x4 gr = cr[rt], gi = ci[rt], sr = lr[rt], si = li[rt];
#define AMP_MF(acc, x, y) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(x), as_bf16x8(y), acc, 0, 0, 0)
            // gemm_x3's product order (smallest terms first), HL form
            AMP_MF(sr, a[0], w[2]);  AMP_MF(si, a[0], w[5]);
            AMP_MF(sr, a[1], w[1]);  AMP_MF(si, a[1], w[4]);
            AMP_MF(sr, a[2], w[0]);  AMP_MF(si, a[2], w[3]);
            AMP_MF(sr, na[0], w[5]); AMP_MF(si, a[3], w[2]);
            AMP_MF(sr, na[1], w[4]); AMP_MF(si, a[4], w[1]);
            AMP_MF(sr, na[2], w[3]); AMP_MF(si, a[5], w[0]);
            AMP_MF(sr, a[0], w[1]);  AMP_MF(si, a[0], w[4]);
            AMP_MF(sr, a[1], w[0]);  AMP_MF(si, a[1], w[3]);
            AMP_MF(sr, na[0], w[4]); AMP_MF(si, a[3], w[1]);
            AMP_MF(sr, na[1], w[3]); AMP_MF(si, a[4], w[0]);
            AMP_MF(gr, a[0], w[0]);  AMP_MF(gi, a[0], w[3]);
            AMP_MF(gr, na[0], w[3]); AMP_MF(gi, a[3], w[0]);
#undef AMP_MF
            cr[rt] = gr; ci[rt] = gi; lr[rt] = sr; li[rt] = si;
            if (rt == 0 || g + 1 < GH) {
#pragma unroll
                for (int f = 0; f < 6; ++f) acur[f] = anx[f];
            }
        }
        if (g + D < GH) {
#pragma unroll
            for (int f = 0; f < 6; ++f)
                ring[g % D][f] = __builtin_amdgcn_raw_buffer_load_b128(wr, vo, ((gbase + g + D) * 6 + f) * 1024, 0);
        }
        if (g == 0) hook();
        __builtin_amdgcn_sched_barrier(0);
    }
}

#ifndef AMP_YTIL_RING
#define AMP_YTIL_RING 3
#endif
template <int GH, int NH>
__global__ __launch_bounds__(512, 1) void ytil_x3_r2_kernel(const float* __restrict__ y, int rows, const void* wq,
                                                             float* __restrict__ ytil, int k, int rows_per_op,
                                                             long long wq_stride, unsigned* zero, int nzero) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    unsigned short* sP0 = reinterpret_cast<unsigned short*>(lds);
    ytil_zero_words(zero, nzero);
    constexpr int KS = 32 * GH, n = KS * NH, G = GH * NH;
    const int ldx = pl_ldx(KS);
    unsigned short* sP1 = sP0 + 6 * 16 * ldx;
    const int row0 = blockIdx.x * 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ct = blockIdx.y * 8 + wave;   // this wave's 16-column output tile
    const int ctu = __builtin_amdgcn_readfirstlane(ct);
    const char* wop = (const char*)wq + (long long)(row0 / rows_per_op) * wq_stride;
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(wop) + (size_t)ctu * G * 6 * 1024, (short)0, 0x7ffffff0, 0x00020000);
    f32x4 cr[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    f32x4 ci[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    f32x4 lr[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    f32x4 li[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    // stage h's KS columns of the 32 rows: 8 complex values per item, rows fastest; the next
    // stage's loads are in flight while this stage's GEMM runs
    constexpr int ITEMS = 32 * (KS >> 3), PER = ITEMS / 512;
    float4 v[PER][4];
    auto load_stage = [&](int h) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = tid + i * 512, row = e % 32, j0 = 8 * (e / 32);
#pragma unroll
            for (int q = 0; q < 4; ++q)   // clamped row, no branch (see ytil_x3_kernel); rows past `rows` are never stored
                v[i][q] = *reinterpret_cast<const float4*>(y + (size_t)min(row0 + row, rows - 1) * 2 * n + 2 * (h * KS + j0) + 4 * q);
        }
    };
    load_stage(0);
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        if (h > 0) __syncthreads();   // every wave is done with the previous stage's planes
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = tid + i * 512, row = e % 32, j0 = 8 * (e / 32);
            float re[8], im[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                re[2 * q] = v[i][q].x; im[2 * q] = v[i][q].y; re[2 * q + 1] = v[i][q].z; im[2 * q + 1] = v[i][q].w;
            }
            x3_store8(row < 16 ? sP0 : sP1, ldx, row & 15, j0, re, im);
        }
        __syncthreads();
        x3_rows2<GH, AMP_YTIL_RING>(sP0, sP1, ldx, wr, h * GH, cr, ci, lr, li, [&] {
            if (h + 1 < NH) load_stage(h + 1);
        });
    }
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) { cr[rt] += lr[rt]; ci[rt] += li[rt]; }
    const int o = 16 * ct + (lane & 15);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 16 * rt + 4 * (lane >> 4) + r;
            if (row < rows) *reinterpret_cast<float2*>(ytil + (size_t)row * 2 * k + 2 * o) = make_float2(cr[rt][r], ci[rt][r]);
        }
}

static int ytil_x3_r2_launch(const float* y, int rows, const void* wq, float* ytil, int k, int rows_per_op,
                             long long wq_stride, unsigned* zero, int nzero, hipStream_t st) {
    const void* fn = (const void*)ytil_x3_r2_kernel<8, 2>;
    const size_t lds = (size_t)2 * 6 * 16 * pl_ldx(256) * 2;
    static int attr = -1;
    if (attr < 0) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            set_error("ytil_x3_r2: hipFuncSetAttribute: %s", hipGetErrorString(e));
            return AMP_E_LAUNCH;
        }
        attr = 1;
    }
    hipLaunchKernelGGL((ytil_x3_r2_kernel<8, 2>), dim3(cdiv(rows, 32), 2), dim3(512), lds, st, y, rows, wq, ytil, k,
                       rows_per_op, wq_stride, zero, nzero);
    AMP_LAUNCH_CHECK("ytil_x3_r2");
    return AMP_OK;
}

// AMP_YTIL_R2=0 keeps the 16-trial form at k = 256 (A/B runs; read per launch, so a test can
// compare both forms in one process)
static bool ytil_r2_env() {
    const char* e = getenv("AMP_YTIL_R2");
    return !(e && e[0] == '0');
}

template <int NC, int G, int NWV = 4>
static int ytil_x3_launch_t(const float* y, int rows, const void* wq, float* ytil, int k, int rows_per_op,
                            long long wq_stride, unsigned* zero, int nzero, hipStream_t st) {
    const void* fn = (const void*)ytil_x3_kernel<NC, G, NWV>;
    const size_t lds = (size_t)6 * PBM * pl_ldx(32 * G) * 2;
    static int attr = -1;   // once per instantiation (single-threaded host use, like the rest of the ABI)
    if (attr < 0) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            set_error("ytil_x3: hipFuncSetAttribute: %s", hipGetErrorString(e));
            return AMP_E_LAUNCH;
        }
        attr = 1;
    }
    hipLaunchKernelGGL((ytil_x3_kernel<NC, G, NWV>), dim3(cdiv(rows, PBM)), dim3(64 * NWV), lds, st, y, rows, wq, ytil, k,
                       rows_per_op, wq_stride, zero, nzero);
    AMP_LAUNCH_CHECK("ytil_x3");
    return AMP_OK;
}

// The shapes of the split-precision engines (k == N, n == 2N): false for any other.
bool ytil_x3_fits(int n, int k) { return n == 2 * k && (k == 64 || k == 128 || k == 256); }

int ytil_x3_launch(const float* y, int n, int rows, const void* wq, float* ytil, int k, hipStream_t st,
                   int rows_per_op, long long wq_stride, unsigned* zero, int nzero) {
    if (rows_per_op <= 0) rows_per_op = rows;   // one operator for every row
    AMP_REQUIRE(rows_per_op % PBM == 0 || rows_per_op >= rows, "ytil_x3: rows per operator %d", rows_per_op);
    switch (k) {
    case 64: return ytil_x3_launch_t<1, 4>(y, rows, wq, ytil, k, rows_per_op, wq_stride, zero, nzero, st);
    case 128: return ytil_x3_launch_t<2, 8>(y, rows, wq, ytil, k, rows_per_op, wq_stride, zero, nzero, st);
    case 256:   // 32 trials x half the outputs per workgroup (every operator group feeds two row
                // tiles); else eight waves of 16 trials, as in the engine
        if (ytil_r2_env() && (rows_per_op % 32 == 0 || rows_per_op >= rows))
            return ytil_x3_r2_launch(y, rows, wq, ytil, k, rows_per_op, wq_stride, zero, nzero, st);
        return ytil_x3_launch_t<2, 16, 8>(y, rows, wq, ytil, k, rows_per_op, wq_stride, zero, nzero, st);
    default: break;
    }
    set_error("ytil_x3: n = %d / k = %d not supported", n, k);
    return AMP_E_ARG;
}

}  // namespace amp

// Diagnostic (amp_x3_planes_debug): the A-operand plane writers of vamp_persist on caller-supplied
// rows.  One workgroup of eight waves, N = 256, as the cfg4 kernel runs them: the row-item map of
// the r~ build (item tid: row tid % 16, columns 8 (tid / 16) ...) and the accumulator map of the w
// store (wave w: complex column tiles 2 w, 2 w + 1).  Form 0: x3_store8, 1: x3_store8_item,
// 2: x3_store_acc, 3: x3_store_acc_item; each form's planes are copied out in LDS order.
namespace amp {

constexpr int XPD_N = 256, XPD_WG = 512, XPD_WORDS = 6 * PBM * XPD_N / 2;

__global__ __launch_bounds__(XPD_WG) void x3_planes_debug_kernel(const float* __restrict__ rows, int nrows, int ldx,
                                                                  unsigned* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    unsigned short* sP = reinterpret_cast<unsigned short*>(lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto at = [&](int row, int col) {   // rows past nrows are zero rows, as the engine's padded trials
        const float2 v = *reinterpret_cast<const float2*>(rows + ((size_t)min(row, nrows - 1) * XPD_N + col) * 2);
        return row < nrows ? v : make_float2(0.f, 0.f);
    };
    for (int form = 0; form < 4; ++form) {
        if (form < 2) {
            static_assert(PBM * (XPD_N >> 3) == XPD_WG, "one item per thread");
            const int row = tid % PBM, j0 = 8 * (tid / PBM);
            float re[8], im[8];
#pragma unroll
            for (int h = 0; h < 8; ++h) {
                const float2 v = at(row, j0 + h);
                re[h] = v.x; im[h] = v.y;
            }
            if (form == 0) x3_store8(sP, ldx, row, j0, re, im);
            else x3_store8_item<XPD_N>(sP, row, j0, re, im);
        } else {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int o = 16 * (2 * wave + t) + (lane & 15);
                float vr[4], vi[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float2 v = at(4 * (lane >> 4) + r, o);
                    vr[r] = v.x; vi[r] = v.y;
                }
                if (form == 2) x3_store_acc(sP, ldx, o, vr, vi);
                else x3_store_acc_item<XPD_N>(sP, o, vr, vi);
            }
        }
        __syncthreads();
        for (int e = tid; e < XPD_WORDS; e += XPD_WG) out[(size_t)form * XPD_WORDS + e] = reinterpret_cast<const unsigned*>(sP)[e];
        __syncthreads();
    }
}

}  // namespace amp

int amp_x3_planes_debug(const void* rows, int32_t nrows, void* planes, void* stream) {
    using namespace amp;
    AMP_REQUIRE(rows && planes, "amp_x3_planes_debug: null pointer argument");
    AMP_REQUIRE(nrows >= 1 && nrows <= PBM, "amp_x3_planes_debug: nrows = %d (1 ... %d)", nrows, PBM);
    hipLaunchKernelGGL(x3_planes_debug_kernel, dim3(1), dim3(XPD_WG), (size_t)XPD_WORDS * 4, (hipStream_t)stream,
                       (const float*)rows, (int)nrows, x3_ldx(XPD_N), (unsigned*)planes);
    AMP_LAUNCH_CHECK("amp_x3_planes_debug");
    return AMP_OK;
}

// Diagnostic (amp_x3_pack_store_debug): the two halves of x3_store_acc_item as vamp_persist's w epilogue
// runs them, on caller-supplied rows in amp_x3_planes_debug's accumulator map: every wave packs its two
// tiles (x3_pack_acc_item), the workgroup meets at a barrier, every wave stores the words it holds
// (x3_store_packed_item).  The planes are copied out in LDS order: form 3 of amp_x3_planes_debug, bit for bit.
namespace amp {

__global__ __launch_bounds__(XPD_WG) void x3_pack_store_debug_kernel(const float* __restrict__ rows, int nrows,
                                                                      unsigned* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    unsigned short* sP = reinterpret_cast<unsigned short*>(lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned w[2][2][6];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int o = 16 * (2 * wave + t) + (lane & 15);
        float vr[4], vi[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * (lane >> 4) + r;
            const float2 v = *reinterpret_cast<const float2*>(rows + ((size_t)min(row, nrows - 1) * XPD_N + o) * 2);
            vr[r] = row < nrows ? v.x : 0.f; vi[r] = row < nrows ? v.y : 0.f;
        }
        x3_pack_acc_item<XPD_N>(vr, vi, w[t]);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2; ++t) x3_store_packed_item<XPD_N>(sP, 16 * (2 * wave + t) + (lane & 15), w[t]);
    __syncthreads();
    for (int e = tid; e < XPD_WORDS; e += XPD_WG) out[e] = reinterpret_cast<const unsigned*>(sP)[e];
}

}  // namespace amp

int amp_x3_pack_store_debug(const void* rows, int32_t nrows, void* planes, void* stream) {
    using namespace amp;
    AMP_REQUIRE(rows && planes, "amp_x3_pack_store_debug: null pointer argument");
    AMP_REQUIRE(nrows >= 1 && nrows <= PBM, "amp_x3_pack_store_debug: nrows = %d (1 ... %d)", nrows, PBM);
    hipLaunchKernelGGL(x3_pack_store_debug_kernel, dim3(1), dim3(XPD_WG), (size_t)XPD_WORDS * 4, (hipStream_t)stream,
                       (const float*)rows, (int)nrows, (unsigned*)planes);
    AMP_LAUNCH_CHECK("amp_x3_pack_store_debug");
    return AMP_OK;
}

// Diagnostic (amp_exchange_reduce_debug): the reduction chain of vamp_persist's exchange on
// caller-supplied values, today's forms and the key forms of the eight-wave bf16x3 kernel side by
// side.  One workgroup of eight waves: part_publish and part_publish_keys on one PartAcc per thread
// (the granules land in `out`, the waves' Partials are copied from the scratch), part_gather and
// part_gather_keys on up to 256 granule pairs (the kernel stamps the tag it then sweeps for into a
// staging copy, so the sweep passes at once), and the mean's quotient in both forms per thread.
namespace amp {

constexpr int XRD_WG = 512, XRD_MAXG = 256;
constexpr unsigned XRD_PUB = 0, XRD_WAVES = 64, XRD_GATHER = 576, XRD_FLAGS = 640, XRD_MEAN = 672,
                   XRD_STAGE = XRD_MEAN + 2 * XRD_WG * 8, XRD_BYTES = XRD_STAGE + XRD_MAXG * 32;

__global__ __launch_bounds__(XRD_WG) void exchange_reduce_debug_kernel(const Partial* __restrict__ vals,
                                                                        const u32x4* __restrict__ grans, int ngran,
                                                                        const double* __restrict__ sums,
                                                                        const int2* __restrict__ divs, unsigned* out) {
    __shared__ __attribute__((aligned(16))) unsigned scr[256];
    __shared__ int s_flag;
    const int tid = threadIdx.x;
    const unsigned tag = 1u;
    u32x4* stage = reinterpret_cast<u32x4*>(reinterpret_cast<char*>(out) + XRD_STAGE);
    if (tid < XRD_MAXG) {
        u32x4 a = {0u, 0u, 0u, 0u}, b = a;
        if (tid < ngran) { a = grans[2 * tid]; b = grans[2 * tid + 1]; a.w = tag; b.w = tag; }
        stage[2 * tid] = a; stage[2 * tid + 1] = b;
    }
    if (tid < 8) out[XRD_FLAGS / 4 + tid] = 0u;
    __threadfence();
    __syncthreads();
    const __amdgpu_buffer_rsrc_t ors = gran_rsrc(out, XRD_BYTES);
    const __amdgpu_buffer_rsrc_t srs = gran_rsrc(stage, XRD_MAXG * 32);
    PartAcc p;
    p.sumvar = vals[tid].sumvar; p.maxabs = vals[tid].maxabs; p.minsecmax = vals[tid].minsecmax; p.notclose = vals[tid].notclose;
    for (int form = 0; form < 2; ++form) {
        if (form == 0) part_publish(p, ors, XRD_PUB, 0u, scr);
        else part_publish_keys<XRD_WG / 64>(p, ors, XRD_PUB + 32, 0u, scr);
        if (tid < 64) out[(XRD_WAVES + 256 * form) / 4 + tid] = scr[tid];   // the eight waves' Partials
        __syncthreads();
    }
    for (int form = 0; form < 2; ++form) {
        PartAcc g;
        const bool ok = form == 0 ? part_gather(srs, 0u, ngran, tag, out + XRD_FLAGS / 4, g, scr, &s_flag)
                                  : part_gather_keys<AMP_X3_W8_POLL>(srs, 0u, ngran, tag, out + XRD_FLAGS / 4, g, scr, &s_flag);
        if (tid == 0) {
            Partial o;
            o.sumvar = g.sumvar; o.maxabs = g.maxabs; o.minsecmax = g.minsecmax; o.notclose = g.notclose;
            o.pad = ok ? 1u : 0u;
            *reinterpret_cast<Partial*>(reinterpret_cast<char*>(out) + XRD_GATHER + 32 * form) = o;
        }
    }
    double* mean = reinterpret_cast<double*>(reinterpret_cast<char*>(out) + XRD_MEAN);
    mean[tid] = var_mean_div(sums[tid], divs[tid].x, divs[tid].y);
    mean[XRD_WG + tid] = var_mean_pow2(sums[tid], divs[tid].x, divs[tid].y);
}

}  // namespace amp

int amp_exchange_reduce_debug(const void* vals, const void* grans, int32_t ngran, const void* sums, const void* divs,
                              void* out, void* stream) {
    using namespace amp;
    AMP_REQUIRE(vals && grans && sums && divs && out, "amp_exchange_reduce_debug: null pointer argument");
    AMP_REQUIRE(ngran >= 1 && ngran <= XRD_MAXG, "amp_exchange_reduce_debug: ngran = %d (1 ... %d)", ngran, XRD_MAXG);
    hipLaunchKernelGGL(exchange_reduce_debug_kernel, dim3(1), dim3(XRD_WG), 0, (hipStream_t)stream, (const Partial*)vals,
                       (const u32x4*)grans, (int)ngran, (const double*)sums, (const int2*)divs, (unsigned*)out);
    AMP_LAUNCH_CHECK("amp_exchange_reduce_debug");
    return AMP_OK;
}

// Diagnostic (amp_exchange_poll_debug): the gather of the eight-wave bf16x3 kernel's exchange as the
// kernel calls it (part_gather_keys with the kernel's retry loop), one workgroup of eight waves on
// caller-supplied granule pairs whose tag words are the caller's, with the abort word preset.  A
// call that would wait (a tag absent and the word not raised) is not run: the kernel looks at the
// tags first and leaves code 2.
namespace amp {

constexpr unsigned XPL_REC = 0, XPL_ABORT = 32, XPL_SWEEPS = 36, XPL_CODE = 40, XPL_TICKS = 48;   // (out: 64 bytes)

__global__ __launch_bounds__(XRD_WG) void exchange_poll_debug_kernel(const u32x4* grans, int ngran, unsigned tag,
                                                                      unsigned raised, unsigned* out) {
    __shared__ __attribute__((aligned(16))) unsigned scr[256];
    __shared__ int s_flag;
    const int tid = threadIdx.x;
    int present = 1;
    if (tid < ngran) present = (grans[2 * tid].w == tag) & (grans[2 * tid + 1].w == tag);
    const int all = __syncthreads_and(present);
    if (tid == 0) {
        out[XPL_ABORT / 4] = raised;
        out[XPL_SWEEPS / 4] = 0u;
        out[XPL_CODE / 4] = (all || raised != 0u) ? 0u : 2u;
    }
    if (!all && raised == 0u) return;
    __threadfence();
    __syncthreads();
    const __amdgpu_buffer_rsrc_t srs = gran_rsrc(const_cast<u32x4*>(grans), (unsigned)ngran * 32u);
    PartAcc g;
    unsigned nsw = 0;
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    const bool ok = part_gather_keys<AMP_X3_W8_POLL>(srs, 0u, ngran, tag, out + XPL_ABORT / 4, g, scr, &s_flag, &nsw);
    const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) {
        Partial o;
        o.sumvar = g.sumvar; o.maxabs = g.maxabs; o.minsecmax = g.minsecmax; o.notclose = g.notclose;
        o.pad = ok ? 1u : 0u;
        *reinterpret_cast<Partial*>(reinterpret_cast<char*>(out) + XPL_REC) = o;
        out[XPL_SWEEPS / 4] = nsw;
        *reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(out) + XPL_TICKS) = t1 - t0;
    }
}

}  // namespace amp

int amp_exchange_poll_debug(const void* grans, int32_t ngran, uint32_t tag, int32_t raised, void* out, void* stream) {
    using namespace amp;
    AMP_REQUIRE(grans && out, "amp_exchange_poll_debug: null pointer argument");
    AMP_REQUIRE(ngran >= 1 && ngran <= XRD_MAXG, "amp_exchange_poll_debug: ngran = %d (1 ... %d)", ngran, XRD_MAXG);
    AMP_REQUIRE(tag != 0u, "amp_exchange_poll_debug: tag 0 (never published)");
    hipLaunchKernelGGL(exchange_poll_debug_kernel, dim3(1), dim3(XRD_WG), 0, (hipStream_t)stream, (const u32x4*)grans,
                       (int)ngran, (unsigned)tag, raised != 0 ? 1u : 0u, (unsigned*)out);
    AMP_LAUNCH_CHECK("amp_exchange_poll_debug");
    return AMP_OK;
}

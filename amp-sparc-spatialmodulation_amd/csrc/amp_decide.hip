// amp_decide.hip — MAP hard decision + error counters on the GPU.
//
// Restates Loss.error_rate (loss.py:67-103) for generator_mode='sparc':
//   MAP_decision (loss.py:282-302): per section of M entries, argmax over the flattened
//     (m, k) grid of Re(x_m conj(a_k)) in float64.  The value is formed exactly as numpy's
//     complex multiply forms it (measured: fma(xr, ar, xi*ai)), first index wins ties,
//     an all/partly-NaN section picks its first NaN (np.argmax semantics).
//   mean_square_error / vector_error_rate / frame_error_rate / bit_error_rate
//     (loss.py:105-179) as integer counters and float64 sums.
// Kernel 1 (grid): one lane group per section -> decision, per-section mismatch byte,
//   per-workgroup partial counters.  Kernel 2 (one workgroup): deterministic sums and the
//   channel-use / trial "any mismatch" reductions.
#include <algorithm>

#include "amp_common.h"
#include "amp_decide.h"
#include "amp_host.h"

namespace amp {

struct DecK {
    int B, L, M, Na, Lin, S;
    int ibits;
    long long s_off;    // section offset of these rows in the whole batch (trial-sharded decision)
    const float2* xmap;
    const float2* xmmse;
    const float2* x;
    const long long* sym;
    const long long* idx;
    unsigned char* mism;
    int* dec;
    DecPart* parts;
    int nblk;
    amp_counts* out;
    int rule;            // 0: MAP (sparc), 1: segmented, 2: random
    DecConst c;
};

template <int KK, int G>
__global__ __launch_bounds__(AMP_WG) void map_decide_kernel(DecK P) {
    // one section per group of G = min(M, 64) lanes (coalesced loads of consecutive positions)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int M = P.M;
    constexpr int gpw = 64 / G;
    const int gid = lane / G, g = lane % G;
    DecPart q = decpart_zero();
    const long long ibmask = dec_ibmask(P.ibits);
    const int stride = gridDim.x * (AMP_WG / 64) * gpw;
    for (int base = (blockIdx.x * (AMP_WG / 64) + wave) * gpw; base < P.S; base += stride) {   // wave-uniform
        const int s = base + gid;
        const bool act = s < P.S;
        const size_t o0 = (size_t)(act ? s : P.S - 1) * M;
        auto ld = [&](int m, float2& xv, float2& xt, float2& xe) {
            xv = P.xmap[o0 + m]; xt = P.x[o0 + m]; xe = P.xmmse[o0 + m];
        };
        int bi, mm;
        double se;
        if (P.rule == 1)
            decide_section_seg<KK, G>(P.c, M, g, ld, bi, mm, se);
        else
            decide_section<KK, G, false>(P.c, M, g, ld, bi, mm, se);
        if (act && g == 0) {
            P.mism[s] = (unsigned char)mm;
            if (P.dec) P.dec[s] = bi;
            count_section<KK>(P.c, s + P.s_off, M, P.L, P.Na, P.Lin, bi, se, P.sym[s], P.idx[s], ibmask, q);
        }
    }
    long long ier = q.ier, ser = q.ser, iber = q.iber, sber = q.sber;
    double mse = q.mse, msef = q.msef, msem = q.msem, mseL = q.mseL;
    // workgroup reduction (fixed order)
    ier = group_sum(ier, 64); ser = group_sum(ser, 64); iber = group_sum(iber, 64); sber = group_sum(sber, 64);
    mse = group_sum(mse, 64); msef = group_sum(msef, 64); msem = group_sum(msem, 64); mseL = group_sum(mseL, 64);
    __shared__ DecPart sp[AMP_WG / 64];
    if (lane == 0) sp[wave] = DecPart{ier, ser, iber, sber, mse, msef, msem, mseL};
    __syncthreads();
    if (threadIdx.x == 0) {
        DecPart o = sp[0];
        for (int w = 1; w < AMP_WG / 64; ++w) {
            o.ier += sp[w].ier; o.ser += sp[w].ser; o.iber += sp[w].iber; o.sber += sp[w].sber;
            o.mse += sp[w].mse; o.msef += sp[w].msef; o.msem += sp[w].msem; o.mseL += sp[w].mseL;
        }
        P.parts[blockIdx.x] = o;
    }
}


// Random decision (Loss.random_decision, loss.py:252-280; generator_mode='random'): one thread per
// channel use (random_decide_row, amp_decide.h, shared with the per-trial form of
// amp_trials_decide.hip): the reference runs this only for B = 1 (its reshape drops the batch axis).
template <int KK>
__global__ __launch_bounds__(AMP_WG) void random_decide_kernel(DecK P, int Nt, int R) {
    DecPart q = decpart_zero();
    const long long ibmask = dec_ibmask(P.ibits);
    for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < R; row += gridDim.x * blockDim.x)
        random_decide_row<KK>(P.c, Nt, P.Na, P.Lin, row, P.xmap, P.x, P.xmmse, P.sym, P.idx, ibmask, P.dec,
                              P.mism + (size_t)(row / P.Lin) * P.L + (size_t)(row % P.Lin) * P.Na, q);
    random_part_store(q, P.parts + blockIdx.x);
}

__global__ __launch_bounds__(1024) void map_count_kernel(DecK P) {
    // channel-use / trial "any mismatch" counts (loss.py:133-136, 150) ...
    long long ver = 0, verf = 0, verm = 0, verL = 0, fer = 0;
    for (int b = threadIdx.x; b < P.B; b += blockDim.x) {
        int trial = 0;
        for (int lin = 0; lin < P.Lin; ++lin) {
            int cu = 0;
            const unsigned char* m = P.mism + (size_t)b * P.L + (size_t)lin * P.Na;
            for (int a = 0; a < P.Na; ++a) cu |= m[a];
            ver += cu;
            if (lin == 0) verf += cu;
            if (lin == P.Lin / 2) verm += cu;
            if (lin == P.Lin - 1) verL += cu;
            trial |= cu;
        }
        fer += trial;
    }
    // ... and the per-workgroup partials of map_decide_kernel, folded in a fixed order
    DecPart t = DecPart{0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < P.nblk; i += blockDim.x) {
        const DecPart q = P.parts[i];
        t.ier += q.ier; t.ser += q.ser; t.iber += q.iber; t.sber += q.sber;
        t.mse += q.mse; t.msef += q.msef; t.msem += q.msem; t.mseL += q.mseL;
    }
    ver = group_sum(ver, 64); verf = group_sum(verf, 64); verm = group_sum(verm, 64); verL = group_sum(verL, 64);
    fer = group_sum(fer, 64);
    t.ier = group_sum(t.ier, 64); t.ser = group_sum(t.ser, 64); t.iber = group_sum(t.iber, 64);
    t.sber = group_sum(t.sber, 64);
    t.mse = group_sum(t.mse, 64); t.msef = group_sum(t.msef, 64); t.msem = group_sum(t.msem, 64);
    t.mseL = group_sum(t.mseL, 64);
    __shared__ long long sc[16][5];
    __shared__ DecPart sp[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        sc[wave][0] = ver; sc[wave][1] = verf; sc[wave][2] = verm; sc[wave][3] = verL; sc[wave][4] = fer;
        sp[wave] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        amp_counts c;
        c.ver = c.verf = c.verm = c.verL = c.fer = 0;
        c.ier = c.ser = c.iber = c.sber = 0;
        c.mse = c.msef = c.msem = c.mseL = 0.0;
        for (int w = 0; w < (int)(blockDim.x / 64); ++w) {
            c.ver += sc[w][0]; c.verf += sc[w][1]; c.verm += sc[w][2]; c.verL += sc[w][3]; c.fer += sc[w][4];
            c.ier += sp[w].ier; c.ser += sp[w].ser; c.iber += sp[w].iber; c.sber += sp[w].sber;
            c.mse += sp[w].mse; c.msef += sp[w].msef; c.msem += sp[w].msem; c.mseL += sp[w].mseL;
        }
        *P.out = c;
    }
}

// Diagnostic (amp_decide_debug_sections): the fused epilogue's section decision on caller-supplied
// rows.  As decide_epilogue (amp_decide_fused.h) does it: a workgroup of eight waves holds 16 rows
// of the decision input, xmmse and the truth in LDS at the engines' row stride, a group of four
// lanes decides one section with the prefiltered decide_section (NARROW: its narrowed scan), 16
// sections per wave step; instead of counting, lane 0 of the group stores the section's results.
constexpr int DBG_WG = 512, DBG_ROWS = 16;

struct DecDbgK {
    int B, L, M, N, ldr;
    const float* xmap;
    const float* xmmse;
    const float* x;
    int* bi;
    int* mm;
    double* se;
    DecConst c;
};

template <int KK, bool NARROW>
__global__ __launch_bounds__(DBG_WG) void decide_debug_kernel(DecDbgK P) {
    extern __shared__ __attribute__((aligned(16))) float dbg_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = P.M, L = P.L, N = P.N, ldr = P.ldr;
    const int row0 = blockIdx.x * DBG_ROWS, nrows = min(DBG_ROWS, P.B - row0);
    float* sR = dbg_lds;
    float* sX = sR + DBG_ROWS * ldr;
    float* sT = sX + DBG_ROWS * ldr;
    for (int e = tid; e < nrows * (N >> 1); e += DBG_WG) {   // float4: two complex entries
        const int row = e / (N >> 1), c4 = 4 * (e - row * (N >> 1));
        const size_t go = (size_t)(row0 + row) * 2 * N + c4;
        *reinterpret_cast<float4*>(sR + row * ldr + c4) = *reinterpret_cast<const float4*>(P.xmap + go);
        *reinterpret_cast<float4*>(sX + row * ldr + c4) = *reinterpret_cast<const float4*>(P.xmmse + go);
        *reinterpret_cast<float4*>(sT + row * ldr + c4) = *reinterpret_cast<const float4*>(P.x + go);
    }
    __syncthreads();
    const int S = nrows * L;
    constexpr int DG = 4;
    const int g = lane % DG;
    for (int base = wave * (64 / DG); base < S; base += (DBG_WG / 64) * (64 / DG)) {   // wave-uniform
        const int ls = base + lane / DG;
        const bool act = ls < S;
        const int lsc = act ? ls : S - 1;
        const int row = lsc / L, l = lsc - row * L;
        const float* rp = sR + row * ldr + 2 * l * M;
        const float* xp = sX + row * ldr + 2 * l * M;
        const float* tp = sT + row * ldr + 2 * l * M;
        auto ld = [&](int m, float2& xv, float2& xt, float2& xe) {
            xv = *reinterpret_cast<const float2*>(rp + 2 * m);
            xe = *reinterpret_cast<const float2*>(xp + 2 * m);
            xt = *reinterpret_cast<const float2*>(tp + 2 * m);
        };
        int bi, mm;
        double se;
        decide_section<KK, DG, true, NARROW>(P.c, M, g, ld, bi, mm, se);
        if (act && g == 0) {
            const size_t s = (size_t)(row0 + row) * L + l;
            P.bi[s] = bi;
            P.mm[s] = mm;
            P.se[s] = se;
        }
    }
}

template <int KK>
static hipError_t launch_decide_debug(const DecDbgK& P, bool narrow, hipStream_t st) {
    const size_t lds = (size_t)3 * DBG_ROWS * P.ldr * sizeof(float);
    const void* fn = narrow ? (const void*)decide_debug_kernel<KK, true> : (const void*)decide_debug_kernel<KK, false>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    DecDbgK Pc = P;
    void* args[] = {(void*)&Pc};
    return hipLaunchKernel(fn, dim3(cdiv(P.B, DBG_ROWS)), dim3(DBG_WG), args, lds, st);
}

static int decide_nblk(const amp_dims* d) {
    const int G = d->M < 64 ? d->M : 64;
    const int per = (AMP_WG / 64) * (64 / G);
    return std::max(1, std::min(cdiv(d->B * d->L, per), 2048));
}

template <int KK>
static void launch_decide_k(const DecK& P, int M, hipStream_t st) {
    const dim3 g(P.nblk), b(AMP_WG);
    switch (M) {
    case 1: hipLaunchKernelGGL((map_decide_kernel<KK, 1>), g, b, 0, st, P); break;
    case 2: hipLaunchKernelGGL((map_decide_kernel<KK, 2>), g, b, 0, st, P); break;
    case 4: hipLaunchKernelGGL((map_decide_kernel<KK, 4>), g, b, 0, st, P); break;
    case 8: hipLaunchKernelGGL((map_decide_kernel<KK, 8>), g, b, 0, st, P); break;
    case 16: hipLaunchKernelGGL((map_decide_kernel<KK, 16>), g, b, 0, st, P); break;
    case 32: hipLaunchKernelGGL((map_decide_kernel<KK, 32>), g, b, 0, st, P); break;
    default: hipLaunchKernelGGL((map_decide_kernel<KK, 64>), g, b, 0, st, P); break;   // M >= 64 (power of 2)
    }
}

static void launch_decide(const DecK& P, int M, hipStream_t st) {
    switch (P.c.K) {
    case 1: launch_decide_k<1>(P, M, st); break;
    case 2: launch_decide_k<2>(P, M, st); break;
    case 4: launch_decide_k<4>(P, M, st); break;
    case 8: launch_decide_k<8>(P, M, st); break;
    case 16: launch_decide_k<16>(P, M, st); break;
    default: launch_decide_k<64>(P, M, st); break;     // check_dims: K in {1, 2, 4, 8, 16, 64}
    }
}

}  // namespace amp

using namespace amp;

extern "C" {

size_t amp_map_decide_workspace_bytes(const amp_dims* d) {
    if (!d) return 0;
    Carve cv(nullptr);
    cv.take<unsigned char>((size_t)d->B * d->L);
    cv.take<DecPart>((size_t)decide_nblk(d));
    return cv.off;
}

static int decide_count(int rule, const amp_dims* d, const amp_constellation* c, const void* xmap, const void* xmmse,
                        const void* x, const void* sym, const void* idx, int32_t ibits_trunc, void* counts,
                        void* decisions, void* ws, size_t ws_bytes, void* stream, long long row0 = 0) {
    int rc = check_dims(d, c, false);
    if (rc) return rc;
    AMP_REQUIRE(xmap && xmmse && x && sym && idx && counts && ws, "amp_map_decide_count: null pointer argument");
    AMP_REQUIRE(ws_bytes >= amp_map_decide_workspace_bytes(d), "amp_map_decide_count: workspace too small");
    AMP_REQUIRE(ibits_trunc >= 0 && ibits_trunc < 64, "amp_map_decide_count: ibits_trunc out of range");
    DecK P;
    P.B = d->B; P.L = d->L; P.M = d->M; P.Na = d->Na; P.Lin = d->Lin; P.S = d->B * d->L;
    P.ibits = ibits_trunc;
    P.s_off = row0 * d->L;
    P.xmap = (const float2*)xmap; P.xmmse = (const float2*)xmmse; P.x = (const float2*)x;
    P.sym = (const long long*)sym; P.idx = (const long long*)idx;
    Carve cv(ws);
    P.mism = cv.take<unsigned char>((size_t)P.S);
    P.nblk = decide_nblk(d);
    P.parts = cv.take<DecPart>((size_t)P.nblk);
    P.out = (amp_counts*)counts;
    P.dec = (int*)decisions;
    P.c = to_decconst(c);
    P.rule = rule;
    hipStream_t st = (hipStream_t)stream;
    launch_decide(P, d->M, st);
    AMP_LAUNCH_CHECK("map_decide");
    hipLaunchKernelGGL(map_count_kernel, dim3(1), dim3(1024), 0, st, P);
    AMP_LAUNCH_CHECK("map_count");
    return AMP_OK;
}

int amp_map_decide_count(const amp_dims* d, const amp_constellation* c, const void* xmap, const void* xmmse,
                         const void* x, const void* sym, const void* idx, int32_t ibits_trunc, void* counts,
                         void* decisions, void* ws, size_t ws_bytes, void* stream) {
    return decide_count(0, d, c, xmap, xmmse, x, sym, idx, ibits_trunc, counts, decisions, ws, ws_bytes, stream);
}

int amp_map_decide_count_rows(const amp_dims* d, const amp_constellation* c, const void* xmap, const void* xmmse,
                              const void* x, const void* sym, const void* idx, int32_t ibits_trunc, int64_t row0,
                              void* counts, void* decisions, void* ws, size_t ws_bytes, void* stream) {
    AMP_REQUIRE(row0 >= 0, "amp_map_decide_count_rows: row0 = %lld", (long long)row0);
    return decide_count(0, d, c, xmap, xmmse, x, sym, idx, ibits_trunc, counts, decisions, ws, ws_bytes, stream,
                        (long long)row0);
}

int amp_decide_debug_sections(const amp_dims* d, const amp_constellation* c, const void* xmap, const void* xmmse,
                              const void* x, int32_t narrow, void* decisions, void* mismatch, void* sqerr,
                              void* stream) {
    int rc = check_dims(d, c, false);
    if (rc) return rc;
    AMP_REQUIRE(xmap && xmmse && x && decisions && mismatch && sqerr, "amp_decide_debug_sections: null pointer argument");
    AMP_REQUIRE(d->N >= 2 && d->N <= 256 && d->N % 2 == 0 && d->M >= 1 && d->M <= 64 && is_pow2(d->M) &&
                    d->N == d->L * d->M,
                "amp_decide_debug_sections: N = %d (even, <= 256), M = %d (a power of two <= 64), L = %d", d->N, d->M,
                d->L);
    DecDbgK P;
    P.B = d->B; P.L = d->L; P.M = d->M; P.N = d->N;
    P.ldr = 2 * d->N + 8;   // the split-precision engines' row stride (amp_vamp_persist_kernel.h playout)
    P.xmap = (const float*)xmap; P.xmmse = (const float*)xmmse; P.x = (const float*)x;
    P.bi = (int*)decisions; P.mm = (int*)mismatch; P.se = (double*)sqerr;
    P.c = to_decconst(c);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    switch (P.c.K) {
    case 1: e = launch_decide_debug<1>(P, narrow != 0, st); break;
    case 2: e = launch_decide_debug<2>(P, narrow != 0, st); break;
    case 4: e = launch_decide_debug<4>(P, narrow != 0, st); break;
    case 8: e = launch_decide_debug<8>(P, narrow != 0, st); break;
    case 16: e = launch_decide_debug<16>(P, narrow != 0, st); break;
    default: e = launch_decide_debug<64>(P, narrow != 0, st); break;
    }
    if (e != hipSuccess) {
        set_error("amp_decide_debug_sections: %s", hipGetErrorString(e));
        return AMP_E_LAUNCH;
    }
    return AMP_OK;
}

int amp_segmented_decide_count(const amp_dims* d, const amp_constellation* c, const void* xmap, const void* xmmse,
                               const void* x, const void* sym, const void* idx, int32_t ibits_trunc, void* counts,
                               void* decisions, void* ws, size_t ws_bytes, void* stream) {
    return decide_count(1, d, c, xmap, xmmse, x, sym, idx, ibits_trunc, counts, decisions, ws, ws_bytes, stream);
}

int amp_random_decide_count(const amp_dims* d, const amp_constellation* c, const void* xmap, const void* xmmse,
                            const void* x, const void* sym, const void* idx, int32_t ibits_trunc, void* counts,
                            void* decisions, void* ws, size_t ws_bytes, void* stream) {
    AMP_REQUIRE(d && c && d->B > 0 && d->Nt > 0 && d->Lin > 0 && d->Na >= 1 && d->Na <= AMP_DEC_MAX_NA &&
                    d->Na <= d->Nt && d->L == d->Na * d->Lin && c->K >= 1 && c->K <= AMP_MAX_K &&
                    is_pow2(c->K) && c->K != 32,
                "amp_random_decide_count: bad dims (Na <= %d)", AMP_DEC_MAX_NA);
    AMP_REQUIRE(xmap && xmmse && x && sym && idx && counts && ws, "amp_random_decide_count: null pointer argument");
    AMP_REQUIRE(ws_bytes >= amp_map_decide_workspace_bytes(d), "amp_random_decide_count: workspace too small");
    AMP_REQUIRE(ibits_trunc >= 0 && ibits_trunc < 64, "amp_random_decide_count: ibits_trunc out of range");
    DecK P;
    P.B = d->B; P.L = d->L; P.M = d->M; P.Na = d->Na; P.Lin = d->Lin; P.S = d->B * d->L;
    P.ibits = ibits_trunc;
    P.s_off = 0;
    P.xmap = (const float2*)xmap; P.xmmse = (const float2*)xmmse; P.x = (const float2*)x;
    P.sym = (const long long*)sym; P.idx = (const long long*)idx;
    Carve cv(ws);
    P.mism = cv.take<unsigned char>((size_t)P.S);
    const int R = d->B * d->Lin;
    P.nblk = std::max(1, std::min(cdiv(R, AMP_WG), decide_nblk(d)));
    P.parts = cv.take<DecPart>((size_t)decide_nblk(d));
    P.out = (amp_counts*)counts;
    P.dec = (int*)decisions;
    P.c = to_decconst(c);
    P.rule = 2;
    hipStream_t st = (hipStream_t)stream;
    const dim3 g(P.nblk), b(AMP_WG);
    switch (P.c.K) {
    case 1: hipLaunchKernelGGL(random_decide_kernel<1>, g, b, 0, st, P, d->Nt, R); break;
    case 2: hipLaunchKernelGGL(random_decide_kernel<2>, g, b, 0, st, P, d->Nt, R); break;
    case 4: hipLaunchKernelGGL(random_decide_kernel<4>, g, b, 0, st, P, d->Nt, R); break;
    case 8: hipLaunchKernelGGL(random_decide_kernel<8>, g, b, 0, st, P, d->Nt, R); break;
    case 16: hipLaunchKernelGGL(random_decide_kernel<16>, g, b, 0, st, P, d->Nt, R); break;
    default: hipLaunchKernelGGL(random_decide_kernel<64>, g, b, 0, st, P, d->Nt, R); break;
    }
    AMP_LAUNCH_CHECK("random_decide");
    hipLaunchKernelGGL(map_count_kernel, dim3(1), dim3(1024), 0, st, P);
    AMP_LAUNCH_CHECK("map_count");
    return AMP_OK;
}

}  // extern "C"

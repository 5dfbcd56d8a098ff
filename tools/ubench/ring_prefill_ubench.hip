// Operator-ring prefill microbenchmark (cfg4 shapes).
// 256 workgroups x 8 waves (one per CU), REPS iterations of the GEMM half of a VAMP iteration,
// through the engine's own device functions (amp_persist.h):
//   an x3_store8 pass over 16 x 256 complex (the r~ plane build's LDS work), barrier,
//   GEMM1 on the Vh planes, barrier, an x3_store_acc pass (the w store), barrier,
//   GEMM2 on the V planes, barrier.
//   FORM 0 (printed as A): the engine before the prefill — gemm_x3 issues its ring fill at its own entry;
//   FORM 1 (B): x3_ring_fill(Vh) before the x3_store8 pass, GEMM1 refills the ring with V's first
//               group in its last group, GEMM2 consumes the ring GEMM1 left;
//   FORM 2 (C): FORM 1 with the Vh fill split around the x3_store8 pass (tile 0 before it, tile 1
//               behind it, before the barrier): the engine's form.
// Reports cycles per iteration (median over the workgroups) and, from a stamped build of the same
// kernel, each GEMM's start-up: s_memtime at the GEMM's entry to s_memtime behind group 0's last
// MFMA (wave 0 of each workgroup, mean over the iterations, median over the workgroups).  The
// outputs of all forms must be bit-identical.
// hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -o bin/ring_prefill tools/ubench/ring_prefill_ubench.hip
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../amp-sparc-spatialmodulation_amd/csrc/amp_persist.h"

using namespace amp;

constexpr int KC = 256, OC = 256, REPS = 20, NWG = 256, G = KC / 32, NC = 2;
constexpr int LDR = 2 * KC + 8;   // the engine's r / x~ row stride (floats)

struct Stamp {
    unsigned long long* t;
    __device__ __forceinline__ void operator()(int g) const {
        if (g == 0) *t = __builtin_amdgcn_s_memtime();
    }
};

template <int FORM, bool STAMP>
__global__ __launch_bounds__(512, 1) void kring(const float* __restrict__ A, const void* w1, const void* w2, float* out,
                                                unsigned long long* cyc) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    unsigned short* sP = reinterpret_cast<unsigned short*>(lds);
    float* sX = lds + 6 * 16 * KC / 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wg = blockIdx.x;
    const int ldx = pl_ldx(KC), cc0 = wave * NC;
    for (int e = tid; e < 16 * 2 * KC; e += 512) sX[(e / (2 * KC)) * LDR + e % (2 * KC)] = A[e];
    __syncthreads();
    f32x4 cr[NC], ci[NC];
    unsigned long long su1 = 0, su2 = 0;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int rep = 0; rep < REPS; ++rep) {
        X3Ring<NC, 1> ring;
        if constexpr (FORM == 1) x3_ring_fill<NC, G, 1>(ring, w1, cc0);
        if constexpr (FORM == 2) {
            x3_ring_fill<NC, G, 1, 0, 1>(ring, w1, cc0);
            __builtin_amdgcn_sched_barrier(0);
        }
        {
            const int tdx = pl_opaque(tid);
            const int row = tdx % 16, j0 = 8 * (tdx / 16);
            float re[8], im[8];
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const float4 x = *reinterpret_cast<const float4*>(sX + row * LDR + 2 * j0 + 4 * h);
                re[2 * h] = x.x; im[2 * h] = x.y; re[2 * h + 1] = x.z; im[2 * h + 1] = x.w;
            }
            x3_store8(sP, ldx, row, j0, re, im);
        }
        if constexpr (FORM == 2) {
            __builtin_amdgcn_sched_barrier(0);
            x3_ring_fill<NC, G, 1, 1, NC>(ring, w1, cc0);
        }
        __syncthreads();
        unsigned long long ta = 0, tb = 0;
        if constexpr (STAMP) ta = __builtin_amdgcn_s_memtime();
        if constexpr (FORM == 0) {
            if constexpr (STAMP) {
                x3_ring_fill<NC, G, 1>(ring, w1, cc0);
                gemm_x3_ring<NC, G, 1, false, true, false>(sP, ldx, w1, cc0, ring, cr, ci, nullptr, Stamp{&tb});
            } else {
                gemm_x3<NC, G, 1, false, true>(sP, ldx, w1, cc0, cr, ci);
            }
        } else {
            if constexpr (STAMP) gemm_x3_ring<NC, G, 1, false, true, true>(sP, ldx, w1, cc0, ring, cr, ci, w2, Stamp{&tb});
            else gemm_x3_ring<NC, G, 1, false, true, true>(sP, ldx, w1, cc0, ring, cr, ci, w2);
        }
        if constexpr (STAMP) su1 += tb - ta;
        __syncthreads();
        {
            const int lnx = pl_opaque(lane);
#pragma unroll
            for (int t = 0; t < NC; ++t) {
                float wr[4], wi[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { wr[r] = cr[t][r]; wi[r] = ci[t][r]; }
                x3_store_acc(sP, ldx, 16 * (cc0 + t) + (lnx & 15), wr, wi);
            }
        }
        __syncthreads();
        if constexpr (STAMP) ta = __builtin_amdgcn_s_memtime();
        if constexpr (FORM == 0) {
            if constexpr (STAMP) {
                x3_ring_fill<NC, G, 1>(ring, w2, cc0);
                gemm_x3_ring<NC, G, 1, false, true, false>(sP, ldx, w2, cc0, ring, cr, ci, nullptr, Stamp{&tb});
            } else {
                gemm_x3<NC, G, 1, false, true>(sP, ldx, w2, cc0, cr, ci);
            }
        } else {
            if constexpr (STAMP) gemm_x3_ring<NC, G, 1, false, true, false>(sP, ldx, w2, cc0, ring, cr, ci, nullptr, Stamp{&tb});
            else gemm_x3_ring<NC, G, 1, false, true>(sP, ldx, w2, cc0, ring, cr, ci);
        }
        if constexpr (STAMP) su2 += tb - ta;
        __syncthreads();
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (wg == 0) {
        for (int t = 0; t < NC; ++t)
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * (lane >> 4) + r, o = 16 * (cc0 + t) + (lane & 15);
                out[(row * OC + o) * 2] = cr[t][r];
                out[(row * OC + o) * 2 + 1] = ci[t][r];
            }
    }
    if (tid == 0) { cyc[wg] = t1 - t0; cyc[NWG + wg] = su1; cyc[2 * NWG + wg] = su2; }
}

static unsigned short bf16_rn(float x) {
    unsigned u;
    memcpy(&u, &x, 4);
    const unsigned r = 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)((u + r) >> 16);
}
static float bf2f(unsigned short h) {
    unsigned u = (unsigned)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static void split3(float x, unsigned short p[3]) {
    p[0] = bf16_rn(x);
    const float r1 = x - bf2f(p[0]);
    p[1] = bf16_rn(r1);
    const float r2 = r1 - bf2f(p[1]);
    p[2] = bf16_rn(r2);
}

static double med(std::vector<unsigned long long> c) {
    std::sort(c.begin(), c.end());
    return (double)c[c.size() / 2];
}

template <int FORM, bool STAMP>
static std::vector<float> run(const float* dA, void* dW1, void* dW2) {
    float* dO;
    unsigned long long* dc;
    hipMalloc(&dO, 16 * OC * 2 * 4);
    hipMalloc(&dc, 3 * NWG * 8);
    const size_t lds = 6 * 16 * KC * 2 + 16 * LDR * 4;
    hipFuncSetAttribute((const void*)kring<FORM, STAMP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    for (int i = 0; i < 4; ++i) hipLaunchKernelGGL((kring<FORM, STAMP>), dim3(NWG), dim3(512), lds, 0, dA, dW1, dW2, dO, dc);
    hipDeviceSynchronize();
    std::vector<unsigned long long> c(3 * NWG, 0);
    hipMemcpy(c.data(), dc, c.size() * 8, hipMemcpyDeviceToHost);
    std::vector<float> o(16 * OC * 2);
    hipMemcpy(o.data(), dO, o.size() * 4, hipMemcpyDeviceToHost);
    std::vector<unsigned long long> it(c.begin(), c.begin() + NWG), s1(c.begin() + NWG, c.begin() + 2 * NWG),
        s2(c.begin() + 2 * NWG, c.end());
    std::sort(it.begin(), it.end());
    if (STAMP)
        printf("form %c (stamped): start-up, entry -> behind group 0's last MFMA: GEMM1 median %.0f  GEMM2 median %.0f cycles"
               "   (iteration median %.0f)\n", "ABC"[FORM], med(s1) / REPS, med(s2) / REPS, (double)it[NWG / 2] / REPS);
    else
        printf("form %c: cycles per iteration median %.0f  p10 %.0f  p90 %.0f  max %.0f\n", "ABC"[FORM],
               (double)it[NWG / 2] / REPS, (double)it[NWG / 10] / REPS, (double)it[NWG * 9 / 10] / REPS,
               (double)it[NWG - 1] / REPS);
    hipFree(dO);
    hipFree(dc);
    return o;
}

int main() {
    srand(1);
    auto rnd = [] { return (float)rand() / RAND_MAX * 2.f - 1.f; };
    std::vector<float> A(16 * KC * 2), X(OC * KC * 2);
    for (auto& v : A) v = rnd();
    for (auto& v : X) v = rnd() * 0.0625f;
    std::vector<unsigned short> wp((size_t)(OC / 16) * G * 6 * 64 * 8);
    for (int o = 0; o < OC; ++o)
        for (int k = 0; k < KC; ++k) {
            unsigned short p[3], q[3];
            split3(X[(o * KC + k) * 2], p);
            split3(X[(o * KC + k) * 2 + 1], q);
            const int ct = o >> 4, g = k >> 5, kk = k & 31, lane = (o & 15) + 16 * (kk >> 3), j = kk & 7;
            for (int s = 0; s < 3; ++s) {
                wp[((((size_t)ct * G + g) * 6 + s) * 64 + lane) * 8 + j] = p[s];
                wp[((((size_t)ct * G + g) * 6 + 3 + s) * 64 + lane) * 8 + j] = q[s];
            }
        }
    int ncu = 0;
    hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0);
    if (ncu < NWG) {
        printf("needs %d CUs (one workgroup each), device has %d\n", NWG, ncu);
        return 1;
    }
    float* dA;
    void *dW1, *dW2;
    hipMalloc(&dA, A.size() * 4);
    hipMalloc(&dW1, wp.size() * 2);
    hipMalloc(&dW2, wp.size() * 2);
    hipMemcpy(dA, A.data(), A.size() * 4, hipMemcpyHostToDevice);
    hipMemcpy(dW1, wp.data(), wp.size() * 2, hipMemcpyHostToDevice);
    std::reverse(wp.begin(), wp.end());   // (another operator for GEMM2)
    hipMemcpy(dW2, wp.data(), wp.size() * 2, hipMemcpyHostToDevice);
    bool same = true;
    for (int it = 0; it < 3; ++it) {
        const std::vector<float> a = run<0, false>(dA, dW1, dW2);
        const std::vector<float> b = run<1, false>(dA, dW1, dW2);
        const std::vector<float> c = run<2, false>(dA, dW1, dW2);
        same = same && memcmp(a.data(), b.data(), a.size() * 4) == 0 && memcmp(a.data(), c.data(), a.size() * 4) == 0;
    }
    for (int it = 0; it < 2; ++it) {
        const std::vector<float> a = run<0, true>(dA, dW1, dW2);
        const std::vector<float> b = run<1, true>(dA, dW1, dW2);
        const std::vector<float> c = run<2, true>(dA, dW1, dW2);
        same = same && memcmp(a.data(), b.data(), a.size() * 4) == 0 && memcmp(a.data(), c.data(), a.size() * 4) == 0;
    }
    double mx = 0;
    {
        const std::vector<float> a = run<0, false>(dA, dW1, dW2);
        for (float v : a) mx = std::max(mx, (double)fabsf(v));
    }
    printf("outputs of forms A, B and C bit-identical: %s  (max |C| %.3f)\n", same ? "yes" : "NO", mx);
    return same ? 0 : 2;
}

// amp_denoise.h — block-sparse constellation denoiser (posterior mean/variance of a
// section holding exactly one nonzero drawn from the constellation).
//
// Restates VAMPLayer.segmented_denoiser (vamp.py:96-119), BAMPLayer.segmented_denoiser
// (bamp.py:66-77) and SCAMPLayer.denoiser (scamp.py:61-68):
//   xi[m,k]   = Re((r_m / tau_m) * conj(a_k))
//   eta[m,k]  = exp(xi[m,k] - shift)
//   xmmse_m   = sum_k a_k eta[m,k] / Z,      Z = sum_{m,k} eta
//   var_m     = |xmmse_m|^2 (1 - P_m) + sum_k |xmmse_m - a_k|^2 eta[m,k] / Z,  P_m = sum_k eta[m,k] / Z
//
// Fast path: each section is shifted by its OWN max (the softmax is shift-invariant): float32
// logits, exp((xi - max) * log2 e) as one v_mul + v_exp_f32 (scaling AFTER the subtraction keeps
// the dominant weights' exponents exact; folding log2 e into the symbols costs one more
// rounding of |xi| and measurably moves the allclose early exit), float32 sums per position,
// float64 section sum Z so that 1 - P_m = (Z - Z_m)/Z has no cancellation.
// The reference shifts by max|xi| over the WHOLE batch in float64 (vamp.py:112); the few
// sections for which that matters (normaliser out of the normal float64 range) are redone by
// exact_section_f64 after the batch reduction — the fast path reports per section its max
// logit and its max |logit| (natural units) for that decision.
//
// Mapping: one section per group of G = min(M, 64) lanes (M a power of two), each lane owns
// PPL = M / G positions; reductions are xor-shuffles inside the group.
#pragma once

#include <float.h>

#include "amp_common.h"

namespace amp {

#define AMP_LOG2E 1.44269504088896340736f

// Diagnostic precision switches (default 0: the product arithmetic).  AMP_DEN_EXACT_EXP: every
// softmax weight as float(exp(double(x) - double(m))) (correctly rounded); AMP_DEN_DIV: 1 / Z by
// an IEEE division instead of v_rcp_f32.  tools/den_isolate.py measures their effect on the
// early exit.
#ifndef AMP_DEN_EXACT_EXP
#define AMP_DEN_EXACT_EXP 0
#endif
#ifndef AMP_DEN_DIV
#define AMP_DEN_DIV 0
#endif
// exp(x - m) for a logit x and its shift m (natural units)
__device__ __forceinline__ float den_exp(float x, float m) {
#if AMP_DEN_EXACT_EXP
    return (float)exp((double)x - (double)m);
#else
    return __builtin_amdgcn_exp2f((x - m) * AMP_LOG2E);
#endif
}
__device__ __forceinline__ float den_rcp(float z) {
#if AMP_DEN_DIV
    return 1.0f / z;
#else
    return __builtin_amdgcn_rcpf(z);
#endif
}

// Which waves of the workgroup share a denoiser call: this wave's index among them and their
// count (default: every wave of the workgroup).  The wave-specialized engine
// (amp_vamp_persist_kernel.h, WS) hands half the sections to a subset of its waves.
struct DenWaves {
    int wave, nw;
    __device__ static DenWaves block() { return DenWaves{(int)(threadIdx.x >> 6), (int)(blockDim.x >> 6)}; }
};

// A uniform kernel-argument value taken through readfirstlane: the loads stay scalar loads of
// the kernarg segment (left alone, memcpyopt merged consecutive constellation loads into a copy
// of c.re into a private array, i.e. scratch memory, once Const held 64 points).
__device__ __forceinline__ float kval(const float& x) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}

// Policy interface (per lane; `sec` is the caller's local section id):
//   void load(int sec, int m, float& rr, float& ri, float& inv_tau) const;
//   void store(int sec, int m, float xr, float xi, float var, PartAcc& pa) const;
//   void section(int sec, float secmax, float secabs) const;     // group lane 0
// KK: the constellation size as a compile-time constant (1, 2, 4, 8, 16 or 64).
//
// M <= 64 form (G = M lanes per section, compile-time): one position per lane, U sections
// per lane group in flight (independent dependency chains for the scheduler).  Everything is
// float32: Z and the exclusive sums Z - Z_m by group_sum_excl_c, 1 / Z by v_rcp_f32 (Z >= 1:
// the section max term is exp(0)).  The constellation is held in VGPRs (uniform values, but
// as SGPR operands they spill in the big fused kernels).  Section statistics (max logit,
// max |logit|, non-finite input) are kept per lane in float32 and folded into the float64
// PartAcc once at the end.
template <bool kVar, int KK, int U, int G, class P>
__device__ __forceinline__ void denoise_sections_g(const P& pol, int nsec, const Const& c, PartAcc& pa, DenWaves dw = DenWaves::block()) {
    const int lane = threadIdx.x & 63, wave = dw.wave;
    constexpr int gpw = 64 / G;
    const int gid = lane / G, g = lane % G;
    const int nw = dw.nw;
    float cre[KK], cim[KK];
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        cre[k] = kval(c.re[k]); cim[k] = kval(c.im[k]);
        asm volatile("" : "+v"(cre[k]), "+v"(cim[k]));
    }
    float st_abs = 0.f, st_min = INFINITY;
    bool st_bad = false;
    for (int base = wave * gpw * U; base < nsec; base += nw * gpw * U) {   // wave-uniform trip count
        int sec[U];
        bool act[U];
        float xk[U][KK], smax[U], sabs[U];
        float ur[U], ui[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            sec[u] = base + u * gpw + gid;
            act[u] = sec[u] < nsec;
            float rr, ri, it;
            pol.load(act[u] ? sec[u] : nsec - 1, g, rr, ri, it);
            ur[u] = rr * it; ui[u] = ri * it;   // c64 / f32 == multiply by the reciprocal
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (act[u]) st_bad |= !(fabsf(ur[u]) <= FLT_MAX && fabsf(ui[u]) <= FLT_MAX);
            float lmax = -FLT_MAX, lmin = FLT_MAX;
#pragma unroll
            for (int k = 0; k < KK; ++k) {
                xk[u][k] = fmaf(ur[u], cre[k], ui[u] * cim[k]);
                lmax = fmaxf(lmax, xk[u][k]);
                lmin = fminf(lmin, xk[u][k]);
            }
            smax[u] = lmax;
            sabs[u] = fmaxf(lmax, -lmin);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) { smax[u] = group_fmax_c<G>(smax[u]); sabs[u] = group_fmax_c<G>(sabs[u]); }
        float zt[U], ze[U], sr[U], si[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float zm = 0.f, a = 0.f, b = 0.f;
#pragma unroll
            for (int k = 0; k < KK; ++k) {
                const float e = den_exp(xk[u][k], smax[u]);
                xk[u][k] = e;
                zm += e;
                a = fmaf(cre[k], e, a);
                b = fmaf(cim[k], e, b);
            }
            zt[u] = zm; ze[u] = 0.f; sr[u] = a; si[u] = b;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) group_sum_excl_c<G>(zt[u], ze[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float iz = den_rcp(zt[u]);
            const float xr = sr[u] * iz, xi = si[u] * iz;
            float var = 0.f;
            if (kVar) {
                float vs = 0.f;
#pragma unroll
                for (int k = 0; k < KK; ++k) {
                    const float dr = xr - cre[k], di = xi - cim[k];
                    vs = fmaf(fmaf(dr, dr, di * di), xk[u][k], vs);
                }
                var = (xr * xr + xi * xi) * (ze[u] * iz) + vs * iz;
            }
            if (act[u]) {
                pol.store(sec[u], g, xr, xi, var, pa);
                st_abs = nan_max(st_abs, sabs[u]);
                st_min = nan_min(st_min, smax[u]);
                if (g == 0) pol.section(sec[u], smax[u], sabs[u]);
            }
        }
    }
    pa.maxabs = st_bad ? __longlong_as_double(0x7ff8000000000000LL) : nan_max(pa.maxabs, (double)st_abs);
    pa.minsecmax = nan_min(pa.minsecmax, (double)st_min);
}

// Packed-math form of denoise_sections_g (KK even): the per-symbol work runs on
// v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 over pairs — two symbols per instruction for
// the logits and their shift, the (re, im) pair for the sums and the variance — so one
// position costs ~140 VALU instructions instead of ~300.  Same rounding per element as the
// scalar form (each packed lane is the same IEEE operation).
typedef float f32x2 __attribute__((ext_vector_type(2)));

// The constellation as packed operands, kept in VGPRs: (re_k, re_k+1), (im_k, im_k+1) and
// (re_k, im_k).
template <int KK>
struct DenRegs {
    f32x2 pre[KK / 2], pim[KK / 2], sym[KK];
    __device__ __forceinline__ void load(const Const& c) {
#pragma unroll
        for (int h = 0; h < KK / 2; ++h) {
            pre[h] = f32x2{kval(c.re[2 * h]), kval(c.re[2 * h + 1])};
            pim[h] = f32x2{kval(c.im[2 * h]), kval(c.im[2 * h + 1])};
            asm volatile("" : "+v"(pre[h]), "+v"(pim[h]));
        }
#pragma unroll
        for (int k = 0; k < KK; ++k) {
            sym[k] = f32x2{kval(c.re[k]), kval(c.im[k])};
            asm volatile("" : "+v"(sym[k]));
        }
    }
};

// Diagnostic hook (amp_vamp_debug_dump): a policy may record the intermediate ze / vs of the
// variance; the generic form records nothing.
template <class P>
__device__ __forceinline__ void den_debug(const P&, int, int, float, float) {}

// Per-lane section statistics, folded into the float64 PartAcc once at the end.
struct DenStat {
    float st_abs = 0.f, st_min = INFINITY;
    bool st_bad = false;
    __device__ __forceinline__ void fold(PartAcc& pa) const {
        pa.maxabs = st_bad ? __longlong_as_double(0x7ff8000000000000LL) : nan_max(pa.maxabs, (double)st_abs);
        pa.minsecmax = nan_min(pa.minsecmax, (double)st_min);
    }
};

// One step of the packed denoiser: sections base + u * gpw + gid (u < U) of this wave.
// FULL: every one of them exists (< nsec): no branches at all, so the step can be scheduled
// into a surrounding MFMA stream (the section statistics are then stored by every lane of the
// group — the same value).
template <bool kVar, int KK, int U, int G, bool FULL, class P>
__device__ __forceinline__ void denoise_step_gp(const P& pol, int base, int nsec, const DenRegs<KK>& R, PartAcc& pa,
                                                DenStat& S) {
    static_assert(KK % 2 == 0, "packed form needs an even constellation size");
    constexpr int KH = KK / 2;
    const int lane = threadIdx.x & 63;
    constexpr int gpw = 64 / G;
    const int gid = lane / G, g = lane % G;
    int sec[U];
    bool act[U];
    f32x2 xk[U][KH];
    float smax[U], sabs[U], ur[U], ui[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        sec[u] = base + u * gpw + gid;
        act[u] = FULL || sec[u] < nsec;
        float rr, ri, it;
        pol.load(act[u] ? sec[u] : nsec - 1, g, rr, ri, it);
        ur[u] = rr * it; ui[u] = ri * it;   // c64 / f32 == multiply by the reciprocal
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool bad = !(fabsf(ur[u]) <= FLT_MAX && fabsf(ui[u]) <= FLT_MAX);
        S.st_bad |= act[u] && bad;
        const f32x2 u2 = f32x2{ur[u], ur[u]}, v2 = f32x2{ui[u], ui[u]};
        float lmax = -FLT_MAX, lmin = FLT_MAX;
#pragma unroll
        for (int h = 0; h < KH; ++h) {
            xk[u][h] = __builtin_elementwise_fma(u2, R.pre[h], v2 * R.pim[h]);
            lmax = fmaxf(lmax, fmaxf(xk[u][h].x, xk[u][h].y));
            lmin = fminf(lmin, fminf(xk[u][h].x, xk[u][h].y));
        }
        smax[u] = lmax;
        sabs[u] = fmaxf(lmax, -lmin);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) { smax[u] = group_fmax_c<G>(smax[u]); sabs[u] = group_fmax_c<G>(sabs[u]); }
    float zt[U], ze[U];
    f32x2 s2[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const f32x2 m2 = f32x2{smax[u], smax[u]};
        const f32x2 l2 = f32x2{AMP_LOG2E, AMP_LOG2E};
        f32x2 z2 = f32x2{0.f, 0.f}, a2 = f32x2{0.f, 0.f};
#pragma unroll
        for (int h = 0; h < KH; ++h) {
#if AMP_DEN_EXACT_EXP
            const f32x2 e = f32x2{den_exp(xk[u][h].x, smax[u]), den_exp(xk[u][h].y, smax[u])};
            (void)m2; (void)l2;
#else
            const f32x2 d = (xk[u][h] - m2) * l2;
            const f32x2 e = f32x2{__builtin_amdgcn_exp2f(d.x), __builtin_amdgcn_exp2f(d.y)};
#endif
            xk[u][h] = e;
            z2 += e;
            a2 = __builtin_elementwise_fma(R.sym[2 * h], f32x2{e.x, e.x}, a2);
            a2 = __builtin_elementwise_fma(R.sym[2 * h + 1], f32x2{e.y, e.y}, a2);
        }
        zt[u] = z2.x + z2.y; ze[u] = 0.f; s2[u] = a2;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) group_sum_excl_c<G>(zt[u], ze[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const float iz = den_rcp(zt[u]);
        const f32x2 x2 = s2[u] * f32x2{iz, iz};
        float var = 0.f;
        if (kVar) {
            f32x2 v2 = f32x2{0.f, 0.f};
#pragma unroll
            for (int h = 0; h < KH; ++h) {
                const f32x2 d0 = x2 - R.sym[2 * h], d1 = x2 - R.sym[2 * h + 1];
                v2 = __builtin_elementwise_fma(d0 * d0, f32x2{xk[u][h].x, xk[u][h].x}, v2);
                v2 = __builtin_elementwise_fma(d1 * d1, f32x2{xk[u][h].y, xk[u][h].y}, v2);
            }
            var = (x2.x * x2.x + x2.y * x2.y) * (ze[u] * iz) + (v2.x + v2.y) * iz;
            den_debug(pol, sec[u], g, ze[u], v2.x + v2.y);
        }
        if (FULL) {
            pol.store(sec[u], g, x2.x, x2.y, var, pa);
            S.st_abs = nan_max(S.st_abs, sabs[u]);
            S.st_min = nan_min(S.st_min, smax[u]);
            pol.section(sec[u], smax[u], sabs[u]);
        } else if (act[u]) {
            pol.store(sec[u], g, x2.x, x2.y, var, pa);
            S.st_abs = nan_max(S.st_abs, sabs[u]);
            S.st_min = nan_min(S.st_min, smax[u]);
            if (g == 0) pol.section(sec[u], smax[u], sabs[u]);
        }
    }
}

// ---- Product-grid form (square QAM-like alphabets: Const::grid == R) ----
// Every point is (gre[i], gim[j]) of an R x R grid, so the logits and their exponentials factor
// over rows and columns:
//   xi_ij = X_i + Y_j,   X_i = Re(r / tau) gre_i,   Y_j = Im(r / tau) gim_j
//   exp(xi_ij - smax) = er_i ei_j f,  er_i = exp(X_i - max X), ei_j = exp(Y_j - max Y),
//                                     f = exp(max X + max Y - smax)
// and every per-position sum of vamp.py:113-118 is a sum over rows of a row factor times a
// column sum weighted by the table's multiplicities c_ij (0, 1, 2; all 1 for a full grid):
//   z_m = f sum_i er_i S_i,           S_i = sum_j c_ij ei_j
//   sum_k a_k eta_k = f (sum_i gre_i er_i S_i, sum_i er_i T_i),   T_i = sum_j c_ij gim_j ei_j
//   sum_k |x - a_k|^2 eta_k = f sum_i er_i ((Re x - gre_i)^2 S_i + V_i),
//                                     V_i = sum_j c_ij (Im x - gim_j)^2 ei_j
// A position costs 2R + 1 exponentials and O(R^2) FMAs (O(R) for a full grid) instead of K
// exponentials and ~12 K operations.  Every sum adds non-negative terms (a missing grid point
// has weight 0: nothing is subtracted), so nothing cancels; the float32 rounding differs from
// the direct form by a few ulp (the reference works in float64 throughout).  The max / min
// logit of a position are max X + max Y / min X + min Y: a linear form over the grid takes its
// extremes at the corners, which are in the table (checked on the host, amp_host.h).
// Multiplicity patterns of the grid points (compile-time, so the unrolled sums below fold:
// weight 0 drops a term, 1 is an add, 2 an FMA by 2):
//   GRID_FULL  every grid point once (QPSK, square 64-QAM);
//   GRID_REF16 the reference's 16-QAM table (config.py:112) on the sorted grid
//              {-3,-1,1,3}/sqrt(10): -1+3j twice, 1-3j missing.
enum { GRID_FULL = 1, GRID_REF16 = 2 };
template <int PAT>
__device__ __forceinline__ constexpr float grid_cnt(int i, int j) {
    if constexpr (PAT == GRID_REF16) return (i == 1 && j == 3) ? 2.f : (i == 2 && j == 0) ? 0.f : 1.f;
    else return 1.f;
}

template <int R>
struct GridRegs {
    float re[R], im[R];
    __device__ __forceinline__ void load(const Const& c) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            re[i] = kval(c.gre[i]); im[i] = kval(c.gim[i]);
            asm volatile("" : "+v"(re[i]), "+v"(im[i]));
        }
    }
};

template <bool kVar, int R, int PAT, int U, int G, class P>
__device__ __forceinline__ void denoise_step_grid(const P& pol, int base, int nsec, const GridRegs<R>& Q,
                                                  PartAcc& pa, DenStat& S) {
    constexpr bool FULLG = PAT == GRID_FULL;
    const int lane = threadIdx.x & 63;
    constexpr int gpw = 64 / G;
    const int gid = lane / G, g = lane % G;
    int sec[U];
    bool act[U];
    float X[U][R], Y[U][R], mx[U], my[U], lmx[U], smax[U], sabs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        sec[u] = base + u * gpw + gid;
        act[u] = sec[u] < nsec;
        float rr, ri, it;
        pol.load(act[u] ? sec[u] : nsec - 1, g, rr, ri, it);
        const float ur = rr * it, ui = ri * it;   // c64 / f32 == multiply by the reciprocal
        S.st_bad |= act[u] && !(fabsf(ur) <= FLT_MAX && fabsf(ui) <= FLT_MAX);
        float ax = -FLT_MAX, nx = FLT_MAX, ay = -FLT_MAX, ny = FLT_MAX;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            X[u][i] = ur * Q.re[i];
            Y[u][i] = ui * Q.im[i];
            ax = fmaxf(ax, X[u][i]); nx = fminf(nx, X[u][i]);
            ay = fmaxf(ay, Y[u][i]); ny = fminf(ny, Y[u][i]);
        }
        mx[u] = ax; my[u] = ay;
        lmx[u] = ax + ay;                          // max logit of the position (a corner)
        smax[u] = lmx[u];
        sabs[u] = fmaxf(lmx[u], -(nx + ny));       // max |logit|
    }
#pragma unroll
    for (int u = 0; u < U; ++u) { smax[u] = group_fmax_c<G>(smax[u]); sabs[u] = group_fmax_c<G>(sabs[u]); }
    float zt[U], ze[U], ar[U], ai[U], f[U];
    float er[U][R], ei[U][R], Sr[U][FULLG ? 1 : R];
    float SI[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        f[u] = den_exp(lmx[u], smax[u]);
#pragma unroll
        for (int i = 0; i < R; ++i) {
            er[u][i] = den_exp(X[u][i], mx[u]);
            ei[u][i] = den_exp(Y[u][i], my[u]);
        }
        if constexpr (FULLG) {
            float sr = 0.f, si = 0.f, a = 0.f, b = 0.f;
#pragma unroll
            for (int i = 0; i < R; ++i) {
                sr += er[u][i]; si += ei[u][i];
                a = fmaf(Q.re[i], er[u][i], a);
                b = fmaf(Q.im[i], ei[u][i], b);
            }
            SI[u] = si; Sr[u][0] = sr;
            zt[u] = (sr * si) * f[u];
            ar[u] = (a * si) * f[u];
            ai[u] = (sr * b) * f[u];
        } else {
            float z = 0.f, a = 0.f, b = 0.f, w[R];
#pragma unroll
            for (int j = 0; j < R; ++j) w[j] = Q.im[j] * ei[u][j];
#pragma unroll
            for (int i = 0; i < R; ++i) {
                float si = 0.f, ti = 0.f;
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const float cw = grid_cnt<PAT>(i, j);
                    if (cw == 1.f) { si += ei[u][j]; ti += w[j]; }
                    else if (cw == 2.f) { si = fmaf(2.f, ei[u][j], si); ti = fmaf(2.f, w[j], ti); }
                }
                Sr[u][i] = si;
                const float es = er[u][i] * si;
                z += es;
                a = fmaf(Q.re[i], es, a);
                b = fmaf(er[u][i], ti, b);
            }
            zt[u] = z * f[u];
            ar[u] = a * f[u];
            ai[u] = b * f[u];
        }
        ze[u] = 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) group_sum_excl_c<G>(zt[u], ze[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const float iz = den_rcp(zt[u]);
        const float xr = ar[u] * iz, xi = ai[u] * iz;
        float var = 0.f;
        if (kVar) {
            float vs;
            if constexpr (FULLG) {
                float vr = 0.f, vi = 0.f;
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const float dr = xr - Q.re[i], di = xi - Q.im[i];
                    vr = fmaf(dr * dr, er[u][i], vr);
                    vi = fmaf(di * di, ei[u][i], vi);
                }
                vs = fmaf(vr, SI[u], Sr[u][0] * vi) * f[u];
            } else {
                float d[R];
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const float di = xi - Q.im[j];
                    d[j] = (di * di) * ei[u][j];
                }
                float acc = 0.f;
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    float vi = 0.f;
#pragma unroll
                    for (int j = 0; j < R; ++j) {
                        const float cw = grid_cnt<PAT>(i, j);
                        if (cw == 1.f) vi += d[j];
                        else if (cw == 2.f) vi = fmaf(2.f, d[j], vi);
                    }
                    const float dr = xr - Q.re[i];
                    acc = fmaf(er[u][i], fmaf(dr * dr, Sr[u][i], vi), acc);
                }
                vs = acc * f[u];
            }
            var = (xr * xr + xi * xi) * (ze[u] * iz) + vs * iz;
        }
        if (act[u]) {
            pol.store(sec[u], g, xr, xi, var, pa);
            S.st_abs = nan_max(S.st_abs, sabs[u]);
            S.st_min = nan_min(S.st_min, smax[u]);
            if (g == 0) pol.section(sec[u], smax[u], sabs[u]);
        }
    }
}

// denoise_step_grid with U = 2 written on float pairs (one element per section in flight): the
// same operations in the same order per element — bit-identical results — issued as packed
// v_pk_mul / v_pk_add / v_pk_fma (two positions per instruction); max / min, exp, rcp and the
// DPP reductions stay per element.
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2v f2fma(f2v a, f2v b, f2v c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2v f2splat(float v) { return f2v{v, v}; }

template <bool kVar, int R, int PAT, int G, class P>
__device__ __forceinline__ void denoise_step_grid2(const P& pol, int base, int nsec, const GridRegs<R>& Q,
                                                   PartAcc& pa, DenStat& S) {
    constexpr bool FULLG = PAT == GRID_FULL;
    const int lane = threadIdx.x & 63;
    constexpr int gpw = 64 / G;
    const int gid = lane / G, g = lane % G;
    int sec[2];
    bool act[2];
    f2v ur, ui;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        sec[u] = base + u * gpw + gid;
        act[u] = sec[u] < nsec;
        float rr, ri, it;
        pol.load(act[u] ? sec[u] : nsec - 1, g, rr, ri, it);
        ur[u] = rr * it;   // c64 / f32 == multiply by the reciprocal
        ui[u] = ri * it;
        S.st_bad |= act[u] && !(fabsf(ur[u]) <= FLT_MAX && fabsf(ui[u]) <= FLT_MAX);
    }
    f2v X[R], Y[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        X[i] = ur * f2splat(Q.re[i]);
        Y[i] = ui * f2splat(Q.im[i]);
    }
    f2v mx, my, lmx, smax, sabs;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        float ax = -FLT_MAX, nx = FLT_MAX, ay = -FLT_MAX, ny = FLT_MAX;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            ax = fmaxf(ax, X[i][u]); nx = fminf(nx, X[i][u]);
            ay = fmaxf(ay, Y[i][u]); ny = fminf(ny, Y[i][u]);
        }
        mx[u] = ax; my[u] = ay;
        lmx[u] = ax + ay;                          // max logit of the position (a corner)
        smax[u] = group_fmax_c<G>(lmx[u]);
        sabs[u] = group_fmax_c<G>(fmaxf(lmx[u], -(nx + ny)));   // max |logit|
    }
    const f2v l2e = f2splat(AMP_LOG2E);
#if AMP_DEN_EXACT_EXP
    f2v f = {den_exp(lmx.x, smax.x), den_exp(lmx.y, smax.y)};
#else
    f2v targ = (lmx - smax) * l2e;
    f2v f = {__builtin_amdgcn_exp2f(targ.x), __builtin_amdgcn_exp2f(targ.y)};
#endif
    f2v er[R], ei[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
#if AMP_DEN_EXACT_EXP
        er[i] = f2v{den_exp(X[i].x, mx.x), den_exp(X[i].y, mx.y)};
        ei[i] = f2v{den_exp(Y[i].x, my.x), den_exp(Y[i].y, my.y)};
#else
        const f2v xa = (X[i] - mx) * l2e, ya = (Y[i] - my) * l2e;
        er[i] = f2v{__builtin_amdgcn_exp2f(xa.x), __builtin_amdgcn_exp2f(xa.y)};
        ei[i] = f2v{__builtin_amdgcn_exp2f(ya.x), __builtin_amdgcn_exp2f(ya.y)};
#endif
    }
    f2v zt, ar, ai, SI = f2splat(0.f);
    f2v Sr[FULLG ? 1 : R];
    if constexpr (FULLG) {
        f2v sr = f2splat(0.f), si = f2splat(0.f), a = f2splat(0.f), b = f2splat(0.f);
#pragma unroll
        for (int i = 0; i < R; ++i) {
            sr += er[i]; si += ei[i];
            a = f2fma(f2splat(Q.re[i]), er[i], a);
            b = f2fma(f2splat(Q.im[i]), ei[i], b);
        }
        SI = si; Sr[0] = sr;
        zt = (sr * si) * f;
        ar = (a * si) * f;
        ai = (sr * b) * f;
    } else {
        f2v z = f2splat(0.f), a = f2splat(0.f), b = f2splat(0.f), w[R];
#pragma unroll
        for (int j = 0; j < R; ++j) w[j] = f2splat(Q.im[j]) * ei[j];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            f2v si = f2splat(0.f), ti = f2splat(0.f);
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const float cw = grid_cnt<PAT>(i, j);
                if (cw == 1.f) { si += ei[j]; ti += w[j]; }
                else if (cw == 2.f) { si = f2fma(f2splat(2.f), ei[j], si); ti = f2fma(f2splat(2.f), w[j], ti); }
            }
            Sr[i] = si;
            const f2v es = er[i] * si;
            z += es;
            a = f2fma(f2splat(Q.re[i]), es, a);
            b = f2fma(er[i], ti, b);
        }
        zt = z * f;
        ar = a * f;
        ai = b * f;
    }
    float ze[2] = {0.f, 0.f}, zt1[2] = {zt.x, zt.y};
#pragma unroll
    for (int u = 0; u < 2; ++u) group_sum_excl_c<G>(zt1[u], ze[u]);
    const f2v iz = {den_rcp(zt1[0]), den_rcp(zt1[1])};
    const f2v xr = ar * iz, xi = ai * iz;
    f2v var = f2splat(0.f);
    if (kVar) {
        f2v vs;
        if constexpr (FULLG) {
            f2v vr = f2splat(0.f), vi = f2splat(0.f);
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const f2v dr = xr - f2splat(Q.re[i]), di = xi - f2splat(Q.im[i]);
                vr = f2fma(dr * dr, er[i], vr);
                vi = f2fma(di * di, ei[i], vi);
            }
            vs = f2fma(vr, SI, Sr[0] * vi) * f;
        } else {
            f2v d[R];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const f2v di = xi - f2splat(Q.im[j]);
                d[j] = (di * di) * ei[j];
            }
            f2v acc = f2splat(0.f);
#pragma unroll
            for (int i = 0; i < R; ++i) {
                f2v vi = f2splat(0.f);
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const float cw = grid_cnt<PAT>(i, j);
                    if (cw == 1.f) vi += d[j];
                    else if (cw == 2.f) vi = f2fma(f2splat(2.f), d[j], vi);
                }
                const f2v dr = xr - f2splat(Q.re[i]);
                acc = f2fma(er[i], f2fma(dr * dr, Sr[i], vi), acc);
            }
            vs = acc * f;
        }
        const f2v zev = {ze[0], ze[1]};
        var = (xr * xr + xi * xi) * (zev * iz) + vs * iz;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        if (act[u]) {
            pol.store(sec[u], g, xr[u], xi[u], var[u], pa);
            S.st_abs = nan_max(S.st_abs, sabs[u]);
            S.st_min = nan_min(S.st_min, smax[u]);
            if (g == 0) pol.section(sec[u], smax[u], sabs[u]);
        }
    }
}

// denoise_step_grid2's arithmetic on the scaled inputs (ur, ui) of its two sections, for the
// full-round step below: the posterior mean (xr, xi), the variance and the sections' max logit /
// max |logit|.  A restatement, operation for operation, and not a function both steps share: the
// engines that keep denoise_step_grid2 must keep their code objects unchanged.
// mid(er, ei): called between the exponentials and the section sums (DenPrio below; the default: no code).
struct DenNoMid {
    template <class T>
    __device__ __forceinline__ void operator()(T&, T&) const {}
};
template <bool kVar, int R, int PAT, int G, class Mid = DenNoMid>
__device__ __forceinline__ void grid2_core(const f2v ur, const f2v ui, const GridRegs<R>& Q, f2v& xr_out, f2v& xi_out,
                                           f2v& var_out, f2v& smax_out, f2v& sabs_out, Mid&& mid = Mid()) {
    constexpr bool FULLG = PAT == GRID_FULL;
    f2v X[R], Y[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        X[i] = ur * f2splat(Q.re[i]);
        Y[i] = ui * f2splat(Q.im[i]);
    }
    f2v mx, my, lmx, smax, sabs;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        float ax = -FLT_MAX, nx = FLT_MAX, ay = -FLT_MAX, ny = FLT_MAX;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            ax = fmaxf(ax, X[i][u]); nx = fminf(nx, X[i][u]);
            ay = fmaxf(ay, Y[i][u]); ny = fminf(ny, Y[i][u]);
        }
        mx[u] = ax; my[u] = ay;
        lmx[u] = ax + ay;                          // max logit of the position (a corner)
        smax[u] = group_fmax_c<G>(lmx[u]);
        sabs[u] = group_fmax_c<G>(fmaxf(lmx[u], -(nx + ny)));   // max |logit|
    }
    const f2v l2e = f2splat(AMP_LOG2E);
#if AMP_DEN_EXACT_EXP
    f2v f = {den_exp(lmx.x, smax.x), den_exp(lmx.y, smax.y)};
#else
    f2v targ = (lmx - smax) * l2e;
    f2v f = {__builtin_amdgcn_exp2f(targ.x), __builtin_amdgcn_exp2f(targ.y)};
#endif
    f2v er[R], ei[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
#if AMP_DEN_EXACT_EXP
        er[i] = f2v{den_exp(X[i].x, mx.x), den_exp(X[i].y, mx.y)};
        ei[i] = f2v{den_exp(Y[i].x, my.x), den_exp(Y[i].y, my.y)};
#else
        const f2v xa = (X[i] - mx) * l2e, ya = (Y[i] - my) * l2e;
        er[i] = f2v{__builtin_amdgcn_exp2f(xa.x), __builtin_amdgcn_exp2f(xa.y)};
        ei[i] = f2v{__builtin_amdgcn_exp2f(ya.x), __builtin_amdgcn_exp2f(ya.y)};
#endif
    }
    mid(er, ei);
    f2v zt, ar, ai, SI = f2splat(0.f);
    f2v Sr[FULLG ? 1 : R];
    if constexpr (FULLG) {
        f2v sr = f2splat(0.f), si = f2splat(0.f), a = f2splat(0.f), b = f2splat(0.f);
#pragma unroll
        for (int i = 0; i < R; ++i) {
            sr += er[i]; si += ei[i];
            a = f2fma(f2splat(Q.re[i]), er[i], a);
            b = f2fma(f2splat(Q.im[i]), ei[i], b);
        }
        SI = si; Sr[0] = sr;
        zt = (sr * si) * f;
        ar = (a * si) * f;
        ai = (sr * b) * f;
    } else {
        f2v z = f2splat(0.f), a = f2splat(0.f), b = f2splat(0.f), w[R];
#pragma unroll
        for (int j = 0; j < R; ++j) w[j] = f2splat(Q.im[j]) * ei[j];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            f2v si = f2splat(0.f), ti = f2splat(0.f);
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const float cw = grid_cnt<PAT>(i, j);
                if (cw == 1.f) { si += ei[j]; ti += w[j]; }
                else if (cw == 2.f) { si = f2fma(f2splat(2.f), ei[j], si); ti = f2fma(f2splat(2.f), w[j], ti); }
            }
            Sr[i] = si;
            const f2v es = er[i] * si;
            z += es;
            a = f2fma(f2splat(Q.re[i]), es, a);
            b = f2fma(er[i], ti, b);
        }
        zt = z * f;
        ar = a * f;
        ai = b * f;
    }
    float ze[2] = {0.f, 0.f}, zt1[2] = {zt.x, zt.y};
#pragma unroll
    for (int u = 0; u < 2; ++u) group_sum_excl_c<G>(zt1[u], ze[u]);
    const f2v iz = {den_rcp(zt1[0]), den_rcp(zt1[1])};
    const f2v xr = ar * iz, xi = ai * iz;
    f2v var = f2splat(0.f);
    if (kVar) {
        f2v vs;
        if constexpr (FULLG) {
            f2v vr = f2splat(0.f), vi = f2splat(0.f);
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const f2v dr = xr - f2splat(Q.re[i]), di = xi - f2splat(Q.im[i]);
                vr = f2fma(dr * dr, er[i], vr);
                vi = f2fma(di * di, ei[i], vi);
            }
            vs = f2fma(vr, SI, Sr[0] * vi) * f;
        } else {
            f2v d[R];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const f2v di = xi - f2splat(Q.im[j]);
                d[j] = (di * di) * ei[j];
            }
            f2v acc = f2splat(0.f);
#pragma unroll
            for (int i = 0; i < R; ++i) {
                f2v vi = f2splat(0.f);
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const float cw = grid_cnt<PAT>(i, j);
                    if (cw == 1.f) vi += d[j];
                    else if (cw == 2.f) vi = f2fma(f2splat(2.f), d[j], vi);
                }
                const f2v dr = xr - f2splat(Q.re[i]);
                acc = f2fma(er[i], f2fma(dr * dr, Sr[i], vi), acc);
            }
            vs = acc * f;
        }
        const f2v zev = {ze[0], ze[1]};
        var = (xr * xr + xi * xi) * (zev * iz) + vs * iz;
    }
    xr_out = xr; xi_out = xi; var_out = var; smax_out = smax; sabs_out = sabs;
}

// The packed step for a full round (both sections exist) with its inputs already loaded (rr, ri:
// the two sections' r, vp: their previous variances; Grid2In): no masking and no control flow
// between the loads and the stores.  The same operations on the same operands as
// denoise_step_grid2, the accumulator updates in its order (u = 0, then u = 1); the section
// statistics are stored by every lane of the group (the same value).  The policy supplies
// load_r / load_prev / store_prev (the store with the previous variance handed in).
struct Grid2In {
    f2v rr, ri, vp;
};
template <int G, class P>
__device__ __forceinline__ Grid2In grid2_load(const P& pol, int base) {
    const int lane = threadIdx.x & 63;
    constexpr int gpw = 64 / G;
    const int gid = lane / G, g = lane % G;
    Grid2In in;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        float rr, ri;
        pol.load_r(base + u * gpw + gid, g, rr, ri);
        in.rr[u] = rr; in.ri[u] = ri;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) in.vp[u] = pol.load_prev(base + u * gpw + gid, g);
    return in;
}
template <bool kVar, int R, int PAT, int G, class Mid = DenNoMid, class P>
__device__ __forceinline__ void denoise_step_grid2_full(const P& pol, int base, const Grid2In& in, const GridRegs<R>& Q,
                                                        PartAcc& pa, DenStat& S, Mid&& mid = Mid()) {
    const int lane = threadIdx.x & 63;
    constexpr int gpw = 64 / G;
    const int gid = lane / G, g = lane % G;
    const f2v it = f2splat(pol.inv);
    const f2v ur = in.rr * it, ui = in.ri * it;   // c64 / f32 == multiply by the reciprocal
    const int bad = (int)!(fabsf(ur.x) <= FLT_MAX) | (int)!(fabsf(ui.x) <= FLT_MAX) | (int)!(fabsf(ur.y) <= FLT_MAX) |
                    (int)!(fabsf(ui.y) <= FLT_MAX);
    S.st_bad |= bad != 0;
    f2v xr, xi, var, smax, sabs;
    grid2_core<kVar, R, PAT, G>(ur, ui, Q, xr, xi, var, smax, sabs, mid);
    pol.store_xv(base + gid, g, xr.x, xi.x, var.x);
    pol.store_xv(base + gpw + gid, g, xr.y, xi.y, var.y);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        pol.account(var[u], in.vp[u], pa);
        S.st_abs = nan_max(S.st_abs, sabs[u]);
        S.st_min = nan_min(S.st_min, smax[u]);
        pol.section(base + u * gpw + gid, smax[u], sabs[u]);
    }
}

// The full-round step at G = 32 with the two halves of every f2v on positions 2j and 2j + 1 of ONE
// section (16 lanes per section; a wave step covers the same four sections base .. base + 3, section
// base + q in lanes 16 q .. 16 q + 15).  Every section reduction then runs once per step instead of
// once per half, its first butterfly step is an in-lane operation and the other four stay inside one
// DPP row (no permlane), one v_rcp_f32 serves both positions, and the policy moves a position pair
// per access (load_r2 / load_prev2 / store_xv2).
//
// grid2_pair_core restates grid2_core with ur, ui, X, Y, er, ei, f, zt, ar, ai, var over the lane's
// two positions: every per-position operation keeps its operands, type and order.  A copy, like
// grid2_core itself.  The section reductions keep group_fmax_c<32>'s and
// group_sum_excl_c<32>'s results bit for bit:
//   max   an integer max over fkey keys is exact and order-free; the in-lane step is an integer max
//         too (v_max_f32 would drop a NaN);
//   sums  group_sum_excl_c<32> runs xor 1, 2, 4, 8, 16 over positions, and its first step pairs
//         exactly positions 2j and 2j + 1: with a, b the lane's two values, excl_a = 0 + b,
//         excl_b = 0 + a, tot = a + b, then the DPP distances 1, 2, 4, 8 over j are the old
//         2, 4, 8, 16 (float addition is commutative: the same tree term for term).
template <bool kVar, int R, int PAT, class Mid = DenNoMid>
__device__ __forceinline__ void grid2_pair_core(const f2v ur, const f2v ui, const GridRegs<R>& Q, f2v& xr_out, f2v& xi_out,
                                                f2v& var_out, float& smax_out, float& sabs_out, Mid&& mid = Mid()) {
    constexpr bool FULLG = PAT == GRID_FULL;
    f2v X[R], Y[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        X[i] = ur * f2splat(Q.re[i]);
        Y[i] = ui * f2splat(Q.im[i]);
    }
    f2v mx, my, lmx, lab;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        float ax = -FLT_MAX, nx = FLT_MAX, ay = -FLT_MAX, ny = FLT_MAX;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            ax = fmaxf(ax, X[i][u]); nx = fminf(nx, X[i][u]);
            ay = fmaxf(ay, Y[i][u]); ny = fminf(ny, Y[i][u]);
        }
        mx[u] = ax; my[u] = ay;
        lmx[u] = ax + ay;                          // max logit of the position (a corner)
        lab[u] = fmaxf(lmx[u], -(nx + ny));        // max |logit| of the position
    }
    int kmax = max(fkey(lmx.x), fkey(lmx.y)), kabs = max(fkey(lab.x), fkey(lab.y));
    kmax = imax_step<1>(kmax); kabs = imax_step<1>(kabs);
    kmax = imax_step<2>(kmax); kabs = imax_step<2>(kabs);
    kmax = imax_step<4>(kmax); kabs = imax_step<4>(kabs);
    kmax = imax_step<8>(kmax); kabs = imax_step<8>(kabs);
    const float smax1 = funkey(kmax), sabs1 = funkey(kabs);
    const f2v smax = f2splat(smax1);
    const f2v l2e = f2splat(AMP_LOG2E);
#if AMP_DEN_EXACT_EXP
    f2v f = {den_exp(lmx.x, smax.x), den_exp(lmx.y, smax.y)};
#else
    f2v targ = (lmx - smax) * l2e;
    f2v f = {__builtin_amdgcn_exp2f(targ.x), __builtin_amdgcn_exp2f(targ.y)};
#endif
    f2v er[R], ei[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
#if AMP_DEN_EXACT_EXP
        er[i] = f2v{den_exp(X[i].x, mx.x), den_exp(X[i].y, mx.y)};
        ei[i] = f2v{den_exp(Y[i].x, my.x), den_exp(Y[i].y, my.y)};
#else
        const f2v xa = (X[i] - mx) * l2e, ya = (Y[i] - my) * l2e;
        er[i] = f2v{__builtin_amdgcn_exp2f(xa.x), __builtin_amdgcn_exp2f(xa.y)};
        ei[i] = f2v{__builtin_amdgcn_exp2f(ya.x), __builtin_amdgcn_exp2f(ya.y)};
#endif
    }
    mid(er, ei);
    f2v zt, ar, ai, SI = f2splat(0.f);
    f2v Sr[FULLG ? 1 : R];
    if constexpr (FULLG) {
        f2v sr = f2splat(0.f), si = f2splat(0.f), a = f2splat(0.f), b = f2splat(0.f);
#pragma unroll
        for (int i = 0; i < R; ++i) {
            sr += er[i]; si += ei[i];
            a = f2fma(f2splat(Q.re[i]), er[i], a);
            b = f2fma(f2splat(Q.im[i]), ei[i], b);
        }
        SI = si; Sr[0] = sr;
        zt = (sr * si) * f;
        ar = (a * si) * f;
        ai = (sr * b) * f;
    } else {
        f2v z = f2splat(0.f), a = f2splat(0.f), b = f2splat(0.f), w[R];
#pragma unroll
        for (int j = 0; j < R; ++j) w[j] = f2splat(Q.im[j]) * ei[j];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            f2v si = f2splat(0.f), ti = f2splat(0.f);
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const float cw = grid_cnt<PAT>(i, j);
                if (cw == 1.f) { si += ei[j]; ti += w[j]; }
                else if (cw == 2.f) { si = f2fma(f2splat(2.f), ei[j], si); ti = f2fma(f2splat(2.f), w[j], ti); }
            }
            Sr[i] = si;
            const f2v es = er[i] * si;
            z += es;
            a = f2fma(f2splat(Q.re[i]), es, a);
            b = f2fma(er[i], ti, b);
        }
        zt = z * f;
        ar = a * f;
        ai = b * f;
    }
    // Z and the exclusive sums: group_sum_excl_c<32>'s tree, its xor-1 step in the lane
    float tot = zt.x + zt.y;
    f2v zev = {0.f + zt.y, 0.f + zt.x};
    {
        float p = xl<1>(tot);
        zev.x += p; zev.y += p; tot = tot + p;
        p = xl<2>(tot);
        zev.x += p; zev.y += p; tot = tot + p;
        p = xl<4>(tot);
        zev.x += p; zev.y += p; tot = tot + p;
        p = xl<8>(tot);
        zev.x += p; zev.y += p; tot = tot + p;
    }
    const f2v iz = f2splat(den_rcp(tot));
    const f2v xr = ar * iz, xi = ai * iz;
    f2v var = f2splat(0.f);
    if (kVar) {
        f2v vs;
        if constexpr (FULLG) {
            f2v vr = f2splat(0.f), vi = f2splat(0.f);
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const f2v dr = xr - f2splat(Q.re[i]), di = xi - f2splat(Q.im[i]);
                vr = f2fma(dr * dr, er[i], vr);
                vi = f2fma(di * di, ei[i], vi);
            }
            vs = f2fma(vr, SI, Sr[0] * vi) * f;
        } else {
            f2v d[R];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const f2v di = xi - f2splat(Q.im[j]);
                d[j] = (di * di) * ei[j];
            }
            f2v acc = f2splat(0.f);
#pragma unroll
            for (int i = 0; i < R; ++i) {
                f2v vi = f2splat(0.f);
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const float cw = grid_cnt<PAT>(i, j);
                    if (cw == 1.f) vi += d[j];
                    else if (cw == 2.f) vi = f2fma(f2splat(2.f), d[j], vi);
                }
                const f2v dr = xr - f2splat(Q.re[i]);
                acc = f2fma(er[i], f2fma(dr * dr, Sr[i], vi), acc);
            }
            vs = acc * f;
        }
        var = (xr * xr + xi * xi) * (zev * iz) + vs * iz;
    }
    xr_out = xr; xi_out = xi; var_out = var; smax_out = smax1; sabs_out = sabs1;
}

// sumvar is a float64 sum whose order reaches the batch mean, so the pair step keeps the old
// chains.  Old lane (gid, g) of the 32-lane map adds, per step, var[base + gid][g] and then
// var[base + 2 + gid][g].  In the pair map lane n < 32 holds positions 2j, 2j + 1 (j = n & 15) of
// section base + (n >> 4) and lane n + 32 the same positions of section base + 2 + (n >> 4): one
// v_permlane32_swap of (var.x, var.y) leaves lane n with var.x of both sections and lane n + 32
// with var.y of both, so pair lane n carries the chain of old lane
//   (n >> 4 & 1) * 32 + 2 (n & 15) + (n >> 5)
// in one float64 accumulator, with the old two additions per step.  pair_acc_in / pair_acc_out move
// the accumulators between the maps (once per denoiser call), so that steps of the 32-lane map
// before or after (the masked remainder) continue the same chains and part_wave_reduce's tree is
// the one it was.
__device__ __forceinline__ double pair_acc_move(double v, int src_lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_ds_bpermute(4 * src_lane, (int)(unsigned)b);
    const int hi = __builtin_amdgcn_ds_bpermute(4 * src_lane, (int)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
// (the lane index goes through an empty asm so that the source lane is formed where it is used:
// hoisted to the kernel's start it is one more value held, or spilled, across the whole loop)
__device__ __forceinline__ int pair_lane() {
    int l = threadIdx.x & 63;
    asm volatile("" : "+v"(l));
    return l;
}
__device__ __forceinline__ double pair_acc_in(double sumvar) {   // 32-lane map -> pair map
    const int n = pair_lane();
    return pair_acc_move(sumvar, ((n >> 4) & 1) * 32 + 2 * (n & 15) + (n >> 5));
}
__device__ __forceinline__ double pair_acc_out(double acc) {     // pair map -> 32-lane map
    const int l = pair_lane();
    return pair_acc_move(acc, (l & 1) * 32 + (l >> 5) * 16 + ((l & 31) >> 1));
}

struct GridPairIn {
    f2v rr, ri, vp;   // the lane's two positions: r (re, im) and the previous variances
};
template <class P>
__device__ __forceinline__ GridPairIn grid2_pair_load(const P& pol, int base, int lane) {
    const int sec = base + (lane >> 4), m = 2 * (lane & 15);
    GridPairIn in;
    const float4 v = pol.load_r2(sec, m);
    const float2 p = pol.load_prev2(sec, m);
    in.rr = f2v{v.x, v.z}; in.ri = f2v{v.y, v.w};
    in.vp = f2v{p.x, p.y};
    // both loads issued here and waited for together (left alone, the previous variances' load sinks
    // to its use, the step's last instructions, and its latency stands before the stores)
    asm volatile("" : "+v"(in.vp));
    return in;
}
template <bool kVar, int R, int PAT, class Mid = DenNoMid, class P>
__device__ __forceinline__ void denoise_step_grid2_pair(const P& pol, int base, int lane, const GridPairIn& in,
                                                        const GridRegs<R>& Q, PartAcc& pa, double& acc, DenStat& S,
                                                        Mid&& mid = Mid()) {
    const int sec = base + (lane >> 4), m = 2 * (lane & 15);
    const f2v it = f2splat(pol.inv);
    const f2v ur = in.rr * it, ui = in.ri * it;   // c64 / f32 == multiply by the reciprocal
    const int bad = (int)!(fabsf(ur.x) <= FLT_MAX) | (int)!(fabsf(ui.x) <= FLT_MAX) | (int)!(fabsf(ur.y) <= FLT_MAX) |
                    (int)!(fabsf(ui.y) <= FLT_MAX);
    S.st_bad |= bad != 0;
    f2v xr, xi, var;
    float smax, sabs;
    grid2_pair_core<kVar, R, PAT>(ur, ui, Q, xr, xi, var, smax, sabs, mid);
    pol.store_xv2(sec, m, make_float4(xr.x, xi.x, xr.y, xi.y), make_float2(var.x, var.y));
    // lanes < 32: var.x of sections base + gid, base + 2 + gid; lanes >= 32: var.y of the same two
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(var.x), __float_as_uint(var.y), false, false);
    acc += (double)__uint_as_float(sw[0]);
    acc += (double)__uint_as_float(sw[1]);
    pol.account_close(var.x, in.vp.x, pa);
    pol.account_close(var.y, in.vp.y, pa);
    S.st_abs = nan_max(S.st_abs, sabs);
    S.st_min = nan_min(S.st_min, smax);
    pol.section(sec, smax, sabs);
}

#ifndef AMP_DEN_PACKED_GRID
#define AMP_DEN_PACKED_GRID 1
#endif

// denoise_sections_grid's FAST: DEN_FAST_FULL the full-round step, DEN_FAST_PAIR the same with the
// position-pair step where G = 32 and the grid is the packed GRID_REF16 (any other G: DEN_FAST_FULL).
enum { DEN_FAST_NONE = 0, DEN_FAST_FULL = 1, DEN_FAST_PAIR = 2 };

// Grid dimension of a compile-time constellation size (0: no product-grid form).
template <int KK>
constexpr int grid_r() { return KK == 4 ? 2 : KK == 16 ? 4 : KK == 64 ? 8 : 0; }

// The grid loop over this wave's sections; returns false (nothing done) when c is not a grid of
// the size KK admits.  c.grid / c.gfull are kernel arguments: the branch is uniform.
// FAST (with the packed grid, U = 2; the policy supplies load_r / load_prev / store_xv / account):
// this wave's full rounds (both sections of a step exist: base + 2 gpw <= nsec, wave-uniform) run
// denoise_step_grid2_full; a partial last round runs the masked step.  The same bits either way.
// FAST == DEN_FAST_PAIR at G = 32: the full rounds run denoise_step_grid2_pair instead (the policy
// supplies load_r2 / load_prev2 / store_xv2 / account_close); the same bits again.
// (Requesting the next round's inputs before the current round's arithmetic was measured slower:
// the six values held across the step spilled)
//
// PRIO (vamp_persist's eight-wave bf16x3 kernels, two waves per SIMD: AMP_X3_DEN_PRIO): the issue priority of
// this wave through its full rounds (DEN_FAST_PAIR / DEN_FAST_FULL; the masked remainder and every other
// form run at priority 0), by the half it belongs to (half: wave-uniform, in an SGPR, as x3_gemm_prio takes
// it; 0 the SIMD's older wave, 1 the younger).  0: none, no code.  1: the younger half at priority 1
// throughout.  2: priority 1 in alternate rounds, the younger half in even rounds and the older in odd ones,
// set at the top of a round.  3: as 2, and flipped once more inside the step, between the exponentials and
// the section sums: the two waves stand half a step apart (the top of a round then changes nothing but in
// round 0).  4: the younger half at priority 1 from the top of every round to that point, the older half
// from there to the round's end.  5, 6: the younger half at priority 1 through its first two / three rounds
// and at 0 from then on (age decides again: the older half runs ahead for the rest), so that the halves end
// together instead of one running half its rounds alone (6 is vamp_persist's default: DESIGN.md §3.3).
// s_setprio takes an immediate, so each one stands behind a scalar branch; every form leaves the loop at
// priority 0, also a wave without a full round (it never raised it).  Only the time at which instructions
// issue differs.
template <int PRIO>
struct DenPrio {
    int half, p, rd;   // p: this wave's priority from the next top() on (forms 2, 3); rd: its round (forms 5, 6)
    __device__ __forceinline__ explicit DenPrio(int h) : half(h), p(h), rd(0) {}
    __device__ __forceinline__ static void set(int one) {
        if (one) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
    }
    __device__ __forceinline__ void top() {
        if constexpr (PRIO == 1) {
            if (half) __builtin_amdgcn_s_setprio(1);
        } else if constexpr (PRIO == 2) {
            set(p);
            p ^= 1;
        } else if constexpr (PRIO == 3) {
            set(p);
        } else if constexpr (PRIO == 4) {
            set(half);
        } else if constexpr (PRIO == 5 || PRIO == 6) {
            if (half) {
                if (rd == 0) __builtin_amdgcn_s_setprio(1);
                else if (rd == PRIO - 3) __builtin_amdgcn_s_setprio(0);
            }
            ++rd;
        }
    }
    // (the compiler is free to move s_setprio over plain arithmetic, and put it ahead of the exponentials: the
    // exponentials' results go through an empty asm on either side of it, which holds them behind it and the
    // sums ahead of it.  The pins change the operand order of the sums behind them: finite results keep their
    // bits, a NaN row's NaNs come out with another payload, so forms 3 and 4 are for timing A/B runs only)
    __device__ __forceinline__ static void pin(f2v (&er)[4], f2v (&ei)[4]) {
        asm volatile("" : "+v"(er[0]), "+v"(er[1]), "+v"(er[2]), "+v"(er[3]), "+v"(ei[0]), "+v"(ei[1]), "+v"(ei[2]), "+v"(ei[3]));
    }
    __device__ __forceinline__ void operator()(f2v (&er)[4], f2v (&ei)[4]) {   // grid2_core's / grid2_pair_core's mid()
        if constexpr (PRIO == 3 || PRIO == 4) {
            pin(er, ei);
            if constexpr (PRIO == 3) {
                p ^= 1;
                set(p);
            } else {
                set(half ^ 1);
            }
            pin(er, ei);
        }
    }
    __device__ __forceinline__ void leave() const {
        if constexpr (PRIO == 1 || PRIO == 5 || PRIO == 6) {
            if (half) __builtin_amdgcn_s_setprio(0);
        } else if constexpr (PRIO != 0) {
            if (half) __builtin_amdgcn_s_setprio(0);
            else __builtin_amdgcn_s_setprio(0);
        }
    }
};
// hook(rd): called behind full round rd of this wave (the trace builds' per-round stamps; the default: no code)
struct DenNoHook {
    __device__ __forceinline__ void operator()(int) const {}
};
template <bool kVar, int KK, int U, int G, bool PKG = true, int FAST = DEN_FAST_NONE, int PRIO = 0, class Hook = DenNoHook, class P>
__device__ __forceinline__ bool denoise_sections_grid(const P& pol, int nsec, const Const& c, PartAcc& pa, DenWaves dw = DenWaves::block(),
                                                      int half = 0, Hook&& hook = Hook()) {
    constexpr int R = grid_r<KK>();
    if constexpr (R == 0) {
        return false;
    } else {
        const int grid = __builtin_amdgcn_readfirstlane(c.grid), gfull = __builtin_amdgcn_readfirstlane(c.gfull);
        if (grid != R) return false;
        const int wave = dw.wave;
        constexpr int gpw = 64 / G;
        const int nw = dw.nw;
        DenStat S;
        GridRegs<R> Q;
        Q.load(c);
        if (gfull == GRID_FULL) {
            for (int base = wave * gpw * U; base < nsec; base += nw * gpw * U) {   // wave-uniform trip count
                if constexpr (PKG && U == 2 && AMP_DEN_PACKED_GRID)
                    denoise_step_grid2<kVar, R, GRID_FULL, G>(pol, base, nsec, Q, pa, S);
                else
                    denoise_step_grid<kVar, R, GRID_FULL, U, G>(pol, base, nsec, Q, pa, S);
            }
        } else if constexpr (R == 4) {
            int base = wave * gpw * U;
            if constexpr (FAST && PKG && U == 2 && AMP_DEN_PACKED_GRID) {
                const int step = nw * gpw * 2;
                DenPrio<PRIO> pr(half);
                int rd = 0;   // (the hook's round index: dead without one)
                if constexpr (FAST == DEN_FAST_PAIR && G == 32) {
                    // (a wave without a full round moves its sums there and back: no branch around the loop;
                    // the wave-uniform base as a scalar: the loop branches on SCC, not on an exec mask)
                    base = __builtin_amdgcn_readfirstlane(base);
                    double acc = pair_acc_in(pa.sumvar);
                    for (; base + 2 * gpw <= nsec; base += step) {
                        pr.top();
                        const int lane = pair_lane();   // the step's addresses formed in the step
                        denoise_step_grid2_pair<kVar, R, GRID_REF16>(pol, base, lane, grid2_pair_load(pol, base, lane), Q, pa,
                                                                     acc, S, pr);
                        hook(rd++);
                    }
                    pr.leave();
                    pa.sumvar = pair_acc_out(acc);
                } else {
                    for (; base + 2 * gpw <= nsec; base += step) {
                        pr.top();
                        denoise_step_grid2_full<kVar, R, GRID_REF16, G>(pol, base, grid2_load<G>(pol, base), Q, pa, S, pr);
                        hook(rd++);
                    }
                    pr.leave();
                }
            }
            for (; base < nsec; base += nw * gpw * U) {
                if constexpr (PKG && U == 2 && AMP_DEN_PACKED_GRID)
                    denoise_step_grid2<kVar, R, GRID_REF16, G>(pol, base, nsec, Q, pa, S);
                else
                    denoise_step_grid<kVar, R, GRID_REF16, U, G>(pol, base, nsec, Q, pa, S);
            }
        }
        S.fold(pa);
        return true;
    }
}

template <bool kVar, int KK, int U, int G, class P>
__device__ __forceinline__ void denoise_sections_gp(const P& pol, int nsec, const Const& c, PartAcc& pa, DenWaves dw = DenWaves::block()) {
    if (denoise_sections_grid<kVar, KK, U, G>(pol, nsec, c, pa, dw)) return;
    const int wave = dw.wave;
    constexpr int gpw = 64 / G;
    const int nw = dw.nw;
    DenRegs<KK> R;
    R.load(c);
    DenStat S;
    for (int base = wave * gpw * U; base < nsec; base += nw * gpw * U)   // wave-uniform trip count
        denoise_step_gp<kVar, KK, U, G, false>(pol, base, nsec, R, pa, S);
    S.fold(pa);
}

// Which float32 forms run on the packed VALU (v_pk_*_f32):
//   PK_NONE  every float32 operation scalar (the product grid still applies);
//   PK_ALL   the packed per-point form (denoise_step_gp) and the packed product grid (grid2);
//   PK_GRID  the packed product grid only; alphabets that are not a grid of the compile-time
//            size (16PSK at KK = 16, QPSK {1, j, -1, -j}) run the scalar per-point form.
// The engines that place two waves on one SIMD use PK_NONE or PK_GRID, because there the packed
// per-point variance accumulation of denoise_step_gp was measured to lose one half of a
// v_pk_fma_f32 result in lanes 48-63 now and then (results not reproducible run to
// run; the scalar form was bit-identical in every run).  PK_ALL == true keeps the old bool callers.
enum { PK_NONE = 0, PK_ALL = 1, PK_GRID = 2 };

// Runtime M (a power of two <= 64) -> the compile-time group size.
// (PRIO, half, hook: denoise_sections_grid's, for its full rounds alone)
template <bool kVar, int KK, int U, int G, int PK, int FAST = DEN_FAST_NONE, int PRIO = 0, class Hook = DenNoHook, class P>
__device__ __forceinline__ void denoise_sections_sel(const P& pol, int nsec, const Const& c, PartAcc& pa, DenWaves dw = DenWaves::block(),
                                                     int half = 0, Hook&& hook = Hook()) {
    if constexpr (PK == PK_ALL && KK % 2 == 0) {
        denoise_sections_gp<kVar, KK, U, G>(pol, nsec, c, pa, dw);
    } else {
        if (denoise_sections_grid<kVar, KK, U, G, PK == PK_GRID, FAST, PRIO>(pol, nsec, c, pa, dw, half, hook)) return;
        denoise_sections_g<kVar, KK, U, G>(pol, nsec, c, pa, dw);
    }
}
template <bool kVar, int KK, int U, int PK = PK_ALL, int FAST = DEN_FAST_NONE, int PRIO = 0, class Hook = DenNoHook, class P>
__device__ __forceinline__ void denoise_sections_u(const P& pol, int nsec, int M, const Const& c, PartAcc& pa, DenWaves dw = DenWaves::block(),
                                                   int half = 0, Hook&& hook = Hook()) {
    switch (M) {
    case 64: denoise_sections_sel<kVar, KK, U, 64, PK, FAST, PRIO>(pol, nsec, c, pa, dw, half, hook); break;
    case 32: denoise_sections_sel<kVar, KK, U, 32, PK, FAST, PRIO>(pol, nsec, c, pa, dw, half, hook); break;
    case 16: denoise_sections_sel<kVar, KK, U, 16, PK, FAST, PRIO>(pol, nsec, c, pa, dw, half, hook); break;
    case 8: denoise_sections_sel<kVar, KK, U, 8, PK, FAST, PRIO>(pol, nsec, c, pa, dw, half, hook); break;
    case 4: denoise_sections_sel<kVar, KK, U, 4, PK, FAST, PRIO>(pol, nsec, c, pa, dw, half, hook); break;
    case 2: denoise_sections_sel<kVar, KK, U, 2, PK, FAST, PRIO>(pol, nsec, c, pa, dw, half, hook); break;
    default: denoise_sections_sel<kVar, KK, U, 1, PK, FAST, PRIO>(pol, nsec, c, pa, dw, half, hook); break;
    }
}

// 64-QAM form (KK > 16): the same arithmetic per element as denoise_sections_g, but the 64
// points are streamed from the scalar cache in chunks of 8 (rolled loop: 128 uniform operands
// do not fit the scalar register file) and nothing per point is kept in registers — the
// logits are re-formed in each of the three passes (max, exp sums, variance) and the
// variance pass recomputes exp(xi - max): the same bits as the first exp (2 x 64 v_exp_f32
// per position instead of 64, against 5 GEMM launches per iteration at cfg5).
// One position per lane (G = M <= 64 lanes per section).
template <bool kVar, int KK, int G, class P>
__device__ __forceinline__ void denoise_sections_wide(const P& pol, int nsec, const Const& c, PartAcc& pa, DenWaves dw = DenWaves::block()) {
    static_assert(KK % 8 == 0, "chunks of 8 points");
    if (denoise_sections_grid<kVar, KK, 1, G>(pol, nsec, c, pa, dw)) return;   // square 64-QAM
    const int lane = threadIdx.x & 63, wave = dw.wave;
    constexpr int gpw = 64 / G;
    const int gid = lane / G, g = lane % G;
    const int nw = dw.nw;
    // the table in LDS: the rolled loops below index it at runtime, which on the by-value kernel
    // argument made the compiler copy the whole Const into scratch memory at every kernel entry
    __shared__ float s_cre[KK], s_cim[KK];
    __syncthreads();
    if (threadIdx.x == 0) {   // constant offsets into the kernel argument (scalar loads)
#pragma unroll
        for (int k = 0; k < KK; ++k) { s_cre[k] = kval(c.re[k]); s_cim[k] = kval(c.im[k]); }
    }
    __syncthreads();
    DenStat S;
    for (int base = wave * gpw; base < nsec; base += nw * gpw) {   // wave-uniform trip count
        const int sec = base + gid;
        const bool act = sec < nsec;
        float rr, ri, it;
        pol.load(act ? sec : nsec - 1, g, rr, ri, it);
        const float ur = rr * it, ui = ri * it;   // c64 / f32 == multiply by the reciprocal
        if (act) S.st_bad |= !(fabsf(ur) <= FLT_MAX && fabsf(ui) <= FLT_MAX);
        float lmax = -FLT_MAX, lmin = FLT_MAX;
#pragma unroll 1
        for (int k0 = 0; k0 < KK; k0 += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = fmaf(ur, s_cre[k0 + j], ui * s_cim[k0 + j]);
                lmax = fmaxf(lmax, x);
                lmin = fminf(lmin, x);
            }
        }
        const float smax = group_fmax_c<G>(lmax), sabs = group_fmax_c<G>(fmaxf(lmax, -lmin));
        float zm = 0.f, a = 0.f, b = 0.f;
#pragma unroll 1
        for (int k0 = 0; k0 < KK; k0 += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float cr = s_cre[k0 + j], ci = s_cim[k0 + j];
                const float e = den_exp(fmaf(ur, cr, ui * ci), smax);
                zm += e;
                a = fmaf(cr, e, a);
                b = fmaf(ci, e, b);
            }
        }
        float zt = zm, ze = 0.f;
        group_sum_excl_c<G>(zt, ze);
        const float iz = den_rcp(zt);
        const float xr = a * iz, xi = b * iz;
        float var = 0.f;
        if (kVar) {
            float vs = 0.f;
#pragma unroll 1
            for (int k0 = 0; k0 < KK; k0 += 8) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float cr = s_cre[k0 + j], ci = s_cim[k0 + j];
                    const float e = den_exp(fmaf(ur, cr, ui * ci), smax);
                    const float dr = xr - cr, di = xi - ci;
                    vs = fmaf(fmaf(dr, dr, di * di), e, vs);
                }
            }
            var = (xr * xr + xi * xi) * (ze * iz) + vs * iz;
        }
        if (act) {
            pol.store(sec, g, xr, xi, var, pa);
            S.st_abs = nan_max(S.st_abs, sabs);
            S.st_min = nan_min(S.st_min, smax);
            if (g == 0) pol.section(sec, smax, sabs);
        }
    }
    S.fold(pa);
}

template <bool kVar, int KK, class P>
__device__ __forceinline__ void denoise_sections_wide_m(const P& pol, int nsec, int M, const Const& c, PartAcc& pa, DenWaves dw = DenWaves::block()) {
    switch (M) {
    case 64: denoise_sections_wide<kVar, KK, 64>(pol, nsec, c, pa, dw); break;
    case 32: denoise_sections_wide<kVar, KK, 32>(pol, nsec, c, pa, dw); break;
    case 16: denoise_sections_wide<kVar, KK, 16>(pol, nsec, c, pa, dw); break;
    case 8: denoise_sections_wide<kVar, KK, 8>(pol, nsec, c, pa, dw); break;
    case 4: denoise_sections_wide<kVar, KK, 4>(pol, nsec, c, pa, dw); break;
    case 2: denoise_sections_wide<kVar, KK, 2>(pol, nsec, c, pa, dw); break;
    default: denoise_sections_wide<kVar, KK, 1>(pol, nsec, c, pa, dw); break;
    }
}

template <bool kVar, int KK, class P>
__device__ __forceinline__ void denoise_sections(const P& pol, int nsec, int M, const Const& c, PartAcc& pa) {
    if constexpr (KK > 16) {
        // 64-QAM: M <= 64 (check_dims); the generic M > 64 form below is not instantiated (its
        // registers would set the whole kernel's occupancy)
        denoise_sections_wide_m<kVar, KK>(pol, nsec, M, c, pa);
        return;
    } else {
    if (M <= 64) {
        denoise_sections_u<kVar, KK, 1>(pol, nsec, M, c, pa);
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int G = M < 64 ? M : 64;
    const int PPL = M / G;
    const int gpw = 64 / G;
    const int gid = lane / G, g = lane - gid * G;
    const int nw = blockDim.x >> 6;
    for (int base = wave * gpw; base < nsec; base += nw * gpw) {   // wave-uniform trip count
        const int sec = base + gid;
        const bool act = sec < nsec;
        const int ss = act ? sec : nsec - 1;
        float lmax = -FLT_MAX, lmin = FLT_MAX;
        bool bad = false;
        {
            // M > 64: PPL positions per lane, logits recomputed per pass.
            for (int p = 0; p < PPL; ++p) {
                float rr, ri, it;
                pol.load(ss, g + p * 64, rr, ri, it);
                const float ur = rr * it, ui = ri * it;
                bad |= !(fabsf(ur) <= FLT_MAX && fabsf(ui) <= FLT_MAX);
#pragma unroll
                for (int k = 0; k < KK; ++k) {
                    {
                        const float x = fmaf(ur, c.re[k], ui * c.im[k]);
                        lmax = fmaxf(lmax, x);
                        lmin = fminf(lmin, x);
                    }
                }
            }
            const float smax = group_fmax(lmax, 64);
            double zl = 0.0;
            for (int p = 0; p < PPL; ++p) {
                float rr, ri, it;
                pol.load(ss, g + p * 64, rr, ri, it);
                const float ur = rr * it, ui = ri * it;
                float zm = 0.f;
#pragma unroll
                for (int k = 0; k < KK; ++k)
                    zm += __builtin_amdgcn_exp2f((fmaf(ur, c.re[k], ui * c.im[k]) - smax) * AMP_LOG2E);
                zl += (double)zm;
            }
            const double z = group_sum(zl, 64);
            const double iz = 1.0 / z;
            for (int p = 0; p < PPL; ++p) {
                float rr, ri, it;
                pol.load(ss, g + p * 64, rr, ri, it);
                const float ur = rr * it, ui = ri * it;
                float zm = 0.f, sr = 0.f, si = 0.f;
                float ek[KK];
#pragma unroll
                for (int k = 0; k < KK; ++k) {
                    {
                        const float e = __builtin_amdgcn_exp2f((fmaf(ur, c.re[k], ui * c.im[k]) - smax) * AMP_LOG2E);
                        ek[k] = e;
                        zm += e;
                        sr = fmaf(c.re[k], e, sr);
                        si = fmaf(c.im[k], e, si);
                    }
                }
                const float xr = (float)((double)sr * iz), xi = (float)((double)si * iz);
                float var = 0.f;
                if (kVar) {
                    const float omp = (float)((z - (double)zm) * iz);
                    float vs = 0.f;
#pragma unroll
                    for (int k = 0; k < KK; ++k) {
                        {
                            const float dr = xr - c.re[k], di = xi - c.im[k];
                            vs = fmaf(fmaf(dr, dr, di * di), ek[k], vs);
                        }
                    }
                    var = (xr * xr + xi * xi) * omp + (float)((double)vs * iz);
                }
                if (act) pol.store(sec, g + p * 64, xr, xi, var, pa);
            }
            const float sabs = group_fmax(fmaxf(lmax, -lmin), 64);
            if (act) {
                const double sm = (double)smax, sa = (double)sabs;
                pa.maxabs = bad ? __longlong_as_double(0x7ff8000000000000LL) : nan_max(pa.maxabs, sa);
                pa.minsecmax = nan_min(pa.minsecmax, sm);
                if (g == 0) pol.section(sec, (float)sm, (float)sa);
            }
        }
    }
    }
}

// max |xi| of one section in float64, exactly as the reference forms the logits.
// ld(m, rr, ri, inv_tau).
template <class LD>
__device__ double section_absmax_f64(const LD& ld, int M, const Const64& c) {
    double mx = 0.0;
    for (int m = 0; m < M; ++m) {
        float rr, ri, it;
        ld(m, rr, ri, it);
        const double ur = (double)(rr * it), ui = (double)(ri * it);
        for (int k = 0; k < c.K; ++k) mx = fmax(mx, fabs(ur * c.re[k] + ui * c.im[k]));
    }
    return mx;
}

// Reference-exact float64 evaluation of ONE section with the batch-global shift G, for the
// sections whose reference softmax leaves the normal float64 range (AMP_DANGER): the exact
// op sequence of vamp.py:111-119 / bamp.py:69-77 / scamp.py:64-67 —
//   xi = Re((r*(1/tau)) conj a) (float64), eta = exp(xi - G), Z = sum_m sum_k eta,
//   xmmse = sum_k a eta / Z  (complex alphabets: * (1/Z), which is inf for a denormal Z;
//                             real alphabets: a true float64 division),
//   var = |xmmse|^2 (1 - Z_m / Z) + sum_k |xmmse - a_k|^2 eta / Z,
// so inf / NaN / denormal-quantised results come out exactly as the reference's do.
// One thread per section (rare path).  ld(m, rr, ri, inv_tau); st(m, xr, xi, var).
template <bool kVar, class LD, class ST>
__device__ void exact_section_f64(const LD& ld, const ST& st, int M, const Const64& c, double G) {
    const int K = c.K;
    double Z = 0.0;
    for (int m = 0; m < M; ++m) {
        float rr, ri, it;
        ld(m, rr, ri, it);
        const double ur = (double)(rr * it), ui = (double)(ri * it);
        double zm = 0.0;
        for (int k = 0; k < K; ++k) zm += exp((ur * c.re[k] + ui * c.im[k]) - G);
        Z += zm;
    }
    const double rz = 1.0 / Z;
    for (int m = 0; m < M; ++m) {
        float rr, ri, it;
        ld(m, rr, ri, it);
        const double ur = (double)(rr * it), ui = (double)(ri * it);
        double zm = 0.0, sr = 0.0, si = 0.0;
        for (int k = 0; k < K; ++k) {
            const double e = exp((ur * c.re[k] + ui * c.im[k]) - G);
            zm += e;
            sr += c.re[k] * e;
            si += c.im[k] * e;
        }
        double xr, xi;
        if (c.real_alpha) { xr = sr / Z; xi = 0.0; }
        else { xr = sr * rz; xi = si * rz; }
        float var = 0.f;
        if (kVar) {
            const double ax = c.real_alpha ? fabs(xr) : hypot(xr, xi);
            const double var0 = ax * ax * (1.0 - zm / Z);
            double vs = 0.0;
            for (int k = 0; k < K; ++k) {
                // eta recomputed (the same bits as above; no per-point array: 64-QAM)
                const double e = exp((ur * c.re[k] + ui * c.im[k]) - G);
                const double dr = xr - c.re[k], di = xi - c.im[k];
                const double h = c.real_alpha ? fabs(dr) : hypot(dr, di);
                vs += h * h * e;
            }
            var = (float)(var0 + vs / Z);
        }
        st(m, (float)xr, (float)xi, var);
    }
}

// The rare-path driver shared by the reduction kernels (one workgroup):
//  1. exact float64 batch max |xi| (G) from the sections whose float32 estimate is within the
//     fast path's slack of the float32 batch max;
//  2. exact recompute of every section whose max logit lies below G + AMP_DANGER (+ slack).
// secmax / secabs: per-section float32 estimates (natural units) written by the fast path.
// LDF(s) returns the section's loader; STF(s) its store functor.  Returns #recomputed
// sections (workgroup-uniform) and the exact G in *G_out.
template <bool kVar, class LDF, class STF>
__device__ int fixup_sections(int S, int M, const float* secmax, const float* secabs, double G32, const Const64& c,
                              const LDF& ldf, const STF& stf, double* G_out, double* lds_d) {
    const double slack = logit_slack(G32);
    double gm = 0.0;
    for (int s = threadIdx.x; s < S; s += blockDim.x)
        if ((double)secabs[s] >= G32 - slack) gm = fmax(gm, section_absmax_f64(ldf(s), M, c));
    gm = group_max(gm, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds_d[threadIdx.x >> 6] = gm;
    __syncthreads();
    double G = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) G = fmax(G, lds_d[w]);
    __syncthreads();
    int cnt = 0;
    for (int s = threadIdx.x; s < S; s += blockDim.x) {
        if ((double)secmax[s] - G < AMP_DANGER + slack) {
            exact_section_f64<kVar>(ldf(s), stf(s), M, c, G);
            ++cnt;
        }
    }
    cnt = group_sum(cnt, 64);
    if ((threadIdx.x & 63) == 0) lds_d[threadIdx.x >> 6] = (double)cnt;
    __syncthreads();
    int total = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) total += (int)lds_d[w];
    __syncthreads();
    *G_out = G;
    return total;
}

}  // namespace amp

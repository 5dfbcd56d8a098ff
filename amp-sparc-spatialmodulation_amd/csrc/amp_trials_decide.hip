// amp_trials_decide.hip — the decision + error counters of E independent single-trial
// detections in two launches (amp_vamp_trials_run / amp_bamp_trials_run).
//
// Restates, for every trial alone, Loss.error_rate at B = 1 (loss.py:67-179): MAP_decision
// (loss.py:282-302) or segmented_decision (loss.py:222-250) per section, then the counters with
// Ns = Lin Na, ibits_trunc = ceil(log2(Lin Na)) (loss.py:20) and flat indices local to the trial.
// The kernels are map_decide_kernel / map_count_kernel (amp_decide.hip) with the trial as
// blockIdx.y: each trial's sections go to the same workgroups, lane groups and partial slots as in
// its own B = 1 call, so its counters and float64 sums are the same bits.
// amp_bamp_random_trials_run alone also decides by random_decision (loss.py:252-280, AMP_RULE_RANDOM):
// random_decide_kernel's row function (amp_decide.h) with the trial as blockIdx.y.
#include <algorithm>

#include "amp_trials.h"

namespace amp {

struct TDecK {
    int L, M, Na, Lin, nblk, ibits, rule;
    const float2* xmap;
    const float2* xmmse;
    const float2* x;
    const long long* sym;
    const long long* idx;
    unsigned char* mism;   // [E][L]
    DecPart* parts;        // [E][nblk]
    amp_counts* out;       // [E]
    DecConst c;
};

template <int KK, int G>
__global__ __launch_bounds__(AMP_WG) void trials_decide_kernel(TDecK P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int M = P.M, S = P.L;
    const size_t s0 = (size_t)blockIdx.y * P.L;   // the trial's first section
    constexpr int gpw = 64 / G;
    const int gid = lane / G, g = lane % G;
    DecPart q = decpart_zero();
    const long long ibmask = dec_ibmask(P.ibits);
    const int stride = gridDim.x * (AMP_WG / 64) * gpw;
    for (int base = (blockIdx.x * (AMP_WG / 64) + wave) * gpw; base < S; base += stride) {   // wave-uniform
        const int s = base + gid;
        const bool act = s < S;
        const size_t o0 = (s0 + (act ? s : S - 1)) * M;
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
            P.mism[s0 + s] = (unsigned char)mm;
            count_section<KK>(P.c, s, M, P.L, P.Na, P.Lin, bi, se, P.sym[s0 + s], P.idx[s0 + s], ibmask, q);
        }
    }
    long long ier = q.ier, ser = q.ser, iber = q.iber, sber = q.sber;
    double mse = q.mse, msef = q.msef, msem = q.msem, mseL = q.mseL;
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
        P.parts[(size_t)blockIdx.y * P.nblk + blockIdx.x] = o;
    }
}

// The 'random' rule (Loss.random_decision, loss.py:252-280) per trial: random_decide_kernel
// (amp_decide.hip) with the trial as blockIdx.y.  Trial e's Lin channel uses go to the threads and
// partial slots of its own B = 1 call (row = its local channel use; sym / idx / the flat indices local
// to the trial), so its counters and float64 sums are the same bits.
template <int KK>
__global__ __launch_bounds__(AMP_WG) void trials_random_decide_kernel(TDecK P, int Nt) {
    const size_t e = blockIdx.y;
    DecPart q = decpart_zero();
    const long long ibmask = dec_ibmask(P.ibits);
    const size_t o = e * (size_t)P.Lin * Nt;
    for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < P.Lin; row += gridDim.x * blockDim.x)
        random_decide_row<KK>(P.c, Nt, P.Na, P.Lin, row, P.xmap + o, P.x + o, P.xmmse + o, P.sym + e * P.L,
                              P.idx + e * P.L, ibmask, nullptr, P.mism + e * P.L + (size_t)row * P.Na, q);
    random_part_store(q, P.parts + e * P.nblk + blockIdx.x);
}

// workgroup e: trial e's channel-use / trial "any mismatch" counts (loss.py:133-136, 150) and its
// partials folded in map_count_kernel's order
__global__ __launch_bounds__(1024) void trials_count_kernel(TDecK P) {
    const int e = blockIdx.x;
    long long ver = 0, verf = 0, verm = 0, verL = 0, fer = 0;
    if (threadIdx.x == 0) {
        int trial = 0;
        for (int lin = 0; lin < P.Lin; ++lin) {
            int cu = 0;
            const unsigned char* m = P.mism + (size_t)e * P.L + (size_t)lin * P.Na;
            for (int a = 0; a < P.Na; ++a) cu |= m[a];
            ver += cu;
            if (lin == 0) verf += cu;
            if (lin == P.Lin / 2) verm += cu;
            if (lin == P.Lin - 1) verL += cu;
            trial |= cu;
        }
        fer += trial;
    }
    DecPart t = DecPart{0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < P.nblk; i += blockDim.x) {
        const DecPart q = P.parts[(size_t)e * P.nblk + i];
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
        P.out[e] = c;
    }
}

// amp_decide.hip's decide_nblk at B = 1
static int trials_decide_nblk(const amp_dims* d) {
    const int G = d->M < 64 ? d->M : 64;
    const int per = (AMP_WG / 64) * (64 / G);
    return std::max(1, std::min(cdiv(d->L, per), 2048));
}

template <int KK>
static void trials_launch_decide_k(const TDecK& P, int E, hipStream_t st) {
    const dim3 g(P.nblk, E), b(AMP_WG);
    switch (P.M) {
    case 1: hipLaunchKernelGGL((trials_decide_kernel<KK, 1>), g, b, 0, st, P); break;
    case 2: hipLaunchKernelGGL((trials_decide_kernel<KK, 2>), g, b, 0, st, P); break;
    case 4: hipLaunchKernelGGL((trials_decide_kernel<KK, 4>), g, b, 0, st, P); break;
    case 8: hipLaunchKernelGGL((trials_decide_kernel<KK, 8>), g, b, 0, st, P); break;
    case 16: hipLaunchKernelGGL((trials_decide_kernel<KK, 16>), g, b, 0, st, P); break;
    case 32: hipLaunchKernelGGL((trials_decide_kernel<KK, 32>), g, b, 0, st, P); break;
    default: hipLaunchKernelGGL((trials_decide_kernel<KK, 64>), g, b, 0, st, P); break;   // M >= 64 (power of 2)
    }
}

size_t trials_decide_ws_bytes(const amp_dims* d, int trials) {
    Carve cv(nullptr);
    cv.take<unsigned char>((size_t)trials * d->L);
    cv.take<DecPart>((size_t)trials * trials_decide_nblk(d));
    return cv.off;
}

int trials_decide_args(const amp_dims* d, const amp_trials_decide_args* dec, const void* xmap, const void* xmmse,
                       TrialsDecide& out, bool random_entry) {
    AMP_REQUIRE(dec->x && dec->sym && dec->idx && dec->counts, "amp_trials_decide_args: null pointer argument");
    if (random_entry) {
        AMP_REQUIRE(dec->rule == AMP_RULE_RANDOM, "amp_trials_decide_args: rule %d (amp_bamp_random_trials_run decides by "
                    "AMP_RULE_RANDOM)", dec->rule);
        AMP_REQUIRE(d->Na >= 1 && d->Na <= AMP_DEC_MAX_NA && d->Na <= d->Nt,
                    "amp_trials_decide_args: the 'random' rule takes Na <= %d (Na = %d)", AMP_DEC_MAX_NA, d->Na);
    }
    AMP_REQUIRE(random_entry || dec->rule == AMP_RULE_SPARC || dec->rule == AMP_RULE_SEGMENTED,
                "amp_trials_decide_args: rule %d (the 'random' rule has no independent-trial form)", dec->rule);
    AMP_REQUIRE(dec->ibits_trunc >= 0 && dec->ibits_trunc < 64, "amp_trials_decide_args: ibits_trunc out of range");
    AMP_REQUIRE(d->Lin * d->Na * d->M == d->N, "amp_trials_decide_args: inconsistent dims");
    out.xmap = (const float2*)xmap; out.xmmse = (const float2*)xmmse; out.x = (const float2*)dec->x;
    out.sym = (const long long*)dec->sym; out.idx = (const long long*)dec->idx;
    out.counts = (amp_counts*)dec->counts;
    out.rule = dec->rule;
    out.ibits = dec->ibits_trunc;
    return AMP_OK;
}

int trials_decide_launch(const amp_dims* d, const amp_constellation* c, const TrialsDecide& a, int trials, void* ws,
                         hipStream_t st) {
    TDecK P;
    P.L = d->L; P.M = d->M; P.Na = d->Na; P.Lin = d->Lin;
    P.nblk = trials_decide_nblk(d);
    P.ibits = a.ibits; P.rule = a.rule;
    P.xmap = a.xmap; P.xmmse = a.xmmse; P.x = a.x; P.sym = a.sym; P.idx = a.idx;
    Carve cv(ws);
    P.mism = cv.take<unsigned char>((size_t)trials * d->L);
    P.parts = cv.take<DecPart>((size_t)trials * P.nblk);
    P.out = a.counts;
    P.c = to_decconst(c);
    if (P.rule == AMP_RULE_RANDOM) {
        // amp_random_decide_count's grid at B = 1, per trial (its partials fit the carve above)
        P.nblk = std::max(1, std::min(cdiv(d->Lin, AMP_WG), P.nblk));
        const dim3 g(P.nblk, trials), b(AMP_WG);
        switch (P.c.K) {
        case 1: hipLaunchKernelGGL(trials_random_decide_kernel<1>, g, b, 0, st, P, d->Nt); break;
        case 2: hipLaunchKernelGGL(trials_random_decide_kernel<2>, g, b, 0, st, P, d->Nt); break;
        case 4: hipLaunchKernelGGL(trials_random_decide_kernel<4>, g, b, 0, st, P, d->Nt); break;
        case 8: hipLaunchKernelGGL(trials_random_decide_kernel<8>, g, b, 0, st, P, d->Nt); break;
        case 16: hipLaunchKernelGGL(trials_random_decide_kernel<16>, g, b, 0, st, P, d->Nt); break;
        default: hipLaunchKernelGGL(trials_random_decide_kernel<64>, g, b, 0, st, P, d->Nt); break;
        }
        AMP_LAUNCH_CHECK("trials_random_decide");
        hipLaunchKernelGGL(trials_count_kernel, dim3(trials), dim3(1024), 0, st, P);
        AMP_LAUNCH_CHECK("trials_count");
        return AMP_OK;
    }
    switch (P.c.K) {
    case 1: trials_launch_decide_k<1>(P, trials, st); break;
    case 2: trials_launch_decide_k<2>(P, trials, st); break;
    case 4: trials_launch_decide_k<4>(P, trials, st); break;
    case 8: trials_launch_decide_k<8>(P, trials, st); break;
    case 16: trials_launch_decide_k<16>(P, trials, st); break;
    default: trials_launch_decide_k<64>(P, trials, st); break;     // check_dims: K in {1, 2, 4, 8, 16, 64}
    }
    AMP_LAUNCH_CHECK("trials_decide");
    hipLaunchKernelGGL(trials_count_kernel, dim3(trials), dim3(1024), 0, st, P);
    AMP_LAUNCH_CHECK("trials_count");
    return AMP_OK;
}

}  // namespace amp

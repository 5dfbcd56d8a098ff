// amp_synth.hip — the inputs of a trial batch drawn on the device (amp_synth_channels,
// amp_synth_trials; throughput mode): all G channels of a forward_trials call in one launch, and
// all E trials' x / sym / idx / noise / y in one launch.
//
// Random numbers are Philox4x32-10 (Salmon et al., SC'11; the Random123 constants) written out
// here: key = (seed low, seed high), counter = (index, id low, id high, stream), so a draw is a
// pure function of (seed, stream, id, index) and no state is kept anywhere.  Stream 0: channel
// taps (id = channel, index = (r Nt + t) Lh + l), 1: message (id = trial, index = section; message = 1:
// index = u Na + j, draw j of channel use u),
// 2: noise (id = trial, index = row).
#include "amp_host.h"

namespace amp {

enum { SYNTH_TAPS = 0, SYNTH_MESSAGE = 1, SYNTH_NOISE = 2 };

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}

__device__ __forceinline__ uint4 synth_draw(uint2 key, unsigned long long id, unsigned stream, unsigned index) {
    return philox4x32_10(make_uint4(index, (unsigned)id, (unsigned)(id >> 32), stream), key);
}

// One complex unit normal pair from a block's first two words (Box-Muller; both uniforms exact in
// float32, u1 in (0, 1) so the logarithm is finite).
__device__ __forceinline__ float2 synth_normal(uint4 w) {
    const float u1 = ((float)(w.x >> 9) + 0.5f) * 0x1p-23f;
    const float u2 = (float)(w.y >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);
    return make_float2(r * c, r * s);
}

struct SynthChK {
    int n, N, Nr, Nt, Lin, Lh;
    uint2 key;
    unsigned long long id0;
    float scale;          // 1 / sqrt(2 Na Lin) (channel.py:59)
    const float* sw;      // [Lout][Lin]
    float2* A;            // [G][n][N]
    float2* At;           // [G][N][n]
};

constexpr int SYNTH_TILE = 32;

// Workgroup (bx, by, g): the 32 x 32 tile of channel g at rows 32 by, columns 32 bx.  Every element
// computes its own tap; the tile goes to A row by row and, through LDS, to At column by column, so
// both stores run along the fastest index.
__global__ __launch_bounds__(256) void synth_channels_kernel(SynthChK P) {
    __shared__ float2 tile[SYNTH_TILE][SYNTH_TILE + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c0 = blockIdx.x * SYNTH_TILE, j0 = blockIdx.y * SYNTH_TILE;
    const unsigned long long id = P.id0 + blockIdx.z;
    const size_t base = (size_t)blockIdx.z * P.n * P.N;
    float2* __restrict__ A = P.A + base;
    float2* __restrict__ At = P.At + base;
    const int col = c0 + tx;
    const int i = col / P.Nt, t = col - i * P.Nt;
#pragma unroll
    for (int k = 0; k < SYNTH_TILE / 8; ++k) {
        const int row = j0 + ty + 8 * k;
        float2 v = make_float2(0.f, 0.f);
        if (row < P.n && col < P.N) {
            const int o = row / P.Nr, r = row - o * P.Nr, l = o - i;
            if (l >= 0 && l < P.Lh) {
                const float2 z = synth_normal(synth_draw(P.key, id, SYNTH_TAPS, ((unsigned)r * P.Nt + t) * P.Lh + l));
                const float s = P.sw[o * P.Lin + i];
                v = make_float2(s * (z.x * P.scale), s * (z.y * P.scale));
            }
            A[(size_t)row * P.N + col] = v;
        }
        tile[ty + 8 * k][tx] = v;
    }
    __syncthreads();
    const int row = j0 + tx;
#pragma unroll
    for (int k = 0; k < SYNTH_TILE / 8; ++k) {
        const int c = c0 + ty + 8 * k;
        if (c < P.N && row < P.n) At[(size_t)c * P.n + row] = tile[tx][ty + 8 * k];
    }
}

struct SynthTrK {
    int n, N, L, M, K, Na, Nr, Nt, Lin, band, per, nb, message;
    uint2 key;
    unsigned long long id0;
    float noise_std;
    const float2* At;     // [G][N][n]
    float2* x;            // [E][N]
    long long* sym;       // [E][L]
    long long* idx;       // [E][L]
    float2* y;            // [E][n]
    float2* noise;        // [E][n] or null
    float re[AMP_MAX_K], im[AMP_MAX_K];
    int gray[AMP_MAX_K];
};

constexpr int SYNTH_ROWS = 256;   // rows of y per workgroup, one per lane

// Workgroup (e, b): rows [256 b, 256 b + 256) of trial e's y, and the b-th slice of its x (workgroup
// 0 also writes sym / idx).  The trial's section list — active column and symbol of each of the L
// sections — is rebuilt by every workgroup in LDS (L Philox blocks), so no workgroup waits for
// another and nothing is accumulated with atomics.  Lane = row: every read of At is one contiguous
// run of a column's row of At.  KK: the constellation size (the table is read with constant indices
// from the kernel arguments).
// P.message = 1 (Data.random, data.py:55-72): the list holds, per channel use u, its Na active
// columns in ascending order with one symbol for all of them; ONE lane builds a channel use's subset
// (Floyd's sampling, amp_sparc.h; the chosen antennas kept sorted in the list itself), once per
// workgroup and not per output row.  Entries [u Na, (u + 1) Na) lie in column block u, as sections
// do, so the band ranges and the accumulation below are the same code for both messages.
template <int KK>
__global__ __launch_bounds__(SYNTH_ROWS) void synth_trials_kernel(SynthTrK P) {
    extern __shared__ float2 synth_lds[];
    float2* sval = synth_lds;             // [L] symbol of the section
    int* scol = (int*)(synth_lds + P.L);  // [L] active column of the section
    const int tid = threadIdx.x;
    const int e = blockIdx.x / P.nb, b = blockIdx.x - e * P.nb;
    const unsigned long long id = P.id0 + (unsigned)e;
    if (P.message == 1) {
        for (int u = tid; u < P.Lin; u += SYNTH_ROWS) {
            int* sub = scol + u * P.Na;                 // the antennas chosen so far, ascending
            int k = 0;
            for (int j = 0; j < P.Na; ++j) {
                const uint4 w = synth_draw(P.key, id, SYNTH_MESSAGE, (unsigned)(u * P.Na + j));
                if (j == 0) k = (int)__umulhi(w.y, (unsigned)P.K);
                const int J = P.Nt - P.Na + j;
                int t = (int)__umulhi(w.x, (unsigned)(J + 1));
                for (int i = 0; i < j; ++i)
                    if (sub[i] == t) { t = J; break; }  // J itself is never in the list yet: every entry is < J
                int i = j;
                for (; i > 0 && sub[i - 1] > t; --i) sub[i] = sub[i - 1];
                sub[i] = t;
            }
            float vr = 0.f, vi = 0.f;
            int gr = 0;
#pragma unroll
            for (int q = 0; q < KK; ++q)
                if (q == k) { vr = P.re[q]; vi = P.im[q]; gr = P.gray[q]; }
            for (int j = 0; j < P.Na; ++j) {
                const int s = u * P.Na + j, col = u * P.Nt + sub[j];
                sval[s] = make_float2(vr, vi);
                sub[j] = col;
                if (b == 0) {
                    P.sym[(size_t)e * P.L + s] = gr;
                    P.idx[(size_t)e * P.L + s] = col;
                }
            }
        }
    } else
    for (int s = tid; s < P.L; s += SYNTH_ROWS) {
        const uint4 w = synth_draw(P.key, id, SYNTH_MESSAGE, (unsigned)s);
        const int pos = (int)__umulhi(w.x, (unsigned)P.M), k = (int)__umulhi(w.y, (unsigned)P.K);
        float vr = 0.f, vi = 0.f;
        int gr = 0;
#pragma unroll
        for (int q = 0; q < KK; ++q)
            if (q == k) { vr = P.re[q]; vi = P.im[q]; gr = P.gray[q]; }
        const int col = s * P.M + pos;
        sval[s] = make_float2(vr, vi);
        scol[s] = col;
        if (b == 0) {
            P.sym[(size_t)e * P.L + s] = gr;
            P.idx[(size_t)e * P.L + s] = col;
        }
    }
    __syncthreads();
    {   // x: this workgroup's slice of the trial's N columns, zeros and symbols alike
        const int chunk = (P.N + P.nb - 1) / P.nb;
        const int c1 = min(P.N, (b + 1) * chunk);
        const int sh = __ffs(P.M) - 1;          // M is a power of two
        float2* __restrict__ x = P.x + (size_t)e * P.N;
        if (P.message == 1) {
            for (int c = b * chunk + tid; c < c1; c += SYNTH_ROWS) {
                const int s0 = (c / P.Nt) * P.Na;       // the channel use's Na entries
                float2 v = make_float2(0.f, 0.f);
                for (int j = 0; j < P.Na; ++j)
                    if (scol[s0 + j] == c) v = sval[s0 + j];
                x[c] = v;
            }
        } else
        for (int c = b * chunk + tid; c < c1; c += SYNTH_ROWS) {
            const int s = c >> sh;
            x[c] = scol[s] == c ? sval[s] : make_float2(0.f, 0.f);
        }
    }
    const int jw0 = b * SYNTH_ROWS + (tid & ~63);    // the wave's first row
    if (jw0 >= P.n) return;
    const int j = b * SYNTH_ROWS + tid;
    const bool live = j < P.n;
    int s_lo = 0, s_hi = P.L, my_lo = 0, my_hi = P.L;
    if (P.band > 0) {
        // the wave walks the sections any of its rows needs (one coalesced read of At per section);
        // a row adds only those of its own column blocks (o - Lh, o]
        const int o0 = jw0 / P.Nr, o1 = min(jw0 + 63, P.n - 1) / P.Nr, o = (live ? j : P.n - 1) / P.Nr;
        s_lo = max(0, o0 - P.band + 1) * P.Na;
        s_hi = (min(o1, P.Lin - 1) + 1) * P.Na;
        my_lo = max(0, o - P.band + 1) * P.Na;
        my_hi = (min(o, P.Lin - 1) + 1) * P.Na;
    }
    const float2* __restrict__ At = P.At + (size_t)(e / P.per) * P.N * P.n;
    float2 acc = make_float2(0.f, 0.f);
#pragma unroll 4
    for (int s = s_lo; s < s_hi; ++s) {
        const int col = scol[s];
        const float2 v = sval[s];
        if (live && s >= my_lo && s < my_hi) {
            const float2 a = At[(size_t)col * P.n + j];
            acc.x += a.x * v.x - a.y * v.y;
            acc.y += a.x * v.y + a.y * v.x;
        }
    }
    if (!live) return;
    const float2 z = synth_normal(synth_draw(P.key, id, SYNTH_NOISE, (unsigned)j));
    const float2 nz = make_float2(z.x * P.noise_std, z.y * P.noise_std);
    const size_t at = (size_t)e * P.n + j;
    P.y[at] = make_float2(acc.x + nz.x, acc.y + nz.y);
    if (P.noise) P.noise[at] = nz;
}

constexpr int SYNTH_MAX_L = 4096;   // 12 bytes of LDS per section

static int synth_check(const amp_dims* d, const char* what) {
    AMP_REQUIRE(d, "%s: null dims", what);
    AMP_REQUIRE(d->B == 1, "%s: d describes one trial (d->B = %d)", what, d->B);
    AMP_REQUIRE(d->Nt > 0 && d->Na > 0 && d->Nr > 0 && d->Lin > 0 && d->Lout > 0, "%s: non-positive dimension", what);
    AMP_REQUIRE(d->Nt % d->Na == 0, "%s: Na must divide Nt (config.py:133)", what);
    AMP_REQUIRE(d->M == d->Nt / d->Na && d->L == d->Na * d->Lin && d->N == d->Nt * d->Lin && d->n == d->Nr * d->Lout,
                "%s: inconsistent derived dimensions", what);
    AMP_REQUIRE(is_pow2(d->M), "%s: section size M = Nt/Na = %d must be a power of two", what, d->M);
    AMP_REQUIRE(d->N % 2 == 0, "%s: N (%d) must be even", what, d->N);
    return AMP_OK;
}

}  // namespace amp

using namespace amp;

extern "C" {

int amp_synth_channels(const amp_dims* d, const amp_synth_args* a, int32_t channels, void* stream) {
    if (int rc = synth_check(d, "amp_synth_channels")) return rc;
    AMP_REQUIRE(a && a->sw && a->A && a->At, "amp_synth_channels: null pointer argument");
    AMP_REQUIRE(channels >= 1 && channels <= WCH_MAX, "amp_synth_channels: channels = %d (1 .. %d: a grid axis)",
                channels, WCH_MAX);
    AMP_REQUIRE(a->Lh >= 1 && a->Lh <= d->Lout, "amp_synth_channels: Lh = %d outside [1, Lout = %d]", a->Lh, d->Lout);
    AMP_REQUIRE((long long)d->Nr * d->Nt * a->Lh <= 0xffffffffLL, "amp_synth_channels: Nr Nt Lh beyond 32 bits");
    const int tx = cdiv(d->N, SYNTH_TILE), ty = cdiv(d->n, SYNTH_TILE);
    AMP_REQUIRE(ty <= 65535, "amp_synth_channels: n = %d beyond the grid (%d row tiles)", d->n, ty);
    SynthChK P;
    P.n = d->n; P.N = d->N; P.Nr = d->Nr; P.Nt = d->Nt; P.Lin = d->Lin; P.Lh = a->Lh;
    P.key = make_uint2((unsigned)a->seed, (unsigned)(a->seed >> 32));
    P.id0 = a->channel0;
    P.scale = (float)(1.0 / sqrt(2.0 * d->Na * d->Lin));
    P.sw = (const float*)a->sw;
    P.A = (float2*)a->A;
    P.At = (float2*)a->At;
    hipLaunchKernelGGL(synth_channels_kernel, dim3(tx, ty, channels), dim3(256), 0, (hipStream_t)stream, P);
    AMP_LAUNCH_CHECK("synth_channels");
    return AMP_OK;
}

int amp_synth_trials(const amp_dims* d, const amp_constellation* c, const amp_synth_args* a, int32_t trials,
                     int32_t per_channel, void* stream) {
    if (int rc = synth_check(d, "amp_synth_trials")) return rc;
    AMP_REQUIRE(c, "amp_synth_trials: null constellation");
    AMP_REQUIRE(c->K >= 1 && c->K <= AMP_MAX_K && is_pow2(c->K) && c->K != 32,
                "amp_synth_trials: constellation size K = %d must be 1, 2, 4, 8, 16 or 64", c->K);
    AMP_REQUIRE(a && a->At && a->x && a->sym && a->idx && a->y, "amp_synth_trials: null pointer argument");
    AMP_REQUIRE(trials >= 1 && per_channel >= 1, "amp_synth_trials: trials = %d, per_channel = %d (both >= 1)", trials,
                per_channel);
    AMP_REQUIRE(cdiv(trials, per_channel) <= WCH_MAX, "amp_synth_trials: more than %d channels", WCH_MAX);
    AMP_REQUIRE(a->band_blocks >= 0 && a->band_blocks <= d->Lout, "amp_synth_trials: band_blocks = %d outside [0, Lout = %d]",
                a->band_blocks, d->Lout);
    AMP_REQUIRE(a->message == 0 || a->message == 1, "amp_synth_trials: message = %d (0: one point per section, 1: Na "
                "antennas per channel use)", a->message);
    AMP_REQUIRE(d->L <= SYNTH_MAX_L, "amp_synth_trials: L = Na Lin = %d sections beyond %d (the section list lives in LDS)",
                d->L, SYNTH_MAX_L);
    const int nb = cdiv(d->n, SYNTH_ROWS);
    AMP_REQUIRE((long long)trials * nb <= 0x7fffffffLL, "amp_synth_trials: trials x row tiles beyond the grid");
    SynthTrK P;
    P.n = d->n; P.N = d->N; P.L = d->L; P.M = d->M; P.K = c->K; P.Na = d->Na; P.Nr = d->Nr; P.Nt = d->Nt; P.Lin = d->Lin;
    P.band = a->band_blocks; P.per = per_channel; P.nb = nb; P.message = a->message;
    P.key = make_uint2((unsigned)a->seed, (unsigned)(a->seed >> 32));
    P.id0 = a->trial0;
    P.noise_std = a->noise_std;
    P.At = (const float2*)a->At;
    P.x = (float2*)a->x; P.sym = (long long*)a->sym; P.idx = (long long*)a->idx;
    P.y = (float2*)a->y; P.noise = (float2*)a->noise;
    for (int i = 0; i < AMP_MAX_K; ++i) {
        const bool v = i < c->K;
        P.re[i] = v ? c->re[i] : 0.f;
        P.im[i] = v ? c->im[i] : 0.f;
        P.gray[i] = v ? c->gray[i] : 0;
    }
    const size_t lds = (size_t)d->L * (sizeof(float2) + sizeof(int));
    const dim3 g((unsigned)(trials * nb)), b(SYNTH_ROWS);
    hipStream_t st = (hipStream_t)stream;
    switch (c->K) {
    case 1: hipLaunchKernelGGL(synth_trials_kernel<1>, g, b, lds, st, P); break;
    case 2: hipLaunchKernelGGL(synth_trials_kernel<2>, g, b, lds, st, P); break;
    case 4: hipLaunchKernelGGL(synth_trials_kernel<4>, g, b, lds, st, P); break;
    case 8: hipLaunchKernelGGL(synth_trials_kernel<8>, g, b, lds, st, P); break;
    case 16: hipLaunchKernelGGL(synth_trials_kernel<16>, g, b, lds, st, P); break;
    default: hipLaunchKernelGGL(synth_trials_kernel<64>, g, b, lds, st, P); break;
    }
    AMP_LAUNCH_CHECK("synth_trials");
    return AMP_OK;
}

}  // extern "C"

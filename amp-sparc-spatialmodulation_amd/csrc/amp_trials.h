// amp_trials.h — independent-trial batches (amp_vamp_trials_run / amp_bamp_trials_run /
// amp_scamp_trials_run; the row guards below are also the launch engines', amp_bamp.h / amp_scamp.h): E
// single-trial detections that share one channel and one SNR, run in one launch sequence.  Each
// trial is the reference's B = 1 forward of that trial alone: at B = 1 the batch-global values
// (var.mean() vamp.py:85, the max|xi| shift vamp.py:112 / bamp.py:70, the allclose exit
// vamp.py:185 / bamp.py:140) are per-trial values, so every row of the GEMM tiles carries its own
// iteration record and its own partials.
#pragma once

#include <type_traits>

#include "amp_decide.h"
#include "amp_denoise.h"
#include "amp_gemm.h"
#include "amp_host.h"

namespace amp {

// The partial slot that column tile `cb` of a one-row-block launch of `nct` column tiles occupies
// in the launch engines (their slot is the workgroup's linear index, their tile the image of that
// index under xcd_tile): the inverse of xcd_tile for gridDim.x == 1, so a trial's partials are
// reduced in the order its own B = 1 forward reduces them.
__device__ __forceinline__ int seq_part_slot(int cb, int nct) {
    constexpr int NXCD = 8;
    const int base = nct / NXCD, rem = nct % NXCD;
    int x = 0;
#pragma unroll
    for (int i = 1; i < NXCD; ++i)
        if (i * base + min(i, rem) <= cb && (base > 0 || i < rem)) x = i;
    const int q = cb - (x * base + min(x, rem));
    return q * NXCD + x;
}

// The rows of one GEMM tile: which trials still iterate.  Called by every thread; returns false
// (workgroup-uniform) when no row of the tile is live, i.e. the tile has nothing to do.
template <class REC>
__device__ __forceinline__ bool tile_rows_live(const REC* recs, int row0, int rows, int* s_stop) {
    if (threadIdx.x < GBM) {
        const int row = row0 + threadIdx.x;
        s_stop[threadIdx.x] = row < rows ? recs[row].stopped : 1;
    }
    __syncthreads();
    int live = 0;
#pragma unroll
    for (int i = 0; i < GBM; ++i) live |= s_stop[i] ^ 1;
    return live != 0;
}

// The channel mapping of a trial batch, the policy every trial GEMM kernel is written over (one
// kernel family; the host launches the OneChannel instantiation for one channel, TrialChannels for
// several).  Trial e uses channel e / per, so channel g owns rows [g per, min((g + 1) per, E)) and
// tpg = ceil(per / 32) row tiles of the grid; row tile rb belongs to channel rb / tpg and starts at
// row g per + (rb % tpg) 32 (no multiple of 32 in general, and possibly odd).  `lim`, the channel's
// last row + 1, is the row limit of the tile's A loader and of tile_rows_live: rows of the next
// channel that fall inside the 32-row tile are staged as zeros and marked stopped, so they are
// neither multiplied with this channel's operator nor stored.  wstride / bstride: floats / ints
// between two channels' packed operators / band ranges (per GEMM operator of the engine).
// Interface: tile(rb, E); of(e), trial e's channel; woff / boff(g, i), what steps operator i's
// weights / band ranges to channel g.
struct ChannelTile {
    int g, row0, lim;
};
struct TrialChannels {
    int per, tpg;
    size_t wstride[4];
    int bstride[4];
    __device__ __forceinline__ ChannelTile tile(int rb, int E) const {
        const int g = rb / tpg;
        return ChannelTile{g, g * per + (rb - g * tpg) * GBM, min((g + 1) * per, E)};
    }
    __device__ __forceinline__ int of(int e) const { return e / per; }
    __device__ __forceinline__ size_t woff(int g, int i) const { return (size_t)g * wstride[i]; }
    __device__ __forceinline__ size_t boff(int g, int i) const { return (size_t)g * bstride[i]; }
};
// One channel: every row tile is channel 0's, the row limit is E and no pointer moves; the constants
// fold, so a kernel's instantiation does the work of a kernel written for one channel.
struct OneChannel {
    __device__ __forceinline__ ChannelTile tile(int rb, int E) const { return ChannelTile{0, rb * GBM, E}; }
    __device__ __forceinline__ int of(int) const { return 0; }
    __device__ __forceinline__ size_t woff(int, int) const { return 0; }
    __device__ __forceinline__ size_t boff(int, int) const { return 0; }
};
// ints between two channels' band ranges of an operator with `ntiles` column tiles: whole 256-byte
// workspace granules, so G channels cost exactly G times one channel's bytes
inline int band_stride(int ntiles) { return (2 * ntiles + 63) & ~63; }
// channels of `trials` trials at `per` per channel (both >= 1); per is clamped to the trials, so one
// channel takes exactly the single-channel grid
inline int trial_channels(int trials, int& per) {
    per = per < trials ? per : trials;
    return (trials + per - 1) / per;
}

// The row guard of a GEMM epilogue that the launch engine and the independent-trial engine share
// (amp_bamp.h, amp_scamp.h): which rows of the tile it may store to.  The batch engine stores every
// row (live() is a constant, the test folds away); the trial engine never stores to a stopped row
// (s_stop: tile_rows_live's LDS flags).  PSCR: floats of partial-store scratch the epilogue keeps
// free at the head of its LDS scratch, past the C tile (the trial engine stores one partial per row
// while later rows still read the staged values; the batch engine stores one per tile, at the end).
struct AllRows {
    static constexpr int PSCR = 0;
    __device__ __forceinline__ bool live(int) const { return true; }
};
struct LiveRows {
    static constexpr int PSCR = 64;
    const int* s_stop;
    __device__ __forceinline__ bool live(int rho) const { return !s_stop[rho]; }
};

// Sum of an integer over the workgroup, returned to every thread (s: one word per wavefront).
// Called by every thread; the leading barrier lets consecutive calls share s.
template <class T>
__device__ __forceinline__ T block_sum(T v, T* s) {
    v = group_sum(v, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    T tot = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += s[w];
    return tot;
}

// f(std::integral_constant<int, KK>) for the constellation size K as a compile-time bound
// (check_dims: K in {1, 2, 4, 8, 16, 64})
template <class F>
inline void dispatch_K(int K, const F& f) {
    switch (K) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    default: f(std::integral_constant<int, 64>{}); break;
    }
}

// Per-trial decision + counters (amp_trials_decide.hip): Loss at B = 1 for each of `trials` rows
// (loss.py:67-179 with Ns = Lin Na, flat indices local to the trial), rule 0 MAP (sparc,
// loss.py:282-302), 1 segmented (loss.py:222-250) or 2 random (loss.py:252-280: per channel use the
// Na largest |x_m|; trials_decide_args takes it with random_entry only, amp_bamp_random_trials_run's
// call, and refuses it for every other entry).  ws: trials_decide_ws_bytes.
struct TrialsDecide {
    const float2* xmap;
    const float2* xmmse;
    const float2* x;
    const long long* sym;
    const long long* idx;
    amp_counts* counts;
    int rule, ibits;
};
size_t trials_decide_ws_bytes(const amp_dims* d, int trials);
int trials_decide_launch(const amp_dims* d, const amp_constellation* c, const TrialsDecide& a, int trials, void* ws,
                         hipStream_t st);
int trials_decide_args(const amp_dims* d, const amp_trials_decide_args* dec, const void* xmap, const void* xmmse,
                       TrialsDecide& out, bool random_entry = false);

}  // namespace amp

// amp_trials.h — independent-trial batches (amp_vamp_trials_run / amp_bamp_trials_run): E
// single-trial detections that share one channel and one SNR, run in one launch sequence.  Each
// trial is the reference's B = 1 forward of that trial alone: at B = 1 the batch-global values
// (var.mean() vamp.py:85, the max|xi| shift vamp.py:112 / bamp.py:70, the allclose exit
// vamp.py:185 / bamp.py:140) are per-trial values, so every row of the GEMM tiles carries its own
// iteration record and its own partials.
#pragma once

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

// Per-trial decision + counters (amp_trials_decide.hip): Loss at B = 1 for each of `trials` rows
// (loss.py:67-179 with Ns = Lin Na, flat indices local to the trial), rule 0 MAP (sparc,
// loss.py:282-302) or 1 segmented (loss.py:222-250).  ws: trials_decide_ws_bytes.
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
                       TrialsDecide& out);

}  // namespace amp

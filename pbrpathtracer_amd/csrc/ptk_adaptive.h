// Adaptive render (include/ptk.h ptk_render_adaptive): parameter blocks and launchers of the kernels in ptk_adaptive.hip, and of
// the list compaction it shares with the plain render (ptk_frame.hip).
// The trace kernels are unchanged: they are fed the round's traced mask and list in RenderParams::live_mask / live_list.
#pragma once

#include "ptk_device.h"

namespace ptk {

// what the adaptive accumulate kernel needs beside the pass's RenderParams, whose live_mask is the round's TRACED mask
// (the live mask of a plain render & the active set)
struct AdaptiveParams {
    const unsigned long long* active;   // per owned quadrant: the round's active pixels (each receives the pass's spp)
    uint32_t* counts;                   // [H][W] samples each pixel has received, rows bottom-up
    float* moments;                     // [H][W][3] per-channel sums of squared samples (S2), rows bottom-up
    unsigned long long* stats;          // [0] += active pixels x spp per pass, [1] = max of the counts
};

// converge_kernel: the convergence test after a round, the dilation, and the next round's masks
struct ConvergeParams {
    unsigned long long* active;         // in: the round's active set (unless init); out: the next round's
    unsigned long long* traced;         // out: base & active, what the trace kernel is fed
    const unsigned long long* base;     // the live mask of a plain render (sure misses / lens-culled pixels left out)
    const float* accum;                 // S1
    const float* moments;               // S2
    const uint32_t* counts;             // n
    unsigned* active_count;             // += pixels of the new active set (zeroed by the host before the launch)
    float threshold;
    int init;                           // 1: the active set is every owned pixel on the image (before the first round)
    int test;                           // 1: apply the rule (n >= min_spp); 0: the active set stays as it is
};

void launch_accumulate_adaptive(const RenderParams& p, const AdaptiveParams& a, int owned_tiles, hipStream_t stream);
void launch_converge(const RenderParams& p, const ConvergeParams& cp, int owned_tiles, hipStream_t stream);
// ordered list of the quadrants whose mask is not zero, and their number: launch_live_list's second half (live_compact_kernel)
void launch_compact_list(const unsigned long long* mask, int num_subtiles, unsigned* list, unsigned* count, hipStream_t stream);

}  // namespace ptk

// What the passes over (ground-truth frame) x (the detection tracks of its cell)
// share -- the association (track_association.hip) and the identity's share pass
// (track_identity.hip): the three descriptor tables both build in their
// workspace, and the probe of a detection track's frame list for a timeline
// position (the association's pair kernel, written first, has the same lines in
// its loop: moving them here changed its register allocation, so they stay).
// Args is the pass's argument struct: n_dt, n_gt, n_cells, n_dt_frames,
// n_gt_frames, cell_gt_off, dfoff, dfpos, gfoff, dt_meta, gt_cell, frame_gt.
#pragma once
#include "common.hpp"

namespace taoamd {

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi)
{
    return v < lo ? lo : (v > hi ? hi : v);
}

// lane = detection track: {first frame, end, first and last position} of its frame list
template <class Args> __device__ __forceinline__ void frames_dt_meta(const Args &a)
{
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= a.n_dt) return;
    // (offsets clamped to the table: a bad CSR reads wrong frames, never past an end)
    const int64_t fs = clamp64(a.dfoff[d], 0, a.n_dt_frames);
    const int64_t fe = clamp64(a.dfoff[d + 1], fs, a.n_dt_frames);
    int4 m = make_int4((int32_t)fs, (int32_t)fe, 0, -1);
    if (fe > fs) {
        m.z = a.dfpos[fs];
        m.w = a.dfpos[fe - 1];
    }
    a.dt_meta[d] = m;
}

// lane = cell: the cell of every ground-truth row
template <class Args> __device__ __forceinline__ void frames_gt_cell(const Args &a)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.n_cells) return;
    const int64_t g0 = clamp64(a.cell_gt_off[c], 0, a.n_gt);
    const int64_t g1 = clamp64(a.cell_gt_off[c + 1], g0, a.n_gt);
    for (int64_t g = g0; g < g1; g++) a.gt_cell[g] = (int32_t)c;
}

// wavefront = ground-truth track: the track of every frame
template <class Args> __device__ __forceinline__ void frames_frame_gt(const Args &a)
{
    const int64_t g = (int64_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    if (g >= a.n_gt) return;
    const int64_t s = clamp64(a.gfoff[g], 0, a.n_gt_frames);
    const int64_t e = clamp64(a.gfoff[g + 1], s, a.n_gt_frames);
    for (int64_t k = s + lane_id(); k < e; k += WAVE) a.frame_gt[k] = (int32_t)g;
}

// Whether the list that m describes has a frame at position p, and its index: a
// track without holes is ONE probe, else a bisection between the two indices
// its first and last position allow.
__device__ __forceinline__ bool frames_find(const int32_t *dfpos, const int4 m, int64_t p,
                                            int64_t &lo)
{
    if (p < m.z || p > m.w) return false;       // (a track without frames: z > w)
    // positions ascend strictly: the frame at p, if any, lies no further from
    // the list's first entry than p from its position, nor from its last
    lo = max((int64_t)m.x, (int64_t)m.y - 1 - ((int64_t)m.w - p));
    int64_t hi = min((int64_t)m.y - 1, (int64_t)m.x + (p - (int64_t)m.z));
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (dfpos[mid] < p) lo = mid + 1; else hi = mid;
    }
    return dfpos[lo] == p;
}

}  // namespace taoamd

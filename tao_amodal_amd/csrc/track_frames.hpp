// The frame index of the passes over (ground-truth frame) x (the detection
// tracks of its cell) -- the association, the identity, HOTA and CLEAR: three
// descriptor tables in the call's workspace, the one build of them (called
// through track_index of track_tables.hpp, which holds what else those files
// share), and the probe of a detection track's frame list for a timeline
// position.  (assoc_pair_kernel has frames_find's lines
// written out in its loop: calling it, or a form that takes the hit's body, cost
// the kernel 38 VGPRs for 36 and, on an MI355X beside the written-out form in one
// run, 0.351-0.354 ms for 0.347-0.349.  ident_share_kernel
// calls it.)
//
//   frames_dt_meta_kernel   lane = detection track: {first frame, end, first and
//                           last position} of its frame list, clamped to the tables
//   frames_gt_cell_kernel   lane = cell: the cell of every ground-truth row
//   frames_frame_gt_kernel  wavefront = ground-truth track: the track of every frame
// HOTA (track_hota.hip) builds, beside the three, a fourth table of its own, the
// twin of dt_meta for the ground-truth tracks:
//   frames_gt_meta_kernel   lane = ground-truth track (frames_build_gt_meta)
//
// EMPTY SIDES, the one rule: frames_build leaves every table complete whatever
// is empty -- a table without rows costs neither a memset nor a launch; a ground-
// truth row no cell lists and a frame no track lists read -1, a detection track
// without frames has first position > last, and the frame kernels then find no
// candidate.  A pass returns before the build where it has no ground-truth track
// (n_gt == 0: no row to write) and launches its frame kernel behind it where
// there are ground-truth frames (n_gt_frames > 0).
#pragma once
#include "common.hpp"
#include "workspace.hpp"

namespace taoamd {

struct FrameTables {
    int4 *dt_meta;                   // [n_dt] {first frame, end, first position, last position}
    int32_t *gt_cell;                // [n_gt], -1: in no cell
    int32_t *frame_gt;               // [n_gt_frames], -1: of no track
};

// The tables come first in the workspace of either pass
static inline void frames_layout(Carve &c, int64_t n_dt, int64_t n_gt, int64_t n_gt_frames,
                                 FrameTables &t)
{
    t.dt_meta = c.take<int4>((size_t)n_dt);
    t.gt_cell = c.take<int32_t>((size_t)n_gt);
    t.frame_gt = c.take<int32_t>((size_t)n_gt_frames);
}

// What the tables are built from
struct FrameSource {
    int64_t n_dt, n_gt, n_cells, n_dt_frames, n_gt_frames;
    const int32_t *cell_gt_off, *dfoff, *dfpos, *gfoff;
};

static __global__ __launch_bounds__(256) void frames_dt_meta_kernel(FrameSource a, FrameTables t)
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
    t.dt_meta[d] = m;
}

static __global__ __launch_bounds__(256) void frames_gt_cell_kernel(FrameSource a, FrameTables t)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.n_cells) return;
    const int64_t g0 = clamp64(a.cell_gt_off[c], 0, a.n_gt);
    const int64_t g1 = clamp64(a.cell_gt_off[c + 1], g0, a.n_gt);
    for (int64_t g = g0; g < g1; g++) t.gt_cell[g] = (int32_t)c;
}

static __global__ __launch_bounds__(256) void frames_frame_gt_kernel(FrameSource a, FrameTables t)
{
    const int64_t g = (int64_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    if (g >= a.n_gt) return;
    const int64_t s = clamp64(a.gfoff[g], 0, a.n_gt_frames);
    const int64_t e = clamp64(a.gfoff[g + 1], s, a.n_gt_frames);
    for (int64_t k = s + lane_id(); k < e; k += WAVE) t.frame_gt[k] = (int32_t)g;
}

// The three tables on stream s, complete for any sizes (see EMPTY SIDES above)
static inline int frames_build(const FrameSource &a, const FrameTables &t, hipStream_t s)
{
    if (a.n_gt > 0) TAO_HIP(hipMemsetAsync(t.gt_cell, 0xff, (size_t)a.n_gt * sizeof(int32_t), s));
    if (a.n_gt_frames > 0)
        TAO_HIP(hipMemsetAsync(t.frame_gt, 0xff, (size_t)a.n_gt_frames * sizeof(int32_t), s));
    if (a.n_dt > 0)
        TAO_TIMED("frames_dt_meta_kernel", s,
                  frames_dt_meta_kernel<<<(unsigned)((a.n_dt + 255) / 256), 256, 0, s>>>(a, t));
    if (a.n_cells > 0 && a.n_gt > 0)
        TAO_TIMED("frames_gt_cell_kernel", s,
                  frames_gt_cell_kernel<<<(unsigned)((a.n_cells + 255) / 256), 256, 0, s>>>(a, t));
    if (a.n_gt > 0 && a.n_gt_frames > 0) {
        const int per = 256 / WAVE;
        TAO_TIMED("frames_frame_gt_kernel", s,
                  frames_frame_gt_kernel<<<(unsigned)((a.n_gt + per - 1) / per), 256, 0, s>>>(a, t));
    }
    return TAOAMD_OK;
}

// The twin of dt_meta for the ground-truth tracks, for the pass that also asks
// which OTHER ground truths of a cell have a frame at a position (track_hota.hip):
// gt_meta[n_gt] = {first frame, end, first and last position}, a table of the
// pass's own beside the three above, probed by frames_find like dt_meta.
static __global__ __launch_bounds__(256) void frames_gt_meta_kernel(int64_t n_gt,
                                                                    int64_t n_gt_frames,
                                                                    const int32_t *gfoff,
                                                                    const int32_t *gfpos,
                                                                    int4 *gt_meta)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_gt) return;
    const int64_t fs = clamp64(gfoff[g], 0, n_gt_frames);
    const int64_t fe = clamp64(gfoff[g + 1], fs, n_gt_frames);
    int4 m = make_int4((int32_t)fs, (int32_t)fe, 0, -1);
    if (fe > fs) {
        m.z = gfpos[fs];
        m.w = gfpos[fe - 1];
    }
    gt_meta[g] = m;
}

static inline int frames_build_gt_meta(int64_t n_gt, int64_t n_gt_frames, const int32_t *gfoff,
                                       const int32_t *gfpos, int4 *gt_meta, hipStream_t s)
{
    if (n_gt > 0)
        TAO_TIMED("frames_gt_meta_kernel", s,
                  frames_gt_meta_kernel<<<(unsigned)((n_gt + 255) / 256), 256, 0, s>>>(
                      n_gt, n_gt_frames, gfoff, gfpos, gt_meta));
    return TAOAMD_OK;
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

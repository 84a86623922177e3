// What the track analyses share besides the frame index (track_frames.hpp): the
// argument block of their kernels, the view of a cell, and the host side of an
// entry point -- the refusals, the carved workspace, the build of the index.
// HOTA (track_hota.hip) uses all of it.  The association, the identity and CLEAR
// (track_association.hip, track_identity.hip, track_clear.hip) use the host side
// and the views; their kernels keep the argument blocks they had, filled from
// TrackTables by track_fill, because a kernel of each measured slower over the
// common head (the note at each block says which).  The occlusion episodes
// (track_occlusion.hip: no cells) use the span alone.
//
// Device side.  Rows are those of the use_cats = 1 track table; a cell (video,
// category) owns the detection rows [d0, d0 + D), the ground-truth rows [g0, g0 +
// G) and, where the call has the layout of the IoU matrix, the words off + d * G
// + g of a per-pair table.  Every offset is clamped to its table: a bad CSR reads
// wrong entries, never past an end (a word of a per-pair table is guarded by its
// user, 0 <= i < n_iou).
// Host side.  An entry point sets TrackTables from its parameters (0 / null for
// what it does not take), refuses what is its own, and calls track_args with the
// TT_* flags of the tables it reads: TAOAMD_ERR_ARG, then TAOAMD_ERR_WORKSPACE,
// both before any device work.
#pragma once
#include "track_frames.hpp"

namespace taoamd {

// The common head of an analysis's kernel arguments: { TrackTables t; its own }.
// (A field a kernel never reads costs it no load; where the fields lie does
// decide how the compiler groups and places the loads of the others.)
struct TrackTables {
    int64_t n_dt, n_gt, n_cells, n_iou, n_dt_frames, n_gt_frames;
    const int32_t *cell_dt_off, *cell_gt_off;
    const int64_t *cell_iou_off;
    const int32_t *gt_cat;
    const uint8_t *gt_flags;
    const int32_t *dfoff, *dfpos;
    const double4 *dfbox;
    const int32_t *gfoff, *gfpos;
    const double4 *gfbox;
    FrameTables ft;                  // the frame index, in the call's workspace
};

struct TrackCell {
    int64_t d0, D, g0, G, off;
};

// The views read any block that names the tables as TrackTables does.
// (OFF = false: a call without cell_iou_off -- CLEAR -- gets off = 0)
template <bool OFF = true, class T>
__device__ __forceinline__ TrackCell track_cell(const T &t, int64_t cell)
{
    TrackCell c;
    c.d0 = clamp64(t.cell_dt_off[cell], 0, t.n_dt);
    c.D = clamp64(t.cell_dt_off[cell + 1], c.d0, t.n_dt) - c.d0;
    c.g0 = clamp64(t.cell_gt_off[cell], 0, t.n_gt);
    c.G = clamp64(t.cell_gt_off[cell + 1], c.g0, t.n_gt) - c.g0;
    c.off = 0;
    if constexpr (OFF) c.off = t.cell_iou_off[cell];
    return c;
}

template <class T> __device__ __forceinline__ bool track_eligible(const T &t, int64_t g)
{
    return !(t.gt_flags[g] & TAOAMD_GT_IGNORE);
}

// The frames [first, end) of row r of a CSR frame list of n_frames entries
struct TrackSpan {
    int64_t first, end;
    __device__ __forceinline__ int64_t len() const { return end - first; }
};

__device__ __forceinline__ TrackSpan track_span(const int32_t *off, int64_t r, int64_t n_frames)
{
    TrackSpan s;
    s.first = clamp64(off[r], 0, n_frames);
    s.end = clamp64(off[r + 1], s.first, n_frames);
    return s;
}

// ---------------------------------------------------------------------------
// the host side of an entry point
// ---------------------------------------------------------------------------
// Which tables a call reads (cell_dt_off, cell_gt_off and gt_frame_off: every call
// that passes the size they belong to), and what its workspace holds
enum : unsigned {
    TT_IOU = 1u,                     // cell_iou_off
    TT_GT_CAT = 2u,
    TT_GT_FLAGS = 4u,
    TT_DT_OFF = 8u,                  // dt_frame_off
    TT_DT_FRAMES = 16u,              // dt_frame_pos and dt_frame_box
    TT_GT_POS = 32u,
    TT_GT_BOX = 64u,
    TT_BOXES = TT_DT_OFF | TT_DT_FRAMES | TT_GT_POS | TT_GT_BOX,
    // a search store (assign_solve.hpp): arrays of n_dt + n_gt entries
    TT_STORE = 128u,
};

static inline bool track_sizes_ok(int64_t n_dt, int64_t n_gt, int64_t n_gt_frames, unsigned need)
{
    const int64_t lim = 0x7fffffff;
    return n_dt >= 0 && n_dt <= lim && n_gt >= 0 && n_gt <= lim && n_gt_frames >= 0 &&
           n_gt_frames <= lim && (!(need & TT_STORE) || n_dt + n_gt <= lim);
}

static inline const double4 *track_boxes(const double *box)
{
    return reinterpret_cast<const double4 *>(box);
}

// The refusals every entry point shares, then the workspace: layout(Carve &) takes
// the call's tables (the frame index among them) from the caller's pointer
template <class Layout>
static inline int track_args(const TrackTables &t, unsigned need, void *workspace,
                             size_t workspace_bytes, Layout layout)
{
    const int64_t lim = 0x7fffffff;
    if (!track_sizes_ok(t.n_dt, t.n_gt, t.n_gt_frames, need) || t.n_cells < 0 ||
        t.n_cells > lim || t.n_iou < 0 || t.n_dt_frames < 0 || t.n_dt_frames > lim)
        return TAOAMD_ERR_ARG;
    if (!workspace) return TAOAMD_ERR_ARG;
    if (t.n_cells > 0 &&
        (!t.cell_dt_off || !t.cell_gt_off || ((need & TT_IOU) && !t.cell_iou_off)))
        return TAOAMD_ERR_ARG;
    if (t.n_dt > 0 && (need & TT_DT_OFF) && !t.dfoff) return TAOAMD_ERR_ARG;
    if (t.n_dt_frames > 0 && (need & TT_DT_FRAMES) && (!t.dfpos || !t.dfbox))
        return TAOAMD_ERR_ARG;
    if (t.n_gt > 0 && (!t.gfoff || ((need & TT_GT_CAT) && !t.gt_cat) ||
                       ((need & TT_GT_FLAGS) && !t.gt_flags)))
        return TAOAMD_ERR_ARG;
    if (t.n_gt_frames > 0 &&
        (((need & TT_GT_POS) && !t.gfpos) || ((need & TT_GT_BOX) && !t.gfbox)))
        return TAOAMD_ERR_ARG;
    Carve c(workspace);
    layout(c);
    return c.fits(workspace, workspace_bytes) ? TAOAMD_OK : TAOAMD_ERR_WORKSPACE;
}

// The common fields of a kernel's own argument block from t (IOU = false: a block
// without n_iou and cell_iou_off)
template <bool IOU = true, class A> static inline void track_fill(A &a, const TrackTables &t)
{
    a.n_dt = t.n_dt; a.n_gt = t.n_gt; a.n_cells = t.n_cells;
    a.n_dt_frames = t.n_dt_frames; a.n_gt_frames = t.n_gt_frames;
    a.cell_dt_off = t.cell_dt_off; a.cell_gt_off = t.cell_gt_off;
    if constexpr (IOU) {
        a.n_iou = t.n_iou;
        a.cell_iou_off = t.cell_iou_off;
    }
    a.gt_cat = t.gt_cat; a.gt_flags = t.gt_flags;
    a.dfoff = t.dfoff; a.dfpos = t.dfpos; a.dfbox = t.dfbox;
    a.gfoff = t.gfoff; a.gfpos = t.gfpos; a.gfbox = t.gfbox;
    a.ft = t.ft;
}

// The frame index of t on stream s (frames_build: complete for any sizes)
static inline int track_index(const TrackTables &t, hipStream_t s)
{
    const FrameSource src = {t.n_dt, t.n_gt, t.n_cells, t.n_dt_frames, t.n_gt_frames,
                             t.cell_gt_off, t.dfoff, t.dfpos, t.gfoff};
    return frames_build(src, t.ft, s);
}

}  // namespace taoamd

// Track-level association (gfx950): WHICH detection track follows a ground-
// truth track, frame by frame.  The reference has no such table; the definition
// is this library's, stated in include/tao_amodal_hip.h and DESIGN.md section 8.
//
// Rows are those of the use_cats = 1 track table.  Ground-truth track g lies in
// one cell (video, category); its candidates are the detection tracks of that
// cell.  For frame k of g at timeline position p_k, f(d, g, k) = box_iou(d's box
// at p_k, g's box) where d has a frame at p_k, and best_k(g) = the candidate of
// the greatest f >= frame_thr, the lowest row among equal values, -1 if none.
//
//   track_index           the frame index (track_frames.hpp); the entry point's
//                         common part is track_tables.hpp's
//   assoc_pair_kernel     THE HOT ONE.  lane = ground-truth frame, the whole table
//                         as one flat list: a lane holds its frame's box and
//                         position in registers and walks the cell's detection
//                         tracks in ascending row, so a strict `>` keeps the lowest
//                         row and the (max, row) state never leaves the lane -- no
//                         LDS, no barrier, no cross-lane step, no rounds: a cell of
//                         any size is the same loop.  A candidate's frame at p_k is
//                         found in its position list (strictly ascending integers)
//                         between the two indices the track's first and last
//                         position allow: a track without holes is ONE probe, else
//                         a binary search between them (frames_find's lines,
//                         written out: see track_frames.hpp).  Lanes of a
//                         wavefront are consecutive frames, as a rule of one track:
//                         the candidate's descriptor is one address for all of
//                         them, the probes touch neighbouring entries.
//   assoc_walk_kernel     wavefront = ground-truth track, lane = frame of a chunk of
//                         64: best[] is read coalesced; covered, fragments and
//                         switches are popcounts of ballots (the covered frame
//                         before a lane's is the highest covered lane below it, or
//                         the carry of the chunk before); the follow counts are one
//                         INTEGER add per distinct follower of a chunk into the
//                         track's own column -- order-free, nothing is decided by
//                         arrival
//   assoc_column_kernel   wavefront = ground-truth track, behind a kernel boundary:
//                         ids and the primary from the finished column (lanes
//                         stride it; the greatest (count, ~index) of the wavefront),
//                         then the frames once more for the visibility windows,
//                         which need the primary
//   assoc_tally_kernel    lane = ground-truth track: its row into the two count
//                         tables, integer adds, one per (wavefront, category,
//                         column) (wave_add of common.hpp)
// (A lane per track that walks its own frames, the first form of the three, took
// 0.63 ms at 20 000 tracks of 150 frames: 300 wavefronts, every load 64 cache
// lines, two dependent walks.  See DESIGN.md section 8.)
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   assoc_pair_kernel 36 VGPRs, 34 SGPRs, 8 waves/SIMD, no scratch, no LDS.
// box_iou is common.hpp's, compiled with -ffp-contract=off like every other use:
// the bits of taoamd_bb_iou.  Everything else is an integer.
#include "track_tables.hpp"

using namespace taoamd;

#define TA_TILE TAOAMD_TRACK_ASSOCIATION_TILE   // ground-truth frames per workgroup of the pair kernel
#define TA_VMAX TAOAMD_TRACK_ASSOCIATION_VIS    // visibility windows
#define TA_NASSOC 7
#define TA_NCAT 8
#define TA_NVIS 3

static_assert(TA_TILE % WAVE == 0, "whole wavefronts");

// The kernels' argument block is this file's own, the common fields where they
// were (track_fill sets them): over { TrackTables t; ... } assoc_pair_kernel
// compiled to the same 36 VGPRs and the same loop, its argument loads scheduled
// otherwise, and measured 0.3499-0.3516 ms beside 0.3445-0.3457 of the parent,
// whose code this form compiles to, five runs each in turn on one MI355X (a run
// of its own: other runs lie up to 1 % apart as a whole) -- the sensitivity the
// note in track_frames.hpp records.
struct AssocArgs {
    int64_t n_dt, n_gt, n_cells, n_iou, n_dt_frames, n_gt_frames;
    int32_t n_cat, n_vis;
    double thr;
    const int32_t *cell_dt_off, *cell_gt_off;
    const int64_t *cell_iou_off;
    const int32_t *gt_cat;
    const uint8_t *gt_flags;
    const int32_t *dfoff, *dfpos;
    const double4 *dfbox;
    const int32_t *gfoff, *gfpos;
    const double4 *gfbox;
    const double *gfvis, *vis_rng;
    int32_t *follow;                 // [n_iou], the layout of the IoU matrix
    int32_t *gt_assoc;               // [n_gt][7]
    unsigned long long *cat_counts;  // [n_cat][8]
    unsigned long long *vis_counts;  // [n_vis][n_cat][3]
    int32_t *best;                   // [n_gt_frames]
    double *best_iou;                // [n_gt_frames] or null
    FrameTables ft;                  // the frame index (track_frames.hpp)
    int32_t *trk_vis;                // [n_gt][8][3]: a track's counts per visibility window
};

__global__ __launch_bounds__(TA_TILE) void assoc_pair_kernel(AssocArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * TA_TILE + threadIdx.x;
    if (k >= a.n_gt_frames) return;
    const int32_t g = a.ft.frame_gt[k];
    const int32_t cell = g >= 0 ? a.ft.gt_cell[g] : -1;
    int64_t d0 = 0, d1 = 0;
    if (cell >= 0) {
        d0 = clamp64(a.cell_dt_off[cell], 0, a.n_dt);
        d1 = clamp64(a.cell_dt_off[cell + 1], d0, a.n_dt);
    }
    int32_t arg = -1;
    double top = 0.0;
    if (d1 > d0) {
        const int64_t p = a.gfpos[k];
        const double4 G = a.gfbox[k];
        for (int64_t d = d0; d < d1; d++) {
            // (frames_find of track_frames.hpp, written out: see the note there)
            const int4 m = a.ft.dt_meta[d];
            if (p < m.z || p > m.w) continue;          // (a track without frames: z > w)
            int64_t lo = max((int64_t)m.x, (int64_t)m.y - 1 - ((int64_t)m.w - p));
            int64_t hi = min((int64_t)m.y - 1, (int64_t)m.x + (p - (int64_t)m.z));
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (a.dfpos[mid] < p) lo = mid + 1; else hi = mid;
            }
            if (a.dfpos[lo] != p) continue;
            const double4 D = a.dfbox[lo];
            const double v = box_iou(D.x, D.y, D.z, D.w, G.x, G.y, G.z, G.w);
            // (ascending rows: an equal overlap never replaces the follower; a NaN compares
            // false; frame_thr > 0 = the empty maximum)
            if (v >= a.thr && v > top) {
                top = v;
                arg = (int32_t)(d - d0);
            }
        }
    }
    a.best[k] = arg;
    if (a.best_iou) a.best_iou[k] = top;
}

// A wavefront's ground-truth track: its frames [s, e), its candidates [d0, d0 + D)
// and its column of `follow` (entry d at col + d * G), clamped to the tables.
struct OwnColumn {
    int64_t s, e, d0, D, G, col;
    __device__ __forceinline__ void init(const AssocArgs &a, int64_t g)
    {
        const TrackSpan f = track_span(a.gfoff, g, a.n_gt_frames);
        s = f.first;
        e = f.end;
        d0 = D = G = col = 0;
        const int32_t cell = a.ft.gt_cell[g];
        if (cell >= 0) {
            const TrackCell c = track_cell(a, cell);
            d0 = c.d0;
            D = c.D;
            G = c.G;
            col = c.off + (g - c.g0);
        }
    }
    // where the count of in-cell index d lies, -1: nowhere
    __device__ __forceinline__ int64_t at(const AssocArgs &a, int64_t d) const
    {
        const int64_t i = col + d * G;
        return d < D && i >= 0 && i < a.n_iou ? i : -1;
    }
};

// wavefront = ground-truth track, lane = frame of a chunk of 64: one coalesced read
// of best[] a chunk; covered, fragments and switches are popcounts of ballots (the
// covered frame before a lane's = the highest covered lane below it, or the carry
// of the chunk before), the follow counts one integer add per distinct follower of
// the chunk.  Everything counted is the same in every lane.
__global__ __launch_bounds__(256) void assoc_walk_kernel(AssocArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    if (g >= a.n_gt) return;                 // (whole wavefronts)
    const int lane = lane_id();
    OwnColumn o;
    o.init(a, g);
    int32_t covered = 0, switches = 0, fragments = 0;
    int32_t last = -1;                       // the follower of the last covered frame so far
    bool gap = true;                         // the frame before the chunk is uncovered (or there is none)
    for (int64_t base = o.s; base < o.e; base += WAVE) {
        const int64_t k = base + lane;
        const int32_t b = k < o.e ? a.best[k] : -1;
        const bool cov = b >= 0;
        const uint64_t m = __ballot(cov);
        if (m == 0) { gap = true; continue; }           // (uniform)
        covered += __popcll(m);
        const bool open = lane == 0 ? gap : !((m >> ((lane + WAVE - 1) & (WAVE - 1))) & 1ull);
        fragments += __popcll(__ballot(cov && open));
        const uint64_t below = m & ((1ull << lane) - 1ull);
        int32_t before = __shfl(b, below ? 63 - __builtin_clzll(below) : 0);
        before = below ? before : last;
        switches += __popcll(__ballot(cov && before >= 0 && before != b));
        uint64_t left = m;
        while (left) {
            const int lead = __builtin_ctzll(left);
            const int32_t d = __builtin_amdgcn_readlane(b, lead);
            const uint64_t same = __ballot(b == d);
            const int64_t at = o.at(a, d);
            if (lane == lead && at >= 0) atomicAdd(a.follow + at, (int32_t)__popcll(same));
            left &= ~same;
        }
        last = __builtin_amdgcn_readlane(b, 63 - __builtin_clzll(m));
        gap = !((m >> (WAVE - 1)) & 1ull);
    }
    if (lane == 0) {
        int32_t *out = a.gt_assoc + g * TA_NASSOC;
        out[0] = (int32_t)(o.e - o.s);
        out[1] = covered;
        out[3] = switches;
        out[4] = fragments;
    }
}

// wavefront = ground-truth track, behind the walk (a kernel boundary: the column
// is complete).  Lanes stride the column: ids, and the primary as the greatest
// (count, ~index); then the frames once more, coalesced, for the visibility
// windows, which need the primary: the track's [window][3] counts go to trk_vis.
__global__ __launch_bounds__(256) void assoc_column_kernel(AssocArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    if (g >= a.n_gt) return;                 // (whole wavefronts)
    const int lane = lane_id();
    OwnColumn o;
    o.init(a, g);
    int32_t ids = 0;
    unsigned long long top = 0;              // count << 32 | ~index: the greatest count, the lowest index
    for (int64_t d = lane; d < o.D; d += WAVE) {
        const int64_t at = o.at(a, d);
        const int32_t c = at >= 0 ? a.follow[at] : 0;
        const unsigned long long key = ((unsigned long long)(uint32_t)c << 32) | (uint32_t)~(uint32_t)d;
        ids += c > 0;
        top = c > 0 && key > top ? key : top;
    }
    ids = wave_sum(ids);
    top = wave_max(top);
    const int32_t prim = top ? (int32_t)~(uint32_t)top : -1;
    int32_t cnt[TA_VMAX][TA_NVIS];
#pragma unroll
    for (int w = 0; w < TA_VMAX; w++) cnt[w][0] = cnt[w][1] = cnt[w][2] = 0;
    if (a.n_vis > 0)                         // (uniform)
        for (int64_t base = o.s; base < o.e; base += WAVE) {
            const int64_t k = base + lane;
            const bool live = k < o.e;
            const int32_t b = live ? a.best[k] : -1;
            const double vis = live ? a.gfvis[k] : 0.0;
#pragma unroll
            for (int w = 0; w < TA_VMAX; w++) {
                if (w >= a.n_vis) continue;  // (uniform)
                // (closed windows; a NaN visibility compares false: in no window)
                const bool in = live && a.vis_rng[2 * w] <= vis && vis <= a.vis_rng[2 * w + 1];
                cnt[w][0] += __popcll(__ballot(in));
                cnt[w][1] += __popcll(__ballot(in && b >= 0));
                cnt[w][2] += __popcll(__ballot(in && b >= 0 && b == prim));
            }
        }
    if (lane == 0) {
        int32_t *out = a.gt_assoc + g * TA_NASSOC;
        out[2] = ids;
        out[5] = prim >= 0 ? (int32_t)(o.d0 + prim) : -1;
        out[6] = (int32_t)(top >> 32);
        int32_t *v = a.trk_vis + g * (TA_VMAX * TA_NVIS);
#pragma unroll
        for (int w = 0; w < TA_VMAX; w++) {
            v[w * TA_NVIS] = cnt[w][0];
            v[w * TA_NVIS + 1] = cnt[w][1];
            v[w * TA_NVIS + 2] = cnt[w][2];
        }
    }
}

// lane = ground-truth track: its row of gt_assoc and of trk_vis into the two count
// tables, one integer add per (wavefront, category, column)
__global__ __launch_bounds__(256) void assoc_tally_kernel(AssocArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = g < a.n_gt;
    const int32_t cat = valid ? a.gt_cat[g] : 0;
    const bool ok = valid && track_eligible(a, g) && cat >= 0 && cat < a.n_cat;
    int32_t frames = 0, covered = 0, ids = 0, switches = 0, fragments = 0;
    if (ok) {
        const int32_t *in = a.gt_assoc + g * TA_NASSOC;
        frames = in[0]; covered = in[1]; ids = in[2]; switches = in[3]; fragments = in[4];
    }
    const int32_t row[TA_NCAT] = {1, frames, covered, ids, switches, fragments,
                                  5 * (int64_t)covered >= 4 * (int64_t)frames,
                                  5 * (int64_t)covered < (int64_t)frames};
    wave_add(a.cat_counts, TA_NCAT, ok, cat, row);
#pragma unroll
    for (int w = 0; w < TA_VMAX; w++) {
        if (w >= a.n_vis) continue;          // (uniform)
        int32_t cnt[TA_NVIS] = {0, 0, 0};
        if (ok) {
            const int32_t *v = a.trk_vis + g * (TA_VMAX * TA_NVIS) + w * TA_NVIS;
            cnt[0] = v[0]; cnt[1] = v[1]; cnt[2] = v[2];
        }
        wave_add(a.vis_counts + (int64_t)w * a.n_cat * TA_NVIS, TA_NVIS, ok, cat, cnt);
    }
}

// The tables of the pass, in buffer order: a function of (n_dt, n_gt, n_gt_frames)
static void assoc_layout(Carve &c, int64_t n_dt, int64_t n_gt, int64_t n_gt_frames,
                         FrameTables &ft, AssocArgs &a)
{
    frames_layout(c, n_dt, n_gt, n_gt_frames, ft);
    a.trk_vis = c.take<int32_t>((size_t)n_gt * TA_VMAX * TA_NVIS);
}

extern "C" size_t taoamd_track_association_workspace(int64_t n_dt, int64_t n_gt,
                                                     int64_t n_gt_frames)
{
    if (!track_sizes_ok(n_dt, n_gt, n_gt_frames, 0)) return 0;
    AssocArgs a;
    return measure([&](Carve &c) { assoc_layout(c, n_dt, n_gt, n_gt_frames, a.ft, a); });
}

extern "C" int taoamd_track_association(
    int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou, int64_t n_dt_frames,
    int64_t n_gt_frames, int32_t n_cat, int32_t n_vis, double frame_thr,
    const int32_t *cell_dt_off, const int32_t *cell_gt_off, const int64_t *cell_iou_off,
    const int32_t *gt_cat, const uint8_t *gt_flags, const int32_t *dt_frame_off,
    const int32_t *dt_frame_pos, const double *dt_frame_box, const int32_t *gt_frame_off,
    const int32_t *gt_frame_pos, const double *gt_frame_box, const double *gt_frame_vis,
    const double *vis_rng, int32_t *follow, int32_t *gt_assoc, int64_t *cat_counts,
    int64_t *vis_counts, int32_t *best, double *best_iou, void *workspace,
    size_t workspace_bytes, void *stream)
{
    TrackTables t = {n_dt, n_gt, n_cells, n_iou, n_dt_frames, n_gt_frames, cell_dt_off,
                     cell_gt_off, cell_iou_off, gt_cat, gt_flags, dt_frame_off, dt_frame_pos,
                     track_boxes(dt_frame_box), gt_frame_off, gt_frame_pos,
                     track_boxes(gt_frame_box)};
    if (n_cat <= 0 || n_vis < 0 || n_vis > TA_VMAX) return TAOAMD_ERR_ARG;
    // (a NaN compares false both times)
    if (!(frame_thr > 0) || !(frame_thr <= 1)) return TAOAMD_ERR_ARG;
    if (!cat_counts || (n_gt > 0 && !gt_assoc) || (n_gt_frames > 0 && !best)) return TAOAMD_ERR_ARG;
    if (n_vis > 0 && (!vis_rng || !vis_counts || (n_gt_frames > 0 && !gt_frame_vis)))
        return TAOAMD_ERR_ARG;
    if (n_iou > 0 && !follow) return TAOAMD_ERR_ARG;
    AssocArgs a;
    const int st = track_args(t, TT_IOU | TT_GT_CAT | TT_GT_FLAGS | TT_BOXES, workspace,
                              workspace_bytes,
                              [&](Carve &c) { assoc_layout(c, n_dt, n_gt, n_gt_frames, t.ft, a); });
    if (st != TAOAMD_OK) return st;
    track_fill(a, t);
    hipStream_t s = (hipStream_t)stream;
    a.n_cat = n_cat; a.n_vis = n_vis; a.thr = frame_thr;
    a.gfvis = gt_frame_vis; a.vis_rng = vis_rng;
    a.follow = follow; a.gt_assoc = gt_assoc;
    a.cat_counts = (unsigned long long *)cat_counts;
    a.vis_counts = (unsigned long long *)vis_counts;
    a.best = best; a.best_iou = best_iou;
    TAO_HIP(hipMemsetAsync(cat_counts, 0, (size_t)n_cat * TA_NCAT * sizeof(int64_t), s));
    if (n_vis > 0)
        TAO_HIP(hipMemsetAsync(vis_counts, 0, (size_t)n_vis * n_cat * TA_NVIS * sizeof(int64_t), s));
    if (n_iou > 0) TAO_HIP(hipMemsetAsync(follow, 0, (size_t)n_iou * sizeof(int32_t), s));
    if (n_gt == 0) return TAOAMD_OK;
    // (empty sides: the rule of track_frames.hpp.  A ground-truth row no cell lists has
    // no candidates, a frame no track lists no follower)
    const int si = track_index(t, s);
    if (si != TAOAMD_OK) return si;
    if (n_gt_frames > 0)
        TAO_TIMED("assoc_pair_kernel", s,
                  assoc_pair_kernel<<<(unsigned)((n_gt_frames + TA_TILE - 1) / TA_TILE), TA_TILE,
                                      0, s>>>(a));
    const int per = 256 / WAVE;
    const unsigned track_blocks = (unsigned)((n_gt + per - 1) / per);
    TAO_TIMED("assoc_walk_kernel", s, assoc_walk_kernel<<<track_blocks, 256, 0, s>>>(a));
    TAO_TIMED("assoc_column_kernel", s, assoc_column_kernel<<<track_blocks, 256, 0, s>>>(a));
    TAO_TIMED("assoc_tally_kernel", s,
              assoc_tally_kernel<<<(unsigned)((n_gt + 255) / 256), 256, 0, s>>>(a));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

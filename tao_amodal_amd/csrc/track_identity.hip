// Track-level identity (gfx950): IDF1 / IDP / IDR from an optimal one-to-one
// assignment of detection tracks to ground-truth tracks (Ristani et al., ECCV
// 2016).  The reference has no such table; the definition is this library's,
// stated in include/tao_amodal_hip.h and DESIGN.md section 8.
//
// Rows, cells, frame lists and the entry points' common part are those of every
// track analysis (track_tables.hpp, track_frames.hpp).  Two calls:
//
// taoamd_track_identity_share: share[cell_iou_off[cell] + d * G + g] = the frames
// of ground-truth track g on which detection track d has a frame with box_iou >=
// frame_thr -- per pair a COUNT, neither the 3D IoU's sum nor the association's
// arg-max.
//   ident_share_kernel   lane = ground-truth frame, the whole table as one flat
//                        list: the association's pair loop with frames_find as
//                        its probe, but every candidate with an overlap
//                        >= frame_thr counts, not the greatest:
//                        an integer atomic add per (pair, wavefront) with a hit,
//                        the lanes of one pair found by ballot.  No LDS, no limit
//                        on a cell or a track.
//
// taoamd_track_identity_assign: a maximum-weight bipartite assignment per cell.
//   ident_init_kernel    lane = row: {-1, 0} into gt_ident and dt_ident (rows no
//                        cell lists stay so)
//   ident_assign_kernel  workgroup = ONE wavefront = cell.
//                        1  lane = detection track: its greatest share with an
//                           eligible and with an ignored ground truth -> kept;
//                           the kept ones with a positive share are compacted (a
//                           ballot and a prefix popcount) into the cell's slice
//                           of idx[]
//                        2  lane = ground-truth track: the eligible ones with a
//                           positive share in a compacted row are compacted
//                        3  the smaller side becomes the rows, the detections
//                           when equal
//                        4  assign_solve (assign_solve.hpp), its state in LDS
//                           where m <= TI_LDS, else in the cell's slice of the
//                           search store
//                        A bound of the solver that runs out stores 1 to *status
//                        and ends the cell with its pairs at -1; nothing spins.
//                        A pair weighs share * (n + 1) + (share > 0): among equal
//                        sums of shares the most pairs with a positive one, so
//                        that `pairs` is unique as well.
//                        The count tables are integer adds, one per (wavefront
//                        step, category, column) (wave_add of common.hpp).
//
// taoamd_track_score_pass, taoamd_track_identity_assign_at (the header's section
// "track-level score thresholds"): which detection tracks take part at a score.
//   score_pass_kernel    lane = (layer, detection track): the pass rule
//   ident_assign_kernel<true>  the kernel above with the layer as blockIdx.y: a
//                        wavefront per (cell, layer); kept is kept AND pass; the
//                        layer's slice of idx[], of the search store and of the
//                        outputs; *status by an atomic max
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   ident_share_kernel 38 VGPRs, 30 SGPRs, 8 waves/SIMD, no scratch, no LDS;
//   ident_assign_kernel 54 VGPRs, 11 264 B of LDS (a workgroup is one wavefront:
//   14 cells a CU by LDS), the same for both instances; score_pass_kernel 6 VGPRs.
#include "assign_solve.hpp"
#include "track_tables.hpp"

using namespace taoamd;

#define TI_TILE 64          // ground-truth frames per workgroup of the share kernel
#define TI_LDS 256          // columns (and rows) of a cell whose search state is in LDS
#define TI_NCAT 6

// The kernels' argument block is this file's own, the common fields where they
// were (track_fill sets them): ident_assign_kernel measured slower over
// { TrackTables t; ... } (the note in that kernel).
struct IdentArgs {
    int64_t n_dt, n_gt, n_cells, n_iou, n_dt_frames, n_gt_frames;
    int32_t n_cat;
    double thr;
    const int32_t *cell_dt_off, *cell_gt_off;
    const int64_t *cell_iou_off;
    const int32_t *gt_cat, *dt_cat;
    const uint8_t *gt_flags, *dt_flags;
    const int32_t *dfoff, *dfpos;
    const double4 *dfbox;
    const int32_t *gfoff, *gfpos;
    const double4 *gfbox;
    int32_t *share;                  // [n_iou], the layout of the IoU matrix
    unsigned long long *cat_counts;  // [n_cat][6]
    int32_t *gt_ident, *dt_ident;    // [n_gt][2], [n_dt][2]
    int32_t *status;
    FrameTables ft;                  // the frame index (track_frames.hpp)
    SearchStore store;               // the cells that do not fit in LDS
    int32_t *sidx;                   // [n_dt + n_gt]: the cells' two index lists
    // the layered call alone (taoamd_track_identity_assign_at): layer t has the
    // outputs, the store and sidx at t times their size, and reads dt_pass[t][.]
    int32_t n_thr;
    const uint8_t *dt_pass;          // [n_thr][n_dt]
};

__global__ __launch_bounds__(TI_TILE) void ident_share_kernel(IdentArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * TI_TILE + threadIdx.x;
    if (k >= a.n_gt_frames) return;
    const int32_t g = a.ft.frame_gt[k];
    const int32_t cell = g >= 0 ? a.ft.gt_cell[g] : -1;
    if (cell < 0) return;
    const TrackCell c = track_cell(a, cell);
    const int64_t col = c.off + (g - c.g0);
    const int64_t p = a.gfpos[k];
    const double4 B = a.gfbox[k];
    for (int64_t d = c.d0; d < c.d0 + c.D; d++) {
        int64_t at = -1, lo;
        if (frames_find(a.dfpos, a.ft.dt_meta[d], p, lo)) {
            const double4 D = a.dfbox[lo];
            const double v = box_iou(D.x, D.y, D.z, D.w, B.x, B.y, B.z, B.w);
            const int64_t i = col + (d - c.d0) * c.G;
            // (a NaN compares false: no overlap)
            if (v >= a.thr && i >= 0 && i < a.n_iou) at = i;
        }
        // One add per distinct pair among the lanes that are here together: a
        // wavefront's lanes are consecutive frames, as a rule of one track, and then
        // all its hits on d are one add.  (Lanes of other cells may be at another d
        // or gone; whoever is here is grouped by address, so any grouping is right.)
        uint64_t left = __ballot(at >= 0);
        while (left) {
            const int lead = __builtin_ctzll(left);
            const int64_t to = __shfl(at, lead);
            const uint64_t same = __ballot(at == to);
            if (lane_id() == lead) atomicAdd(a.share + to, (int32_t)__popcll(same));
            left &= ~same;
        }
    }
}

__global__ __launch_bounds__(256) void ident_init_kernel(IdentArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n_gt) reinterpret_cast<int2 *>(a.gt_ident)[i] = make_int2(-1, 0);
    if (i < a.n_dt) reinterpret_cast<int2 *>(a.dt_ident)[i] = make_int2(-1, 0);
}

// {-1, 0} into the rows of every layer: n_gi = n_thr * n_gt words of gt_ident (0
// without one), n_di = n_thr * n_dt of dt_ident
__global__ __launch_bounds__(256) void ident_init_layers_kernel(int2 *gt_ident, int64_t n_gi,
                                                                int2 *dt_ident, int64_t n_di)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_gi) gt_ident[i] = make_int2(-1, 0);
    if (i < n_di) dt_ident[i] = make_int2(-1, 0);
}

// The pass rule of the track-level score thresholds: lane = detection track,
// blockIdx.y = layer.  A NaN on either side compares false.
__global__ __launch_bounds__(256) void score_pass_kernel(int64_t n_dt, int32_t n_cat,
                                                         const double *dt_score,
                                                         const int32_t *dt_cat, const double *thr,
                                                         const uint8_t *base, uint8_t *pass)
{
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n_dt) return;
    const int32_t cat = dt_cat[d];
    bool on = cat >= 0 && cat < n_cat && (!base || base[d] != 0);
    if (on) on = dt_score[d] >= thr[(int64_t)blockIdx.y * n_cat + cat];
    pass[(int64_t)blockIdx.y * n_dt + d] = on ? 1 : 0;
}

// A cell's share matrix: entry (d, g) in-cell, 0 outside the table; a share is a
// count, so a negative word reads as 0 too
struct CellShare {
    const int32_t *share;
    int64_t off, G, n_iou;
    __device__ __forceinline__ int32_t at(int64_t d, int64_t g) const
    {
        const int64_t i = off + d * G + g;
        const int32_t s = i >= 0 && i < n_iou ? share[i] : 0;
        return s > 0 ? s : 0;
    }
};

// The weight of a pair for the solver: share * (n + 1) + (share > 0) -- the sum
// of shares decides, among equal sums the number of pairs with a positive share
// (fewer than n + 1), so that both numbers are unique.
struct IdentWeight {
    CellShare S;
    long long scale;                 // n + 1
    bool rows_are_dt;
    __device__ __forceinline__ long long operator()(int64_t r, int64_t c) const
    {
        const long long w = rows_are_dt ? S.at(r, c) : S.at(c, r);
        return w * scale + (w > 0);
    }
};

// AT: the layered call -- blockIdx.y is the layer, a wavefront per (cell, layer);
// the one-layer, mask-free instance is the kernel as it was.
template <bool AT> __global__ __launch_bounds__(WAVE) void ident_assign_kernel(IdentArgs a)
{
    // (SearchLds, track_cell, assign_sides and assign_pairs, written out; the tie
    // rule here is the other one: the detections become the rows when equal.
    // With the shared forms the kernel compiles to other code -- the cell's offset
    // loaded before the early return, the selects the other way round -- and
    // measured 0.0545-0.0549 ms beside 0.0536-0.0541 of the parent, five runs each
    // in turn on one MI355X (a run of its own).  These lines compile to the
    // instructions the kernel had.)
    __shared__ long long l_u[TI_LDS], l_v[TI_LDS], l_minv[TI_LDS];
    __shared__ int32_t l_p[TI_LDS], l_way[TI_LDS], l_used[TI_LDS], l_ridx[TI_LDS], l_cidx[TI_LDS];
    const int64_t cell = blockIdx.x;
    const int lane = lane_id();
    const int64_t d0 = clamp64(a.cell_dt_off[cell], 0, a.n_dt);
    const int64_t D = clamp64(a.cell_dt_off[cell + 1], d0, a.n_dt) - d0;
    const int64_t g0 = clamp64(a.cell_gt_off[cell], 0, a.n_gt);
    const int64_t G = clamp64(a.cell_gt_off[cell + 1], g0, a.n_gt) - g0;
    if (D == 0 && G == 0) return;
    CellShare S = {a.share, a.cell_iou_off[cell], G, a.n_iou};
    int64_t base = d0 + g0;                          // the cell's slice of the state arrays
    const uint8_t *pass = nullptr;
    if constexpr (AT) {
        const int64_t layer = blockIdx.y;
        base += layer * (a.n_dt + a.n_gt);           // ... of the layer's slice
        a.cat_counts += layer * a.n_cat * TI_NCAT;
        if (a.gt_ident) a.gt_ident += layer * a.n_gt * 2;
        a.dt_ident += layer * a.n_dt * 2;
        pass = a.dt_pass + layer * a.n_dt;
    }
    int32_t *dlist = a.sidx + base, *glist = a.sidx + base + D;
    const uint64_t below = (1ull << lane) - 1ull;

    // 1: kept detection tracks; those with a positive share in an eligible row
    int nd = 0;
    int32_t top = 0;                                 // the greatest share that can be assigned
    for (int64_t db = 0; db < D; db += WAVE) {
        const int64_t d = db + lane;
        const bool live = d < D;
        int32_t me = 0, mi = 0;
        if (live)
            for (int64_t g = 0; g < G; g++) {
                const int32_t v = S.at(d, g);
                if (track_eligible(a, g0 + g)) me = v > me ? v : me;
                else mi = v > mi ? v : mi;
            }
        bool kept = false;
        int32_t cat = 0;
        long long frames = 0;
        if (live) {
            kept = !(mi > me) && !((a.dt_flags[d0 + d] & TAOAMD_DT_IGNORE_UNMATCHED) && me == 0);
            if constexpr (AT) {
                // kept at a layer is kept AND pass: a track that does not pass is
                // neither compacted nor counted, so no column is kept for its sake
                if (!pass[d0 + d]) kept = false;
            }
            cat = a.dt_cat[d0 + d];
            frames = track_span(a.dfoff, d0 + d, a.n_dt_frames).len();
            a.dt_ident[(d0 + d) * 2 + 1] = kept;
        }
        const long long dt_cols[2] = {1, frames};                 // dt_tracks, dt_frames
        wave_add(a.cat_counts + 2, TI_NCAT, kept && cat >= 0 && cat < a.n_cat, cat, dt_cols);
        const bool act = kept && me > 0;
        top = act && me > top ? me : top;
        const uint64_t m = __ballot(act);
        if (act) dlist[nd + __popcll(m & below)] = (int32_t)d;
        nd += __popcll(m);
    }
    __syncthreads();
    // 2: eligible ground-truth tracks; those with a positive share in such a row
    int ng = 0;
    for (int64_t gb = 0; gb < G; gb += WAVE) {
        const int64_t g = gb + lane;
        const bool live = g < G;
        const bool elig = live && track_eligible(a, g0 + g);
        bool act = false;
        int32_t cat = 0;
        long long frames = 0;
        if (elig) {
            for (int i = 0; i < nd && !act; i++) act = S.at(dlist[i], g) > 0;
            cat = a.gt_cat[g0 + g];
            frames = track_span(a.gfoff, g0 + g, a.n_gt_frames).len();
        }
        const long long gt_cols[2] = {1, frames};                 // gt_tracks, gt_frames
        wave_add(a.cat_counts, TI_NCAT, elig && cat >= 0 && cat < a.n_cat, cat, gt_cols);
        const uint64_t m = __ballot(act);
        if (act) glist[ng + __popcll(m & below)] = (int32_t)g;
        ng += __popcll(m);
    }
    __syncthreads();
    if (nd == 0 || ng == 0) return;                  // (uniform)
    // 3: the smaller side as rows, the detections when equal
    const bool rows_are_dt = nd <= ng;
    const int n = rows_are_dt ? nd : ng, m = rows_are_dt ? ng : nd;
    // a potential is a sum of at most n weights, each at most top * (n + 1) + 1: in
    // 64 bits while n * (n + 1) * (top + 1) < 2^62.  A share of the share kernel is
    // at most a track's frames, so real tables are far inside; a table that is not
    // is refused, never solved wrongly
    top = wave_max(top);
    const unsigned long long nn = (unsigned long long)n * ((unsigned long long)n + 1);
    const unsigned long long ww = (unsigned long long)top + 1;
    if (__umul64hi(nn, ww) != 0 || nn * ww >= (1ull << 62)) {
        if (lane == 0) {
            if constexpr (AT) atomicMax(a.status, 2);
            else *a.status = 2;
        }
        return;
    }
    const int32_t *rl = rows_are_dt ? dlist : glist, *cl = rows_are_dt ? glist : dlist;
    // 4: the search, its state in LDS or in the cell's slice of the store.  (One
    // call on each side: inlined, the solver then knows which memory its state is
    // in; one call behind the choice goes through flat addresses.)
    const IdentWeight W = {S, (long long)n + 1, rows_are_dt};
    Search s;
    bool ok;
    if (m <= TI_LDS) {
        for (int i = lane; i < n; i += WAVE) l_ridx[i] = rl[i];
        for (int j = lane; j < m; j += WAVE) l_cidx[j] = cl[j];
        s = {l_u, l_v, l_minv, l_p, l_way, l_used, l_ridx, l_cidx};
        ok = assign_solve(W, s, n, m);
    } else {
        s = a.store.at(base);
        s.ridx = rl;
        s.cidx = cl;
        ok = assign_solve(W, s, n, m);
    }
    if (!ok) {
        if (lane == 0) {
            if constexpr (AT) atomicMax(a.status, 1);
            else *a.status = 1;
        }
        return;
    }
    // the pairs with a positive share
    for (int jb = 0; jb < m; jb += WAVE) {
        const int j = jb + lane;
        const int i = j < m ? s.p[j] : 0;
        int32_t w = 0, cat = 0;
        if (i > 0) {
            const int64_t r = s.ridx[i - 1], c = s.cidx[j];
            const int64_t d = rows_are_dt ? r : c, g = rows_are_dt ? c : r;
            w = S.at(d, g);
            if (w > 0) {
                if (!AT || a.gt_ident)
                    reinterpret_cast<int2 *>(a.gt_ident)[g0 + g] = make_int2((int32_t)(d0 + d), w);
                a.dt_ident[(d0 + d) * 2] = (int32_t)(g0 + g);
                cat = a.gt_cat[g0 + g];
            }
        }
        const int32_t pair_cols[2] = {w, 1};                      // idtp, pairs
        wave_add(a.cat_counts + 4, TI_NCAT, w > 0 && cat >= 0 && cat < a.n_cat, cat, pair_cols);
    }
}

// The tables of the calls, in buffer order: a function of (n_dt, n_gt, n_gt_frames)
// and the layers (1 but for the layered assignment: a slice of the search store
// and of the index lists per layer)
static void ident_layout(Carve &c, int64_t n_dt, int64_t n_gt, int64_t n_gt_frames,
                         FrameTables &ft, IdentArgs &a, int32_t n_thr = 1)
{
    frames_layout(c, n_dt, n_gt, n_gt_frames, ft);
    a.store.layout(c, (size_t)n_thr * (size_t)(n_dt + n_gt));
    a.sidx = c.take<int32_t>((size_t)n_thr * (size_t)(n_dt + n_gt));
}

static inline bool ident_layers_ok(int32_t n_thr)
{
    return n_thr >= 1 && n_thr <= TAOAMD_TRACK_SCORE_THRS;
}

extern "C" size_t taoamd_track_identity_workspace(int64_t n_dt, int64_t n_gt, int64_t n_gt_frames)
{
    if (!track_sizes_ok(n_dt, n_gt, n_gt_frames, TT_STORE)) return 0;
    IdentArgs a;
    return measure([&](Carve &c) { ident_layout(c, n_dt, n_gt, n_gt_frames, a.ft, a); });
}

extern "C" size_t taoamd_track_identity_layers_workspace(int64_t n_dt, int64_t n_gt,
                                                         int64_t n_gt_frames, int32_t n_thr)
{
    if (!track_sizes_ok(n_dt, n_gt, n_gt_frames, TT_STORE) || !ident_layers_ok(n_thr)) return 0;
    IdentArgs a;
    return measure([&](Carve &c) { ident_layout(c, n_dt, n_gt, n_gt_frames, a.ft, a, n_thr); });
}

// What the entry points share: the common refusals, the carved workspace and
// the common fields of the kernels' block
static int ident_args(IdentArgs &a, TrackTables &t, unsigned need, void *workspace,
                      size_t workspace_bytes, int32_t n_thr = 1)
{
    a = {};
    const int st = track_args(
        t, need | TT_IOU | TT_DT_OFF | TT_STORE, workspace, workspace_bytes,
        [&](Carve &c) { ident_layout(c, t.n_dt, t.n_gt, t.n_gt_frames, t.ft, a, n_thr); });
    track_fill(a, t);
    return st;
}

extern "C" int taoamd_track_identity_share(
    int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou, int64_t n_dt_frames,
    int64_t n_gt_frames, double frame_thr, const int32_t *cell_dt_off, const int32_t *cell_gt_off,
    const int64_t *cell_iou_off, const int32_t *dt_frame_off, const int32_t *dt_frame_pos,
    const double *dt_frame_box, const int32_t *gt_frame_off, const int32_t *gt_frame_pos,
    const double *gt_frame_box, int32_t *share, void *workspace, size_t workspace_bytes,
    void *stream)
{
    TrackTables t = {n_dt, n_gt, n_cells, n_iou, n_dt_frames, n_gt_frames, cell_dt_off,
                     cell_gt_off, cell_iou_off, nullptr, nullptr, dt_frame_off, dt_frame_pos,
                     track_boxes(dt_frame_box), gt_frame_off, gt_frame_pos,
                     track_boxes(gt_frame_box)};
    IdentArgs a;
    // (a NaN compares false both times)
    if (!(frame_thr > 0) || !(frame_thr <= 1)) return TAOAMD_ERR_ARG;
    if (n_iou > 0 && !share) return TAOAMD_ERR_ARG;
    const int st = ident_args(a, t, TT_BOXES, workspace, workspace_bytes);
    if (st != TAOAMD_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    a.thr = frame_thr;
    a.share = share;
    if (n_iou > 0) TAO_HIP(hipMemsetAsync(share, 0, (size_t)n_iou * sizeof(int32_t), s));
    if (n_gt == 0) return TAOAMD_OK;
    // (empty sides: the rule of track_frames.hpp.  A ground-truth row no cell lists has
    // no candidates, a frame no track lists counts nowhere: share stays 0)
    const int si = track_index(t, s);
    if (si != TAOAMD_OK) return si;
    if (n_gt_frames > 0)
        TAO_TIMED("ident_share_kernel", s,
                  ident_share_kernel<<<(unsigned)((n_gt_frames + TI_TILE - 1) / TI_TILE), TI_TILE,
                                       0, s>>>(a));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

// Both assignments: n_thr layers read dt_pass (AT), or the one layer without a
// mask that taoamd_track_identity_assign is (gt_ident is then required)
template <bool AT>
static int ident_assign(TrackTables &t, int32_t n_cat, int32_t n_thr, const int32_t *dt_cat,
                        const uint8_t *dt_flags, const uint8_t *dt_pass, const int32_t *share,
                        int64_t *cat_counts, int32_t *gt_ident, int32_t *dt_ident, int32_t *status,
                        void *workspace, size_t workspace_bytes, void *stream)
{
    IdentArgs a;
    if (n_cat <= 0 || !cat_counts || !status) return TAOAMD_ERR_ARG;
    if (AT && !ident_layers_ok(n_thr)) return TAOAMD_ERR_ARG;
    if (t.n_dt > 0 && (!dt_cat || !dt_flags || !dt_ident || (AT && !dt_pass)))
        return TAOAMD_ERR_ARG;
    if (!AT && t.n_gt > 0 && !gt_ident) return TAOAMD_ERR_ARG;
    if (t.n_iou > 0 && !share) return TAOAMD_ERR_ARG;
    const int st = ident_args(a, t, TT_GT_CAT | TT_GT_FLAGS, workspace, workspace_bytes, n_thr);
    if (st != TAOAMD_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    a.n_cat = n_cat;
    a.dt_cat = dt_cat; a.dt_flags = dt_flags;
    a.share = const_cast<int32_t *>(share);
    a.cat_counts = (unsigned long long *)cat_counts;
    a.gt_ident = gt_ident; a.dt_ident = dt_ident; a.status = status;
    a.n_thr = n_thr; a.dt_pass = dt_pass;
    TAO_HIP(hipMemsetAsync(cat_counts, 0, (size_t)n_thr * n_cat * TI_NCAT * sizeof(int64_t), s));
    TAO_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if constexpr (AT) {
        const int64_t n_gi = gt_ident ? n_thr * t.n_gt : 0, n_di = n_thr * t.n_dt;
        const int64_t rows = n_di > n_gi ? n_di : n_gi;
        if (rows > 0)
            TAO_TIMED("ident_init_layers_kernel", s,
                      ident_init_layers_kernel<<<(unsigned)((rows + 255) / 256), 256, 0, s>>>(
                          reinterpret_cast<int2 *>(gt_ident), n_gi,
                          reinterpret_cast<int2 *>(dt_ident), n_di));
        if (t.n_cells > 0)
            TAO_TIMED("ident_assign_at_kernel", s,
                      ident_assign_kernel<true><<<dim3((unsigned)t.n_cells, (unsigned)n_thr), WAVE,
                                                  0, s>>>(a));
    } else {
        const int64_t rows = t.n_dt > t.n_gt ? t.n_dt : t.n_gt;
        if (rows > 0)
            TAO_TIMED("ident_init_kernel", s,
                      ident_init_kernel<<<(unsigned)((rows + 255) / 256), 256, 0, s>>>(a));
        if (t.n_cells > 0)
            TAO_TIMED("ident_assign_kernel", s,
                      ident_assign_kernel<false><<<(unsigned)t.n_cells, WAVE, 0, s>>>(a));
    }
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

extern "C" int taoamd_track_identity_assign(
    int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou, int64_t n_dt_frames,
    int64_t n_gt_frames, int32_t n_cat, const int32_t *cell_dt_off, const int32_t *cell_gt_off,
    const int64_t *cell_iou_off, const int32_t *gt_cat, const uint8_t *gt_flags,
    const int32_t *dt_cat, const uint8_t *dt_flags, const int32_t *dt_frame_off,
    const int32_t *gt_frame_off, const int32_t *share, int64_t *cat_counts, int32_t *gt_ident,
    int32_t *dt_ident, int32_t *status, void *workspace, size_t workspace_bytes, void *stream)
{
    TrackTables t = {n_dt, n_gt, n_cells, n_iou, n_dt_frames, n_gt_frames, cell_dt_off,
                     cell_gt_off, cell_iou_off, gt_cat, gt_flags, dt_frame_off, nullptr, nullptr,
                     gt_frame_off, nullptr, nullptr};
    return ident_assign<false>(t, n_cat, 1, dt_cat, dt_flags, nullptr, share, cat_counts, gt_ident,
                               dt_ident, status, workspace, workspace_bytes, stream);
}

extern "C" int taoamd_track_identity_assign_at(
    int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou, int64_t n_dt_frames,
    int64_t n_gt_frames, int32_t n_cat, int32_t n_thr, const int32_t *cell_dt_off,
    const int32_t *cell_gt_off, const int64_t *cell_iou_off, const int32_t *gt_cat,
    const uint8_t *gt_flags, const int32_t *dt_cat, const uint8_t *dt_flags,
    const uint8_t *dt_pass, const int32_t *dt_frame_off, const int32_t *gt_frame_off,
    const int32_t *share, int64_t *cat_counts, int32_t *gt_ident, int32_t *dt_ident,
    int32_t *status, void *workspace, size_t workspace_bytes, void *stream)
{
    TrackTables t = {n_dt, n_gt, n_cells, n_iou, n_dt_frames, n_gt_frames, cell_dt_off,
                     cell_gt_off, cell_iou_off, gt_cat, gt_flags, dt_frame_off, nullptr, nullptr,
                     gt_frame_off, nullptr, nullptr};
    return ident_assign<true>(t, n_cat, n_thr, dt_cat, dt_flags, dt_pass, share, cat_counts,
                              gt_ident, dt_ident, status, workspace, workspace_bytes, stream);
}

extern "C" int taoamd_track_score_pass(int64_t n_dt, int32_t n_cat, int32_t n_thr,
                                       const double *dt_score, const int32_t *dt_cat,
                                       const double *thr, const uint8_t *base, uint8_t *pass,
                                       void *stream)
{
    if (n_dt < 0 || n_dt > 0x7fffffff || n_cat <= 0 || !ident_layers_ok(n_thr) || !thr)
        return TAOAMD_ERR_ARG;
    if (n_dt > 0 && (!dt_score || !dt_cat || !pass)) return TAOAMD_ERR_ARG;
    if (n_dt == 0) return TAOAMD_OK;
    hipStream_t s = (hipStream_t)stream;
    TAO_TIMED("score_pass_kernel", s,
              score_pass_kernel<<<dim3((unsigned)((n_dt + 255) / 256), (unsigned)n_thr), 256, 0,
                                  s>>>(n_dt, n_cat, dt_score, dt_cat, thr, base, pass));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

// Track-level HOTA (gfx950): HOTA / DetA / AssA (Luiten et al., IJCV 2021) from a
// one-to-one assignment per FRAME, weighted by how well each pair of tracks
// aligns over the whole video.  The reference has no such table; the definition
// is this library's, after TrackEval's HOTA class, stated in
// include/tao_amodal_hip.h ("track-level HOTA") and DESIGN.md section 8.
//
// Rows, cells, frame lists and the entry points' common part are those of every
// track analysis (track_tables.hpp, track_frames.hpp).
// Every fractional sum is carried in fixed point (ONE = 2^30): every device
// output is an integer (match_iou: one box_iou value) and the same from run to
// run; no float is ever added atomically.  Three calls:
//
// taoamd_track_hota_align: pot[pair] = the sum over the frames both tracks have of
// q(c / (rowsum + colsum - c)), the per-frame "similarity IoU" of TrackEval.
//   track_index, frames_build_gt_meta    the frame index and its twin for the
//                        ground-truth tracks (track_frames.hpp)
//   hota_align_kernel    lane = ground-truth frame of an eligible track.  Pass 1
//                        walks the cell's kept detection tracks for rowsum; pass 2
//                        walks them again and, for a d that overlaps, the cell's
//                        eligible ground truths at the position for colsum (a cell
//                        of one ground truth: colsum = c).  The float adds run in
//                        ascending row from 0.0, so whichever lane forms a sum
//                        gets the same bits.  Pass 2's loop is uniform over the
//                        wavefront: the lanes of one pair are found by ballot,
//                        their q(a) summed across the group, one 64-bit integer
//                        atomic per (pair, wavefront step).
//
// taoamd_track_hota_match: the assignment of every frame group (cell, position).
//   hota_frame_kernel    lane = ground-truth frame.  The only eligible ground truth
//                        at its position: the greatest w > 0 among the kept
//                        detection tracks, lowest row among equal -- the one-row
//                        assignment, the great majority of frames.  The group's
//                        LEADER (no lower eligible row has a frame there) of a
//                        larger group marks its frame pending (-2 in match).
//   hota_group           one wavefront, one pending group: compacts Gp and Dp with
//                        their frame indices, drops the rows and columns without
//                        a positive w, takes the smaller side as rows (the ground
//                        truths when equal: assign_sides) and runs assign_solve
//                        (assign_solve.hpp) with w computed on the fly.  An
//                        exhausted bound stores 1 to *status and leaves the
//                        group's frames at -1.  w <= 2^30 and n < 2^31: the 64-bit
//                        potentials cannot overflow.
//                        A match adds 1 and q(c) to BIN b - 1 of the pair's words
//                        (b = the alphas <= c): one int32 and one int64 atomic,
//                        not n_alpha of each.
//   hota_group_kernel    workgroup = ONE wavefront = a tile of 64 ground-truth
//                        frames: it ballots for the tile's pending leaders whose
//                        cell has both sides <= TH_LDS and takes them in order,
//                        the state in LDS.  Groups are independent (a frame is in
//                        one group, the bins are integer adds), so any order
//                        gives the same tables.
//   hota_cell_kernel     workgroup = ONE wavefront = a cell with a side beyond
//                        TH_LDS: the same walk over the cell's own frames, the
//                        state in the cell's slice of the search store and of
//                        three lists beside it (a frame's Gp + Dp never exceeds
//                        its cell's G + D), which one wavefront must own.
//                        (A first version walked EVERY cell's groups with one
//                        wavefront a cell: 8.1 ms at benchmark size, where 40 % of
//                        the frame groups hold two ground truths; a wavefront a
//                        tile 6.5 ms with 15 360 B of LDS and 4.3 ms with 7 680 B:
//                        a group is a chain of dependent loads, and wavefronts in
//                        flight are what hides it.  DESIGN.md section 8.)
//   hota_suffix_kernel   lane = pair: the bins into mc[a] = the sum over b >= a,
//                        lc likewise, in place.
//
// taoamd_track_hota_reduce: tp, loc and the three association sums per (category,
// alpha).
//   hota_reduce_kernel   lane = ground-truth row (consecutive lanes read
//                        consecutive words of a detection row); per alpha it walks
//                        the cell's detection rows with private sums, then one
//                        wave_add per table (common.hpp).
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950); no kernel uses
// scratch:
//   hota_align_kernel  60 VGPRs, no LDS;  hota_frame_kernel 52 VGPRs, no LDS;
//   hota_group_kernel  85 VGPRs, 7 680 B of LDS (a workgroup is one wavefront: 20
//   tiles a CU by registers, 21 by LDS);  hota_cell_kernel 77 VGPRs, no LDS;
//   hota_suffix_kernel 10 VGPRs;  hota_reduce_kernel 64 VGPRs.
#include "assign_solve.hpp"
#include "track_tables.hpp"

using namespace taoamd;

#define TH_TILE 64          // ground-truth frames per workgroup of the frame kernels
#define TH_LDS 128          // rows and columns of a cell whose group state is in LDS
#define TH_ONE ((double)TAOAMD_HOTA_ONE)
#define TH_PENDING (-2)     // match[k] of a larger group's leader between the two kernels
#define TH_NALPHA TAOAMD_TRACK_HOTA_ALPHAS

struct AlphaTab {
    double v[TH_NALPHA];
};

struct HotaArgs {
    TrackTables t;
    int32_t n_cat, n_alpha;
    const uint8_t *dt_keep;                      // NULL: all kept
    long long *pot;                              // [n_iou]
    int32_t *mc;                                 // [n_alpha][n_iou]
    long long *lc;                               // [n_alpha][n_iou]
    int32_t *match;                              // [n_gt_frames]
    double *match_iou;                           // [n_gt_frames] or NULL
    int32_t *status;
    unsigned long long *tp, *loc, *ass;          // [n_cat][n_alpha], .., [n_cat][n_alpha][3]
    int4 *gt_meta;                               // [n_gt]
    SearchStore store;                           // the cells that do not fit in LDS
    int32_t *sent, *sfrm, *sidx;                 // [n_dt + n_gt] each: the groups' lists
};

__device__ __forceinline__ bool hota_kept(const HotaArgs &a, int64_t d)
{
    return a.dt_keep ? a.dt_keep[d] != 0 : true;
}

// c(s): 0 unless s > 0 (a NaN is 0), else min(s, 1)
__device__ __forceinline__ double hota_c(double s) { return s > 0 ? (s < 1.0 ? s : 1.0) : 0.0; }

// q(x) = (int64) rint(x * ONE)
__device__ __forceinline__ long long hota_q(double x) { return __double2ll_rn(x * TH_ONE); }

__device__ __forceinline__ double hota_iou(const HotaArgs &a, int64_t df, int64_t gf)
{
    const double4 D = a.t.dfbox[df], B = a.t.gfbox[gf];
    return box_iou(D.x, D.y, D.z, D.w, B.x, B.y, B.z, B.w);
}

// w(g, d) = q(gas * c(s)) of the in-cell pair (d, g) with the frames df, gf; s and
// c(s) come back where w > 0
__device__ __forceinline__ long long hota_w(const HotaArgs &a, const TrackCell &c, int64_t d,
                                            int64_t g, int64_t df, int64_t gf, double &s,
                                            double &cs)
{
    const int64_t i = c.off + d * c.G + g;
    const long long pv = i >= 0 && i < a.t.n_iou ? a.pot[i] : 0;
    if (pv <= 0) return 0;
    s = hota_iou(a, df, gf);
    cs = hota_c(s);
    if (!(cs > 0)) return 0;
    const double P = (double)pv / TH_ONE;
    const double den = (double)(track_span(a.t.gfoff, c.g0 + g, a.t.n_gt_frames).len() +
                                track_span(a.t.dfoff, c.d0 + d, a.t.n_dt_frames).len()) - P;
    double gas = P / den;
    gas = gas > 0 ? (gas < 1.0 ? gas : 1.0) : 0.0;
    return hota_q(gas * cs);
}

// A match of the pair at word i with c(s) = cs: 1 and q(cs) into bin b - 1
__device__ __forceinline__ void hota_bin(const HotaArgs &a, const AlphaTab &al, int64_t i,
                                         double cs)
{
    int b = 0;
    for (int t = 0; t < a.n_alpha; t++) b += al.v[t] <= cs;
    if (b == 0 || i < 0 || i >= a.t.n_iou) return;
    const int64_t at = (int64_t)(b - 1) * a.t.n_iou + i;
    atomicAdd(a.mc + at, 1);
    atomicAdd(reinterpret_cast<unsigned long long *>(a.lc) + at, (unsigned long long)hota_q(cs));
}

// ---------------------------------------------------------------------------
// align
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TH_TILE) void hota_align_kernel(HotaArgs a)
{
    // (no lane leaves early: pass 2's loop and its ballots are the wavefront's)
    const TrackTables &t = a.t;
    const int64_t k = (int64_t)blockIdx.x * TH_TILE + threadIdx.x;
    const int32_t g = k < t.n_gt_frames ? t.ft.frame_gt[k] : -1;
    const int32_t cell = g >= 0 ? t.ft.gt_cell[g] : -1;
    const bool live = cell >= 0 && track_eligible(t, g);
    TrackCell c = {0, 0, 0, 0, 0};
    int64_t p = 0;
    if (live) {
        c = track_cell(t, cell);
        p = t.gfpos[k];
    }
    const int64_t gl = g - c.g0;
    // 1: rowsum over the kept detection tracks with a frame at p, ascending row
    double rowsum = 0.0;
    for (int64_t d = 0; d < c.D; d++) {
        int64_t lo;
        if (hota_kept(a, c.d0 + d) && frames_find(t.dfpos, t.ft.dt_meta[c.d0 + d], p, lo))
            rowsum += hota_c(hota_iou(a, lo, k));
    }
    // 2: colsum of every d that overlaps, a, and one add per pair of the wavefront
    const int64_t steps = wave_max(rowsum > 0 ? c.D : (int64_t)0);
    for (int64_t d = 0; d < steps; d++) {
        int64_t at = -1, lo;
        long long qa = 0;
        if (rowsum > 0 && d < c.D && hota_kept(a, c.d0 + d) &&
            frames_find(t.dfpos, t.ft.dt_meta[c.d0 + d], p, lo)) {
            const double cs = hota_c(hota_iou(a, lo, k));
            if (cs > 0) {
                double colsum = 0.0;
                if (c.G == 1) {
                    colsum = cs;
                } else {
                    for (int64_t o = 0; o < c.G; o++) {
                        int64_t go;
                        if (track_eligible(t, c.g0 + o) &&
                            frames_find(t.gfpos, a.gt_meta[c.g0 + o], p, go))
                            colsum += hota_c(hota_iou(a, lo, go));
                    }
                }
                const double den = (rowsum + colsum) - cs;
                const double al = den > 0x1p-52 ? (cs / den < 1.0 ? cs / den : 1.0) : 0.0;
                qa = hota_q(al);
                const int64_t i = c.off + d * c.G + gl;
                if (qa > 0 && i >= 0 && i < t.n_iou) at = i;
            }
        }
        uint64_t left = __ballot(at >= 0);
        while (left) {
            const int lead = __builtin_ctzll(left);
            const int64_t to = __shfl(at, lead);
            const bool mine = at == to;
            const uint64_t same = __ballot(mine);
            const long long sum = wave_sum(mine ? qa : 0ll);
            if (lane_id() == lead)
                atomicAdd(reinterpret_cast<unsigned long long *>(a.pot) + to,
                          (unsigned long long)sum);
            left &= ~same;
        }
    }
}

// ---------------------------------------------------------------------------
// match
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TH_TILE) void hota_frame_kernel(HotaArgs a, AlphaTab al)
{
    const TrackTables &t = a.t;
    const int64_t k = (int64_t)blockIdx.x * TH_TILE + threadIdx.x;
    if (k >= t.n_gt_frames) return;
    int32_t out = -1;
    double out_s = 0.0;
    const int32_t g = t.ft.frame_gt[k];
    const int32_t cell = g >= 0 ? t.ft.gt_cell[g] : -1;
    if (cell >= 0 && track_eligible(t, g)) {
        const TrackCell c = track_cell(t, cell);
        const int64_t p = t.gfpos[k], gl = g - c.g0;
        // the other eligible ground truths with a frame at p: a lower one makes this
        // frame a follower of its group, a higher one its leader
        bool lower = false, other = false;
        for (int64_t o = 0; o < c.G && !lower && !other; o++) {
            int64_t go;
            if (o != gl && track_eligible(t, c.g0 + o) &&
                frames_find(t.gfpos, a.gt_meta[c.g0 + o], p, go)) {
                lower = o < gl;
                other = o > gl;
            }
        }
        if (other) {
            out = TH_PENDING;
        } else if (!lower) {
            long long best = 0;
            double best_c = 0.0;
            for (int64_t d = 0; d < c.D; d++) {
                int64_t lo;
                if (!hota_kept(a, c.d0 + d) ||
                    !frames_find(t.dfpos, t.ft.dt_meta[c.d0 + d], p, lo))
                    continue;
                double s, cs;
                const long long w = hota_w(a, c, d, gl, lo, k, s, cs);
                if (w > best) {              // (ascending d: the lowest among equal weights)
                    best = w;
                    best_c = cs;
                    out = (int32_t)d;
                    out_s = s;
                }
            }
            if (out >= 0) hota_bin(a, al, c.off + (int64_t)out * c.G + gl, best_c);
        }
    }
    a.match[k] = out;
    if (a.match_iou) a.match_iou[k] = out_s;
}

// The weight of the solver: row and column are places in the group's lists
struct HotaWeight {
    const HotaArgs &a;
    const TrackCell &c;
    const int32_t *ge, *gf, *de, *df;            // in-cell row and frame of list entry i
    bool rows_are_gt;
    __device__ __forceinline__ long long at(int64_t gi, int64_t di, double &s, double &cs) const
    {
        return hota_w(a, c, de[di], ge[gi], df[di], gf[gi], s, cs);
    }
    __device__ __forceinline__ long long operator()(int64_t r, int64_t cc) const
    {
        double s, cs;
        return rows_are_gt ? at(r, cc, s, cs) : at(cc, r, s, cs);
    }
};

// Where one group's lists and search state live: LDS or the cell's slice of the
// workspace
struct HotaState {
    int32_t *de, *df, *ge, *gf;      // Dp and Gp: in-cell row and frame of entry i
    int32_t *didx, *gidx;            // the entries with a positive w
    Search s;
};

__device__ __forceinline__ bool hota_fits_lds(const TrackCell &c)
{
    return c.G <= TH_LDS && c.D <= TH_LDS;
}

// The group of the pending leader frame kl of cell c, by one wavefront (uniform)
__device__ __forceinline__ void hota_group(const HotaArgs &a, const AlphaTab &al,
                                           const TrackCell &c, HotaState st, int64_t kl)
{
    const TrackTables &t = a.t;
    const int lane = lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    int32_t *de = st.de, *df = st.df, *ge = st.ge, *gf = st.gf;
    int32_t *didx = st.didx, *gidx = st.gidx;
    Search s = st.s;
    const int64_t p = t.gfpos[kl];
    const int64_t gl = (int64_t)t.ft.frame_gt[kl] - c.g0;
    // Gp from the leader on (no lower eligible row has a frame at p), Dp
    int ng = 0, nd = 0;
    for (int64_t gb = gl; gb < c.G; gb += WAVE) {
        const int64_t o = gb + lane;
        int64_t lo = 0;
        const bool has = o < c.G && track_eligible(t, c.g0 + o) &&
                         frames_find(t.gfpos, a.gt_meta[c.g0 + o], p, lo);
        const uint64_t m = __ballot(has);
        if (has) {
            ge[ng + __popcll(m & below)] = (int32_t)o;
            gf[ng + __popcll(m & below)] = (int32_t)lo;
        }
        ng += __popcll(m);
    }
    for (int64_t db = 0; db < c.D; db += WAVE) {
        const int64_t d = db + lane;
        int64_t lo = 0;
        const bool has = d < c.D && hota_kept(a, c.d0 + d) &&
                         frames_find(t.dfpos, t.ft.dt_meta[c.d0 + d], p, lo);
        const uint64_t m = __ballot(has);
        if (has) {
            de[nd + __popcll(m & below)] = (int32_t)d;
            df[nd + __popcll(m & below)] = (int32_t)lo;
        }
        nd += __popcll(m);
    }
    __syncthreads();
    // every frame of the group unmatched, the leader's pending mark gone
    for (int i = lane; i < ng; i += WAVE) {
        a.match[gf[i]] = -1;
        if (a.match_iou) a.match_iou[gf[i]] = 0.0;
    }
    HotaWeight W = {a, c, ge, gf, de, df, true};
    // the columns, then the rows, with a positive w
    int md = 0, mg = 0;
    for (int jb = 0; jb < nd; jb += WAVE) {
        const int j = jb + lane;
        bool act = false;
        double s_, cs_;
        if (j < nd)
            for (int i = 0; i < ng && !act; i++) act = W.at(i, j, s_, cs_) > 0;
        const uint64_t m = __ballot(act);
        if (act) didx[md + __popcll(m & below)] = j;
        md += __popcll(m);
    }
    __syncthreads();
    for (int ib = 0; ib < ng; ib += WAVE) {
        const int i = ib + lane;
        bool act = false;
        double s_, cs_;
        if (i < ng)
            for (int x = 0; x < md && !act; x++) act = W.at(i, didx[x], s_, cs_) > 0;
        const uint64_t m = __ballot(act);
        if (act) gidx[mg + __popcll(m & below)] = i;
        mg += __popcll(m);
    }
    __syncthreads();
    if (md == 0 || mg == 0) return;                  // (uniform)
    // the smaller side as rows, the ground truths when equal
    const Sides sd = assign_sides(gidx, mg, didx, md);
    W.rows_are_gt = sd.first;
    s.ridx = sd.rows;
    s.cidx = sd.cols;
    if (!assign_solve(W, s, sd.n, sd.m)) {
        if (lane == 0) *a.status = 1;
        __syncthreads();
        return;
    }
    // the pairs with a positive w
    assign_pairs(s, sd, [&](bool has, int64_t gi, int64_t di) {
        double sv, cs;
        if (has && W.at(gi, di, sv, cs) > 0) {
            a.match[gf[gi]] = de[di];
            if (a.match_iou) a.match_iou[gf[gi]] = sv;
            hota_bin(a, al, c.off + (int64_t)de[di] * c.G + ge[gi], cs);
        }
    });
    __syncthreads();
}

// The groups of the cells whose sides both fit in LDS: a wavefront per tile of
// ground-truth frames takes the tile's pending leaders in order
__global__ __launch_bounds__(WAVE) void hota_group_kernel(HotaArgs a, AlphaTab al)
{
    __shared__ SearchLds<TH_LDS> lds;
    __shared__ int32_t l_ge[TH_LDS], l_gf[TH_LDS], l_de[TH_LDS], l_df[TH_LDS];
    const TrackTables &t = a.t;
    const int64_t kb = (int64_t)blockIdx.x * TH_TILE;
    const int64_t k = kb + lane_id();
    int32_t cell = -1;
    if (k < t.n_gt_frames && a.match[k] == TH_PENDING) {
        const int32_t g = t.ft.frame_gt[k];
        cell = g >= 0 ? t.ft.gt_cell[g] : -1;
        if (cell >= 0 && !hota_fits_lds(track_cell(t, cell))) cell = -1;
    }
    uint64_t todo = __ballot(cell >= 0);
    const HotaState st = {l_de, l_df, l_ge, l_gf, lds.idx1, lds.idx0, lds.search()};
    while (todo) {
        const int lead = __builtin_ctzll(todo);
        todo &= todo - 1;
        const TrackCell c = track_cell(t, __shfl(cell, lead));
        hota_group(a, al, c, st, kb + lead);
    }
}

// The groups of a cell with a side beyond LDS: workgroup = ONE wavefront = cell,
// which owns its slice of the workspace arrays and walks its frames in order
__global__ __launch_bounds__(WAVE) void hota_cell_kernel(HotaArgs a, AlphaTab al)
{
    const TrackTables &t = a.t;
    const int lane = lane_id();
    const TrackCell c = track_cell(t, blockIdx.x);
    if (c.G < 2 || hota_fits_lds(c)) return;         // (uniform)
    const int64_t base = c.d0 + c.g0;                // the cell's slice of the state arrays
    const HotaState st = {a.sent + base, a.sfrm + base, a.sent + base + c.D,
                          a.sfrm + base + c.D, a.sidx + base, a.sidx + base + c.D,
                          a.store.at(base)};
    // the cell's ground-truth frames lie in one run of the CSR table
    const int64_t fs = clamp64(t.gfoff[c.g0], 0, t.n_gt_frames);
    const int64_t fe = clamp64(t.gfoff[c.g0 + c.G], fs, t.n_gt_frames);
    for (int64_t kb = fs; kb < fe; kb += WAVE) {
        bool pend = false;
        if (kb + lane < fe && a.match[kb + lane] == TH_PENDING) {
            const int32_t g = t.ft.frame_gt[kb + lane];
            pend = g >= c.g0 && g < c.g0 + c.G;
        }
        uint64_t todo = __ballot(pend);
        while (todo) {
            const int64_t kl = kb + __builtin_ctzll(todo);
            todo &= todo - 1;
            hota_group(a, al, c, st, kl);
        }
    }
}

__global__ __launch_bounds__(256) void hota_suffix_kernel(HotaArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.t.n_iou) return;
    int32_t m = 0;
    long long l = 0;
    for (int t = a.n_alpha - 1; t >= 0; t--) {
        const int64_t at = (int64_t)t * a.t.n_iou + i;
        m += a.mc[at];
        l += a.lc[at];
        a.mc[at] = m;
        a.lc[at] = l;
    }
}

// ---------------------------------------------------------------------------
// reduce
// ---------------------------------------------------------------------------
// q'(m * min(m / den, 1)); 0 where den is not positive
__device__ __forceinline__ long long hota_term(double m, double den)
{
    if (!(den > 0)) return 0;
    const double r = m / den;
    return hota_q(m * (r < 1.0 ? r : 1.0));
}

__global__ __launch_bounds__(256) void hota_reduce_kernel(HotaArgs a)
{
    // (no lane leaves early: wave_add is the wavefront's)
    const TrackTables &t = a.t;
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t cell = g < t.n_gt ? t.ft.gt_cell[g] : -1;
    bool live = cell >= 0 && track_eligible(t, g);
    int32_t cat = 0;
    TrackCell c = {0, 0, 0, 0, 0};
    double L = 0;
    if (live) {
        cat = t.gt_cat[g];
        live = cat >= 0 && cat < a.n_cat;
        c = track_cell(t, cell);
        L = (double)track_span(t.gfoff, g, t.n_gt_frames).len();
    }
    const int64_t D = live ? c.D : 0;
    for (int x = 0; x < a.n_alpha; x++) {
        long long tp[1] = {0}, loc[1] = {0}, ass[3] = {0, 0, 0};
        for (int64_t d = 0; d < D; d++) {
            const int64_t i = c.off + d * c.G + (g - c.g0);
            if (i < 0 || i >= t.n_iou) continue;
            const int32_t mi = a.mc[(int64_t)x * t.n_iou + i];
            if (mi <= 0) continue;
            const double m = (double)mi;
            const double F = (double)track_span(t.dfoff, c.d0 + d, t.n_dt_frames).len();
            tp[0] += mi;
            loc[0] += a.lc[(int64_t)x * t.n_iou + i];
            ass[0] += hota_term(m, (L + F) - m);
            ass[1] += hota_term(m, L);
            ass[2] += hota_term(m, F);
        }
        wave_add(a.tp + x, a.n_alpha, live, cat, tp);
        wave_add(a.loc + x, a.n_alpha, live, cat, loc);
        wave_add(a.ass + (int64_t)x * 3, (int64_t)a.n_alpha * 3, live, cat, ass);
    }
}

// ---------------------------------------------------------------------------
// the entry points
// ---------------------------------------------------------------------------
// The tables of all three calls, in buffer order: a function of (n_dt, n_gt,
// n_gt_frames)
static void hota_layout(Carve &c, int64_t n_dt, int64_t n_gt, int64_t n_gt_frames, HotaArgs &a)
{
    const size_t n = (size_t)(n_dt + n_gt);
    frames_layout(c, n_dt, n_gt, n_gt_frames, a.t.ft);
    a.gt_meta = c.take<int4>((size_t)n_gt);
    a.store.layout(c, n);
    a.sent = c.take<int32_t>(n);
    a.sfrm = c.take<int32_t>(n);
    a.sidx = c.take<int32_t>(n);
}

extern "C" size_t taoamd_track_hota_workspace(int64_t n_dt, int64_t n_gt, int64_t n_gt_frames)
{
    if (!track_sizes_ok(n_dt, n_gt, n_gt_frames, TT_STORE)) return 0;
    HotaArgs a;
    return measure([&](Carve &c) { hota_layout(c, n_dt, n_gt, n_gt_frames, a); });
}

// What the three entry points share: the common refusals and the carved workspace
static int hota_args(HotaArgs &a, unsigned need, void *workspace, size_t workspace_bytes)
{
    const TrackTables &t = a.t;
    return track_args(t, need | TT_IOU | TT_GT_FLAGS | TT_DT_OFF | TT_STORE, workspace,
                      workspace_bytes,
                      [&](Carve &c) { hota_layout(c, t.n_dt, t.n_gt, t.n_gt_frames, a); });
}

// The frame index and gt_meta on stream s
static int hota_index(const HotaArgs &a, hipStream_t s)
{
    const int st = track_index(a.t, s);
    if (st != TAOAMD_OK) return st;
    return frames_build_gt_meta(a.t.n_gt, a.t.n_gt_frames, a.t.gfoff, a.t.gfpos, a.gt_meta, s);
}

extern "C" int taoamd_track_hota_align(
    int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou, int64_t n_dt_frames,
    int64_t n_gt_frames, const int32_t *cell_dt_off, const int32_t *cell_gt_off,
    const int64_t *cell_iou_off, const uint8_t *gt_flags, const uint8_t *dt_keep,
    const int32_t *dt_frame_off, const int32_t *dt_frame_pos, const double *dt_frame_box,
    const int32_t *gt_frame_off, const int32_t *gt_frame_pos, const double *gt_frame_box,
    int64_t *pot, void *workspace, size_t workspace_bytes, void *stream)
{
    HotaArgs a = {};
    a.t = {n_dt, n_gt, n_cells, n_iou, n_dt_frames, n_gt_frames, cell_dt_off, cell_gt_off,
           cell_iou_off, nullptr, gt_flags, dt_frame_off, dt_frame_pos, track_boxes(dt_frame_box),
           gt_frame_off, gt_frame_pos, track_boxes(gt_frame_box)};
    if (n_iou > 0 && !pot) return TAOAMD_ERR_ARG;
    const int st = hota_args(a, TT_BOXES, workspace, workspace_bytes);
    if (st != TAOAMD_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    a.dt_keep = dt_keep;
    a.pot = reinterpret_cast<long long *>(pot);
    if (n_iou > 0) TAO_HIP(hipMemsetAsync(pot, 0, (size_t)n_iou * sizeof(int64_t), s));
    if (n_gt == 0) return TAOAMD_OK;
    const int si = hota_index(a, s);
    if (si != TAOAMD_OK) return si;
    if (n_gt_frames > 0)
        TAO_TIMED("hota_align_kernel", s,
                  hota_align_kernel<<<(unsigned)((n_gt_frames + TH_TILE - 1) / TH_TILE), TH_TILE,
                                      0, s>>>(a));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

extern "C" int taoamd_track_hota_match(
    int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou, int64_t n_dt_frames,
    int64_t n_gt_frames, int32_t n_alpha, const double *alphas, const int32_t *cell_dt_off,
    const int32_t *cell_gt_off, const int64_t *cell_iou_off, const uint8_t *gt_flags,
    const uint8_t *dt_keep, const int32_t *dt_frame_off, const int32_t *dt_frame_pos,
    const double *dt_frame_box, const int32_t *gt_frame_off, const int32_t *gt_frame_pos,
    const double *gt_frame_box, const int64_t *pot, int32_t *mc, int64_t *lc, int32_t *match,
    double *match_iou, int32_t *status, void *workspace, size_t workspace_bytes, void *stream)
{
    HotaArgs a = {};
    a.t = {n_dt, n_gt, n_cells, n_iou, n_dt_frames, n_gt_frames, cell_dt_off, cell_gt_off,
           cell_iou_off, nullptr, gt_flags, dt_frame_off, dt_frame_pos, track_boxes(dt_frame_box),
           gt_frame_off, gt_frame_pos, track_boxes(gt_frame_box)};
    if (n_alpha < 1 || n_alpha > TH_NALPHA || !alphas) return TAOAMD_ERR_ARG;
    AlphaTab al = {};
    for (int x = 0; x < n_alpha; x++) {
        // (a NaN compares false both times)
        if (!(alphas[x] == alphas[x]) || (x > 0 && !(alphas[x] > alphas[x - 1])))
            return TAOAMD_ERR_ARG;
        al.v[x] = alphas[x];
    }
    if (!status || (n_gt_frames > 0 && !match)) return TAOAMD_ERR_ARG;
    if (n_iou > 0 && (!pot || !mc || !lc)) return TAOAMD_ERR_ARG;
    const int st = hota_args(a, TT_BOXES, workspace, workspace_bytes);
    if (st != TAOAMD_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    a.n_alpha = n_alpha;
    a.dt_keep = dt_keep;
    a.pot = reinterpret_cast<long long *>(const_cast<int64_t *>(pot));
    a.mc = mc; a.lc = reinterpret_cast<long long *>(lc);
    a.match = match; a.match_iou = match_iou; a.status = status;
    if (n_iou > 0) {
        TAO_HIP(hipMemsetAsync(mc, 0, (size_t)n_alpha * (size_t)n_iou * sizeof(int32_t), s));
        TAO_HIP(hipMemsetAsync(lc, 0, (size_t)n_alpha * (size_t)n_iou * sizeof(int64_t), s));
    }
    if (n_gt_frames > 0) {
        TAO_HIP(hipMemsetAsync(match, 0xff, (size_t)n_gt_frames * sizeof(int32_t), s));
        if (match_iou)
            TAO_HIP(hipMemsetAsync(match_iou, 0, (size_t)n_gt_frames * sizeof(double), s));
    }
    TAO_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (n_gt == 0) return TAOAMD_OK;
    const int si = hota_index(a, s);
    if (si != TAOAMD_OK) return si;
    if (n_gt_frames > 0) {
        TAO_TIMED("hota_frame_kernel", s,
                  hota_frame_kernel<<<(unsigned)((n_gt_frames + TH_TILE - 1) / TH_TILE), TH_TILE,
                                      0, s>>>(a, al));
        TAO_TIMED("hota_group_kernel", s,
                  hota_group_kernel<<<(unsigned)((n_gt_frames + TH_TILE - 1) / TH_TILE), WAVE, 0,
                                      s>>>(a, al));
        if (n_cells > 0)
            TAO_TIMED("hota_cell_kernel", s,
                      hota_cell_kernel<<<(unsigned)n_cells, WAVE, 0, s>>>(a, al));
    }
    if (n_iou > 0 && n_alpha > 1)
        TAO_TIMED("hota_suffix_kernel", s,
                  hota_suffix_kernel<<<(unsigned)((n_iou + 255) / 256), 256, 0, s>>>(a));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

extern "C" int taoamd_track_hota_reduce(
    int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou, int64_t n_dt_frames,
    int64_t n_gt_frames, int32_t n_cat, int32_t n_alpha, const int32_t *cell_dt_off,
    const int32_t *cell_gt_off, const int64_t *cell_iou_off, const int32_t *gt_cat,
    const uint8_t *gt_flags, const int32_t *dt_frame_off, const int32_t *gt_frame_off,
    const int32_t *mc, const int64_t *lc, int64_t *tp, int64_t *loc, int64_t *ass,
    void *workspace, size_t workspace_bytes, void *stream)
{
    HotaArgs a = {};
    a.t = {n_dt, n_gt, n_cells, n_iou, n_dt_frames, n_gt_frames, cell_dt_off, cell_gt_off,
           cell_iou_off, gt_cat, gt_flags, dt_frame_off, nullptr, nullptr,
           gt_frame_off, nullptr, nullptr};
    if (n_cat <= 0 || n_alpha < 1 || n_alpha > TH_NALPHA) return TAOAMD_ERR_ARG;
    if (!tp || !loc || !ass) return TAOAMD_ERR_ARG;
    if (n_iou > 0 && (!mc || !lc)) return TAOAMD_ERR_ARG;
    const int st = hota_args(a, TT_GT_CAT, workspace, workspace_bytes);
    if (st != TAOAMD_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    a.n_cat = n_cat; a.n_alpha = n_alpha;
    a.mc = const_cast<int32_t *>(mc);
    a.lc = reinterpret_cast<long long *>(const_cast<int64_t *>(lc));
    a.tp = (unsigned long long *)tp; a.loc = (unsigned long long *)loc;
    a.ass = (unsigned long long *)ass;
    const size_t words = (size_t)n_cat * (size_t)n_alpha;
    TAO_HIP(hipMemsetAsync(tp, 0, words * sizeof(int64_t), s));
    TAO_HIP(hipMemsetAsync(loc, 0, words * sizeof(int64_t), s));
    TAO_HIP(hipMemsetAsync(ass, 0, words * 3 * sizeof(int64_t), s));
    if (n_gt == 0) return TAOAMD_OK;
    // the cell of every ground-truth row: that table of the frame index alone
    TAO_HIP(hipMemsetAsync(a.t.ft.gt_cell, 0xff, (size_t)n_gt * sizeof(int32_t), s));
    if (n_cells > 0) {
        const FrameSource src = {n_dt, n_gt, n_cells, n_dt_frames, n_gt_frames,
                                 cell_gt_off, nullptr, nullptr, nullptr};
        TAO_TIMED("frames_gt_cell_kernel", s,
                  frames_gt_cell_kernel<<<(unsigned)((n_cells + 255) / 256), 256, 0, s>>>(
                      src, a.t.ft));
    }
    TAO_TIMED("hota_reduce_kernel", s,
              hota_reduce_kernel<<<(unsigned)((n_gt + 255) / 256), 256, 0, s>>>(a));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

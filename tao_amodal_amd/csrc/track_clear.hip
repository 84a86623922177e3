// Track-level CLEAR MOT (gfx950): MOTA / MOTP / ID switches / fragmentations /
// mostly tracked and lost (Bernardin & Stiefelhagen, 2008) from a one-to-one
// assignment per STEP whose weights depend on the step before: the pair matched a
// step ago gets a bonus, an ID switch is scored against the last match however
// long ago.  The steps of a cell are a serial chain.  The reference has no such
// table; the definition is this library's, after TrackEval's CLEAR class, stated
// in include/tao_amodal_hip.h ("track-level CLEAR") and DESIGN.md section 8.
//
// Rows, cells, frame lists and the entry points' common part are those of every
// track analysis (track_tables.hpp, track_frames.hpp; CLEAR has no per-pair table,
// so its cells come without `off`); q and c(s) are HOTA's (ONE = 2^30): every
// output is an integer (match_iou: one box_iou value) and the same from run to
// run.  Three stages:
//
// taoamd_track_clear_count / _fill: the candidates, in parallel.
//   track_index           the frame index (track_frames.hpp)
//   clear_cand_kernel     lane = ground-truth frame of an eligible track: walks the
//                         cell's kept detection tracks in ascending row
//                         (frames_find); a track with a frame at the position sets
//                         the frame's STEP bit, one with s >= frame_thr and q(c(s))
//                         > 0 is a candidate.  COUNT stores the number and the bit,
//                         FILL the candidates' in-cell row, q and s at the frame's
//                         place of the CSR.  Everything that needs a box or a probe
//                         happens here.
//   clear_scan_*_kernel   the frames' counts -> cand_off: sums within blocks of 1024,
//                         the blocks' totals by one workgroup, their addition
//
// taoamd_track_clear_walk: the chain.  workgroup = ONE wavefront = cell.
//   clear_walk1_kernel    the cells with ONE eligible ground truth, the great
//                         majority: its frames are the positions in order.  A chunk
//                         of 64 frames, a lane per frame: the descriptors {first
//                         candidate, end, step bit} are loaded coalesced, the chunk
//                         behind a step ahead; every lane finds its frame's best
//                         candidate (greatest q, first among equal) on its own --
//                         that part does not depend on the chain.  Then a wave-
//                         uniform loop over the chunk's step bits carries {last,
//                         the step of last}: only where the match of the step
//                         before is not the frame's best does the wavefront scan
//                         that frame's list for it (the one dependent load of a
//                         step).  No LDS.
//                         THE ONE-ROW ASSIGNMENT.  With one row the assignment is
//                         the column of the greatest w.  A bonus is 1000 * 2^30 and
//                         every q <= 2^30, so a candidate equal to prev outweighs
//                         all others: it is taken if there is one; else every w is
//                         a q and the greatest wins.  Among equal w the solver takes
//                         the lowest compacted column, which is the lowest row
//                         (columns are compacted in ascending row): the first of
//                         the list.  The same closed form serves a step of a
//                         larger cell in which one ground truth has candidates.
//   clear_walk_kernel     every other cell.  The state per in-cell ground truth
//                         {cursor, end, the position under the cursor, last, the
//                         step of last, matched, idsw, started} and the solver's lie
//                         in LDS where both sides of the cell are <= TC_LDS = 64,
//                         else in the cell's slice of the workspace (the search
//                         store of assign_solve.hpp and arrays like it).  prev[g] is
//                         last[g] where its step is the step before: "every ground
//                         truth of the cell loses prev unless matched" costs
//                         nothing.  An iteration: the least position under the
//                         eligible tracks' cursors (lanes stride the tracks, a
//                         wavefront minimum over LDS), the tracks there compacted by
//                         ballot in ascending row, their cursors advanced -- and the
//                         NEXT frame's position, list bounds and step bit loaded
//                         there, a step ahead of their use; no step bit: no state
//                         changes.  A step: the rows with a candidate; one row: the
//                         closed form.  More: up to TC_STAGE = 64 candidates of the
//                         step are staged in LDS, and the CERTIFIED STEP is tried, a
//                         lane a row: where every row's greatest w is strict and
//                         the rows' columns differ, those pairs are the one optimum
//                         (the sum of the rows' maxima bounds every assignment) and
//                         no search runs.  Else the columns are the rows' candidates
//                         (marked in a cell-wide table, compacted in ascending
//                         row), the smaller side becomes the solver's rows (the
//                         ground truths when equal: assign_sides), assign_solve
//                         with a weight functor that finds the pair in the
//                         frame's list -- staged or in the store -- by bisection
//                         and adds the bonus.
//                         Iterations are bounded by the eligible tracks' frames,
//                         counted at entry.
//                         A cell whose smaller side exceeds TC_NMAX = 2^18 stores 2
//                         to *status and is not walked: a weight is below 2^41, a
//                         potential a sum of at most n of them, and the solver adds
//                         three such terms: 3 * 2^18 * 2^41 < 2^61 = ASSIGN_INF.
//                         (At benchmark size -- 10 000 cells of two ground truths,
//                         215 steps a cell, 40 % of them with both -- the first
//                         form, every list read from the store inside the solver,
//                         took 5.2 ms; LDS for 64 rows, the positions under the
//                         cursors in LDS and the staged lists 4.6 ms; the look-ahead
//                         loads and the certified step 3.6 ms, beside 4.2 ms of
//                         hota_group_kernel in the same run.  DESIGN.md section 8.)
//
// taoamd_track_clear_reduce: the tables, integer adds only.
//   clear_reduce_kernel   wavefront = eligible ground-truth track: lanes stride its
//                         frames, look the match's q up in the frame's list, count
//                         per visibility window in registers (the window loop is
//                         unrolled: no indexed register array), wavefront sums, then
//                         one add per non-zero word by lane 0.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950); no kernel uses
// scratch:
//   clear_cand_kernel<COUNT> 36 VGPRs, <FILL> 38 VGPRs, no LDS;  clear_scan_tile_kernel
//   62 VGPRs, clear_scan_top_kernel 60, 128 B of LDS each;  clear_scan_add_kernel 4;
//   clear_walk1_kernel 40 VGPRs, no LDS;  clear_walk_kernel 107 VGPRs, 8 720 B of LDS
//   (a workgroup is one wavefront: 16 cells a CU by registers, 18 by LDS);
//   clear_reduce_kernel 59 VGPRs, no LDS.
#include "assign_solve.hpp"
#include "track_tables.hpp"

using namespace taoamd;

#define TC_TILE 64                                 // ground-truth frames per workgroup of the candidate kernel
#define TC_LDS 64                                  // rows and columns of a cell whose state is in LDS
#define TC_STAGE 64                                // candidates of a step that are staged in LDS
#define TC_SCAN 1024                               // counts a workgroup of the scan takes
#define TC_END 0x7fffffffffffffffll                // the position under a cursor at its track's end
#define TC_NMAX TAOAMD_TRACK_CLEAR_NMAX            // the smaller side of a cell, at most
#define TC_ONE ((long long)TAOAMD_HOTA_ONE)
#define TC_BONUS (TAOAMD_TRACK_CLEAR_BONUS * TC_ONE)
#define TC_VMAX TAOAMD_TRACK_ASSOCIATION_VIS
#define TC_NGT 4
#define TC_NCAT 7
#define TC_NVIS 4

static_assert(TC_LDS <= WAVE, "a step's rows of a cell in LDS are one pass of the wavefront");

// The kernels' argument block is this file's own, the common fields where they
// were (track_fill<false> sets them; no cell_iou_off: track_cell<false>): over
// { TrackTables t; ... } clear_cand_kernel<COUNT>, the same lines, measured
// 0.4149-0.4170 ms beside 0.4119-0.4129 of the parent, whose code this form
// compiles to, five runs each in turn on one MI355X (a run of its own: other
// runs lie up to 1 % apart as a whole).
struct ClearArgs {
    int64_t n_dt, n_gt, n_cells, n_dt_frames, n_gt_frames, n_cand;
    int32_t n_cat, n_vis;
    double thr;
    const int32_t *cell_dt_off, *cell_gt_off;
    const int32_t *gt_cat;
    const uint8_t *gt_flags, *dt_keep;           // dt_keep NULL: all kept
    const int32_t *dfoff, *dfpos;
    const double4 *dfbox;
    const int32_t *gfoff, *gfpos;
    const double4 *gfbox;
    const double *gfvis, *vis_rng;
    int64_t *cand_off_out;                       // COUNT: [n_gt_frames + 1]
    const int64_t *cand_off;                     // [n_gt_frames + 1]
    int32_t *cand_row_out, *cand_q_out;          // FILL: [n_cand]
    double *cand_iou_out;                        // FILL: [n_cand] or NULL
    const int32_t *cand_row, *cand_q;
    const double *cand_iou;                      // or NULL
    uint8_t *step_out;                           // COUNT: [n_gt_frames]
    const uint8_t *step;
    int32_t *match;                              // [n_gt_frames]
    double *match_iou;                           // [n_gt_frames] or NULL
    uint8_t *sw;                                 // [n_gt_frames]
    int32_t *gt_clear;                           // [n_gt][4]
    int32_t *status;
    unsigned long long *cat_counts, *vis_counts; // [n_cat][7], [n_vis][n_cat][4]
    FrameTables ft;
    int32_t *n_cnt;                              // [n_gt_frames]: COUNT's numbers before the scan
    long long *blk;                              // [n_gt_frames / TC_SCAN + 1]: the scan's block sums
    // the state of the cells that do not fit in LDS, n_dt + n_gt entries each:
    // cell c owns [cell_dt_off[c] + cell_gt_off[c], the next cell's)
    SearchStore store;
    long long *snpos, *sc0, *sc1, *stc0;
    int32_t *sgidx, *sdidx, *sge, *sgf, *smark;
    int32_t *scur, *send, *slast, *slstep, *smat, *sidsw, *sstart, *stn, *stbit, *sbit0;
};

// (offsets clamped to the tables: a bad CSR reads wrong entries, never past an end)
__device__ __forceinline__ int64_t clear_c0(const ClearArgs &a, int64_t k)
{
    return clamp64(a.cand_off[k], 0, a.n_cand);
}
__device__ __forceinline__ int64_t clear_c1(const ClearArgs &a, int64_t k)
{
    return clamp64(a.cand_off[k + 1], clear_c0(a, k), a.n_cand);
}

// q of the stored candidate x of a cell with D detection rows: 0 (no candidate)
// unless its row lies in the cell and its q is positive; a q above ONE reads ONE
__device__ __forceinline__ long long clear_q(const ClearArgs &a, int64_t x, int64_t D, int32_t &row)
{
    row = a.cand_row[x];
    const int32_t q = a.cand_q[x];
    if (row < 0 || row >= D || q <= 0) return 0;
    return q < TC_ONE ? (long long)q : TC_ONE;
}

// ---------------------------------------------------------------------------
// the candidates
// ---------------------------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(TC_TILE) void clear_cand_kernel(ClearArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * TC_TILE + threadIdx.x;
    if (k >= a.n_gt_frames) return;
    int32_t n = 0;
    uint8_t bit = 0;
    int64_t at = 0, end = 0;
    if (FILL) {
        at = clear_c0(a, k);
        end = clear_c1(a, k);
    }
    const int32_t g = a.ft.frame_gt[k];
    const int32_t cell = g >= 0 ? a.ft.gt_cell[g] : -1;
    if (cell >= 0 && track_eligible(a, g)) {
        const TrackCell c = track_cell<false>(a, cell);
        const int64_t p = a.gfpos[k];
        const double4 B = a.gfbox[k];
        for (int64_t d = 0; d < c.D; d++) {
            int64_t lo;
            if (a.dt_keep && !a.dt_keep[c.d0 + d]) continue;
            if (!frames_find(a.dfpos, a.ft.dt_meta[c.d0 + d], p, lo)) continue;
            bit = 1;
            const double4 T = a.dfbox[lo];
            const double s = box_iou(T.x, T.y, T.z, T.w, B.x, B.y, B.z, B.w);
            if (!(s >= a.thr)) continue;                 // (a NaN compares false)
            const long long qv = __double2ll_rn((s < 1.0 ? s : 1.0) * (double)TC_ONE);
            if (qv <= 0) continue;
            if (FILL && at + n < end) {
                a.cand_row_out[at + n] = (int32_t)d;
                a.cand_q_out[at + n] = (int32_t)qv;
                if (a.cand_iou_out) a.cand_iou_out[at + n] = s;
            }
            n++;
        }
    }
    if (!FILL) {
        a.n_cnt[k] = n;
        a.step_out[k] = bit;
    }
}

// off[i] = the sum of cnt[0 .. i), off[n] the total, in three launches: the sums
// within a block of TC_SCAN counts and the block's total; the totals' own sums by
// one workgroup; their addition.  (One workgroup over all the frames, the first
// form, took 4.8 ms at 3 million frames: more than the walk.  The scan itself is
// written out in both kernels: the note at occ_scan_kernel, track_occlusion.hip.)
__global__ __launch_bounds__(TC_SCAN) void clear_scan_tile_kernel(const int32_t *__restrict__ cnt,
                                                                  int64_t *__restrict__ off,
                                                                  long long *__restrict__ blk,
                                                                  int64_t n)
{
    __shared__ long long s_w[TC_SCAN / WAVE];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t i = (int64_t)blockIdx.x * TC_SCAN + tid;
    const long long v = i < n ? cnt[i] : 0;
    const long long incl = wave_prefix(v);
    if (lane_id() == WAVE - 1) s_w[wave] = incl;
    __syncthreads();
    long long before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < TC_SCAN / WAVE; w++) {
        const long long t = s_w[w];
        if (w < wave) before += t;
        total += t;
    }
    if (i < n) off[i] = before + incl - v;
    if (tid == 0) blk[blockIdx.x] = total;
}

// blk[b] = the sum of blk[0 .. b) in place, off[n] = the total; one workgroup
__global__ __launch_bounds__(TC_SCAN) void clear_scan_top_kernel(long long *__restrict__ blk,
                                                                 int64_t nb,
                                                                 int64_t *__restrict__ off,
                                                                 int64_t n)
{
    __shared__ long long s_w[TC_SCAN / WAVE];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    long long carry = 0;
    for (int64_t base = 0; base < nb; base += TC_SCAN) {
        const int64_t i = base + tid;
        const long long v = i < nb ? blk[i] : 0;
        long long incl = v;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const long long u = __shfl_up(incl, o, WAVE);
            if (lane_id() >= o) incl += u;
        }
        if (lane_id() == WAVE - 1) s_w[wave] = incl;
        __syncthreads();
        long long before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < TC_SCAN / WAVE; w++) {
            const long long t = s_w[w];
            if (w < wave) before += t;
            total += t;
        }
        if (i < nb) blk[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();                           // s_w is read
    }
    if (tid == 0) off[n] = carry;
}

__global__ __launch_bounds__(TC_SCAN) void clear_scan_add_kernel(int64_t *__restrict__ off,
                                                                 const long long *__restrict__ blk,
                                                                 int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * TC_SCAN + threadIdx.x;
    if (i < n) off[i] += blk[blockIdx.x];
}

// ---------------------------------------------------------------------------
// the chain
// ---------------------------------------------------------------------------
// The number of eligible rows of the cell and the first of them (uniform)
__device__ __forceinline__ int64_t clear_count_eligible(const ClearArgs &a, const TrackCell &c,
                                                        int64_t &first)
{
    int64_t n = 0;
    first = -1;
    for (int64_t gb = 0; gb < c.G; gb += WAVE) {
        const int64_t o = gb + lane_id();
        const uint64_t m = __ballot(o < c.G && track_eligible(a, c.g0 + o));
        if (m && first < 0) first = gb + __builtin_ctzll(m);
        n += __popcll(m);
    }
    return n;
}

// The one-row assignment of the list [x0, x1) against prev (-1: none), by the wavefront
// (uniform): the place of the chosen candidate in the store, or -1
__device__ __forceinline__ int64_t clear_one_row(const ClearArgs &a, int64_t D, int64_t x0,
                                                 int64_t x1, int32_t prev, int32_t &d)
{
    long long bq = 0;
    int64_t bx = 0x7fffffffffffffffll, hit = 0x7fffffffffffffffll;
    for (int64_t xb = x0; xb < x1; xb += WAVE) {
        const int64_t x = xb + lane_id();
        int32_t row = -1;
        const long long q = x < x1 ? clear_q(a, x, D, row) : 0;
        if (q > 0 && row == prev && x < hit) hit = x;
        if (q > bq) {                        // (ascending x: the first among equal q)
            bq = q;
            bx = x;
        }
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        const long long oq = __shfl_xor(bq, o);
        const int64_t ox = __shfl_xor(bx, o), oh = __shfl_xor(hit, o);
        if (oq > bq || (oq == bq && ox < bx)) {
            bq = oq;
            bx = ox;
        }
        hit = oh < hit ? oh : hit;
    }
    d = -1;
    if (prev >= 0 && hit != 0x7fffffffffffffffll) {
        d = prev;
        return hit;
    }
    if (bq <= 0) return -1;
    d = a.cand_row[bx];
    return bx;
}

__global__ __launch_bounds__(WAVE) void clear_walk1_kernel(ClearArgs a)
{
    const int lane = lane_id();
    const TrackCell c = track_cell<false>(a, blockIdx.x);
    int64_t o1;
    if (clear_count_eligible(a, c, o1) != 1) return;                     // (uniform)
    const int64_t g = c.g0 + o1;
    const TrackSpan f = track_span(a.gfoff, g, a.n_gt_frames);
    const int64_t fs = f.first, fe = f.end;
    int32_t last = -1, lstep = -1, stepno = 0, mat = 0, idsw = 0, start = 0;
    // the chunk's descriptors: the lane's frame {first candidate, end, step bit}
    int64_t x0 = 0, x1 = 0, nx0 = 0, nx1 = 0;
    bool st = false, nst = false;
    if (fs + lane < fe) {
        x0 = clear_c0(a, fs + lane);
        x1 = clear_c1(a, fs + lane);
        st = a.step[fs + lane] != 0;
    }
    for (int64_t base = fs; base < fe; base += WAVE) {
        const int64_t k = base + lane;
        nx0 = nx1 = 0;
        nst = false;
        if (k + WAVE < fe) {                                 // the chunk behind, a step ahead
            nx0 = clear_c0(a, k + WAVE);
            nx1 = clear_c1(a, k + WAVE);
            nst = a.step[k + WAVE] != 0;
        }
        // the lane's own best candidate: the greatest q, the first among equal
        long long bq = 0;
        int64_t bx = -1;
        int32_t br = -1;
        for (int64_t x = x0; x < x1; x++) {
            int32_t row;
            const long long q = clear_q(a, x, c.D, row);
            if (q > bq) {
                bq = q;
                bx = x;
                br = row;
            }
        }
        int32_t om = -1;
        int64_t ox = -1;
        uint8_t osw = 0;
        uint64_t steps = __ballot(k < fe && st);
        while (steps) {                                      // (uniform; at most 64)
            const int j = __builtin_ctzll(steps);
            steps &= steps - 1ull;
            stepno++;
            const int32_t brj = __builtin_amdgcn_readlane(br, j);
            if (brj < 0) continue;                           // no candidate: prev is lost
            const int32_t prev = lstep == stepno - 1 ? last : -1;
            int32_t d = brj;
            int64_t x = -1;                                  // -1: the lane's own best
            if (prev >= 0 && prev != brj) {
                const int64_t j0 = __shfl(x0, j), j1 = __shfl(x1, j);
                for (int64_t xb = j0; xb < j1 && x < 0; xb += WAVE) {
                    int32_t row = -1;
                    const bool hit = xb + lane < j1 && clear_q(a, xb + lane, c.D, row) > 0 &&
                                     row == prev;
                    const uint64_t m = __ballot(hit);
                    if (m) x = xb + __builtin_ctzll(m);
                }
                if (x >= 0) d = prev;
            }
            const bool s = last >= 0 && last != d;
            idsw += s;
            start += lstep != stepno - 1;
            last = d;
            lstep = stepno;
            mat++;
            if (lane == j) {
                om = d;
                ox = x >= 0 ? x : bx;
                osw = s;
            }
        }
        if (k < fe) {
            a.match[k] = om;
            a.sw[k] = osw;
            if (a.match_iou) a.match_iou[k] = om >= 0 && a.cand_iou ? a.cand_iou[ox] : 0.0;
        }
        x0 = nx0;
        x1 = nx1;
        st = nst;
    }
    if (lane == 0) {
        int32_t *out = a.gt_clear + g * TC_NGT;
        out[0] = (int32_t)(fe - fs);
        out[1] = mat;
        out[2] = idsw;
        out[3] = start;
    }
}

// Where the cell's lists and state live: LDS or the cell's slice of the workspace
struct ClearState {
    Search s;
    int32_t *gidx, *didx, *ge, *gf, *mark;
    int32_t *cur, *end, *last, *lstep, *mat, *idsw, *start;
    long long *npos, *c0, *c1;           // the position under a cursor; a step row's list
    // of the frame under a track's cursor, loaded when the cursor moved there (a
    // step ahead of their use): its list's start and length, its step bit; and the
    // step bit of the frame in slot 0 of the step at hand
    long long *tc0;
    int32_t *tn, *tbit, *bit0;
    // the step's candidates staged in LDS (null: read from the store): row i's are
    // [s0[i], s0[i + 1]) of srow / sq, sq 0 where clear_q says "no candidate"
    int32_t *s0, *srow, *sq;
};

// The weight of the shared solver: a row / column is a place in the step's list
// of ground truths / an in-cell detection row
struct ClearWeight {
    const ClearArgs &a;
    int64_t D;
    const ClearState &st;
    bool staged;
    int32_t stepno;
    bool rows_are_gt;
    // the pair's place in the store (x) and its weight; 0: no candidate
    __device__ __forceinline__ long long at(int64_t gi, int64_t d, int64_t &x) const
    {
        long long q;
        if (staged) {
            int lo = st.s0[gi], hi = st.s0[gi + 1];
            const int first = lo;
            if (lo >= hi) return 0;
            hi--;
            while (lo < hi) {                                // (rows ascend in a frame's list)
                const int mid = (lo + hi) >> 1;
                if (st.srow[mid] < d) lo = mid + 1; else hi = mid;
            }
            q = st.sq[lo];
            if (st.srow[lo] != d || q <= 0) return 0;
            x = st.c0[gi] + (lo - first);
        } else {
            int64_t lo = st.c0[gi], hi = st.c1[gi];
            if (lo >= hi) return 0;
            hi--;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (a.cand_row[mid] < d) lo = mid + 1; else hi = mid;
            }
            int32_t row;
            q = clear_q(a, lo, D, row);
            if (row != d || q <= 0) return 0;
            x = lo;
        }
        const int32_t g = st.ge[gi];
        return q + (st.lstep[g] == stepno - 1 && st.last[g] == (int32_t)d ? TC_BONUS : 0ll);
    }
    __device__ __forceinline__ long long operator()(int64_t r, int64_t cc) const
    {
        int64_t x;
        return rows_are_gt ? at(r, cc, x) : at(cc, r, x);
    }
};

// The match (g, frame k, d, place x in the store) of step `stepno`, by one lane
__device__ __forceinline__ void clear_take(const ClearArgs &a, const ClearState &st, int32_t g,
                                           int64_t k, int32_t d, int64_t x, int32_t stepno)
{
    a.match[k] = d;
    if (a.match_iou) a.match_iou[k] = a.cand_iou ? a.cand_iou[x] : 0.0;
    if (st.last[g] >= 0 && st.last[g] != d) {
        a.sw[k] = 1;
        st.idsw[g]++;
    }
    if (st.lstep[g] != stepno - 1) st.start[g]++;
    st.last[g] = d;
    st.lstep[g] = stepno;
    st.mat[g]++;
}

__global__ __launch_bounds__(WAVE) void clear_walk_kernel(ClearArgs a)
{
    __shared__ SearchLds<TC_LDS> l_search;           // (idx0: gidx, idx1: didx)
    __shared__ long long l_npos[TC_LDS], l_c0[TC_LDS], l_c1[TC_LDS];
    __shared__ int32_t l_ge[TC_LDS], l_gf[TC_LDS], l_mark[TC_LDS];
    __shared__ int32_t l_cur[TC_LDS], l_end[TC_LDS], l_last[TC_LDS], l_lstep[TC_LDS];
    __shared__ int32_t l_mat[TC_LDS], l_idsw[TC_LDS], l_start[TC_LDS];
    __shared__ int32_t l_s0[TC_LDS + 1], l_srow[TC_STAGE], l_sq[TC_STAGE];
    __shared__ long long l_tc0[TC_LDS];
    __shared__ int32_t l_tn[TC_LDS], l_tbit[TC_LDS], l_bit0[1];
    const int lane = lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    const TrackCell c = track_cell<false>(a, blockIdx.x);
    int64_t o1;
    if (clear_count_eligible(a, c, o1) < 2) return;                      // (uniform)
    if ((c.G < c.D ? c.G : c.D) > TC_NMAX) {                             // (uniform)
        if (lane == 0) *a.status = 2;
        return;
    }
    const bool lds = c.G <= TC_LDS && c.D <= TC_LDS;
    const int64_t base = c.d0 + c.g0;                // the cell's slice of the state arrays
    ClearState st;
    if (lds) {
        st = {l_search.search(), l_search.idx0, l_search.idx1, l_ge, l_gf, l_mark,
              l_cur, l_end, l_last, l_lstep, l_mat, l_idsw, l_start,
              l_npos, l_c0, l_c1, l_tc0, l_tn, l_tbit, l_bit0, l_s0, l_srow, l_sq};
    } else {
        st = {a.store.at(base), a.sgidx + base, a.sdidx + base, a.sge + base, a.sgf + base,
              a.smark + base,
              a.scur + base, a.send + base, a.slast + base, a.slstep + base, a.smat + base,
              a.sidsw + base, a.sstart + base,
              a.snpos + base, a.sc0 + base, a.sc1 + base, a.stc0 + base, a.stn + base,
              a.stbit + base, a.sbit0 + base, nullptr, nullptr, nullptr};
    }
    // the cursors and the positions under them (an ignored track's at its end: it is
    // never there), the frames in all
    int64_t budget = 0;
    for (int64_t ob = 0; ob < c.G; ob += WAVE) {
        const int64_t o = ob + lane;
        int64_t mine = 0;
        if (o < c.G) {
            const TrackSpan f = track_span(a.gfoff, c.g0 + o, a.n_gt_frames);
            const int64_t fs = f.first, fe = f.end;
            const bool el = track_eligible(a, c.g0 + o);
            st.cur[o] = (int32_t)fs;
            st.end[o] = (int32_t)fe;
            st.npos[o] = el && fs < fe ? (long long)a.gfpos[fs] : TC_END;
            if (el && fs < fe) {
                st.tc0[o] = clear_c0(a, fs);
                st.tn[o] = (int32_t)(clear_c1(a, fs) - clear_c0(a, fs));
                st.tbit[o] = a.step[fs];
            }
            st.last[o] = -1;
            st.lstep[o] = -1;
            st.mat[o] = st.idsw[o] = st.start[o] = 0;
            mine = el ? fe - fs : 0;
        }
        budget += wave_sum(mine);
    }
    __syncthreads();
    int32_t stepno = 0;
    for (int64_t it = 0; it < budget; it++) {
        // the least position under the cursors
        long long p = TC_END;
        for (int64_t o = lane; o < c.G; o += WAVE) {
            const long long q = st.npos[o];
            p = q < p ? q : p;
        }
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            const long long q = __shfl_xor(p, o);
            p = q < p ? q : p;
        }
        if (p == TC_END) break;                                          // (uniform)
        // the tracks with a frame there, ascending row; their cursors move on
        int ng = 0;
        for (int64_t ob = 0; ob < c.G; ob += WAVE) {
            const int64_t o = ob + lane;
            const bool has = o < c.G && st.npos[o] == p;
            const uint64_t m = __ballot(has);
            if (has) {
                const int32_t k = st.cur[o];
                const int slot = ng + __popcll(m & below);
                st.ge[slot] = (int32_t)o;
                st.gf[slot] = k;
                st.c0[slot] = st.tc0[o];
                st.c1[slot] = st.tc0[o] + st.tn[o];
                if (slot == 0) st.bit0[0] = st.tbit[o];
                st.cur[o] = k + 1;
                const bool more = k + 1 < st.end[o];
                st.npos[o] = more ? (long long)a.gfpos[k + 1] : TC_END;
                if (more) {                                  // what the next step there needs
                    st.tc0[o] = clear_c0(a, k + 1);
                    st.tn[o] = (int32_t)(clear_c1(a, k + 1) - clear_c0(a, k + 1));
                    st.tbit[o] = a.step[k + 1];
                }
            }
            ng += __popcll(m);
        }
        __syncthreads();
        if (ng == 0) break;                                              // (cannot be: p was found)
        if (!st.bit0[0]) continue;                                       // no step: no state changes
        stepno++;
        // the rows' lists; the rows with a candidate
        int mg = 0;
        long long total = 0;
        for (int ib = 0; ib < ng; ib += WAVE) {
            const int i = ib + lane;
            long long x0 = 0, x1 = 0;
            if (i < ng) {
                x0 = st.c0[i];
                x1 = st.c1[i];
            }
            const uint64_t m = __ballot(x1 > x0);
            if (x1 > x0) st.gidx[mg + __popcll(m & below)] = i;
            mg += __popcll(m);
            total += wave_sum(x1 - x0);
            if (lds) {                                       // (ng <= TC_LDS = WAVE: one pass)
                const long long incl = wave_prefix(x1 - x0);
                if (incl - (x1 - x0) <= TC_STAGE) l_s0[lane] = (int32_t)(incl - (x1 - x0));
                if (lane == WAVE - 1 && incl <= TC_STAGE) l_s0[WAVE] = (int32_t)incl;
            }
        }
        __syncthreads();
        if (mg == 0) continue;                                           // (uniform)
        if (mg == 1) {
            const int i = st.gidx[0];
            const int32_t g = st.ge[i];
            const int32_t prev = st.lstep[g] == stepno - 1 ? st.last[g] : -1;
            int32_t d;
            const int64_t x = clear_one_row(a, c.D, st.c0[i], st.c1[i], prev, d);
            if (x >= 0 && lane == 0) clear_take(a, st, g, st.gf[i], d, x, stepno);
            __syncthreads();
            continue;
        }
        // the step's candidates into LDS where they fit: the solver then reads no
        // global memory
        const bool staged = lds && total <= TC_STAGE;                    // (uniform)
        if (staged) {
            for (int t = 0; t < mg; t++) {
                const int i = st.gidx[t];
                const long long x0 = st.c0[i], n = st.c1[i] - x0;
                for (long long e = lane; e < n; e += WAVE) {
                    int32_t row;
                    const long long q = clear_q(a, x0 + e, c.D, row);
                    l_srow[l_s0[i] + e] = row;
                    l_sq[l_s0[i] + e] = (int32_t)q;
                }
            }
            __syncthreads();
            // THE CERTIFIED STEP, a lane a row: the sum of the rows' greatest w bounds
            // every assignment's sum from above; where each row's greatest w is
            // strict and the rows' columns differ, that set of pairs reaches the
            // bound and nothing else does: it is what the solver returns, without it.
            // (mark[] decides "differ": a row reads back the slot it wrote.)
            const int i = lane < mg ? st.gidx[lane] : -1;
            long long bw = 0;
            int be = -1;
            bool ok = true;
            if (i >= 0) {
                const int32_t g = st.ge[i];
                const int32_t prev = st.lstep[g] == stepno - 1 ? st.last[g] : -1;
                for (int e = l_s0[i]; e < l_s0[i + 1]; e++) {
                    const long long q = l_sq[e];
                    if (q <= 0) continue;
                    const long long w = q + (l_srow[e] == prev ? TC_BONUS : 0ll);
                    if (w > bw) {
                        bw = w;
                        be = e;
                        ok = true;
                    } else if (w == bw) {
                        ok = false;
                    }
                }
                ok = ok && be >= 0;
                if (ok) st.mark[l_srow[be]] = lane + 1;
            }
            __syncthreads();
            if (i >= 0 && ok) ok = st.mark[l_srow[be]] == lane + 1;
            if (__ballot(!ok) == 0) {                                    // (uniform)
                if (i >= 0)
                    clear_take(a, st, st.ge[i], st.gf[i], l_srow[be], st.c0[i] + (be - l_s0[i]),
                               stepno);
                __syncthreads();
                continue;
            }
        }
        // the columns: the rows' candidates, marked and compacted in ascending row
        for (int64_t d = lane; d < c.D; d += WAVE) st.mark[d] = 0;
        __syncthreads();
        if (staged) {
            for (int e = lane; e < (int)total; e += WAVE)
                if (l_sq[e] > 0) st.mark[l_srow[e]] = 1;
        } else {
            for (int t = 0; t < mg; t++) {
                const int64_t x1 = st.c1[st.gidx[t]];
                for (int64_t x = st.c0[st.gidx[t]] + lane; x < x1; x += WAVE) {
                    int32_t row;
                    if (clear_q(a, x, c.D, row) > 0) st.mark[row] = 1;
                }
            }
        }
        __syncthreads();
        int md = 0;
        for (int64_t db = 0; db < c.D; db += WAVE) {
            const int64_t d = db + lane;
            const bool act = d < c.D && st.mark[d] != 0;
            const uint64_t m = __ballot(act);
            if (act) st.didx[md + __popcll(m & below)] = (int32_t)d;
            md += __popcll(m);
        }
        __syncthreads();
        if (md == 0) continue;                                           // (uniform)
        // the smaller side as rows, the ground truths when equal
        const Sides sd = assign_sides(st.gidx, mg, st.didx, md);
        Search s = st.s;
        s.ridx = sd.rows;
        s.cidx = sd.cols;
        const ClearWeight W = {a, c.D, st, staged, stepno, sd.first};
        if (!assign_solve(W, s, sd.n, sd.m)) {
            if (lane == 0) *a.status = 1;
            __syncthreads();
            continue;
        }
        // the pairs with a positive w (distinct ground truths: a lane a pair)
        assign_pairs(s, sd, [&](bool has, int64_t gi, int64_t d) {
            int64_t x = 0;
            if (has && W.at(gi, d, x) > 0)
                clear_take(a, st, st.ge[gi], st.gf[gi], (int32_t)d, x, stepno);
        });
        __syncthreads();
    }
    __syncthreads();
    for (int64_t o = lane; o < c.G; o += WAVE) {
        if (!track_eligible(a, c.g0 + o)) continue;
        int32_t *out = a.gt_clear + (c.g0 + o) * TC_NGT;
        out[0] = (int32_t)track_span(a.gfoff, c.g0 + o, a.n_gt_frames).len();
        out[1] = st.mat[o];
        out[2] = st.idsw[o];
        out[3] = st.start[o];
    }
}

// ---------------------------------------------------------------------------
// reduce
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clear_reduce_kernel(ClearArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * (256 / WAVE)
                    + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    if (g >= a.n_gt) return;                                 // (whole wavefronts)
    const int32_t cat = a.gt_cat[g];
    if (!track_eligible(a, g) || cat < 0 || cat >= a.n_cat) return;      // (uniform)
    const int lane = lane_id();
    const TrackSpan f = track_span(a.gfoff, g, a.n_gt_frames);
    const int64_t fs = f.first, fe = f.end;
    long long qsum = 0;
    int32_t vf[TC_VMAX], vm[TC_VMAX], vs[TC_VMAX];
    long long vq[TC_VMAX];
#pragma unroll
    for (int w = 0; w < TC_VMAX; w++) {
        vf[w] = vm[w] = vs[w] = 0;
        vq[w] = 0;
    }
    for (int64_t k = fs + lane; k < fe; k += WAVE) {
        const int32_t m = a.match[k];
        long long q = 0;
        if (m >= 0) {
            // the match's q: its row in the frame's list (any D: the row is compared)
            const int64_t x1 = clear_c1(a, k);
            for (int64_t x = clear_c0(a, k); x < x1 && q == 0; x++) {
                int32_t row;
                const long long v = clear_q(a, x, 0x7fffffff, row);
                if (row == m) q = v;
            }
        }
        qsum += q;
        if (a.n_vis > 0) {
            const double v = a.gfvis[k];
            const bool s = a.sw[k] != 0;
#pragma unroll
            for (int w = 0; w < TC_VMAX; w++) {
                // (a closed window; a NaN visibility compares false: in none)
                if (w < a.n_vis && a.vis_rng[2 * w] <= v && v <= a.vis_rng[2 * w + 1]) {
                    vf[w]++;
                    vm[w] += m >= 0;
                    vs[w] += s;
                    vq[w] += q;
                }
            }
        }
    }
    qsum = wave_sum(qsum);
#pragma unroll
    for (int w = 0; w < TC_VMAX; w++) {
        if (w < a.n_vis) {                                   // (uniform)
            const int32_t f = wave_sum(vf[w]), m = wave_sum(vm[w]), s = wave_sum(vs[w]);
            const long long q = wave_sum(vq[w]);
            if (lane == 0) {
                unsigned long long *row = a.vis_counts + ((int64_t)w * a.n_cat + cat) * TC_NVIS;
                if (f) atomicAdd(row + 0, (unsigned long long)f);
                if (m) atomicAdd(row + 1, (unsigned long long)m);
                if (s) atomicAdd(row + 2, (unsigned long long)s);
                if (q) atomicAdd(row + 3, (unsigned long long)q);
            }
        }
    }
    if (lane == 0) {
        const int32_t *in = a.gt_clear + g * TC_NGT;
        const long long present = in[0], matched = in[1];
        const bool mt = 5 * matched > 4 * present;
        const bool pt = !mt && 5 * matched >= present;
        unsigned long long *row = a.cat_counts + (int64_t)cat * TC_NCAT;
        if (in[1] > 0) atomicAdd(row + 0, (unsigned long long)in[1]);
        if (in[2] > 0) atomicAdd(row + 1, (unsigned long long)in[2]);
        if (in[3] > 1) atomicAdd(row + 2, (unsigned long long)(in[3] - 1));
        atomicAdd(row + (mt ? 3 : (pt ? 4 : 5)), 1ull);
        if (qsum) atomicAdd(row + 6, (unsigned long long)qsum);
    }
}

// ---------------------------------------------------------------------------
// the entry points
// ---------------------------------------------------------------------------
// The tables of all stages, in buffer order: a function of (n_dt, n_gt, n_gt_frames)
static void clear_layout(Carve &c, int64_t n_dt, int64_t n_gt, int64_t n_gt_frames,
                         FrameTables &ft, ClearArgs &a)
{
    const size_t n = (size_t)(n_dt + n_gt);
    frames_layout(c, n_dt, n_gt, n_gt_frames, ft);
    a.n_cnt = c.take<int32_t>((size_t)n_gt_frames);
    a.blk = c.take<long long>((size_t)n_gt_frames / TC_SCAN + 1);
    a.store.layout(c, n);
    for (long long **q : {&a.snpos, &a.sc0, &a.sc1, &a.stc0}) *q = c.take<long long>(n);
    for (int32_t **q : {&a.sgidx, &a.sdidx, &a.sge, &a.sgf, &a.smark, &a.scur, &a.send, &a.stn,
                        &a.stbit, &a.sbit0, &a.slast, &a.slstep, &a.smat, &a.sidsw, &a.sstart})
        *q = c.take<int32_t>(n);
}

extern "C" size_t taoamd_track_clear_workspace(int64_t n_dt, int64_t n_gt, int64_t n_gt_frames)
{
    if (!track_sizes_ok(n_dt, n_gt, n_gt_frames, TT_STORE)) return 0;
    ClearArgs a;
    return measure([&](Carve &c) { clear_layout(c, n_dt, n_gt, n_gt_frames, a.ft, a); });
}

// What the entry points share: the common refusals, the carved workspace and the
// common fields of the kernels' block
static int clear_args(ClearArgs &a, TrackTables &t, unsigned need, void *workspace,
                      size_t workspace_bytes)
{
    a = {};
    const int st = track_args(
        t, need | TT_GT_FLAGS | TT_STORE, workspace, workspace_bytes,
        [&](Carve &c) { clear_layout(c, t.n_dt, t.n_gt, t.n_gt_frames, t.ft, a); });
    track_fill<false>(a, t);
    return st;
}

static unsigned clear_tiles(int64_t n_gt_frames)
{
    return (unsigned)((n_gt_frames + TC_TILE - 1) / TC_TILE);
}

extern "C" int taoamd_track_clear_count(
    int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_dt_frames, int64_t n_gt_frames,
    double frame_thr, const int32_t *cell_dt_off, const int32_t *cell_gt_off,
    const uint8_t *gt_flags, const uint8_t *dt_keep, const int32_t *dt_frame_off,
    const int32_t *dt_frame_pos, const double *dt_frame_box, const int32_t *gt_frame_off,
    const int32_t *gt_frame_pos, const double *gt_frame_box, int64_t *cand_off, uint8_t *step,
    void *workspace, size_t workspace_bytes, void *stream)
{
    ClearArgs a;
    TrackTables t = {n_dt, n_gt, n_cells, 0, n_dt_frames, n_gt_frames, cell_dt_off, cell_gt_off, nullptr,
           nullptr, gt_flags, dt_frame_off, dt_frame_pos, track_boxes(dt_frame_box),
           gt_frame_off, gt_frame_pos, track_boxes(gt_frame_box)};
    if (!cand_off || (n_gt_frames > 0 && !step)) return TAOAMD_ERR_ARG;
    if (!(frame_thr > 0.0 && frame_thr <= 1.0)) return TAOAMD_ERR_ARG;   // (a NaN compares false)
    const int st = clear_args(a, t, TT_BOXES, workspace, workspace_bytes);
    if (st != TAOAMD_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    a.thr = frame_thr;
    a.dt_keep = dt_keep;
    a.cand_off_out = cand_off;
    a.step_out = step;
    if (n_gt == 0 || n_gt_frames == 0) {
        TAO_HIP(hipMemsetAsync(cand_off, 0, (size_t)(n_gt_frames + 1) * sizeof(int64_t), s));
        if (n_gt_frames > 0) TAO_HIP(hipMemsetAsync(step, 0, (size_t)n_gt_frames, s));
        return TAOAMD_OK;
    }
    const int si = track_index(t, s);
    if (si != TAOAMD_OK) return si;
    TAO_TIMED("clear_count_kernel", s,
              clear_cand_kernel<false><<<clear_tiles(n_gt_frames), TC_TILE, 0, s>>>(a));
    const int64_t nb = (n_gt_frames + TC_SCAN - 1) / TC_SCAN;
    TAO_TIMED("clear_scan_tile_kernel", s,
              clear_scan_tile_kernel<<<(unsigned)nb, TC_SCAN, 0, s>>>(a.n_cnt, cand_off, a.blk,
                                                                      n_gt_frames));
    TAO_TIMED("clear_scan_top_kernel", s,
              clear_scan_top_kernel<<<1, TC_SCAN, 0, s>>>(a.blk, nb, cand_off, n_gt_frames));
    TAO_TIMED("clear_scan_add_kernel", s,
              clear_scan_add_kernel<<<(unsigned)nb, TC_SCAN, 0, s>>>(cand_off, a.blk, n_gt_frames));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

extern "C" int taoamd_track_clear_fill(
    int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_dt_frames, int64_t n_gt_frames,
    double frame_thr, const int32_t *cell_dt_off, const int32_t *cell_gt_off,
    const uint8_t *gt_flags, const uint8_t *dt_keep, const int32_t *dt_frame_off,
    const int32_t *dt_frame_pos, const double *dt_frame_box, const int32_t *gt_frame_off,
    const int32_t *gt_frame_pos, const double *gt_frame_box, const int64_t *cand_off,
    int64_t n_cand, int32_t *cand_row, int32_t *cand_q, double *cand_iou, void *workspace,
    size_t workspace_bytes, void *stream)
{
    ClearArgs a;
    TrackTables t = {n_dt, n_gt, n_cells, 0, n_dt_frames, n_gt_frames, cell_dt_off, cell_gt_off, nullptr,
           nullptr, gt_flags, dt_frame_off, dt_frame_pos, track_boxes(dt_frame_box),
           gt_frame_off, gt_frame_pos, track_boxes(gt_frame_box)};
    if (n_cand < 0 || !cand_off || (n_cand > 0 && (!cand_row || !cand_q))) return TAOAMD_ERR_ARG;
    if (!(frame_thr > 0.0 && frame_thr <= 1.0)) return TAOAMD_ERR_ARG;   // (a NaN compares false)
    const int st = clear_args(a, t, TT_BOXES, workspace, workspace_bytes);
    if (st != TAOAMD_OK) return st;
    if (n_gt == 0 || n_gt_frames == 0 || n_cand == 0) return TAOAMD_OK;  // no candidate to store
    hipStream_t s = (hipStream_t)stream;
    a.thr = frame_thr;
    a.dt_keep = dt_keep;
    a.cand_off = cand_off;
    a.n_cand = n_cand;
    a.cand_row_out = cand_row;
    a.cand_q_out = cand_q;
    a.cand_iou_out = cand_iou;
    const int si = track_index(t, s);
    if (si != TAOAMD_OK) return si;
    TAO_TIMED("clear_fill_kernel", s,
              clear_cand_kernel<true><<<clear_tiles(n_gt_frames), TC_TILE, 0, s>>>(a));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

extern "C" int taoamd_track_clear_walk(
    int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_gt_frames, int64_t n_cand,
    const int32_t *cell_dt_off, const int32_t *cell_gt_off, const uint8_t *gt_flags,
    const int32_t *gt_frame_off, const int32_t *gt_frame_pos, const int64_t *cand_off,
    const int32_t *cand_row, const int32_t *cand_q, const double *cand_iou, const uint8_t *step,
    int32_t *match, double *match_iou, uint8_t *sw, int32_t *gt_clear, int32_t *status,
    void *workspace, size_t workspace_bytes, void *stream)
{
    ClearArgs a;
    TrackTables t = {n_dt, n_gt, n_cells, 0, 0, n_gt_frames, cell_dt_off, cell_gt_off, nullptr, nullptr,
           gt_flags, nullptr, nullptr, nullptr, gt_frame_off, gt_frame_pos, nullptr};
    if (n_cand < 0 || !status || !cand_off) return TAOAMD_ERR_ARG;
    if (n_gt > 0 && !gt_clear) return TAOAMD_ERR_ARG;
    if (n_gt_frames > 0 && (!step || !match || !sw)) return TAOAMD_ERR_ARG;
    if (n_cand > 0 && (!cand_row || !cand_q)) return TAOAMD_ERR_ARG;
    const int st = clear_args(a, t, TT_GT_POS, workspace, workspace_bytes);
    if (st != TAOAMD_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    a.n_cand = n_cand;
    a.cand_off = cand_off; a.cand_row = cand_row; a.cand_q = cand_q; a.cand_iou = cand_iou;
    a.step = step;
    a.match = match; a.match_iou = match_iou; a.sw = sw; a.gt_clear = gt_clear;
    a.status = status;
    if (n_gt_frames > 0) {
        TAO_HIP(hipMemsetAsync(match, 0xff, (size_t)n_gt_frames * sizeof(int32_t), s));
        TAO_HIP(hipMemsetAsync(sw, 0, (size_t)n_gt_frames, s));
        if (match_iou)
            TAO_HIP(hipMemsetAsync(match_iou, 0, (size_t)n_gt_frames * sizeof(double), s));
    }
    if (n_gt > 0) TAO_HIP(hipMemsetAsync(gt_clear, 0, (size_t)n_gt * TC_NGT * sizeof(int32_t), s));
    TAO_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (n_gt == 0 || n_cells == 0) return TAOAMD_OK;
    TAO_TIMED("clear_walk1_kernel", s,
              clear_walk1_kernel<<<(unsigned)n_cells, WAVE, 0, s>>>(a));
    TAO_TIMED("clear_walk_kernel", s, clear_walk_kernel<<<(unsigned)n_cells, WAVE, 0, s>>>(a));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

extern "C" int taoamd_track_clear_reduce(
    int64_t n_dt, int64_t n_gt, int64_t n_gt_frames, int64_t n_cand, int32_t n_cat, int32_t n_vis,
    const int32_t *gt_cat, const uint8_t *gt_flags, const int32_t *gt_frame_off,
    const double *gt_frame_vis, const double *vis_rng, const int64_t *cand_off,
    const int32_t *cand_row, const int32_t *cand_q, const int32_t *match, const uint8_t *sw,
    const int32_t *gt_clear, int64_t *cat_counts, int64_t *vis_counts, void *workspace,
    size_t workspace_bytes, void *stream)
{
    ClearArgs a;
    TrackTables t = {n_dt, n_gt, 0, 0, 0, n_gt_frames, nullptr, nullptr, nullptr, gt_cat, gt_flags,
           nullptr, nullptr, nullptr, gt_frame_off, nullptr, nullptr};
    if (n_cand < 0 || n_cat <= 0 || n_vis < 0 || n_vis > TC_VMAX) return TAOAMD_ERR_ARG;
    if (n_vis > 0 && (!gt_frame_vis || !vis_rng || !vis_counts)) return TAOAMD_ERR_ARG;
    if (!cat_counts || !cand_off || (n_gt > 0 && !gt_clear)) return TAOAMD_ERR_ARG;
    if (n_gt_frames > 0 && (!match || !sw)) return TAOAMD_ERR_ARG;
    if (n_cand > 0 && (!cand_row || !cand_q)) return TAOAMD_ERR_ARG;
    const int st = clear_args(a, t, TT_GT_CAT, workspace, workspace_bytes);
    if (st != TAOAMD_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    a.n_cand = n_cand;
    a.n_cat = n_cat; a.n_vis = n_vis;
    a.gfvis = gt_frame_vis; a.vis_rng = vis_rng;
    a.cand_off = cand_off; a.cand_row = cand_row; a.cand_q = cand_q;
    a.match = const_cast<int32_t *>(match); a.sw = const_cast<uint8_t *>(sw);
    a.gt_clear = const_cast<int32_t *>(gt_clear);
    a.cat_counts = (unsigned long long *)cat_counts;
    a.vis_counts = (unsigned long long *)vis_counts;
    TAO_HIP(hipMemsetAsync(cat_counts, 0, (size_t)n_cat * TC_NCAT * sizeof(int64_t), s));
    if (n_vis > 0)
        TAO_HIP(hipMemsetAsync(vis_counts, 0,
                               (size_t)n_vis * n_cat * TC_NVIS * sizeof(int64_t), s));
    if (n_gt == 0) return TAOAMD_OK;
    const int per = 256 / WAVE;
    TAO_TIMED("clear_reduce_kernel", s,
              clear_reduce_kernel<<<(unsigned)((n_gt + per - 1) / per), 256, 0, s>>>(a));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

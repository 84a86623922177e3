// Track-level occlusion episodes (gfx950): is a ground-truth track's follower
// KEPT while the object is hidden.  The reference has no such table; the
// definition is this library's, stated in include/tao_amodal_hip.h ("track-level
// occlusion episodes") and DESIGN.md section 8.  In short: frame k of a ground-
// truth track is occluded when lo <= vis_k <= hi; an EPISODE is a maximal run
// a..b of occluded frames of the track's own frame list; entry = the follower of
// frame a - 1; covered / held = the frames of the run with a follower / with
// that follower; after = the follower of the first covered frame among the
// `recover` frames behind b, gap = the uncovered frames before it; one outcome
// of six.  The followers are association's best[] (csrc/track_association.hip).
//
//   occ_walk_kernel   wavefront = ground-truth track, lane = frame of a chunk of
//                     64, as assoc_walk_kernel: best[] and the visibilities are
//                     read once, coalesced; the chunk behind is loaded a step
//                     ahead (an episode's end and its recover window may need it:
//                     recover <= 64, so one chunk is enough) and becomes the next
//                     step's chunk in registers.  occ and cov are ballots, run ends
//                     `occ & ~(occ >> 1 | next occ << 63)`.  The episodes that END
//                     in a chunk are handled in a wave-uniform loop over the end
//                     bits: the start is the highest clear bit of occ below the
//                     end, entry a readlane (or the carry of the chunk before),
//                     held a popcount of ballot(best == entry) under the run's
//                     mask, after a ctz of the 64 cov bits above the end.  A run
//                     open at the chunk's end leaves {entry, a, covered, held} as
//                     the carry.  COUNT: lane j keeps the 11 counters of length
//                     bucket j in registers and adds the non-zero ones to the
//                     category's row when the track is done -- integer adds, order-
//                     free; the track's row of gt_occ and its number of episodes.
//                     FILL: the same walk, the records instead: lanes 0 .. 8 store
//                     the nine columns of an episode as one 36-byte piece.
//   occ_scan_kernel   one workgroup: the tracks' episode counts -> ep_off
// Everything is an integer; every record has one place.
#include "track_tables.hpp"

using namespace taoamd;

#define TO_LEN TAOAMD_TRACK_OCCLUSION_LEN          // length buckets, at most
#define TO_RECOVER TAOAMD_TRACK_OCCLUSION_RECOVER  // recover, at most
#define TO_NEP 9
#define TO_NGT 4
#define TO_NCNT 11

static_assert(TO_RECOVER == WAVE, "the look-ahead is one chunk");
static_assert(TO_LEN <= WAVE && TO_NEP <= WAVE, "a lane per bucket, a lane per column");

enum { OCC_START, OCC_UNFOLLOWED, OCC_END, OCC_KEPT, OCC_SWITCHED, OCC_LOST };

struct OccArgs {
    int64_t n_gt, n_gt_frames;
    int32_t n_cat, n_len, recover;
    double lo, hi;
    int32_t edges[TO_LEN];
    const int32_t *gt_cat;
    const uint8_t *gt_flags;
    const int32_t *gfoff;
    const double *gfvis;
    const int32_t *best;                     // [n_gt_frames] in-cell follower, -1: none
    int32_t *gt_occ;                         // [n_gt][4]
    unsigned long long *counts;              // [n_cat][n_len][11]
    int32_t *n_ep;                           // [n_gt] episodes of the track
    const int64_t *ep_off;                   // FILL: [n_gt + 1]
    int64_t cap;
    int32_t *episodes;                       // [cap][9]
};

// One chunk: the lane's follower (-1 behind the track's end) and the ballots
struct OccChunk {
    int32_t b;
    uint64_t occ, cov;
    __device__ __forceinline__ void none() { b = -1; occ = cov = 0; }
    __device__ __forceinline__ void load(const OccArgs &a, int64_t base, int64_t e)
    {
        const int64_t k = base + lane_id();
        const bool live = k < e;
        b = live ? a.best[k] : -1;
        const double vis = live ? a.gfvis[k] : 0.0;
        // (a closed window; a NaN visibility compares false: not occluded)
        occ = __ballot(live && a.lo <= vis && vis <= a.hi);
        cov = __ballot(b >= 0);
    }
};

// The part of a run that lies in the chunk at hand and ends at its lane `top`,
// joined with the carry where the run came in from the chunk before
struct OccRun {
    int32_t entry, a, covered, held;
};

template <bool FILL>
__global__ __launch_bounds__(256) void occ_walk_kernel(OccArgs a)
{
    // (the wavefront's number as a scalar: the track, its bounds and every episode
    // are the same in all lanes, and the compiler is told so)
    const int64_t g = (int64_t)blockIdx.x * (256 / WAVE)
                    + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    if (g >= a.n_gt) return;                 // (whole wavefronts)
    const int lane = lane_id();
    const TrackSpan f = track_span(a.gfoff, g, a.n_gt_frames);
    const int64_t s = f.first, e = f.end;
    const int32_t L = (int32_t)(e - s);
    int64_t row0 = 0, row1 = 0;
    if (FILL) {
        // the track's episodes lie below cap as a whole, or none of them is stored
        row0 = a.ep_off[g];
        row1 = a.ep_off[g + 1];
        if (!(row0 >= 0 && row0 < row1 && row1 <= a.cap)) return;      // (uniform)
    }
    int32_t episodes = 0, frames = 0, kept = 0, gone = 0;
    int32_t acc[TO_NCNT];                    // COUNT: lane j, the counters of bucket j
#pragma unroll
    for (int c = 0; c < TO_NCNT; c++) acc[c] = 0;
    bool open = false;                       // a run came in from the chunk before
    OccRun carry = {-1, 0, 0, 0};
    int32_t prev = -1;                       // the follower of the frame before the chunk
    OccChunk cur, nxt;
    cur.none();
    if (s < e) cur.load(a, s, e);
    for (int64_t base = s; base < e; base += WAVE) {
        nxt.none();
        if (base + WAVE < e) nxt.load(a, base + WAVE, e);   // (uniform; bounded by the track's end)
        const int32_t at = (int32_t)(base - s);             // lane 0's place in the frame list
        const int32_t b = cur.b;
        const uint64_t occ = cur.occ, cov = cur.cov;
        frames += __popcll(occ);
        // the run that ends at lane `top` (or is open there, top = 63)
        auto run_at = [&](int top) {
            const uint64_t upto = (2ull << top) - 1ull;     // lanes 0 .. top (top = 63: all)
            const uint64_t clear = ~occ & upto;
            const int first = clear ? 64 - __builtin_clzll(clear) : 0;
            const uint64_t mask = upto & ~((1ull << first) - 1ull);
            const bool cont = first == 0 && open;
            const int32_t left = __builtin_amdgcn_readlane(b, first > 0 ? first - 1 : 0);
            OccRun r;
            r.entry = cont ? carry.entry : (first > 0 ? left : prev);
            r.a = cont ? carry.a : at + first;
            r.covered = (cont ? carry.covered : 0) + __popcll(cov & mask);
            // (entry >= 0: no lane behind the track's end compares equal)
            const uint64_t same = __ballot(b == r.entry);
            r.held = (cont ? carry.held : 0) + (r.entry >= 0 ? __popcll(same & mask) : 0);
            return r;
        };
        uint64_t ends = occ & ~((occ >> 1) | (nxt.occ << 63));
        while (ends) {                                      // (uniform)
            const int top = __builtin_ctzll(ends);
            ends &= ends - 1ull;
            const OccRun r = run_at(top);
            const int32_t last = at + top;
            const int32_t n = last - r.a + 1;
            int32_t after = -1, gap = 0, outcome;
            if (r.a == 0) {
                outcome = OCC_START;
            } else if (r.entry < 0) {
                outcome = OCC_UNFOLLOWED;
            } else if (last == L - 1) {
                outcome = OCC_END;
            } else {
                // cov of the 64 frames behind `last`; behind the track's end it is clear
                uint64_t w = (top < 63 ? cov >> (top + 1) : 0ull) | (nxt.cov << (63 - top));
                if (a.recover < 64) w &= (1ull << a.recover) - 1ull;
                if (w) {
                    gap = __builtin_ctzll(w);
                    const int at_lane = top + 1 + gap;
                    const int32_t here = __builtin_amdgcn_readlane(b, at_lane & 63);
                    const int32_t there = __builtin_amdgcn_readlane(nxt.b, at_lane & 63);
                    after = at_lane < 64 ? here : there;
                }
                outcome = after == r.entry ? OCC_KEPT : (after >= 0 ? OCC_SWITCHED : OCC_LOST);
            }
            kept += outcome == OCC_KEPT;
            gone += outcome == OCC_SWITCHED || outcome == OCC_LOST;
            if (FILL) {
                const int64_t p = row0 + episodes;
                if (p < row1 && lane < TO_NEP) {   // (an ep_off of other tables: not past its rows)
                    const int32_t v = lane == 0 ? (int32_t)g : lane == 1 ? r.a : lane == 2 ? n
                                    : lane == 3 ? outcome : lane == 4 ? r.entry : lane == 5 ? after
                                    : lane == 6 ? gap : lane == 7 ? r.covered : r.held;
                    a.episodes[p * TO_NEP + lane] = v;
                }
            } else {
                int j = 0;
#pragma unroll
                for (int i = 1; i < TO_LEN; i++)
                    if (i < a.n_len && n >= a.edges[i]) j = i;
                if (lane == j) {
                    acc[0] += 1;
                    acc[1] += n;
                    acc[2] += r.covered;
                    acc[3] += r.held;
                    acc[4] += outcome == OCC_START;
                    acc[5] += outcome == OCC_UNFOLLOWED;
                    acc[6] += outcome == OCC_END;
                    acc[7] += outcome == OCC_KEPT;
                    acc[8] += outcome == OCC_SWITCHED;
                    acc[9] += outcome == OCC_LOST;
                    acc[10] += gap;
                }
            }
            episodes++;
        }
        const bool trail = ((occ >> 63) & nxt.occ & 1ull) != 0;
        if (trail) carry = run_at(63);
        open = trail;
        prev = __builtin_amdgcn_readlane(b, WAVE - 1);
        cur = nxt;
    }
    if (FILL) return;
    if (lane == 0) {
        int32_t *out = a.gt_occ + g * TO_NGT;
        out[0] = episodes;
        out[1] = frames;
        out[2] = kept;
        out[3] = gone;
        a.n_ep[g] = episodes;
    }
    const int32_t cat = a.gt_cat[g];
    if ((a.gt_flags[g] & TAOAMD_GT_IGNORE) || cat < 0 || cat >= a.n_cat) return;
    if (lane < a.n_len) {
        unsigned long long *row = a.counts + ((int64_t)cat * a.n_len + lane) * TO_NCNT;
#pragma unroll
        for (int c = 0; c < TO_NCNT; c++)
            if (acc[c]) atomicAdd(row + c, (unsigned long long)acc[c]);
    }
}

// ep_off[i] = the sum of n_ep[0 .. i), ep_off[n] the total; one workgroup.
// (The 1024-lane scan stays written out here and in CLEAR's two scan kernels.  One
// helper for the three was tried in two forms, parent and new build in turn on
// one MI355X, five runs each: with the wavefront's number taken in the helper
// this kernel took 0.0415-0.0420 ms beside 0.0337-0.0344, taken once outside
// the loop 0.0341-0.0346 beside 0.0336-0.0338; clear_scan_tile_kernel
// 0.0270-0.0274 beside 0.0215-0.0218.  Each pair is of one run; the runs differ.)
__global__ __launch_bounds__(1024) void occ_scan_kernel(const int32_t *__restrict__ n_ep,
                                                        int64_t *__restrict__ ep_off, int64_t n)
{
    __shared__ long long s_w[1024 / WAVE];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    long long carry = 0;
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + tid;
        const long long v = i < n ? n_ep[i] : 0;
        long long incl = v;
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const long long u = __shfl_up(incl, off, WAVE);
            if (lane_id() >= off) incl += u;
        }
        if (lane_id() == WAVE - 1) s_w[wave] = incl;
        __syncthreads();
        long long before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 1024 / WAVE; w++) {
            const long long t = s_w[w];
            if (w < wave) before += t;
            total += t;
        }
        if (i < n) ep_off[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();                           // s_w is read
    }
    if (tid == 0) ep_off[n] = carry;
}

// The tables of the pass, in buffer order: a function of n_gt (the frames and the
// buckets stay in registers)
static void occ_layout(Carve &c, int64_t n_gt, OccArgs &a)
{
    a.n_ep = c.take<int32_t>((size_t)n_gt);
}

static bool occ_sizes_ok(int64_t n_gt, int64_t n_gt_frames, int32_t n_len)
{
    return track_sizes_ok(0, n_gt, n_gt_frames, 0) && n_len >= 1 && n_len <= TO_LEN;
}

extern "C" size_t taoamd_track_occlusion_workspace(int64_t n_gt, int64_t n_gt_frames,
                                                   int32_t n_len)
{
    if (!occ_sizes_ok(n_gt, n_gt_frames, n_len)) return 0;
    OccArgs a;
    return measure([&](Carve &c) { occ_layout(c, n_gt, a); });
}

// What the two entry points share: the refusals and the carved workspace
static int occ_args(OccArgs &a, int64_t n_gt, int64_t n_gt_frames, int32_t n_cat, int32_t n_len,
                    int32_t recover, double vis_lo, double vis_hi, const int32_t *len_edges,
                    const int32_t *gt_cat, const uint8_t *gt_flags, const int32_t *gt_frame_off,
                    const double *gt_frame_vis, const int32_t *best, const int64_t *ep_off,
                    void *workspace, size_t workspace_bytes)
{
    if (!occ_sizes_ok(n_gt, n_gt_frames, n_len) || n_cat <= 0) return TAOAMD_ERR_ARG;
    if (recover < 1 || recover > TO_RECOVER) return TAOAMD_ERR_ARG;
    if (!(vis_lo <= vis_hi)) return TAOAMD_ERR_ARG;            // (a NaN compares false)
    if (!len_edges || len_edges[0] != 1) return TAOAMD_ERR_ARG;
    for (int i = 1; i < n_len; i++)
        if (len_edges[i] <= len_edges[i - 1]) return TAOAMD_ERR_ARG;
    if (!ep_off || !workspace) return TAOAMD_ERR_ARG;
    if (n_gt > 0 && (!gt_cat || !gt_flags || !gt_frame_off)) return TAOAMD_ERR_ARG;
    if (n_gt_frames > 0 && (!gt_frame_vis || !best)) return TAOAMD_ERR_ARG;
    Carve c(workspace);
    occ_layout(c, n_gt, a);
    if (!c.fits(workspace, workspace_bytes)) return TAOAMD_ERR_WORKSPACE;
    a.n_gt = n_gt; a.n_gt_frames = n_gt_frames;
    a.n_cat = n_cat; a.n_len = n_len; a.recover = recover;
    a.lo = vis_lo; a.hi = vis_hi;
    for (int i = 0; i < TO_LEN; i++) a.edges[i] = i < n_len ? len_edges[i] : 0x7fffffff;
    a.gt_cat = gt_cat; a.gt_flags = gt_flags; a.gfoff = gt_frame_off;
    a.gfvis = gt_frame_vis; a.best = best;
    a.gt_occ = nullptr; a.counts = nullptr;
    a.ep_off = ep_off; a.cap = 0; a.episodes = nullptr;
    return TAOAMD_OK;
}

static unsigned occ_blocks(int64_t n_gt)
{
    const int per = 256 / WAVE;
    return (unsigned)((n_gt + per - 1) / per);
}

extern "C" int taoamd_track_occlusion_count(
    int64_t n_gt, int64_t n_gt_frames, int32_t n_cat, int32_t n_len, int32_t recover,
    double vis_lo, double vis_hi, const int32_t *len_edges, const int32_t *gt_cat,
    const uint8_t *gt_flags, const int32_t *gt_frame_off, const double *gt_frame_vis,
    const int32_t *best, int32_t *gt_occ, int64_t *ep_off, int64_t *counts, void *workspace,
    size_t workspace_bytes, void *stream)
{
    OccArgs a;
    const int st = occ_args(a, n_gt, n_gt_frames, n_cat, n_len, recover, vis_lo, vis_hi,
                            len_edges, gt_cat, gt_flags, gt_frame_off, gt_frame_vis, best, ep_off,
                            workspace, workspace_bytes);
    if (st != TAOAMD_OK) return st;
    if (!counts || (n_gt > 0 && !gt_occ)) return TAOAMD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    a.gt_occ = gt_occ;
    a.counts = (unsigned long long *)counts;
    TAO_HIP(hipMemsetAsync(counts, 0, (size_t)n_cat * n_len * TO_NCNT * sizeof(int64_t), s));
    if (n_gt == 0) {
        TAO_HIP(hipMemsetAsync(ep_off, 0, sizeof(int64_t), s));
        return TAOAMD_OK;
    }
    TAO_TIMED("occ_walk_kernel", s, occ_walk_kernel<false><<<occ_blocks(n_gt), 256, 0, s>>>(a));
    TAO_TIMED("occ_scan_kernel", s, occ_scan_kernel<<<1, 1024, 0, s>>>(a.n_ep, ep_off, n_gt));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

extern "C" int taoamd_track_occlusion_fill(
    int64_t n_gt, int64_t n_gt_frames, int32_t n_cat, int32_t n_len, int32_t recover,
    double vis_lo, double vis_hi, const int32_t *len_edges, const int32_t *gt_cat,
    const uint8_t *gt_flags, const int32_t *gt_frame_off, const double *gt_frame_vis,
    const int32_t *best, const int64_t *ep_off, int64_t cap, int32_t *episodes, void *workspace,
    size_t workspace_bytes, void *stream)
{
    OccArgs a;
    if (cap < 0) return TAOAMD_ERR_ARG;
    const int st = occ_args(a, n_gt, n_gt_frames, n_cat, n_len, recover, vis_lo, vis_hi,
                            len_edges, gt_cat, gt_flags, gt_frame_off, gt_frame_vis, best, ep_off,
                            workspace, workspace_bytes);
    if (st != TAOAMD_OK) return st;
    if (cap > 0 && !episodes) return TAOAMD_ERR_ARG;
    if (n_gt == 0 || n_gt_frames == 0 || cap == 0) return TAOAMD_OK;   // no episode to store
    hipStream_t s = (hipStream_t)stream;
    a.cap = cap;
    a.episodes = episodes;
    TAO_TIMED("occ_fill_kernel", s, occ_walk_kernel<true><<<occ_blocks(n_gt), 256, 0, s>>>(a));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

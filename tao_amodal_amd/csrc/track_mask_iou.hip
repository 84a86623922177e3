// 3D mask IoU of track pairs: TaoEval(iou_type="segm").  The reference names
// the metric -- compute_track_box_iou / compute_avg_track_iou are "modified
// from YTVIS evaluation" (T/eval.py:73-117, ytvoseval.py) -- but never runs it
// for masks (T/eval.py:173-176,306-335: Tao has no ann_to_rle, and compute_iou
// would hand RLE dicts to bb_intersect_union).  The definition below is this project's,
// restated in tests/track_segm_ref.py:
//
// A track maps timeline positions to masks.  For a shared position t of the
// detection track d and the GT track g, i_t = |d_t & g_t| and u_t = |d_t | g_t|
// as the areas of pycocotools' merge give them: both 0 when the two frame sizes
// differ, and both counted only up to the pixel at which rleMerge's loop stops
// (the frame's end, or earlier on coincident empty runs / 2^32 pixels left in
// two runs: rle_walk.hpp).  Then
//   3d_iou:      sum_shared i_t / (sum_shared u_t + pixels of d's frames g lacks
//                + pixels of g's frames d lacks), integers summed exactly;
//   avg_iou:     (sum over shared t, ascending, of i_t / u_t) / |F_d u F_g|;
//   imagenetvid: #{shared t : i_t > u_t / 2} / |F_d u F_g|.
//
// One wavefront per track pair.  Its lanes first sum the pixel counts of both
// tracks' frames, then take the detection's frames 64 at a time and look each
// up in the GT track's sorted positions (binary search); the shared frames of a
// ballot are taken in ascending order and for each the whole wavefront forms
// i_t: the frame sizes and the masks' column spans settle many of them (u_t =
// 0, or i_t = 0), the rest walk the runs as in rle_iou.hip (a lane owns RLE_RPT
// consecutive run boundaries of the detection's mask and merges them against
// the ground truth's (E, P) prefix table: rle_walk.hpp); a pair on which the
// reference's loop may stop early is then walked with its two cursors, also
// where a shortcut has settled it (they assume that every pixel counts).
// Every lane ends a
// frame with the same i_t, so the per-pair sums are wavefront-uniform and the
// ratios of avg_iou are added in timeline order -- no item list, no second
// pass and no workspace beyond the per-mask prefix sums.
#include "rle_walk.hpp"

using namespace taoamd;

#define TMI_THREADS 256         // 4 wavefronts, one track pair each
#define TMI_MAX_BLOCKS 16384    // grid-stride beyond this

struct TrackMaskArgs {
    int64_t n_cells, n_pairs;
    const int32_t *cell_dt_off, *cell_gt_off;
    const int64_t *cell_iou_off;
    const int32_t *dt_frame_off, *dt_frame_pos, *gt_frame_off, *gt_frame_pos;
    const int64_t *dt_off, *gt_off;           // CSR of the run lists, one mask per frame
    const int32_t *dt_hw, *gt_hw;             // (height, width) per mask
    const uint32_t *dt_runs, *gt_runs;        // the run lengths themselves
    const uint32_t *dt_end;                   // E per run of the detections' masks
    const uint2 *gt_pre;                      // (E, P) per run of the GT masks
    const uint32_t *dt_ones, *gt_ones;        // ones per mask
    int32_t mode;
    double *iou;
    unsigned long long *pair_frames;
};

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v)
{
#pragma unroll
    for (int s = WAVE / 2; s > 0; s >>= 1) v += __shfl_xor(v, s, WAVE);
    return v;
}

// |A & B| of detection mask fa and GT mask fb of the same frame size, by the
// whole wavefront (every lane returns it)
__device__ __forceinline__ uint32_t mask_inter(const TrackMaskArgs &a, int lane,
                                               int64_t fa, int64_t fb)
{
    const int64_t ab = a.dt_off[fa], bb = a.gt_off[fb];
    const uint32_t ka = (uint32_t)(a.dt_off[fa + 1] - ab);
    const uint32_t kb = (uint32_t)(a.gt_off[fb + 1] - bb);
    const uint32_t n_pieces = (ka + RLE_RPT * WAVE - 1) / (RLE_RPT * WAVE);
    uint32_t xq[RLE_RPT];
    bool use[RLE_RPT];
    uint32_t acc = 0;
    for (uint32_t piece = 0; piece < n_pieces; piece++) {
        rle_load_piece(piece, lane, a.dt_end + ab, ka, xq, use);
        rle_lane_walk(xq, use, a.gt_pre + bb, kb, a.gt_ones[fb], acc);
    }
#pragma unroll
    for (int s = WAVE / 2; s > 0; s >>= 1) acc += __shfl_xor(acc, s, WAVE);
    return acc;
}

// Whether the column spans of two non-empty masks of height h meet.  A mask's
// ones lie between the start of its first run of ones (E[0]) and the end of
// its last one (E of its last odd-numbered run) -- column-major, so those
// bound its columns exactly.  (The tight boxes of taoamd_rle_copy cannot serve
// here: rleToBbox of the reference's pycocotools takes a run of ones that
// crosses a column for one row, so such a box can miss pixels of the mask --
// harmless to rleIou, which answers 0 for such pairs itself, but not to an
// exact intersection.)
__device__ __forceinline__ bool columns_meet(const TrackMaskArgs &a, int64_t fa,
                                             int64_t fb, uint32_t h)
{
    const int64_t ab = a.dt_off[fa], bb = a.gt_off[fb];
    const int64_t ka = a.dt_off[fa + 1] - ab, kb = a.gt_off[fb + 1] - bb;
    const uint32_t a0 = a.dt_end[ab] / h, a1 = (a.dt_end[ab + ((ka & 1) ? ka - 2 : ka - 1)] - 1) / h;
    const uint32_t b0 = a.gt_pre[bb].x / h, b1 = (a.gt_pre[bb + ((kb & 1) ? kb - 2 : kb - 1)].x - 1) / h;
    return max(a0, b0) <= min(a1, b1);
}

__global__ __launch_bounds__(TMI_THREADS) void track_mask_iou_kernel(TrackMaskArgs a)
{
    const int lane = lane_id();
    const int64_t n_waves = (int64_t)gridDim.x * (TMI_THREADS / WAVE);
    for (int64_t p = (int64_t)blockIdx.x * (TMI_THREADS / WAVE) + (threadIdx.x >> 6);
         p < a.n_pairs; p += n_waves) {
        // the pair's cell: the last c with cell_iou_off[c] <= p (empty cells
        // share their offset with the next one)
        int64_t lo = 0, hi = a.n_cells;
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.cell_iou_off[mid] <= p) lo = mid; else hi = mid;
        }
        const int32_t g0 = a.cell_gt_off[lo];
        const int64_t G = a.cell_gt_off[lo + 1] - g0;
        const int64_t local = p - a.cell_iou_off[lo];
        if (G <= 0 || local >= (int64_t)(a.cell_dt_off[lo + 1] - a.cell_dt_off[lo]) * G)
            continue;                   // (n_pairs beyond cell_iou_off[n_cells])
        const int32_t d = a.cell_dt_off[lo] + (int32_t)(local / G);
        const int32_t g = g0 + (int32_t)(local % G);
        const int32_t fd0 = a.dt_frame_off[d], nd = a.dt_frame_off[d + 1] - fd0;
        const int32_t fg0 = a.gt_frame_off[g], ng = a.gt_frame_off[g + 1] - fg0;
        // pixels of every frame of both tracks
        uint64_t tot = 0;
        for (int32_t i = lane; i < nd; i += WAVE) tot += a.dt_ones[fd0 + i];
        for (int32_t i = lane; i < ng; i += WAVE) tot += a.gt_ones[fg0 + i];
        tot = wave_sum_u64(tot);
        // over the shared frames: I = sum i_t, gone = sum (|d_t| + |g_t| - u_t)
        // (so that U = tot - gone), the ordered ratio sum and the hits
        uint64_t I = 0, gone = 0;
        uint32_t shared = 0, hits = 0;
        double ratios = 0.0;
        const int32_t *__restrict__ gpos = a.gt_frame_pos + fg0;
        for (int32_t base = 0; base < nd; base += WAVE) {
            const int32_t i = base + lane;
            int32_t at = 0;
            bool has = false;
            if (i < nd && ng > 0) {
                const int32_t x = a.dt_frame_pos[fd0 + i];
                int32_t l = 0, h = ng;          // first GT position >= x
                while (l < h) {
                    const int32_t m = (l + h) >> 1;
                    if (gpos[m] < x) l = m + 1; else h = m;
                }
                at = l;
                has = l < ng && gpos[l] == x;
            }
            for (uint64_t live = __ballot(has); live != 0; live &= live - 1) {
                const int src = __builtin_ctzll(live);
                const int64_t fa = fd0 + base + src;
                const int64_t fb = fg0 + __shfl(at, src, WAVE);
                const uint32_t ones_a = a.dt_ones[fa], ones_b = a.gt_ones[fb];
                uint32_t inter = 0;
                uint64_t uni = 0;
                const int32_t h = a.dt_hw[2 * fa];
                if (h == a.gt_hw[2 * fb] && a.dt_hw[2 * fa + 1] == a.gt_hw[2 * fb + 1]) {
                    // (an empty mask is never walked: both run lists of a
                    // walk hold a run of ones, and h > 0)
                    if (h > 0 && ones_a != 0 && ones_b != 0 && columns_meet(a, fa, fb, (uint32_t)h))
                        inter = mask_inter(a, lane, fa, fb);
                    uni = (uint64_t)ones_a + ones_b - inter;
                    // the rare pair on which the reference stops early takes
                    // its two cursors instead, whatever the shortcuts said (they
                    // assume that every pixel counts)
                    const int64_t bb = a.gt_off[fb];
                    const uint32_t kb = (uint32_t)(a.gt_off[fb + 1] - bb);
                    const uint32_t b_flag = kb ? a.gt_pre[bb].y : 0u;
                    const bool rare = b_flag != 0 || rle_big_frame(h, a.dt_hw[2 * fa + 1]);
                    if (__builtin_expect(rare, 0) && kb) {
                        const int64_t ab = a.dt_off[fa];
                        const uint32_t ka = (uint32_t)(a.dt_off[fa + 1] - ab);
                        if (ka && rle_stops_early(lane, a.dt_runs + ab, ka, a.gt_runs + bb, kb,
                                                  b_flag)) {
                            uint32_t u32;
                            rle_two_cursors(a.dt_runs + ab, ka, a.gt_runs + bb, kb, inter, u32);
                            uni = u32;
                        }
                    }
                }
                shared++;
                I += inter;
                gone += (uint64_t)ones_a + ones_b - uni;
                if (a.mode == 1) ratios += uni != 0 ? (double)inter / (double)uni : 0.0;
                else if (a.mode == 2) hits += 2 * (uint64_t)inter > uni;
            }
        }
        const int64_t n_union = (int64_t)nd + ng - shared;
        double v;
        if (a.mode == 0) {
            const uint64_t U = tot - gone;
            v = U != 0 ? (double)I / (double)U : 0.0;
        } else if (a.mode == 1) {
            v = n_union != 0 ? ratios / (double)n_union : 0.0;
        } else {
            v = n_union != 0 ? (double)hits / (double)n_union : 0.0;
        }
        if (lane == 0) {
            a.iou[p] = v;
            if (a.pair_frames != nullptr && shared) atomicAdd(a.pair_frames, shared);
        }
    }
}

extern "C" size_t taoamd_track_mask_iou_workspace(int64_t dt_frames, int64_t dt_total,
                                                  int64_t gt_frames, int64_t gt_total)
{
    TrackMaskArgs a;
    return measure([&](Carve &c) { rle_layout(c, dt_frames, dt_total, gt_frames, gt_total, a); });
}

extern "C" int taoamd_track_mask_iou(
    int64_t n_cells, const int32_t *cell_dt_off, const int32_t *cell_gt_off,
    const int64_t *cell_iou_off, int64_t n_pairs, const int32_t *dt_frame_off,
    const int32_t *dt_frame_pos, int64_t dt_frames, int64_t dt_total,
    const int64_t *dt_off, const uint32_t *dt_runs, const int32_t *dt_hw,
    const int32_t *gt_frame_off, const int32_t *gt_frame_pos, int64_t gt_frames,
    int64_t gt_total, const int64_t *gt_off, const uint32_t *gt_runs,
    const int32_t *gt_hw, int32_t mode, double *iou, int64_t *pair_frames, void *workspace,
    size_t workspace_bytes, void *stream)
{
    if (n_cells < 0 || n_pairs < 0 || dt_frames < 0 || dt_total < 0 ||
        gt_frames < 0 || gt_total < 0 || mode < 0 || mode > 2)
        return TAOAMD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (pair_frames) TAO_HIP(hipMemsetAsync(pair_frames, 0, 8, s));
    if (n_cells == 0 || n_pairs == 0) return TAOAMD_OK;
    if (!cell_dt_off || !cell_gt_off || !cell_iou_off || !dt_frame_off ||
        !dt_frame_pos || !gt_frame_off || !gt_frame_pos || !dt_off || !dt_runs ||
        !dt_hw || !gt_off || !gt_runs || !gt_hw || !iou ||
        !workspace)
        return TAOAMD_ERR_ARG;
    Carve c(workspace);
    TrackMaskArgs a;
    rle_layout(c, dt_frames, dt_total, gt_frames, gt_total, a);
    if (!c.fits(workspace, workspace_bytes)) return TAOAMD_ERR_WORKSPACE;
    if (dt_frames)
        TAO_TIMED("rle_prefix_kernel", s, rle_prefix_kernel<false><<<dim3((unsigned)((dt_frames + 3) / 4)), 256, 0, s>>>(
            dt_frames, dt_off, dt_runs, (void *)a.dt_end, (uint32_t *)a.dt_ones));
    TAO_LAUNCH_CHECK();
    if (gt_frames)
        TAO_TIMED("rle_prefix_kernel", s, rle_prefix_kernel<true><<<dim3((unsigned)((gt_frames + 3) / 4)), 256, 0, s>>>(
            gt_frames, gt_off, gt_runs, (void *)a.gt_pre, (uint32_t *)a.gt_ones));
    TAO_LAUNCH_CHECK();
    a.n_cells = n_cells; a.n_pairs = n_pairs;
    a.cell_dt_off = cell_dt_off; a.cell_gt_off = cell_gt_off;
    a.cell_iou_off = cell_iou_off;
    a.dt_frame_off = dt_frame_off; a.dt_frame_pos = dt_frame_pos;
    a.gt_frame_off = gt_frame_off; a.gt_frame_pos = gt_frame_pos;
    a.dt_off = dt_off; a.gt_off = gt_off;
    a.dt_runs = dt_runs; a.gt_runs = gt_runs;
    a.dt_hw = dt_hw; a.gt_hw = gt_hw;
    a.mode = mode;
    a.iou = iou;
    a.pair_frames = (unsigned long long *)pair_frames;
    const int64_t blocks = (n_pairs + TMI_THREADS / WAVE - 1) / (TMI_THREADS / WAVE);
    TAO_TIMED("track_mask_iou_kernel", s, track_mask_iou_kernel<<<dim3((unsigned)(
        blocks < TMI_MAX_BLOCKS ? blocks : TMI_MAX_BLOCKS)), TMI_THREADS, 0, s>>>(a));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

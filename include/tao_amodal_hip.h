/*
 * tao_amodal_hip.h -- C ABI of the MI355X (gfx950) evaluation hot path.
 *
 * This is the drop-in boundary for the path the reference runs in
 * tools/eval_on_tao_amodal.py (LVISEval + TaoEval).  The reference has exactly
 * one native seam on that path, pycocotools' bbIou; everything else is Python
 * that this library replaces with batched device kernels over flattened cell
 * tables.  Every entry point is extern "C", takes plain pointers and sizes,
 * returns an int status (0 = ok, see taoamd_strerror) and never throws.  All
 * pointers are DEVICE pointers unless the name ends in _host; the caller owns
 * every buffer; `stream` is a hipStream_t passed as void* (NULL = default
 * stream).  Calls are asynchronous on `stream` unless stated otherwise.  One
 * host thread per device.
 *
 * Reference interfaces replaced (paths relative to /root/reference;
 * L/ = tao_amodal/evaluation/lvis_amodal/, T/ = tao_amodal/evaluation/
 * tao_amodal/, C/ = visualization/tao/third_party/pysot/training_dataset/
 * coco/pycocotools/common/):
 *
 *   taoamd_bb_iou[_host]   void bbIou(BB dt, BB gt, siz m, siz n, byte
 *                          *iscrowd, double *o)            C/maskApi.h:41-42,
 *                          C/maskApi.c:109-120, called at L/eval.py:191
 *   taoamd_lvis_ranges     LVISEval.evaluate_img, GT _ignore per visibility
 *                          range + dt_ig_mask              L/eval.py:202-217,
 *                                                          281-288
 *   taoamd_tao_ranges      TaoEval.evaluate_vid, the same for 5 area x 4
 *                          duration ranges                 T/eval.py:348-368,
 *                                                          432-441
 *   taoamd_track_iou       TaoEval.compute_iou / compute_track_box_iou /
 *                          bb_intersect_union              T/eval.py:15-48,
 *                                                          73-96,306-335
 *   taoamd_match           LVISEval.compute_iou + evaluate_img greedy loop,
 *                          TaoEval.evaluate_vid greedy loop
 *                                                          L/eval.py:168-192,
 *                                                          219-290;
 *                                                          T/eval.py:370-443
 *   taoamd_sort_by_cat_score  np.argsort(-dt_scores, kind="mergesort") per
 *                          category                        L/eval.py:353-361,
 *                                                          T/eval.py:508-518
 *   taoamd_accumulate      LVISEval.accumulate / TaoEval.accumulate
 *                                                          L/eval.py:339-426,
 *                                                          T/eval.py:496-584
 *
 * Data model ("cell tables", built by tao_amodal_amd/flatten.py):
 *   a cell = one (image, category) [LVIS] or (video, category) [TAO] pair that
 *   has at least one detection or ground truth.  Detections (LVIS) / detection
 *   tracks (TAO) of a cell are contiguous and sorted by descending score
 *   (stable); ground truths are contiguous in the reference's visiting order.
 *   cell_dt_off / cell_gt_off are CSR offsets (int32, n_cells + 1 entries).
 *
 *   A "combo" is one (range r, IoU threshold t) pair, combo = r*10 + t;
 *   n_rng = 6 (LVIS visibility ranges) or 20 (TAO area x duration, r = a*4+t_).
 *   Per detection the kernels emit n_words = ceil(n_rng*10/64) 64-bit words
 *   of `matched` bits and of `ignored` bits (bit combo%64 of word combo/64):
 *     TP = matched & ~ignored, FP = ~matched & ~ignored.
 */
#ifndef TAO_AMODAL_HIP_H
#define TAO_AMODAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TAOAMD_N_THR 10   /* IoU thresholds 0.50:0.05:0.95 */
#define TAOAMD_N_REC 101  /* recall thresholds 0:0.01:1 */
#define TAOAMD_LVIS_RNG 6
#define TAOAMD_TAO_RNG 20

/* per-ground-truth flag bits */
#define TAOAMD_GT_IGNORE 1     /* truthy "ignore" field */
#define TAOAMD_GT_OOF 2        /* annotation is out_of_frame (LVIS side) */
#define TAOAMD_GT_ID_HIDDEN 4  /* id equals the "unmatched" sentinel (0 / -1) */
/* per-detection flag bits */
#define TAOAMD_DT_IGNORE_UNMATCHED 1 /* not-exhaustive category / area window */
#define TAOAMD_DT_NO_CONSUME 2       /* id <= 0: a match leaves the GT free */

/* status codes */
#define TAOAMD_OK 0
#define TAOAMD_ERR_HIP 1         /* a HIP runtime call failed */
#define TAOAMD_ERR_ARG 2         /* bad argument */
#define TAOAMD_ERR_TOO_LARGE 3   /* a cell exceeds a kernel limit */
#define TAOAMD_ERR_WORKSPACE 4   /* workspace_bytes below what taoamd_*_workspace() reports */
#define TAOAMD_JSON_FALLBACK 16  /* taoamd_json_pred_open: the host reader should take the file */

const char *taoamd_strerror(int status);
/* text of the last failing HIP call on this thread ("" if none) */
const char *taoamd_last_error(void);
int taoamd_version(void);

/* Per-kernel timing for bench.py's roofline: while enabled, every kernel the
 * library launches is bracketed by two HIP events recorded on the stream it
 * is launched on (costs two event records per launch; off by default).
 * taoamd_kernel_timing_collect waits for the recorded events, adds up the
 * launch durations by kernel name and forgets them: names = NUL-separated
 * list in launch order of first appearance, total_ms / calls per name;
 * *n_kernels = number of distinct names.  A call always consumes the records
 * (give room for 64 names).  Host pointers; synchronous. */
int taoamd_kernel_timing_enable(int on);
/* prefix ("label:") of the names recorded by this thread from now on, e.g. the
 * evaluator a pass belongs to; NULL or "" = none */
int taoamd_kernel_timing_label(const char *label);
int taoamd_kernel_timing_collect(char *names_host, size_t names_bytes,
                                 double *total_ms_host, int64_t *calls_host,
                                 int32_t max_kernels, int32_t *n_kernels_host);

/* Exact bit patterns of np.linspace(.5,.95,10) / np.linspace(0,1,101)
 * (L/eval.py:560-565).  Host pointers. */
int taoamd_thresholds_host(double *iou_thrs, double *rec_thrs);

/* The evaluation constants a caller of the class API may edit before run()
 * (`params.iou_thrs`, `rec_thrs`: L/eval.py:234,319-322,407, T/eval.py:385,
 * 473-477,562; `visibility_rng`: L/eval.py:143,205; `area_rng` / `time_rng`:
 * T/eval.py:272-275,348-368,432-441).  They reach the kernels as by-value
 * arguments; these two calls replace the CALLING THREAD's tables for its later
 * launches (NULL = the reference's default for that table).  The counts are
 * the kernels': TAOAMD_N_THR thresholds, TAOAMD_N_REC recall thresholds -- both
 * ASCENDING (equal neighbours allowed; a caller with fewer pads with copies of
 * its last value, one with more or in another order runs blocks and permutes:
 * evaluation/_core.py), else TAOAMD_ERR_ARG --, 5 visibility ranges (the sixth
 * range of the image level is the out-of-frame one and has no bounds), 5 area
 * ranges (the last one is the occlusion range: T/eval.py:272) and 4 duration
 * ranges, each as {lo, hi} pairs, bounds inclusive.  Host pointers. */
int taoamd_set_thresholds(const double *iou_thrs, const double *rec_thrs);
int taoamd_set_ranges(const double *visibility_rng, const double *area_rng,
                      const double *time_rng);

/* ---- bbIou ---------------------------------------------------------------
 * o[g*m + d] = IoU(dt[d], gt[g]); boxes are x,y,w,h doubles.  iscrowd may be
 * NULL (all zero); a non-zero entry selects u = area(dt) as in bbIou. */
int taoamd_bb_iou(const double *dt, const double *gt, size_t m, size_t n,
                  const unsigned char *iscrowd, double *o, void *stream);
/* same, host pointers in and out (allocates, copies, synchronises) */
int taoamd_bb_iou_host(const double *dt, const double *gt, size_t m, size_t n,
                       const unsigned char *iscrowd, double *o);

/* ---- range masks ------------------------------------------------------------
 * gt_rng[g] bit r: GT g is ignored in range r.  dt_rng[d] bit r: detection d
 * is ignored in range r when it ends up unmatched.  num_gt[k*n_rng + r]
 * (int32, written by the call) counts the evaluated GTs of category k.
 * gt_cat_off (optional, int32[n_cat+1], device): when the GTs are grouped by
 * category (category-major cell tables) the counts are formed by one
 * wavefront per category with ballots -- no atomics; NULL selects the
 * atomicAdd histogram over gt_cat.
 * Image level: a detection's mask is "every range" iff TAOAMD_DT_IGNORE_UNMATCHED
 * is set in dt_flags and 0 otherwise, so the table is optional -- dt_rng NULL in
 * taoamd_lvis_ranges skips it, dt_rng NULL in taoamd_match derives the mask
 * from dt_flags (240 MB less traffic per pass at 30 M detections). */
int taoamd_lvis_ranges(int64_t n_gt, const double *gt_vis,
                       const uint8_t *gt_flags, const int32_t *gt_cat,
                       const int32_t *gt_cat_off, int64_t n_dt,
                       const uint8_t *dt_flags, int32_t n_cat,
                       uint32_t *gt_rng, uint32_t *dt_rng, int32_t *num_gt,
                       void *stream);
int taoamd_tao_ranges(int64_t n_gt, const double *gt_area,
                      const int32_t *gt_len, const int32_t *gt_nhp,
                      const uint8_t *gt_flags, const int32_t *gt_cat,
                      const int32_t *gt_cat_off, int64_t n_dt,
                      const double *dt_area, const int32_t *dt_len,
                      const uint8_t *dt_flags, int32_t n_cat,
                      uint32_t *gt_rng, uint32_t *dt_rng, int32_t *num_gt,
                      void *stream);

/* ---- IoU of run-length masks (iou_type="segm") -------------------------------
 * iou[cell_iou_off[c] + d*G + g] for every cell c, iscrowd = 0: replaces
 * mask_utils.iou(dt, gt, iscrowd) on RLE objects (L/eval.py:179-191 ->
 * C/maskApi.c rleIou:77-96).  Masks are CSR run lists (column-major run
 * lengths, zeros first) with their frame size hw[n][2] = (height, width) and
 * tight box bb[n][4] = (x, y, w, h) as taoamd_rle_copy (tao_amodal_ingest.h)
 * produces them; row i belongs to detection / ground truth i of the cell
 * tables (n_dt / n_gt rows, dt_total / gt_total runs in all).  0 where the
 * tight boxes do not overlap, -1 where the frames differ, else |d & g| / |d | g|
 * (an empty intersection over a union of 1), both counted as rleIou's loop
 * counts them: up to the frame's end, or up to the pixel at which both masks
 * finish a run and continue with an empty one, or at which the two current
 * runs have 2^32 pixels left between them -- the reference stops there.  Run
 * lengths of a mask add up to its height * width, less than 2^32.  The two masks of a pair with one
 * frame size must add up to the same total: on unequal totals the reference's
 * loop never returns, and the value here is unspecified.  Workspace:
 * taoamd_rle_iou_workspace(n_dt, dt_total, n_gt, gt_total) bytes (per-run
 * prefix sums, rebuilt by every call). */
size_t taoamd_rle_iou_workspace(int64_t n_dt, int64_t dt_total, int64_t n_gt,
                                int64_t gt_total);
int taoamd_rle_iou(int64_t n_cells, const int32_t *cell_dt_off,
                   const int32_t *cell_gt_off, const int64_t *cell_iou_off,
                   int64_t n_dt, int64_t dt_total, const int64_t *dt_off,
                   const uint32_t *dt_runs, const int32_t *dt_hw,
                   const double *dt_bb, int64_t n_gt, int64_t gt_total,
                   const int64_t *gt_off, const uint32_t *gt_runs,
                   const int32_t *gt_hw, const double *gt_bb, double *iou,
                   void *workspace, size_t workspace_bytes, void *stream);

/* ---- 3D IoU of mask tracks (TaoEval iou_type="segm") ------------------------
 * iou[cell_iou_off[c] + d*G + g] for every cell c, from run-length masks instead
 * of boxes: replaces compute_iou's three track functions (T/eval.py:51-117,
 * 306-335) for the "segmentation" annotation type, a path the reference cannot
 * run (Tao has no ann_to_rle, T/eval.py:173-176).  Tracks are CSR lists of
 * timeline positions sorted ascending (*_frame_off[n_trk + 1],
 * *_frame_pos[*_frames]); frame k of a side has mask k of that side (CSR run
 * lists *_off / *_runs and frame size *_hw[k] = (height, width), as
 * taoamd_rle_copy produces them; no tight box: see the kernel).  Per shared
 * position t: i_t = |d_t & g_t|, u_t = |d_t | g_t|, both 0 when the frame sizes
 * differ, both counted up to the pixel where rleMerge's loop stops (as for
 * taoamd_rle_iou, same domain).  mode 0 = 3d_iou: sum i_t / (sum u_t + the pixels of the frames only
 * one track has), integers summed exactly, 0 when the denominator is 0;
 * 1 = avg_iou: the ratios i_t / u_t (0 where u_t = 0) added in ascending
 * timeline order, over |F_d u F_g|; 2 = imagenetvid: #{t : i_t > u_t / 2} over
 * |F_d u F_g|.  n_pairs = cell_iou_off[n_cells].  pair_frames (optional,
 * int64[1], zeroed by the call) receives the number of shared (pair, frame)
 * items.  Workspace: taoamd_track_mask_iou_workspace(dt_frames, dt_total,
 * gt_frames, gt_total) bytes (per-run prefix sums, rebuilt by every call). */
size_t taoamd_track_mask_iou_workspace(int64_t dt_frames, int64_t dt_total,
                                       int64_t gt_frames, int64_t gt_total);
int taoamd_track_mask_iou(int64_t n_cells, const int32_t *cell_dt_off,
                          const int32_t *cell_gt_off, const int64_t *cell_iou_off,
                          int64_t n_pairs, const int32_t *dt_frame_off,
                          const int32_t *dt_frame_pos, int64_t dt_frames,
                          int64_t dt_total, const int64_t *dt_off,
                          const uint32_t *dt_runs, const int32_t *dt_hw,
                          const int32_t *gt_frame_off,
                          const int32_t *gt_frame_pos, int64_t gt_frames,
                          int64_t gt_total, const int64_t *gt_off,
                          const uint32_t *gt_runs, const int32_t *gt_hw,
                          int32_t mode, double *iou,
                          int64_t *pair_frames, void *workspace,
                          size_t workspace_bytes, void *stream);

/* ---- 3D IoU of track pairs --------------------------------------------------
 * iou[cell_iou_off[c] + d*G + g] for every cell c (G = its GT track count).
 * Tracks are CSR lists of (timeline position, box) sorted by position.
 * pair_frames (optional, int64[1], zeroed by the call) receives the number of
 * same-frame box pairs evaluated (the unit of BASELINE.json's metric).
 * mode: 0 = 3d_iou (sum inter / sum union, the CLI's), 1 = avg_iou (mean of
 * the per-frame IoU over the union of frames, T/eval.py:99-117), 2 =
 * imagenetvid (fraction of frames with inter > 0.5 union, T/eval.py:51-70).
 *
 * taoamd_track_iou is the plan-less form: one lane per track pair walks the two
 * CSR lists with a two-pointer merge (slow; any input).
 *
 * taoamd_track_iou_planned is the fast form.  It follows a launch plan built
 * by taoamd_track_iou_plan_host, one workgroup per task:
 *   tasks      int32[n_tasks][4] {first row, rows (<= 32), first pair, pairs (<= 64)}
 *   task_rows  int32  the tasks' tracks: t for detection track t, n_dt + t for
 *              GT track t (= the row of trk_meta)
 *   task_pairs int32  detection row | GT row << 8 (rows local to the task)
 *   task_out   int64  index of the pair's result in `iou`
 * and reads the tracks' frames from the tasks' FRAME STREAM (taoamd_track_stream):
 *   frames     double[n_pieces * 8][4]  pieces of 8 consecutive timeline
 *              positions (one 256-byte piece = 8 boxes x, y, w, h; the far box
 *              where the track has no frame), in the order the tasks consume
 *              them: task by task, chunk by chunk of the task's timeline, the
 *              rows whose span reaches into the chunk in row order; piece 0 is
 *              eight far boxes
 *   task_base  int32[n_tasks]  a task's first piece
 * A task stages its tracks' frames in LDS chunk by chunk of the timeline and
 * adds the per-frame terms in ascending timeline order, one lane per pair.
 *   zero_out   int64[n_zero]  the zero list of taoamd_track_iou_plan_spans_host:
 *              places in `iou` that receive +0.0 (pairs without a common
 *              timeline position, which that plan keeps out of the tasks).
 *              They are stored by workgroups of the same launch, behind the
 *              tasks', in every call: a pass defines every entry of `iou` that
 *              the tasks and the zero list name, whatever the buffer held.
 *              n_zero = 0, zero_out = NULL: the tasks alone (the plan of
 *              taoamd_track_iou_plan_host, whose tasks hold every pair).
 *              n_tasks = 0 with n_zero > 0 stores the zeros alone.
 * Both forms give bit-identical results. */
int taoamd_track_iou(int64_t n_cells, const int32_t *cell_dt_off,
                     const int32_t *cell_gt_off, const int64_t *cell_iou_off,
                     int64_t n_pairs, const int32_t *dt_frame_off,
                     const int32_t *dt_frame_pos, const double *dt_frame_box,
                     const int32_t *gt_frame_off, const int32_t *gt_frame_pos,
                     const double *gt_frame_box, int32_t mode, double *iou,
                     int64_t *pair_frames, void *stream);
int taoamd_track_iou_planned(int64_t n_tasks, const int32_t *tasks,
                             const int32_t *task_rows, const int32_t *task_pairs,
                             const int64_t *task_out, const double *frames,
                             const int32_t *task_base, const int32_t *trk_meta,
                             int32_t mode, double *iou, int64_t *pair_frames,
                             int64_t n_zero, const int64_t *zero_out,
                             void *stream);

/* The same IoUs when EVERY detection and ground-truth track has exactly one
 * frame (frame k of the lists = the frame of track k): a pair is one box IoU
 * if the two frames are the same timeline position, else 0 -- a single term,
 * so the value does not depend on any order of summation.  dt_group
 * (int32[n_dt][4], device) = {first GT track of the detection's cell, GT
 * tracks of the cell, the detection's place in its cell, the cell}. */
int taoamd_track_iou_single(int64_t n_dt, const int32_t *dt_group,
                            const int64_t *cell_iou_off, const int32_t *dt_frame_pos,
                            const double *dt_frame_box, const int32_t *gt_frame_pos,
                            const double *gt_frame_box, int32_t mode, double *iou,
                            int64_t *pair_frames, void *stream);

/* Padded frame table of a set of CSR tracks: track t owns the slots
 * meta[t].base_minus_first + p for p = first .. last (its first and last
 * timeline position); a slot holds the frame's box (x, y, w, h) or, where the
 * track has no frame, the far box (1e300, 1e300, 0, 0), against which every
 * intersection is exactly 0.  meta (int32[n_trk][4], device, filled by the
 * caller) = {first, last, base - first, 1 for a detection track / 0 for GT}; a
 * track without frames has first > last.  The call fills the slots
 * [slot_first, slot_first + n_slots) of `padded` (double[.][4]) with far boxes
 * and then scatters the n_frames frames.  One call per track set (detections,
 * ground truth) into disjoint slot ranges of ONE table whose slot 0 is a far
 * box (reserve it: slot_first = 0 for the first set, its tracks based at 1).
 * `inexact` (optional, int32[1], zeroed by the caller) collects two flags.
 * Bit 0 is set when some box has a coordinate that is not an integer below
 * 2^20 -- with none the per-frame products and their sums are exact and
 * taoamd_track_iou_near has nothing to do.  Bit 1 is set when some box has an
 * x, y, x + w or y + h that is not a finite number of magnitude below 1e300 (a
 * NaN or an infinity sets it): the far box is an in-band sentinel, so
 * taoamd_track_iou_planned is defined only for tables that leave bit 1 clear;
 * a table that sets it goes to taoamd_track_iou, which takes any double. */
int taoamd_track_pad(int64_t n_trk, int64_t n_frames, const int32_t *frame_off,
                     const int32_t *frame_pos, const double *frame_box,
                     const int32_t *meta, int64_t slot_first, int64_t n_slots,
                     double *padded, int32_t *inexact, void *stream);

/* Frame stream of a launch plan (once per problem): the padded table's frames
 * rearranged into the order taoamd_track_iou_planned's tasks read them, so that
 * what a task requests for one chunk of its timeline is ONE contiguous stretch
 * of memory instead of 32 pieces scattered over the padded table.  A task's
 * chunks are the 8-position windows [8 c, 8 c + 8) from its earliest first to
 * its latest last position; row r of the task (rows in task_rows order, with
 * first <= last) owns a piece in every chunk its span first .. last reaches
 * into.  task_base[t] (int32, device, filled by the caller) = 1 + the pieces
 * of the tasks before t, where a task's pieces = the sum over its rows of
 * (last >> 3) - (first >> 3) + 1; `frames` holds 1 + the pieces of all tasks,
 * 256 bytes each, and a margin of 64 more pieces' bytes behind them (read, never
 * used, by taoamd_track_iou_planned).  Reads tasks, task_rows, trk_meta and the padded table
 * (which may be released afterwards). */
int taoamd_track_stream(int64_t n_tasks, const int32_t *tasks,
                        const int32_t *task_rows, const int32_t *trk_meta,
                        const int32_t *task_base, const double *padded,
                        double *frames, void *stream);

/* Guard of the documented frame-order deviation (frames are added in timeline
 * order; the reference adds them in CPython set order, T/eval.py:83-94): lists
 * the pairs whose IoU lies within max_ulp units in the last place of one of the
 * ten IoU thresholds or of another ground truth's IoU in the same row -- the
 * comparisons of the greedy match that a last-bit difference could flip.
 * *count = number of such pairs (zeroed by the call), list[0 .. min(count,
 * capacity)) = their indices into `iou`.  max_ulp must bound the reordering
 * error: adding n non-negative fp64 terms in two different orders moves a sum
 * by at most 2 (n - 1) units of roundoff, a quotient of two such sums by at
 * most 4 n - 2 units in the last place; callers pass 8 (n_dt + n_gt) + 8 for
 * the longest tracks (two rivals move independently).  The listed pairs are
 * recomputed in the reference's order by taoamd_track_iou_setorder. */
int taoamd_track_iou_near(int64_t n_cells, const int32_t *cell_gt_off,
                          const int64_t *cell_iou_off, int64_t n_pairs,
                          const double *iou, int32_t max_ulp, int32_t capacity,
                          int32_t *count, int64_t *list, void *stream);

/* The listed pairs recomputed on the device in the reference's order
 * (replaces compute_track_box_iou / compute_avg_track_iou, T/eval.py:73-117,
 * for exactly those pairs).  A thread per pair restates CPython's
 * ``set(gt_track.keys()) | set(dt_track.keys())`` (Objects/setobject.c of
 * 3.7 - 3.12, csrc/pyset.hpp), visits the union in slot order and adds the
 * per-frame terms of bb_intersect_union (T/eval.py:32-48) as the reference
 * does: mode 0 sums intersections and unions left to right, mode 1 takes
 * np.mean (numpy's pairwise summation) of the per-frame ratios.
 *   cell_unit      int32  video index of a cell
 *   tl_vid_start   int64  first timeline slot of a video in tl_image_id
 *   tl_image_id    int64  image id at (video, timeline position): the dict key
 *                         (all ids in [0, 2^61 - 1): hash(id) == id)
 *   count, list    device: the output of taoamd_track_iou_near (count read on
 *                  the device: no host round trip); `capacity` = entries of list
 *   scratch        int32[scratch_slots], 3 * table_cap slots per worker thread;
 *                  table_cap >= taoamd_track_iou_setorder_table(longest
 *                  detection track, longest GT track) in frames
 *   status         int32[1], bit 0 set if a pair needed a larger table (skipped)
 * Patches iou[list[k]] in place; asynchronous on `stream`. */
int64_t taoamd_track_iou_setorder_table(int64_t max_dt_frames, int64_t max_gt_frames);
int taoamd_track_iou_setorder(
    int64_t n_cells, const int32_t *cell_dt_off, const int32_t *cell_gt_off,
    const int64_t *cell_iou_off, const int32_t *cell_unit, const int64_t *tl_vid_start,
    const int64_t *tl_image_id, const int32_t *dt_frame_off, const int32_t *dt_frame_pos,
    const double *dt_frame_box, const int32_t *gt_frame_off, const int32_t *gt_frame_pos,
    const double *gt_frame_box, int32_t mode, const int32_t *count, int32_t capacity,
    const int64_t *list, double *iou, int32_t *scratch, int64_t scratch_slots,
    int64_t table_cap, int32_t *status, void *stream);

/* Host statements of the same text (test seams; synchronous, no GPU):
 * one pair's set-order IoU from host arrays (positions ascending, boxes x, y,
 * w, h; tl_image_id indexed by position), and the iteration order of
 * ``set(a) | set(b)`` for two lists of non-negative ints (out: n_a + n_b
 * entries). */
int taoamd_set_order_iou_host(const int64_t *tl_image_id, int32_t n_dt,
                              const int32_t *dt_pos, const double *dt_box, int32_t n_gt,
                              const int32_t *gt_pos, const double *gt_box, int32_t mode,
                              double *out);
int taoamd_pyset_union_order_host(int64_t n_a, const int64_t *a, int64_t n_b,
                                  const int64_t *b, int64_t *out, int64_t *n_out);

/* Launch plan of taoamd_track_iou_planned from HOST copies of the cell offsets
 * and of trk_meta (detection tracks first, then GT tracks).  Call with
 * tasks_host == NULL to get sizes[0..2] = tasks, task_rows entries, task_pairs
 * entries; then with buffers of 4 * sizes[0], sizes[1], sizes[2] int32 and
 * sizes[2] int64.  Every (detection track, GT track) pair of every cell lands
 * in exactly one task, whatever the two tracks' spans.  Synchronous, host only.
 *
 * taoamd_track_iou_plan_spans_host is the span-aware plan, packed by the same
 * rules (cells by descending end of timeline, a cell's detections by first
 * position, GT blocks of at most 31, tasks of <= 64 pairs and <= 32 rows, rows
 * by first position).  A ZERO PAIR -- both tracks have a frame (first <= last)
 * and last_d < first_g or last_g < first_d: no common position, so its result
 * is +0.0 in every mode -- lands in no task: its place in `iou` goes to
 * zero_out (ascending), for taoamd_track_iou_planned's (n_zero, zero_out).
 * Spans that touch (last_d == first_g) share a position and stay in a task, and
 * so does every pair with a track without frames (the reference's 0 / 0).  A
 * detection track whose pairs are all zero pairs is a row of no task; a GT
 * track is a row of a task only if one of that task's pairs uses it.  Every
 * pair is exactly once in task_out or zero_out.  sizes has FOUR entries here:
 * sizes[3] = the zero list's length (zero_out_host: sizes[3] int64, filled
 * whenever it is not NULL).  On an input without zero pairs the four task
 * arrays equal taoamd_track_iou_plan_host's. */
int taoamd_track_iou_plan_host(int64_t n_cells, const int32_t *cell_dt_off_host,
                               const int32_t *cell_gt_off_host,
                               const int64_t *cell_iou_off_host,
                               const int32_t *trk_meta_host, int64_t *sizes,
                               int32_t *tasks_host, int32_t *task_rows_host,
                               int32_t *task_pairs_host, int64_t *task_out_host);
int taoamd_track_iou_plan_spans_host(int64_t n_cells, const int32_t *cell_dt_off_host,
                                     const int32_t *cell_gt_off_host,
                                     const int64_t *cell_iou_off_host,
                                     const int32_t *trk_meta_host, int64_t *sizes,
                                     int32_t *tasks_host, int32_t *task_rows_host,
                                     int32_t *task_pairs_host, int64_t *task_out_host,
                                     int64_t *zero_out_host);

/* ---- greedy assignment --------------------------------------------------------
 * If dt_box/gt_box are non-NULL the IoU matrix of each cell is computed on the
 * fly from the boxes (LVIS, fused); otherwise it is read from `iou` at
 * cell_iou_off (TAO).  dst (optional, int32 per detection) redirects the
 * output row of detection d to dst[d] (used to write in (category, score)
 * order); NULL = identity.
 *   matched, ignored : uint64[n_dt * n_words]
 *   match_gt (opt.)  : int32[n_dt * n_rng*10], in-cell GT index or -1
 *                      (always in identity order)
 *   ious_out (opt.)  : LVIS only, double at cell_iou_off like `iou`
 * out_stride: distance, in 64-bit words, between consecutive output rows of
 * matched / ignored (0 = dense); lets the kernel write straight into an
 * interleaved exchange record.
 * Paired rows: when ignored == matched + 1 the two tables are read as ONE table
 * of (matched, ignored) pairs -- word w of row r is the pair at
 * matched[r * out_stride + 2 * w], dense out_stride = 2 * n_words -- and,
 * where matched is 16-byte aligned and out_stride even, a pair is written with
 * one 16-byte store;
 * taoamd_accumulate* recognise the same layout by the same pointer relation.
 * The pointer relation IS the layout flag of this ABI: `ignored == matched + 1`
 * means interleaved pairs in taoamd_match and every taoamd_accumulate* entry;
 * the entry that only knows DENSE [n][n_words] tables -- taoamd_gather_rows
 * (its destination) -- returns TAOAMD_ERR_ARG when
 * handed that relation instead of scrambling rows (tests/test_abi.py).
 * max_gt_per_cell must be >= the largest GT count of a cell (host knows it
 * from the CSR table); cells with more than 64 GTs take a slower kernel and
 * more than TAOAMD_MAX_GT_PER_CELL is an error.
 * Launch plan (optional, all NULL/0 = one wavefront per cell): `groups`
 * (int32[n_groups][4], device) lists runs of consecutive cells with at most
 * 64 detections and 64 GTs in total and at most 8 GTs per cell, as {first
 * detection, detections, first GT, GTs} of the run -- one wavefront evaluates
 * a whole run with coalesced loads; `singles` (int32[n_singles]) lists the
 * remaining cells that hold detections; `dt_group` (int32[n_dt][4]) gives per
 * detection {first GT of its cell, GT count of its cell, its position inside
 * the cell, cell index}, so the kernel reaches everything with two dependent
 * loads instead of walking detection -> cell -> cell tables.  `dt_meta`
 * (optional, uint32[n_dt]; used where the kernel computes the IoUs itself and
 * stores none) packs what a run's wavefront needs of that row and the flag
 * byte into one word: dt_flags | (first GT of the cell - first GT of the run)
 * << 8 | (GT count of the cell) << 14 | (position inside the cell) << 18 --
 * 4 instead of 17 bytes read per detection. */
#define TAOAMD_MAX_GT_PER_CELL 3072
int taoamd_match(int64_t n_cells, const int32_t *cell_dt_off,
                 const int32_t *cell_gt_off, const int64_t *cell_iou_off,
                 int32_t max_gt_per_cell, const double *dt_box,
                 const double *gt_box, const double *iou, int32_t n_rng,
                 const uint32_t *gt_rng, const uint32_t *dt_rng,
                 const uint8_t *gt_flags, const uint8_t *dt_flags,
                 const int32_t *dst, int64_t out_stride, uint64_t *matched,
                 uint64_t *ignored, int32_t *match_gt, double *ious_out,
                 const int32_t *dt_group, const uint32_t *dt_meta,
                 const int32_t *groups, int32_t n_groups, const int32_t *singles,
                 int32_t n_singles, void *stream);

/* Compact rows (image level: box IoU computed by the kernel, one combo word of
 * at most six ranges, launch plan with dt_meta, rows in cell order).  Where no
 * detection of a cell overlaps two ground truths by the lowest threshold, a row
 * is a function of 18 bits and the match stores those instead of the pair:
 *   compact[d] : bits 0-9   the thresholds the detection is matched at
 *                bits 10-15 the matched ground truth's range mask
 *                bit 16     the detection is ignored when unmatched
 *                bit 17     the matched ground truth's id is hidden
 *                bit 31     escape: the cell went through the sequential greedy
 *                           and the full pair lies at rows[2 * d], as
 *                           taoamd_match stores it
 * rows: uint64[n_dt][2], 16-byte aligned.  taoamd_expand_rows writes the pair of
 * every row that is not escaped (afterwards `rows` holds what taoamd_match would
 * have stored); taoamd_accumulate_by_order_compact sweeps the compact form.
 * TAOAMD_ERR_ARG for a problem outside this shape. */
int taoamd_match_compact(int64_t n_cells, const int32_t *cell_dt_off,
                         const int32_t *cell_gt_off, int32_t max_gt_per_cell,
                         const double *dt_box, const double *gt_box, int32_t n_rng,
                         const uint32_t *gt_rng, const uint8_t *gt_flags,
                         const uint8_t *dt_flags, uint64_t *rows, uint32_t *compact,
                         const int32_t *dt_group, const uint32_t *dt_meta,
                         const int32_t *groups, int32_t n_groups, const int32_t *singles,
                         int32_t n_singles, void *stream);
int taoamd_expand_rows(int64_t n_dt, int32_t n_rng, const uint32_t *compact,
                       uint64_t *rows, void *stream);

/* ---- cell-table build, detection side (csrc/flatten.hip) ----------------------
 * The per-box half of what the reference does with dicts in L/results.py:20-84,
 * L/lvis.py:90-96, L/eval.py:59-110 (and the T/ counterparts): the host keeps
 * the ground-truth half and everything that is O(cells) (flatten_dev.py).
 *
 * taoamd_flat_map     image / category ids -> their positions in the sorted
 *                     unique id lists of the ground truth (-1 = unknown),
 *                     area = w * h unless `area_in` is given,
 *                     boxes per image (img_count[n_img + 1]) and their
 *                     exclusive scan (img_start[n_img + 1]), optionally the
 *                     first box of every image (img_first[n_img], file order;
 *                     0x7f7f7f7f = none); status[0] = boxes of unknown images,
 *                     status[1] = most boxes in one image
 * taoamd_flat_rank_drop   dropped[d] = 1 for boxes beyond the best max_dets of
 *                     their image; `order` = the stable sort by (image, -score)
 * taoamd_flat_filter  key[d] = cat * n_unit + unit for boxes that survive the
 *                     known-category, 0 < area < inf and federated filters
 *                     (the cell has ground truth: key in sorted gkeys; or the
 *                     category is in the unit's negative list), INT32_MAX for
 *                     the others; flags[d] = DT_IGNORE_UNMATCHED when the
 *                     category is in the unit's not-exhaustive list (or, with
 *                     area_flag, the area is outside [0, 1e10]); *n_keep =
 *                     survivors.  unit_row[unit] = row of the CSR lists
 * taoamd_flat_gather  rows of the first n_keep entries of `order` (the stable
 *                     sort by (key, -score)): source row, score, flags, key,
 *                     category = key / n_unit, box (optional)
 * taoamd_flat_runs    runs of equal values of a sorted key array: run_id[i],
 *                     run_key[r], run_start[r], *n_runs
 * taoamd_flat_remap   out[i] = map[id[i]] */
int taoamd_flat_map(int64_t n, const int64_t *image_id, const int64_t *category_id,
                    const double *bbox, const double *area_in, int64_t n_img,
                    const int64_t *img_ids, int64_t n_cat, const int64_t *cat_ids,
                    int32_t *img, int32_t *cat, double *area, int32_t *img_count,
                    int32_t *img_start, int32_t *img_first, int32_t *status,
                    void *stream);
int taoamd_flat_rank_drop(int64_t n, const int32_t *order, const int32_t *img,
                          const int32_t *img_start, int32_t max_dets,
                          uint8_t *dropped, void *stream);
int taoamd_flat_filter(int64_t n, const int32_t *unit, const int32_t *cat,
                       const double *area, const int64_t *category_id,
                       const uint8_t *dropped, int32_t n_unit, int64_t n_gkeys,
                       const int32_t *gkeys, const int32_t *unit_row,
                       const int64_t *neg_off, const int64_t *neg_val,
                       const int64_t *nel_off, const int64_t *nel_val,
                       int32_t area_flag, int32_t *key, uint8_t *flags,
                       int32_t *n_keep, void *stream);
int taoamd_flat_gather(int64_t n_keep, const int32_t *order, const double *score,
                       const uint8_t *flags, const int32_t *key,
                       const double *bbox, int32_t n_unit, int32_t *dt_row,
                       double *dt_score, uint8_t *dt_flags, int32_t *dt_key,
                       int32_t *dt_cat, double *dt_box, void *stream);
/* Track level (T/results.py:20-132, T/tao.py:108-254, T/eval.py:196-243); see
 * csrc/flatten.hip for the stages and flatten_dev.flatten_tao_device for the
 * order they run in.  Sort keys travel as exact doubles, negated (the radix
 * sort is descending in its score argument).
 *   taoamd_flat_ordscore   score of boxes in images beyond max_dets, else 0
 *   taoamd_flat_ordinal    ordinal[d] = place of box d inside its image in the
 *                          post-truncation list, dropped[d] = beyond max_dets
 *   taoamd_flat_merge_cat  merged category id + its index (-1 unknown)
 *   taoamd_flat_split64 / _compose / _gather_cols   helpers of the sorts
 *   taoamd_flat_track_of   trk[d] = run of its track id; status[2] = a box whose
 *                          track spans two videos (else unchanged)
 *   taoamd_flat_keys       list-order / visiting-order / frame / timeline keys,
 *                          track keys of the kept and of the selected boxes
 *   taoamd_flat_track_kept per track: score (np.mean when the boxes' scores
 *                          differ: status[1] = 1), first kept box; status[3] =
 *                          a box whose category differs inside its track
 *   taoamd_flat_track_sel  per track: mean area (left to right), boxes,
 *                          distinct images, first appearance
 *   taoamd_flat_track_filter  federated filter on the video lists, flags, key
 *   taoamd_flat_frames     frame lists of the final tracks
 *   taoamd_flat_scan       exclusive scan of int32 counts (start[n] = total) */
/* *count = kept boxes with a negative corner or an empty side (T/results.py:100-103) */
int taoamd_flat_count_bad(int64_t n, const double *bbox, const uint8_t *dropped,
                          int32_t *count, void *stream);
int taoamd_flat_ordscore(int64_t n, const int32_t *img, const int32_t *img_count,
                         const double *score, int32_t max_dets, double *out,
                         void *stream);
int taoamd_flat_ordinal(int64_t n, const int32_t *order, const int32_t *img,
                        const int32_t *img_start, int32_t max_dets,
                        int32_t *ordinal, uint8_t *dropped, void *stream);
int taoamd_flat_merge_cat(int64_t n, const int64_t *category_id, int64_t n_merge,
                          const int64_t *merge_src, const int64_t *merge_dst,
                          int64_t n_cat, const int64_t *cat_ids, int64_t *merged_id,
                          int32_t *cat, void *stream);
int taoamd_flat_split64(int64_t n, const int64_t *key, const int32_t *order,
                        int32_t *lo, int32_t *hi, void *stream);
int taoamd_flat_compose(int64_t n, const int32_t *outer, const int32_t *inner,
                        int32_t *out, void *stream);
int taoamd_flat_gather_cols(int64_t n, const int32_t *idx, const int32_t *src_i32,
                            int32_t *out_i32, const double *src_f64,
                            double *out_f64, const uint8_t *src_u8,
                            uint8_t *out_u8, void *stream);
int taoamd_flat_track_of(int64_t n, const int32_t *order, const int32_t *run_id,
                         const int32_t *run_start, const int64_t *video_id,
                         int32_t *trk, int32_t *status, void *stream);
int taoamd_flat_keys(int64_t n, const int32_t *img, const int32_t *ordinal,
                     const uint8_t *dropped, const int32_t *cat, const double *area,
                     const int32_t *trk, const int32_t *img_rank,
                     const int32_t *visit_rank, const double *img_frame,
                     const int32_t *tl_pos, double M, double *keep_key,
                     double *visit_key, double *frame_key, double *pos_key,
                     int32_t *trk_keep, int32_t *trk_sel, void *stream);
int taoamd_flat_track_kept(int64_t n_runs, const int32_t *run_trk,
                           const int32_t *run_start, int64_t n_sorted,
                           const int32_t *order_k, const double *score,
                           const int64_t *merged_id, double *trk_score,
                           int32_t *trk_first_kept, int32_t *status, void *stream);
int taoamd_flat_track_sel(int64_t n_runs, const int32_t *run_trk,
                          const int32_t *run_start, int64_t n_sorted,
                          const int32_t *order_s, const double *area,
                          const double *visit_key, const int32_t *img,
                          double *sel_area, int32_t *sel_len, int32_t *sel_frames,
                          double *sel_first, void *stream);
int taoamd_flat_track_filter(int64_t n_runs, const int32_t *run_trk,
                             const int32_t *sel_len, const int32_t *trk_first_kept,
                             const int32_t *cat, const int64_t *merged_id,
                             const int64_t *video_id, const int64_t *track_id,
                             int64_t n_vid, const int64_t *vid_ids, int64_t n_gkeys,
                             const int32_t *gkeys, const int32_t *vid_row,
                             const int64_t *neg_off, const int64_t *neg_val,
                             const int64_t *nel_off, const int64_t *nel_val,
                             int32_t *key, uint8_t *flags, int32_t *n_keep,
                             int32_t *status, void *stream);
int taoamd_flat_frames(int64_t n_trk, const int32_t *trk_run,
                       const int32_t *run_start, int64_t n_runs, int64_t n_sorted,
                       const int32_t *order_s, const int32_t *img,
                       const int32_t *tl_pos, const double *bbox,
                       const int32_t *frame_off, int32_t *frame_pos,
                       double *frame_box, void *stream);
int taoamd_flat_scan(int64_t n, const int32_t *count, int32_t *start,
                     int32_t *status2, void *stream);
size_t taoamd_flat_runs_workspace(int64_t n);
int taoamd_flat_runs(int64_t n, const int32_t *sorted_key, int32_t *run_id,
                     int32_t *run_key, int32_t *run_start, int32_t *n_runs,
                     void *workspace, size_t workspace_bytes, void *stream);
int taoamd_flat_runs_by(int64_t n, const int32_t *key, const int32_t *order,
                        int32_t *run_id, int32_t *run_key, int32_t *run_start,
                        int32_t *n_runs, void *workspace, size_t workspace_bytes,
                        void *stream);
int taoamd_flat_runs64_by(int64_t n, const int64_t *key, const int32_t *order,
                          int32_t *run_id, int64_t *run_key, int32_t *run_start,
                          int32_t *n_runs, void *workspace, size_t workspace_bytes,
                          void *stream);
int taoamd_flat_remap(int64_t n, const int32_t *id, const int32_t *map,
                      int32_t *out, void *stream);

/* Launch plan of taoamd_match (groups / singles arguments) from HOST copies of
 * the cell offsets: runs of consecutive small cells (each <= cap_d detections
 * and <= cap_cell_g ground truths, a run <= cap_d detections and <= cap_g
 * ground truths) -> groups[.][2] = {first cell, end cell}; other cells with
 * detections -> singles.  groups == NULL: sizes only (sizes[0] groups,
 * sizes[1] singles).  The kernels' caps are 64, 64, 8.  Synchronous, host. */
int taoamd_match_plan_host(int64_t n_cells, const int32_t *cell_dt_off_host,
                           const int32_t *cell_gt_off_host, int32_t cap_d,
                           int32_t cap_g, int32_t cap_cell_g, int64_t *sizes,
                           int32_t *groups_host, int32_t *singles_host);

/* ---- stable sort by (category asc, score desc) ---------------------------------
 * order[p] = detection at sorted position p; dst[d] = sorted position of
 * detection d (either may be NULL).  Ties keep input order, i.e. the
 * reference's concatenation order.  dt_cat: any non-negative int32 key;
 * dt_score may be NULL (integer key alone).  Workspace:
 * taoamd_sort_workspace(n). */
size_t taoamd_sort_workspace(int64_t n);
int taoamd_sort_by_cat_score(int64_t n, const int32_t *dt_cat,
                             const double *dt_score, int32_t *order,
                             int32_t *dst, void *workspace,
                             size_t workspace_bytes, void *stream);

/* The same order by SAMPLE SORT (round 3; what the evaluator passes call):
 * every category -- or chunk of TAOAMD_SORT_CHUNK elements of a longer one --
 * is cut into buckets of ~416 elements by splitters taken from a sorted sample,
 * one pass scatters the elements into their buckets, one wavefront sorts a
 * bucket in registers (bitonic network over <= 1024 (key, index) pairs) and
 * writes order / dst; categories longer than a chunk are finished by the
 * merge-path passes of taoamd_sort_segments.  Replaces np.argsort(-dt_scores,
 * kind="mergesort") of lvis_amodal/eval.py:353-361 / tao_amodal/eval.py:508-518.
 * The plan depends on cat_off alone: taoamd_sort_plan_host (host, synchronous;
 * call with chunks == NULL for sizes[0..4] = chunks, split chunks, scatter
 * tiles, buckets, 1 if some category is longer than a chunk; then with buffers
 * of 8 * sizes[0], sizes[1], sizes[2], sizes[3] int32) -- the tables are
 * uploaded by the caller and stay valid while cat_off does.  tile_off / n_tiles
 * as for taoamd_sort_segments (used by the merge passes only).
 * taoamd_sort_sampled_cap_limit: test seam -- buckets beyond `limit` elements
 * take the overflow path (ranking by counting); 0 restores the default. */
#define TAOAMD_SORT_CHUNK (16 * 2816)
int taoamd_sort_plan_host(int32_t n_cat, const int32_t *cat_off_host, int64_t *sizes,
                          int32_t *chunks, int32_t *split_list, int32_t *stile_chunk,
                          int32_t *bucket_chunk);
size_t taoamd_sort_sampled_workspace(int64_t n, int64_t n_buckets, int32_t merge);
int taoamd_sort_sampled_cap_limit(int32_t limit);
int taoamd_sort_sampled(int64_t n, int32_t n_cat, const int32_t *cat_off,
                        const int32_t *tile_off, int32_t n_tiles, int32_t max_segment,
                        const double *dt_score, int32_t n_chunks, const int32_t *chunks,
                        int32_t n_split, const int32_t *split_list, int32_t n_stiles,
                        const int32_t *stile_chunk, int32_t n_buckets,
                        const int32_t *bucket_chunk, int32_t *order, int32_t *dst,
                        void *workspace, size_t workspace_bytes, void *stream);

/* Same result for detections that are already grouped by category (the
 * category-major cell tables).  cat_off (int32[n_cat+1], device) delimits the
 * runs; every run is cut into tiles of TAOAMD_SEGMENT_TILE elements,
 * tile_off (int32[n_cat+1], device) = exclusive prefix of ceil(len/TILE),
 * n_tiles its total; max_segment = host value of the longest run.  Tiles are
 * sorted in LDS, longer runs finished by rank-merge passes.
 * Workspace: taoamd_sort_segments_workspace(n). */
#define TAOAMD_SEGMENT_TILE 2816
size_t taoamd_sort_segments_workspace(int64_t n);
int taoamd_sort_segments(int64_t n, int32_t n_cat, const int32_t *cat_off,
                         const int32_t *tile_off, int32_t n_tiles,
                         int32_t max_segment, const int32_t *dt_cat,
                         const double *dt_score, int32_t *order, int32_t *dst,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ---- row gather -----------------------------------------------------------------
 * dst_*[p*n_words + w] = src_*[order[p]*src_stride + w]: brings exchanged
 * records (multi-GPU path) into sorted order.  Destination tables dense (the
 * pair layout of taoamd_match is refused: TAOAMD_ERR_ARG). */
int taoamd_gather_rows(int64_t n, int32_t n_words, const uint64_t *src_matched,
                       const uint64_t *src_ignored, int64_t src_stride,
                       const int32_t *order, uint64_t *dst_matched,
                       uint64_t *dst_ignored, void *stream);

/* ---- accumulate -------------------------------------------------------------------
 * matched/ignored are in sorted order (row p = sorted position p); cat_off
 * (int32[n_cat+1], device) delimits the categories in that order.  Outputs, C
 * order, -1 where the category has no evaluated GT in the range:
 *   precision[T][R][n_cat][n_rng], recall[T][n_cat][n_rng]
 * Workspace: taoamd_accumulate_workspace(n_dt, n_cat, n_rng). */
size_t taoamd_accumulate_workspace(int64_t n_dt, int32_t n_cat, int32_t n_rng);
/* The two halves of taoamd_accumulate, used separately by the multi-GPU path:
 *  _compact  sweeps the categories [k_begin, k_end) (rows of other categories
 *            must be absent) and writes the category-major tables
 *              val[n_cat][n_rng][T][R]   precision at the recall thresholds,
 *                                        as opaque 8-byte records (tp << 32 |
 *                                        tp + fp of the row that sets the
 *                                        value; declared double for size)
 *              rec[n_cat][n_rng][T]      recall
 *            for every (k, range) with num_gt > 0 in that category range;
 *  _finalize turns complete tables into the reference layout (-1 fill) and a
 *            record into tp / (fp + tp + eps), L/eval.py:384.
 * Category-major tables make a rank's share one contiguous block, so ranks
 * exchange them with a single all-gather.
 * max_segment: rows of the longest category among those swept (the host
 * knows it from cat_off), or 0 if unknown.  When every category fits one
 * workgroup (<= 4096 rows with one combo word, <= 1024 with four) the sweep
 * is a single fused launch with all intermediates in LDS / registers;
 * otherwise (or with 0) categories are cut into chunks spread over the chip.
 * Workspace of _compact: taoamd_accumulate_workspace; its tables end where
 * taoamd_accumulate keeps val and rec, so less is accepted (that much less).
 * Every workspace: any base address (rounded up to 256 bytes inside, the
 * reported size allows for it); contents need not be initialised. */
size_t taoamd_compact_elems(int32_t n_cat, int32_t n_rng); /* 8-byte elements in val */
int taoamd_accumulate_compact(int64_t n_dt, int32_t n_cat, int32_t n_rng,
                              const int32_t *cat_off, const uint64_t *matched,
                              const uint64_t *ignored, const int32_t *num_gt,
                              int32_t k_begin, int32_t k_end, int32_t max_segment,
                              double *val, double *rec, void *workspace,
                              size_t workspace_bytes, void *stream);
int taoamd_finalize(int32_t n_cat, int32_t n_rng, const int32_t *num_gt,
                    const double *val, const double *rec, double *precision,
                    double *recall, void *stream);
int taoamd_accumulate(int64_t n_dt, int32_t n_cat, int32_t n_rng,
                      const int32_t *cat_off, const uint64_t *matched,
                      const uint64_t *ignored,
                      const int32_t *num_gt, int32_t max_segment, double *precision,
                      double *recall, void *workspace, size_t workspace_bytes,
                      void *stream);
/* The same in two steps, for a caller that sweeps the same categories again and
 * again (an evaluation plan replayed per pass): _prepare builds the table that
 * cuts the categories into chunks -- it depends on cat_off alone -- in the
 * workspace, _prepared is taoamd_accumulate without that launch.  Same
 * workspace, n_dt, n_cat, n_rng, cat_off and max_segment in both; nothing else
 * may use the workspace in between. */
/* The one-pass sweep of long categories resolves the counts of a category's
 * earlier rows by a decoupled look-back between workgroups; a wait that does
 * not end within the poll limit (never observed: it would mean workgroups do
 * not start in order, which an idle GPU does and a shared one need not) gives
 * up and sets a flag in the workspace instead of hanging the GPU.
 * *flag_host != 0: the tables of a pass on this workspace are not to be
 * trusted -- run the pass's sweep again with taoamd_accumulate_chunked /
 * taoamd_accumulate_compact_chunked (same arguments as taoamd_accumulate /
 * _compact; the chunked kernels whatever the mode; the rows of the pass are
 * still in place; a prepared plan in the workspace does not survive it, so
 * taoamd_accumulate_prepare again).  Synchronises with `stream`. */
int taoamd_accumulate_error(const void *workspace, void *stream, int32_t *flag_host);
int taoamd_accumulate_chunked(int64_t n_dt, int32_t n_cat, int32_t n_rng,
                      const int32_t *cat_off, const uint64_t *matched,
                      const uint64_t *ignored,
                      const int32_t *num_gt, int32_t max_segment, double *precision,
                      double *recall, void *workspace, size_t workspace_bytes,
                      void *stream);
int taoamd_accumulate_compact_chunked(int64_t n_dt, int32_t n_cat, int32_t n_rng,
                              const int32_t *cat_off, const uint64_t *matched,
                              const uint64_t *ignored, const int32_t *num_gt,
                              int32_t k_begin, int32_t k_end, int32_t max_segment,
                              double *val, double *rec, void *workspace,
                              size_t workspace_bytes, void *stream);
/* Which sweep long categories take, for the process: -1 automatic (the
 * one-pass look-back sweep from 6 M rows up), 0 the chunked kernels, 1 the
 * one-pass sweep with the look-back, 2 the one-pass sweep behind a counting
 * pass.  An explicit 1 / 2 also takes the short categories the fused
 * single-workgroup sweep would have taken (every case of the parity suite runs
 * under each mode that way).  _plan_kind: the kind of plan
 * taoamd_accumulate_prepare builds for these sizes under the current mode (0
 * none, 1 chunk table, 2 / 3 super-chunk table): a prepared workspace serves
 * taoamd_accumulate_prepared while this is the value it was built under.
 * _spin_limit: polls a look-back waits for one predecessor (0: the default,
 * 2^18; < 0: every look-back gives up at once -- fault injection for the
 * caller's recovery path).
 * _giveup_counter: a caller-owned DEVICE word (NULL: none) to which every
 * look-back that gives up adds one, in every pass launched while it is
 * registered, and which the library never clears -- the workspace's flag is per
 * pass (an unprepared pass zeroes it when it starts), so a caller that runs
 * many passes and synchronises once reads this word instead.
 * max_segment, wherever an entry point of this family takes it: 0 = unknown;
 * a positive value MUST be an upper bound of the longest category's rows -- it
 * chooses the single-workgroup kernels and sizes the one-pass sweep's XCD-aware
 * launch, and rows of a category longer than stated would not be swept. */
int taoamd_accumulate_sweep_mode(int32_t mode);
int taoamd_accumulate_plan_kind(int64_t n_dt, int32_t n_rng, int32_t max_segment);
int taoamd_accumulate_spin_limit(int32_t polls);
int taoamd_accumulate_giveup_counter(uint32_t *device_word);
int taoamd_accumulate_prepare(int64_t n_dt, int32_t n_cat, int32_t n_rng,
                              const int32_t *cat_off, int32_t max_segment,
                              void *workspace, size_t workspace_bytes, void *stream);
int taoamd_accumulate_prepared(int64_t n_dt, int32_t n_cat, int32_t n_rng,
                      const int32_t *cat_off, const uint64_t *matched,
                      const uint64_t *ignored,
                      const int32_t *num_gt, int32_t max_segment, double *precision,
                      double *recall, void *workspace, size_t workspace_bytes,
                      void *stream);
/* The same with the rows where the match kernel left them when it ran WITHOUT
 * `dst` (row = detection, cell order): order[p] = detection at sorted position
 * p (taoamd_sort_segments).  The first sweep gathers the rows through it -- the
 * match then neither waits for the sort nor scatters 16-byte rows. */
int taoamd_accumulate_by_order(int64_t n_dt, int32_t n_cat, int32_t n_rng,
                               const int32_t *cat_off, const int32_t *order,
                               const uint64_t *matched, const uint64_t *ignored,
                               const int32_t *num_gt, int32_t max_segment,
                               double *precision, double *recall, void *workspace,
                               size_t workspace_bytes, void *stream);
/* _prepared: on a workspace taoamd_accumulate_prepare planned (the plan depends
 * on cat_off alone, not on where the rows lie); the one-pass sweep then runs its
 * gathered kernel: order[] in coalesced pieces, the 16-byte rows of a chunk
 * gathered in one batch.  _chunked: the chunked kernels whatever the sweep mode
 * -- what a caller runs again when taoamd_accumulate_error reports a look-back
 * that gave up (rows still in cell order, order[] still in place; prepare again
 * afterwards). */
int taoamd_accumulate_by_order_prepared(int64_t n_dt, int32_t n_cat, int32_t n_rng,
                               const int32_t *cat_off, const int32_t *order,
                               const uint64_t *matched, const uint64_t *ignored,
                               const int32_t *num_gt, int32_t max_segment,
                               double *precision, double *recall, void *workspace,
                               size_t workspace_bytes, void *stream);
int taoamd_accumulate_by_order_chunked(int64_t n_dt, int32_t n_cat, int32_t n_rng,
                               const int32_t *cat_off, const int32_t *order,
                               const uint64_t *matched, const uint64_t *ignored,
                               const int32_t *num_gt, int32_t max_segment,
                               double *precision, double *recall, void *workspace,
                               size_t workspace_bytes, void *stream);
/* ... through the compact rows of taoamd_match_compact: the one-pass sweep
 * gathers the 4-byte words through order[] and fetches a 16-byte pair from
 * `rows` only where a word is escaped.  prepared != 0: on a prepared workspace.
 * TAOAMD_ERR_ARG where the pass would not take the one-pass sweep
 * (taoamd_accumulate_plan_kind 2 or 3) -- taoamd_expand_rows and
 * taoamd_accumulate_by_order* serve there. */
int taoamd_accumulate_by_order_compact(int64_t n_dt, int32_t n_cat, int32_t n_rng,
                               const int32_t *cat_off, const int32_t *order,
                               const uint32_t *compact, const uint64_t *rows,
                               const int32_t *num_gt, int32_t max_segment,
                               double *precision, double *recall, void *workspace,
                               size_t workspace_bytes, int32_t prepared, void *stream);

/* ---- score at each recall threshold ----------------------------------------------
 * pycocotools' eval["scores"] (cocoeval.py accumulate: ss[ri] = dtScoresSorted[pi]):
 * the detection score at the row where recall first reaches each recall
 * threshold.  The reference's accumulate computes the index it is read at --
 * rec_thrs_insert_idx = np.searchsorted(rc, rec_thrs, side="left"),
 * lvis_amodal/eval.py:406-417 == tao_amodal/eval.py:562-573 -- and keeps only
 * the precision there.  Inputs as in taoamd_accumulate: cat_off, the rows'
 * matched / ignored words (either layout), num_gt[n_cat][n_rng], the calling
 * thread's recall thresholds -- non-decreasing, which taoamd_set_thresholds
 * enforces (the selection searches the table of crossings along the recall
 * axis); `order` (optional, int32[n_dt], device): sorted position p -> the row
 * of matched / ignored that belongs to it (rows in cell order,
 * taoamd_accumulate_by_order); NULL: row p is that of sorted position p.
 * `score_order` (optional, likewise): sorted position p -> its element of
 * `score`; NULL: the rows' numbering (order[p], or p without `order`) -- so rows
 * in sorted order beside scores per detection pass NULL and the sort's order[].
 * Output, C order, the layout of precision:
 *   scores[T][R][n_cat][n_rng]  -1 where num_gt == 0; else score[pi], pi = the
 *     first row of the category whose inclusive count of true positives
 *     (matched & ~ignored) reaches the smallest count c with
 *     fl(c / num_gt) >= rec_thrs[j] (c == 0: the category's first row); 0 where
 *     the category has no such row (the reference's bare `except`).
 * A value is a copy of an input score: no arithmetic touches it.
 * Workspace: taoamd_score_at_recall_workspace(n_dt, n_cat, n_rng); any base
 * address, contents need not be initialised. */
size_t taoamd_score_at_recall_workspace(int64_t n_dt, int32_t n_cat, int32_t n_rng);
int taoamd_score_at_recall(int64_t n_dt, int32_t n_cat, int32_t n_rng,
                           const int32_t *cat_off, const int32_t *order,
                           const uint64_t *matched, const uint64_t *ignored,
                           const double *score, const int32_t *score_order,
                           const int32_t *num_gt, double *scores, void *workspace, size_t workspace_bytes,
                           void *stream);

/* ---- image-level error breakdown per range (csrc/error_types.hip) ------------------
 * WHY a detection is no true positive, per visibility range and category.  No
 * reference counterpart (pycocotools users reach for TIDE, Bolya et al., ECCV
 * 2020); the definition is this library's.  Image level, boxes only.
 *
 * One call = one IoU threshold slot of the calling thread's iou_thrs (the
 * foreground threshold tf = min(iou_thrs[slot], 1 - 1e-10), the clamp of the
 * match), one background threshold bg_thr = tb with 0 <= tb < tf, and all
 * n_rng <= TAOAMD_ERROR_TYPES_MAX_RNG ranges at once.  Rows are the rows of the
 * use_cats = 1 cell table (what survived the max_dets cut and the federated
 * filter).  For detection d (image u, category c) and range a:
 *   E_a(u) = the ground truths of image u, of ANY category, whose gt_rng bit a
 *            is clear;
 *   s      = the maximum of bbIou(d, g) over g in E_a(u) of category c, 0 for
 *            an empty set; its argmax = the LOWEST ground-truth row among equal
 *            IoUs;
 *   o      = the same maximum over the other categories.
 * A bbIou that is NaN (boxes may hold any double) is NO overlap: such a pair
 * is left out of both maxima and can be no argmax -- a detection whose every
 * overlap is NaN has s = o = 0 and no argmax.
 * Exactly one type per (detection, range), the first rule that applies:
 *   0 TP       match_gt[d][a * 10 + slot] >= 0 and that ground truth is
 *              evaluated in a
 *   1 IGNORED  matched to a ground truth ignored in a, or unmatched with
 *              TAOAMD_DT_IGNORE_UNMATCHED
 *   2 DUP      unmatched, s >= tf
 *   3 LOC      unmatched, tb <= s < tf
 *   4 CLS      unmatched, o >= tf
 *   5 BOTH     unmatched, tb <= o < tf
 *   6 BKG      otherwise
 * (so with tb = 0 every unmatched, unignored detection is DUP or LOC).  An
 * unmatched row with s >= tf always points at a ground truth another detection
 * holds: the greedy match would otherwise have given the row a ground truth.
 * Per (ground truth, range) with the gt_rng bit clear: `evaluated` counts it,
 * `missed` counts it when no detection's match_gt names it at (a, slot),
 * `missed_loc` counts a missed one that is the same-category argmax of at least
 * one LOC detection of range a.
 * The table follows match_gt, the in-cell index: a ground truth that carries
 * TAOAMD_GT_ID_HIDDEN and holds a detection counts as TP / not missed here,
 * whereas the sweep (the reference's dt_m == 0) sees that detection as
 * unmatched.
 *
 *   dt_cat, dt_box, dt_flags   columns of the cell table, n_dt rows
 *   dt_gt0      int32[n_dt]    first ground-truth row of the row's cell (match_gt
 *                              counts from it)
 *   match_gt    int32, row d at match_gt + d * match_stride (>= n_rng * 10
 *               elements), identity order: what taoamd_match writes
 *   gt_cat, gt_box, gt_rng     columns of the ground truths, n_gt rows
 *   img_gt_off  int32[n_img + 1], img_gt int32[n_gt]: the ground-truth rows of
 *               each image (the table is category-major: they are not contiguous);
 *               img_dt_off, img_dt: the same for the detection rows
 * Outputs (zeroed by the call): dt_counts int64[n_rng][n_cat][7],
 * gt_counts int64[n_rng][n_cat][3] = {evaluated, missed, missed_loc}, and, if
 * not NULL, dt_type uint8[n_dt][n_rng] in the table's row order.
 * TAOAMD_ERR_ARG: slot outside [0, 10), bg_thr outside [0, tf), n_rng outside
 * [1, 8]; TAOAMD_ERR_WORKSPACE: fewer bytes than
 * taoamd_error_types_workspace(n_dt, n_gt, n_rng) (two byte tables
 * [n_rng][n_gt] and the types [n_dt][n_rng] the counts are taken from when
 * dt_type is NULL; any base address, contents need not be initialised).  Rows named by the CSR
 * lists or by match_gt that lie outside the tables are skipped, never
 * dereferenced. */
#define TAOAMD_ERROR_TYPES_TILE 256    /* ground truths staged per step; lanes per image */
#define TAOAMD_ERROR_TYPES_MAX_RNG 8
size_t taoamd_error_types_workspace(int64_t n_dt, int64_t n_gt, int32_t n_rng);
int taoamd_error_types(int64_t n_dt, int64_t n_gt, int32_t n_img, int32_t n_cat,
                       int32_t n_rng, int32_t slot, double bg_thr,
                       const int32_t *dt_cat, const double *dt_box,
                       const uint8_t *dt_flags, const int32_t *dt_gt0,
                       const int32_t *match_gt, int64_t match_stride,
                       const int32_t *gt_cat, const double *gt_box,
                       const uint32_t *gt_rng, const int32_t *img_gt_off,
                       const int32_t *img_gt, const int32_t *img_dt_off,
                       const int32_t *img_dt, int64_t *dt_counts, int64_t *gt_counts,
                       uint8_t *dt_type, void *workspace, size_t workspace_bytes,
                       void *stream);

/* taoamd_error_types with the links a fix would hand every detection: the same
 * pass, outputs and workspace (taoamd_error_types_workspace), plus, per
 * (detection d, range a),
 *   link_same   int32[n_dt][n_rng]  the argmax row of s (-1: none), the rule above
 *   link_other  int32[n_dt][n_rng]  the argmax row of o under the same rule: the
 *               LOWEST ground-truth row among equal IoUs, a NaN IoU no overlap
 * for every row, whatever its type (a row no image lists: -1), and
 *   held        uint8[n_rng][n_gt]  1 where some detection's match_gt names the
 *               ground truth at (a, slot): the complement of `missed`.
 * All three are required (TAOAMD_ERR_ARG otherwise) and zeroed / filled by the call. */
int taoamd_error_types_links(int64_t n_dt, int64_t n_gt, int32_t n_img, int32_t n_cat,
                             int32_t n_rng, int32_t slot, double bg_thr,
                             const int32_t *dt_cat, const double *dt_box,
                             const uint8_t *dt_flags, const int32_t *dt_gt0,
                             const int32_t *match_gt, int64_t match_stride,
                             const int32_t *gt_cat, const double *gt_box,
                             const uint32_t *gt_rng, const int32_t *img_gt_off,
                             const int32_t *img_gt, const int32_t *img_dt_off,
                             const int32_t *img_dt, int64_t *dt_counts, int64_t *gt_counts,
                             uint8_t *dt_type, int32_t *link_same, int32_t *link_other,
                             uint8_t *held, void *workspace, size_t workspace_bytes,
                             void *stream);

/* ---- error impact: the AP each error type costs (csrc/error_impact.hip) ------------
 * TIDE's dAP on the tables of an error breakdown: the precision the evaluation
 * would reach if every error of one type were fixed.  The definition is this
 * library's.  Level-agnostic: the call reads type bytes, links, scores and the
 * sort's order[], neither boxes nor images.
 *
 * Context: one error_types call (one slot, tf, tb, all n_rng ranges) and its
 * terms.  link_same / link_other / held as above.
 * Base list of (category c, range a): the rows order[cat_off[c] .. cat_off[c + 1])
 * -- sweep order: stable descending score, NaN scores last --; a row of type TP
 * is a true positive, types DUP to BKG are false positives, IGNORED rows and
 * any byte >= 7 are dropped; num_gt = evaluated.  Precision at the calling
 * thread's rec_thrs (ascending) by the arithmetic of taoamd_accumulate for one
 * threshold (reference lvis_amodal/eval.py:370-417): pr = tp / (fp + tp +
 * np.spacing(1)), the envelope from the right, searchsorted(rc, rec_thrs,
 * "left"), 0 from the first threshold never reached, -1 for the whole
 * category where num_gt == 0.
 * Nine variants, each a fix applied to the base alone, in this order:
 *   0 BASE
 *   1 CLS   a CLS row leaves its category's list.  Where its link_other g is
 *           not held, the WINNER among the CLS rows of range a linking g (of
 *           any category) joins the list of g's category as a true positive,
 *           after every row of that list whose score is >= its own, at the very
 *           end if its score is a NaN.  Adopted rows are all true positives, so
 *           their order among themselves cannot change a precision value.
 *   2 LOC   a LOC row whose link_same is held leaves; among the LOC rows of
 *           range a that link the same missed ground truth the WINNER becomes a
 *           true positive at its own place, the others leave.  (A LOC row
 *           without a link -- tb = 0, no ground truth of its category -- stays a
 *           false positive.)
 *   3 BOTH, 4 DUP, 5 BKG   the rows of that type leave
 *   6 MISS  num_gt' = evaluated - the missed ground truths that no LOC row
 *           links by link_same and no CLS row links by link_other in range a;
 *           the rows are BASE's
 *   7 FP    every row of types DUP to BKG leaves
 *   8 FN    num_gt' = evaluated - missed; the rows are BASE's
 * WINNER: the greatest score; equal scores (-0.0 == 0.0) go to the lowest table
 * row; a NaN score loses to every number, between two NaNs the lower row wins.
 * A (category, range) whose num_gt' is 0 is -1 like num_gt == 0.
 * The table follows match_gt like the breakdown: where a ground truth carries
 * TAOAMD_GT_ID_HIDDEN and holds a detection, BASE differs from the sweep of
 * taoamd_accumulate; everywhere else BASE is bit-identical to its precision at
 * the slot.
 *
 *   cat_off  int32[n_cat + 1], order int32[n_dt]: the sort's tables
 *   score    double[n_dt], dt_cat int32[n_dt], dt_type uint8[n_dt][n_rng]: by table row
 *   gt_cat   int32[n_gt], gt_rng uint32[n_gt]
 * Outputs: precision double[9][101][n_cat][n_rng], num_gt int32[9][n_cat][n_rng]
 * (num_gt' of every variant).  Rows, links and categories outside the tables
 * are skipped, never dereferenced (a CLS row with such a link leaves its list
 * and nothing is adopted; an entry of order[] outside the table is a row of no
 * list, and the place of an adopted row, found by bisection, is then undefined).  TAOAMD_ERR_ARG: n_rng outside [1, 8], n_cat <= 0,
 * sizes outside [0, 2^31), a missing table; TAOAMD_ERR_WORKSPACE: fewer bytes
 * than taoamd_error_impact_workspace(n_dt, n_gt, n_cat, n_rng) (the winners, 12
 * bytes per (table, range, ground truth); the adopted rows per insertion slot,
 * 4 bytes per (range, row); any base address, contents need not be
 * initialised). */
#define TAOAMD_ERROR_IMPACT_FIXES 9
#define TAOAMD_ERROR_IMPACT_CHUNK 256  /* insertion slots + rows of a category per sweep step */
size_t taoamd_error_impact_workspace(int64_t n_dt, int64_t n_gt, int32_t n_cat, int32_t n_rng);
int taoamd_error_impact(int64_t n_dt, int64_t n_gt, int32_t n_cat, int32_t n_rng,
                        const int32_t *cat_off, const int32_t *order, const double *score,
                        const int32_t *dt_cat, const uint8_t *dt_type,
                        const int32_t *link_same, const int32_t *link_other,
                        const int32_t *gt_cat, const uint32_t *gt_rng, const uint8_t *held,
                        double *precision, int32_t *num_gt, void *workspace,
                        size_t workspace_bytes, void *stream);

/* taoamd_error_impact on the tables of the track level
 * (taoamd_track_error_types_links, below): the definition above word for word,
 * with n_rng in [1, TAOAMD_TAO_RNG].  What differs lies in the tables, not in
 * the sweep: the rows are detection tracks, s is taken from the pass's IoU
 * matrix and o from the plan-less 3D IoU, and IGNORED comes by dt_rng.
 * TAOAMD_ERR_ARG: n_rng outside [1, TAOAMD_TAO_RNG], else as above;
 * TAOAMD_ERR_WORKSPACE: fewer bytes than taoamd_track_error_impact_workspace(n_dt,
 * n_gt, n_cat, n_rng), the same function of its sizes.  taoamd_error_impact
 * keeps its limit of 8 ranges. */
size_t taoamd_track_error_impact_workspace(int64_t n_dt, int64_t n_gt, int32_t n_cat,
                                           int32_t n_rng);
int taoamd_track_error_impact(int64_t n_dt, int64_t n_gt, int32_t n_cat, int32_t n_rng,
                              const int32_t *cat_off, const int32_t *order,
                              const double *score, const int32_t *dt_cat,
                              const uint8_t *dt_type, const int32_t *link_same,
                              const int32_t *link_other, const int32_t *gt_cat,
                              const uint32_t *gt_rng, const uint8_t *held, double *precision,
                              int32_t *num_gt, void *workspace, size_t workspace_bytes,
                              void *stream);

/* ---- confusion: which category pairs the CLS and BOTH errors confuse (csrc/confusion.hip)
 * For every CLS or BOTH row: the category of the ground truth it was taken
 * for.  The definition is this library's.  Level-agnostic like the error
 * impact: one entry point serves the tables of taoamd_error_types_links and of
 * taoamd_track_error_types_links, n_rng in [1, TAOAMD_TAO_RNG].
 *
 * Context: one error_types call (one slot, tf, tb, all n_rng ranges) and its
 * tables, as taoamd_error_impact takes them; the rows lie category-major: the
 * rows of category c are [cat_off[c], cat_off[c + 1]), clamped to the table.
 * What a row contributes: row d of the segment of c, with dt_cat[d] == c; for
 * range a let ty = dt_type[d][a] and g = link_other[d][a].  The row contributes
 * only if ty is CLS (4) or BOTH (5), g lies in [0, n_gt) and c' = gt_cat[g]
 * lies in [0, n_cat); then to the pair (a, c, c').  Every other row contributes
 * nothing and is never dereferenced through its link: a link of -1, a link or
 * a category outside the tables, a dt_cat that is not its segment's, a type
 * byte >= 7.
 * Four int32 counters per pair, in this order:
 *   0 cls      the CLS rows
 *   1 both     the BOTH rows
 *   2 unheld   the CLS rows with held[a][g] == 0: the ground truth is missed
 *   3 adopted  the CLS rows that are the WINNER of (a, g) with held[a][g] == 0
 * WINNER: the rule of the error impact word for word -- the greatest score;
 * equal scores (-0.0 == 0.0) go to the lowest table row; a NaN score loses to
 * every number, between two NaNs the lower row wins -- among the CLS rows of
 * range a linking g, of EVERY predicted category (every row of the table whose
 * dt_cat lies in [0, n_cat), as taoamd_error_impact takes them).  These are
 * the rows variant 1 (CLS) of the impact adopts into c', so one missed ground
 * truth is `adopted` in one pair only.
 * It follows that
 *   sum over c' of cls[a, c, :] == dt_counts[a][c][CLS] less the CLS rows
 *     skipped above, likewise both; on tables that taoamd_*_error_types_links
 *     produced nothing is skipped;
 *   adopted <= unheld <= cls for every pair;
 *   sum over c of adopted[a, :, c'] == the rows the impact's CLS variant
 *     adopts into (c', a).
 *
 * Sparse result: the pairs with cls + both > 0 in ascending (a, c, c'), as a
 * CSR over (a, c), the row of (a, c) at a * n_cat + c:
 *   ent_off    int64[n_rng * n_cat + 1]
 *   ent_gt_cat int32[n_ent]       c' of the entry
 *   ent_counts int32[n_ent][4]    16-byte aligned: an entry leaves as one store
 * (dense, [n_rng][K][K][4] int32 is 139 MB at K = 1203 and 6 ranges, 463 MB at
 * 20, nearly all of it zero).  Every value is an integer and every entry has
 * one place: the result is exact and byte-identical from run to run.
 *
 * Two calls, so that the caller sizes the entry arrays between them:
 * taoamd_confusion_count fills the whole of ent_off (ent_off[n_rng * n_cat] =
 * n_ent); taoamd_confusion_fill, with the same tables, the same workspace --
 * its contents are kept between the two calls -- and on the same stream,
 * stores the entries of every (a, c) row with ent_off[row + 1] <= cap and
 * nothing at or beyond entry `cap`.
 * TAOAMD_ERR_ARG: n_rng outside [1, TAOAMD_TAO_RNG], n_cat <= 0, sizes outside
 * [0, 2^31), a missing table, cap < 0, ent_counts not 16-byte aligned;
 * TAOAMD_ERR_WORKSPACE (before any device call): fewer bytes than
 * taoamd_confusion_workspace(n_dt, n_gt, n_cat, n_rng) -- the winners, 12 bytes
 * per (range, ground truth), and the entries per (a, c) row, 4 bytes per
 * (range, category); any base address, contents need not be initialised.
 * TAOAMD_CONFUSION_TILE: the ground-truth categories one LDS table of the
 * histogram holds (16 bytes each, 32 KB); more categories than that and a
 * category's rows are walked once per tile. */
#define TAOAMD_CONFUSION_TILE 2048
size_t taoamd_confusion_workspace(int64_t n_dt, int64_t n_gt, int32_t n_cat, int32_t n_rng);
int taoamd_confusion_count(int64_t n_dt, int64_t n_gt, int32_t n_cat, int32_t n_rng,
                           const int32_t *cat_off, const double *score, const int32_t *dt_cat,
                           const uint8_t *dt_type, const int32_t *link_other,
                           const int32_t *gt_cat, const uint8_t *held, int64_t *ent_off,
                           void *workspace, size_t workspace_bytes, void *stream);
int taoamd_confusion_fill(int64_t n_dt, int64_t n_gt, int32_t n_cat, int32_t n_rng,
                          const int32_t *cat_off, const double *score, const int32_t *dt_cat,
                          const uint8_t *dt_type, const int32_t *link_other,
                          const int32_t *gt_cat, const uint8_t *held, const int64_t *ent_off,
                          int64_t cap, int32_t *ent_gt_cat, int32_t *ent_counts,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ---- track-level error breakdown per range (csrc/track_error_types.hip) ------------
 * WHY a detection track is no true positive, per (area, time) range and
 * category: the section above, rule for rule, on the track tables.  The
 * definition is this library's.  Track level, boxes, the 3d_iou metric (mode 0
 * of taoamd_track_iou) only.
 *
 * One call = one IoU threshold slot (tf = min(iou_thrs[slot], 1 - 1e-10)), one
 * background threshold bg_thr = tb with 0 <= tb < tf, and all n_rng <=
 * TAOAMD_TAO_RNG ranges at once (the reference constants give 20, slot = area
 * index * 4 + time index as taoamd_tao_ranges writes them; the last area slot
 * is "highly-and-partially-occluded").  Rows are the detection tracks of the
 * use_cats = 1 track table (after the max_dets cut and the federated filter);
 * ground truths are the ground-truth tracks.  For detection track d (video v,
 * category c) and range a:
 *   E_a(v) = the ground-truth tracks of video v, of ANY category, whose gt_rng
 *            bit a is clear;
 *   s      = the maximum over g in E_a(v) of category c of the pass's own IoU,
 *            iou[cell_iou_off[cell] + d_local * G + g_local] -- the matrix the
 *            match read, the frame-order guard's patches included -- 0 for an
 *            empty set; its argmax = the LOWEST ground-truth row among equal
 *            IoUs.  Taken from that matrix, an unmatched row with s >= tf
 *            always points at a ground truth another detection holds;
 *   o      = the same maximum over g in E_a(v) of the other categories, of the
 *            IoU the plan-less taoamd_track_iou gives the pair: i and u added
 *            over the union of the two tracks' frames in ascending timeline
 *            order (a frame both have adds i_ and u_, a frame only one has
 *            adds that box's w * h to u), u > 0 ? i / u : 0.  No frame-order
 *            guard here: there is no reference counterpart whose set order
 *            could matter.
 * An IoU that is NaN (boxes may hold any double) is NO overlap, as above.
 * Exactly one type per (detection track, range), the first rule that applies:
 *   0 TP       match_gt[d][a * 10 + slot] >= 0 and that ground truth is
 *              evaluated in a
 *   1 IGNORED  matched to a ground truth ignored in a, or unmatched with bit a
 *              of dt_rng[d] set (the image level tests the flag alone; dt_rng
 *              holds the not-exhaustive flag AND the area / length windows)
 *   2 DUP      unmatched, s >= tf
 *   3 LOC      unmatched, tb <= s < tf
 *   4 CLS      unmatched, o >= tf
 *   5 BOTH     unmatched, tb <= o < tf
 *   6 BKG      otherwise
 * Per (ground-truth track, range) with the gt_rng bit clear: `evaluated`,
 * `missed` (no detection's match_gt names it at (a, slot)), `missed_loc` (a
 * missed one that is the same-category argmax of at least one LOC detection of
 * range a).  The table follows match_gt, the in-cell index: a ground truth that
 * carries TAOAMD_GT_ID_HIDDEN and holds a detection counts as TP / not missed
 * here, whereas the sweep (the reference's dt_m == 0) sees that detection as
 * unmatched.
 *
 *   dt_cat, dt_rng   columns of the track table / of taoamd_tao_ranges, n_dt rows
 *   dt_group    int32[n_dt][4] {first ground-truth row of the row's cell (match_gt
 *               counts from it), ground truths of the cell G, the row's place in
 *               its cell d_local, the cell}
 *   cell_iou_off int64[n_cells + 1], iou double[n_iou]: the pass's IoU matrix
 *   match_gt    int32, row d at match_gt + d * match_stride (>= n_rng * 10
 *               elements), identity order: what taoamd_match writes
 *   gt_cat, gt_rng   columns of the ground-truth tracks, n_gt rows
 *   *_frame_off, *_frame_pos, *_frame_box: the tracks' CSR frame lists of
 *               taoamd_track_iou (positions strictly ascending within a track)
 *   vid_gt_off  int32[n_vid + 1], vid_gt int32[n_gt]: the ground-truth rows of
 *               each video (the table is category-major: they are not
 *               contiguous); vid_dt_off, vid_dt: the same for the detection rows
 * Outputs (zeroed by the call): dt_counts int64[n_rng][n_cat][7], gt_counts
 * int64[n_rng][n_cat][3] = {evaluated, missed, missed_loc}, and, if not NULL,
 * dt_type uint8[n_dt][n_rng] in the table's row order and dt_over
 * uint32[n_dt][2], the cross-category result alone: bit a of word 0 = o >= tf
 * in range a, bit a of word 1 = o >= tb in range a (with tb = 0 every bit below
 * n_rng: the empty maximum is 0).  No (detection track x ground-truth track)
 * matrix is stored: a pair's IoU is folded into the two masks when it is known.
 * TAOAMD_ERR_ARG: slot outside [0, 10), bg_thr outside [0, tf), n_rng outside
 * [1, TAOAMD_TAO_RNG]; TAOAMD_ERR_WORKSPACE: fewer bytes than
 * taoamd_track_error_types_workspace(n_dt, n_gt, n_rng) (the two masks per row
 * and two byte tables [n_rng][n_gt]; any base address, contents need not be
 * initialised).  Rows named by the CSR lists, by dt_group or by match_gt that
 * lie outside the tables are skipped, never dereferenced: such a ground truth
 * is in no E_a, such a match counts as none, a detection row no video lists
 * has o = 0. */
#define TAOAMD_TRACK_ERROR_TYPES_TILE 16    /* ground-truth tracks staged per step */
size_t taoamd_track_error_types_workspace(int64_t n_dt, int64_t n_gt, int32_t n_rng);
int taoamd_track_error_types(int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou,
                             int32_t n_vid, int32_t n_cat, int32_t n_rng, int32_t slot,
                             double bg_thr, const int32_t *dt_cat, const uint32_t *dt_rng,
                             const int32_t *dt_group, const int64_t *cell_iou_off,
                             const double *iou, const int32_t *match_gt, int64_t match_stride,
                             const int32_t *gt_cat, const uint32_t *gt_rng,
                             const int32_t *dt_frame_off, const int32_t *dt_frame_pos,
                             const double *dt_frame_box, const int32_t *gt_frame_off,
                             const int32_t *gt_frame_pos, const double *gt_frame_box,
                             const int32_t *vid_gt_off, const int32_t *vid_gt,
                             const int32_t *vid_dt_off, const int32_t *vid_dt,
                             int64_t *dt_counts, int64_t *gt_counts, uint8_t *dt_type,
                             uint32_t *dt_over, void *workspace, size_t workspace_bytes,
                             void *stream);

/* taoamd_track_error_types with the links a fix would hand every detection
 * track: the same pass, inputs, outputs and workspace
 * (taoamd_track_error_types_workspace), plus, per (detection track d, range a),
 *   link_same   int32[n_dt][n_rng]  the ground-truth TABLE row of the argmax of s
 *               (the first row of d's cell + the in-cell argmax; -1: none)
 *   link_other  int32[n_dt][n_rng]  the argmax row of o under the rule of s: the
 *               LOWEST ground-truth row among equal IoUs -- by row number,
 *               whatever order vid_gt lists the rows in --, a NaN IoU no overlap,
 *               a pair of IoU 0 the argmax where nothing better exists
 * for every row, whatever its type (a row no video lists: link_other -1), and
 *   held        uint8[n_rng][n_gt]  1 where some detection track's match_gt names
 *               the ground truth at (a, slot): the complement of `missed`.
 * All three are required (TAOAMD_ERR_ARG otherwise) and zeroed / filled by the
 * call; they are the tables taoamd_track_error_impact reads. */
int taoamd_track_error_types_links(int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou,
                                   int32_t n_vid, int32_t n_cat, int32_t n_rng, int32_t slot,
                                   double bg_thr, const int32_t *dt_cat, const uint32_t *dt_rng,
                                   const int32_t *dt_group, const int64_t *cell_iou_off,
                                   const double *iou, const int32_t *match_gt,
                                   int64_t match_stride, const int32_t *gt_cat,
                                   const uint32_t *gt_rng, const int32_t *dt_frame_off,
                                   const int32_t *dt_frame_pos, const double *dt_frame_box,
                                   const int32_t *gt_frame_off, const int32_t *gt_frame_pos,
                                   const double *gt_frame_box, const int32_t *vid_gt_off,
                                   const int32_t *vid_gt, const int32_t *vid_dt_off,
                                   const int32_t *vid_dt, int64_t *dt_counts,
                                   int64_t *gt_counts, uint8_t *dt_type, uint32_t *dt_over,
                                   int32_t *link_same, int32_t *link_other, uint8_t *held,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* ---- track-level association: per-frame followers (csrc/track_association.hip) -----
 * WHICH detection track follows a ground-truth track, frame by frame: coverage,
 * ID switches, fragmentation, mostly-tracked / mostly-lost, and coverage by
 * visibility.  The reference has no counterpart; the definition is this
 * library's.  Track level, boxes.  The pass reads the track tables alone: no
 * IoU matrix, no match, none of the evaluation constants.
 *
 * Rows are those of the use_cats = 1 track table (after the max_dets cut and the
 * federated filter).  Ground-truth track g lies in one cell (video, category);
 * its CANDIDATES are the detection tracks of that cell, whatever their dt_flags.
 * g has the frames k = 0 .. L - 1 at timeline positions p_k (strictly
 * ascending) with box b_k and visibility vis_k.
 *   f(d, g, k)  for a candidate d that has a frame at p_k: box_iou(d's box there,
 *               b_k) -- this library's restatement of the reference's bbIou, not
 *               crowd, the detection first, compiled with -ffp-contract=off: the
 *               bits of taoamd_bb_iou.  Boxes may be any double; a NaN is no
 *               overlap.
 *   best_k(g)   the candidate of the greatest f(d, g, k) >= frame_thr; among
 *               equal values the LOWEST table row (the best-scored track: a
 *               cell's rows are in descending score); -1 if there is none.
 *               Frame k is COVERED iff best_k >= 0.
 *   frame_thr   any double in (0, 1], an argument of its own (not one of the IoU
 *               thresholds of taoamd_set_thresholds).
 *   follow[cell_iou_off[cell] + d_local * G + g_local]  the number of frames of g
 *               on which d is best: the layout of the pass's IoU matrix.
 * Per ground-truth track, gt_assoc int32[n_gt][7]:
 *   0 frames          L
 *   1 covered         the covered frames
 *   2 ids             the candidates d with follow > 0
 *   3 switches        over the covered frames in ascending position, uncovered
 *                     ones skipped: those whose best differs from that of the
 *                     covered frame before
 *   4 fragments       the covered k with k = 0 or k - 1 uncovered; neighbours in
 *                     the track's OWN frame list, not in timeline positions: a
 *                     ground truth annotated with holes is not penalised
 *   5 primary         the table row of the d of the greatest follow > 0, the
 *                     lowest row among equal counts; -1 if covered = 0
 *   6 primary_frames  that count
 * Per category, cat_counts int64[n_cat][8], over the ground-truth tracks whose
 * gt_flags lacks TAOAMD_GT_IGNORE: tracks, frames, covered, ids, switches,
 * fragments, mostly_tracked (5 * covered >= 4 * frames), mostly_lost
 * (5 * covered < frames).
 * By visibility, vis_counts int64[n_vis][n_cat][3] = {frames, covered, followed
 * by the track's primary} over the same tracks: n_vis <= 8 closed windows
 * vis_rng double[n_vis][2] (device); a frame counts in EVERY window with lo <=
 * vis_k <= hi (they overlap, as the image level's do), a NaN visibility in none.
 * n_vis = 0 with vis_rng, gt_frame_vis and vis_counts NULL is allowed.
 * Per frame: best int32[n_gt_frames] = the in-cell index of best_k or -1, and,
 * if not NULL, best_iou double[n_gt_frames] = its overlap, 0.0 where uncovered.
 *
 *   cell_dt_off, cell_gt_off, cell_iou_off   the cell tables (n_cells + 1 entries)
 *   gt_cat, gt_flags   columns of the ground-truth tracks, n_gt rows
 *   *_frame_off, *_frame_pos, *_frame_box: the tracks' CSR frame lists of
 *               taoamd_track_iou, n_dt_frames / n_gt_frames frames in all
 *   gt_frame_vis double[n_gt_frames]: the visibility of every ground-truth frame
 * Every output is zeroed / filled by the call; all but best_iou are integers and
 * best_iou is one box_iou value, so every output is exact and the same from run
 * to run: the follow counts and the count tables are integer adds, whose sum
 * does not depend on the order of arrival; no float is ever added.
 * TAOAMD_ERR_ARG: frame_thr outside (0, 1] (a NaN included), n_vis outside
 * [0, 8], a size below 0; TAOAMD_ERR_WORKSPACE: fewer bytes than
 * taoamd_track_association_workspace(n_dt, n_gt, n_gt_frames) (the frame index
 * -- a descriptor per detection track, the cell of every ground-truth row, the
 * track of every ground-truth frame: csrc/track_frames.hpp builds it, for this
 * pass and for taoamd_track_identity_share alike, in the call's own workspace --
 * and a track's counts per window; any base address, contents need not be
 * initialised).  Both
 * are answered before the first device call.  Rows and frames named by the CSR
 * tables that lie outside the tables are skipped, never dereferenced: a ground-
 * truth row no cell lists has no candidates, a frame no track lists no follower. */
#define TAOAMD_TRACK_ASSOCIATION_TILE 64    /* ground-truth frames a workgroup takes */
#define TAOAMD_TRACK_ASSOCIATION_VIS 8      /* visibility windows, at most */
size_t taoamd_track_association_workspace(int64_t n_dt, int64_t n_gt, int64_t n_gt_frames);
int taoamd_track_association(int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou,
                             int64_t n_dt_frames, int64_t n_gt_frames, int32_t n_cat,
                             int32_t n_vis, double frame_thr, const int32_t *cell_dt_off,
                             const int32_t *cell_gt_off, const int64_t *cell_iou_off,
                             const int32_t *gt_cat, const uint8_t *gt_flags,
                             const int32_t *dt_frame_off, const int32_t *dt_frame_pos,
                             const double *dt_frame_box, const int32_t *gt_frame_off,
                             const int32_t *gt_frame_pos, const double *gt_frame_box,
                             const double *gt_frame_vis, const double *vis_rng,
                             int32_t *follow, int32_t *gt_assoc, int64_t *cat_counts,
                             int64_t *vis_counts, int32_t *best, double *best_iou,
                             void *workspace, size_t workspace_bytes, void *stream);

/* ---- track-level occlusion episodes: is the follower kept (csrc/track_occlusion.hip)
 * Whether the detection track that follows a ground-truth track HOLDS it while
 * the object is hidden: what the association's per-window coverage, which counts
 * every frame on its own, cannot say.  The reference has no counterpart; the
 * definition is this library's.  The pass reads the per-frame followers of
 * taoamd_track_association (its `best`) and the frames' visibility, nothing else.
 *
 * Ground-truth track g has the frames k = 0 .. L - 1 of its OWN frame list
 * (neighbours are list neighbours, not timeline positions, as for `fragments`),
 * each with a visibility vis_k and a follower best_k: the association's in-cell
 * index, or -1.
 *   occ_k     lo <= vis_k <= hi: the window is closed; a NaN visibility is not
 *             occluded.
 *   EPISODE   a maximal run a .. b of occluded frames; its length n = b - a + 1.
 *   entry     best_{a-1}, or -1 if a == 0: no look-back beyond that one frame.
 *   covered   the frames of a .. b with best_k >= 0.
 *   held      the frames of a .. b with best_k == entry; 0 when entry < 0.
 *   after, gap  from the frames b + 1 .. min(b + recover, L - 1), whatever their
 *             visibility: with frame b + r the first covered one among them,
 *             after = best_{b+r} and gap = r - 1; if none is covered, after = -1
 *             and gap = 0.  recover is an integer in [1, 64].
 *   outcome   one value, the first rule that applies:
 *               0 START       a == 0
 *               1 UNFOLLOWED  entry < 0
 *               2 END         b == L - 1
 *               3 KEPT        after == entry
 *               4 SWITCHED    after >= 0 and after != entry
 *               5 LOST        after < 0
 *             For START, UNFOLLOWED and END, after = -1 and gap = 0.
 *   bucket    len_edges int32[n_len] (HOST memory), n_len in [1, 8], len_edges[0]
 *             == 1, strictly ascending: bucket j holds len_edges[j] <= n <
 *             len_edges[j + 1], the last bucket is open.
 * Per episode, episodes int32[n_ep][9] = {ground-truth row, a, n, outcome, entry,
 * after, gap, covered, held}, rows ascending by (ground-truth row, a).
 * Per ground-truth track, gt_occ int32[n_gt][4] = {episodes, occluded frames,
 * kept, switched + lost}.
 * Per (category, bucket), counts int64[n_cat][n_len][11] over the tracks whose
 * gt_flags lacks TAOAMD_GT_IGNORE (and whose category lies in [0, n_cat)):
 * {episodes, frames, covered, held, start, unfollowed, end, kept, switched, lost,
 * gap}, the sums of n, covered, held and gap and the number of episodes of each
 * outcome.  Ignored tracks appear in episodes and gt_occ, and in no count.
 * Example, window [0, 0.1]: best = [0,0,-1,0,0,1,1,-1,-1,0], vis = [1,.1,0,1,.05,
 * .05,1,0,1,1] has three episodes (a, n, outcome, entry, after, gap, covered,
 * held): (1,2,KEPT,0,0,0,1,1), (4,2,SWITCHED,0,1,0,2,1) and (7,1,LOST,1,-1,0,0,0)
 * at recover = 1, (7,1,SWITCHED,1,0,1,0,0) at recover >= 2.
 *
 * Two calls, so that the caller sizes the records between them:
 * taoamd_track_occlusion_count fills gt_occ, counts and the whole of ep_off
 * int64[n_gt + 1], the exclusive prefix sum of the tracks' episode counts
 * (ep_off[n_gt] = n_ep); taoamd_track_occlusion_fill, with the same tables,
 * stores the episodes of the tracks with ep_off[g + 1] <= cap and nothing at or
 * beyond record `cap`.  Every output is an integer and every record has one
 * place; the counts are integer adds, whose sum does not depend on the order of
 * arrival; no float is ever added: the result is exact and the same from run to
 * run.
 * TAOAMD_ERR_ARG: recover outside [1, 64], n_len outside [1, 8], edges that do
 * not start at 1 or do not strictly ascend, vis_lo > vis_hi or either a NaN, a
 * size below 0, n_cat <= 0, cap < 0, a missing table; TAOAMD_ERR_WORKSPACE:
 * fewer bytes than taoamd_track_occlusion_workspace(n_gt, n_gt_frames, n_len)
 * (the episodes of every track, 4 bytes each; any base address, contents need
 * not be initialised; the size function answers 0 to sizes it refuses).  Both
 * are answered before the first device call.  Rows and frames named by the CSR
 * table that lie outside the tables are skipped, never dereferenced. */
#define TAOAMD_TRACK_OCCLUSION_LEN 8        /* length buckets, at most */
#define TAOAMD_TRACK_OCCLUSION_RECOVER 64   /* recover, at most: a chunk of frames */
size_t taoamd_track_occlusion_workspace(int64_t n_gt, int64_t n_gt_frames, int32_t n_len);
int taoamd_track_occlusion_count(int64_t n_gt, int64_t n_gt_frames, int32_t n_cat,
                                 int32_t n_len, int32_t recover, double vis_lo, double vis_hi,
                                 const int32_t *len_edges, const int32_t *gt_cat,
                                 const uint8_t *gt_flags, const int32_t *gt_frame_off,
                                 const double *gt_frame_vis, const int32_t *best,
                                 int32_t *gt_occ, int64_t *ep_off, int64_t *counts,
                                 void *workspace, size_t workspace_bytes, void *stream);
int taoamd_track_occlusion_fill(int64_t n_gt, int64_t n_gt_frames, int32_t n_cat,
                                int32_t n_len, int32_t recover, double vis_lo, double vis_hi,
                                const int32_t *len_edges, const int32_t *gt_cat,
                                const uint8_t *gt_flags, const int32_t *gt_frame_off,
                                const double *gt_frame_vis, const int32_t *best,
                                const int64_t *ep_off, int64_t cap, int32_t *episodes,
                                void *workspace, size_t workspace_bytes, void *stream);

/* ---- track-level identity: IDF1 / IDP / IDR (csrc/track_identity.hip) ----------------
 * The association above is many-to-one: one detection track may be the primary
 * of several ground-truth tracks, and a ground truth's covered frames may be
 * spread over many ids.  The identity measures (Ristani et al., ECCV 2016) ask
 * the global question: each ground-truth track may own ONE detection track and
 * each detection track at most one ground truth -- how many frames can be
 * explained?  A maximum-weight bipartite assignment per cell.  The reference has
 * no counterpart; the definition is this library's.  Track level, boxes.
 *
 * Rows are those of the use_cats = 1 track table, as for
 * taoamd_track_association.  A cell is (video, category) with D detection-track
 * rows and G ground-truth rows; F_d and L_g are their frame counts.
 *   share[cell_iou_off[cell] + d_local * G + g_local]  int32: the frames k of g
 *               on which d has a frame at p_k and box_iou(d's box there, b_k) >=
 *               frame_thr -- box_iou has the bits of taoamd_bb_iou (not crowd,
 *               the detection first); a NaN is no overlap.  Counted for EVERY
 *               pair of the cell, ignored ground truths included.  frame_thr: any
 *               double in (0, 1].  Elementwise, share >= follow of the
 *               association at the same threshold.
 *   eligible    g whose gt_flags lacks TAOAMD_GT_IGNORE; other flags do not matter.
 *   set aside   a detection track d is neither a candidate nor counted if
 *               (a) its greatest share with an ignored ground truth of the cell
 *                   is strictly greater than its greatest share with an eligible
 *                   one (it follows something that is not evaluated), or
 *               (b) dt_flags[d] has TAOAMD_DT_IGNORE_UNMATCHED and its share
 *                   with every eligible ground truth is 0 (so also in a cell
 *                   without ground truth).
 *               Every other d is KEPT.  Both rules read share alone, never the
 *               assignment: the counts below are unique.
 *   assignment  a set of pairs (kept d, eligible g) of one cell, each d and each
 *               g at most once, that maximises the sum of share.  IDTP(cell) is
 *               that maximum, a unique integer.  Where several assignments
 *               reach it ([[2, 1], [1, 0]]: 2 + 0 and 1 + 1), the one with the
 *               most pairs of share > 0 is taken, so that their number is
 *               unique too.
 * Per category, cat_counts int64[n_cat][6]:
 *   0 gt_tracks   the eligible ground-truth tracks
 *   1 gt_frames   the sum of their L_g
 *   2 dt_tracks   the kept detection tracks (category: the dt_cat column; cells
 *                 without ground truth count too)
 *   3 dt_frames   the sum of their F_d
 *   4 idtp        the cells' IDTP summed
 *   5 pairs       the assigned pairs with share > 0
 * Rows with a category outside [0, n_cat) count nowhere.  IDFN = gt_frames -
 * idtp, IDFP = dt_frames - idtp; the caller forms IDR = idtp / gt_frames, IDP =
 * idtp / dt_frames, IDF1 = 2 idtp / (gt_frames + dt_frames).
 * Per track: gt_ident int32[n_gt][2] = {the assigned detection row or -1, its
 * share} -- {-1, 0} for an ignored or unassigned g, and a pair of share 0 is
 * reported as unassigned --; dt_ident int32[n_dt][2] = {the assigned ground-truth
 * row or -1, kept ? 1 : 0}.  Rows no cell lists hold {-1, 0}.  Under ties the
 * optimal assignment is not unique; any optimal one is correct, and the one
 * returned is a function of the input alone: one wavefront owns a cell, equal
 * minima go to the lowest column, and no atomic decides anything -- the same from
 * run to run.  Every output is an integer; share and cat_counts are integer adds,
 * whose sum does not depend on the order of arrival.
 *
 * Two calls, so that each kernel can be driven alone.
 * taoamd_track_identity_share zeroes and fills share from the cell tables and the
 * CSR frame lists of taoamd_track_association: a lane per ground-truth frame
 * walks its cell's detection tracks; no tile of the pair matrix, no limit on D, G
 * or a track's length.
 * taoamd_track_identity_assign reads share (any int32 table in that layout; a
 * negative word reads as 0) and the columns, and writes cat_counts, gt_ident,
 * dt_ident and one int32 *status (device): a wavefront per cell marks eligible
 * and kept rows, keeps the rows and columns with a positive share, takes the
 * smaller side as rows and runs the shortest-augmenting-path search (potentials
 * in 64 bits; the state in LDS where the larger side is <= 256, else in the
 * cell's slice of the workspace).  There is no size limit and no
 * TAOAMD_ERR_TOO_LARGE.  Every loop has a bound known at entry; were one ever
 * exhausted, the wavefront stores 1 to *status, leaves the cell's pairs at -1 and
 * returns; nothing spins.  The potentials are sums of up to n weights share *
 * (n + 1) + 1 (n: the smaller side of the cell after compaction), in 64 bits: a
 * cell with n * (n + 1) * (its greatest share + 1) >= 2^62 is not solved but
 * stores 2 to *status (a share of taoamd_track_identity_share is at most a
 * track's frames: such tables are far inside).  *status is 0 otherwise.
 * TAOAMD_ERR_ARG: frame_thr outside (0, 1] (a NaN included), a size below 0 or
 * beyond int32, n_cat <= 0, a missing table; TAOAMD_ERR_WORKSPACE: fewer bytes
 * than taoamd_track_identity_workspace(n_dt, n_gt, n_gt_frames), one size for both
 * calls (the association's frame index, built by the same code of
 * csrc/track_frames.hpp, and 40 bytes of search state per row; any base address, contents need not be initialised, and nothing is
 * carried from one call to the other; the size function answers 0 to sizes it
 * refuses).  Both are answered before the first device call.  Rows and frames
 * named by the tables that lie outside them are skipped, never dereferenced. */
size_t taoamd_track_identity_workspace(int64_t n_dt, int64_t n_gt, int64_t n_gt_frames);
int taoamd_track_identity_share(int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou,
                                int64_t n_dt_frames, int64_t n_gt_frames, double frame_thr,
                                const int32_t *cell_dt_off, const int32_t *cell_gt_off,
                                const int64_t *cell_iou_off, const int32_t *dt_frame_off,
                                const int32_t *dt_frame_pos, const double *dt_frame_box,
                                const int32_t *gt_frame_off, const int32_t *gt_frame_pos,
                                const double *gt_frame_box, int32_t *share, void *workspace,
                                size_t workspace_bytes, void *stream);
int taoamd_track_identity_assign(int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou,
                                 int64_t n_dt_frames, int64_t n_gt_frames, int32_t n_cat,
                                 const int32_t *cell_dt_off, const int32_t *cell_gt_off,
                                 const int64_t *cell_iou_off, const int32_t *gt_cat,
                                 const uint8_t *gt_flags, const int32_t *dt_cat,
                                 const uint8_t *dt_flags, const int32_t *dt_frame_off,
                                 const int32_t *gt_frame_off, const int32_t *share,
                                 int64_t *cat_counts, int32_t *gt_ident, int32_t *dt_ident,
                                 int32_t *status, void *workspace, size_t workspace_bytes,
                                 void *stream);

/* ---- track-level HOTA: HOTA / DetA / AssA (csrc/track_hota.hip) ----------------------
 * The association is a per-frame arg-max (many-to-one), the identity one
 * assignment per cell over whole tracks.  HOTA (Luiten et al., IJCV 2021) asks
 * for a ONE-TO-ONE assignment per FRAME, weighted by how well each pair of tracks
 * aligns over the whole video, and then for an association score per matched
 * pair.  The reference has no counterpart; the definition is this library's,
 * after TrackEval's HOTA class.  Track level, boxes.
 *
 * Every device output is an integer (match_iou: one box_iou value) and identical
 * from run to run; no float is ever added atomically.  HOTA's sums are
 * fractional, so they are carried in fixed point: ONE = 2^30 (TAOAMD_HOTA_ONE),
 * q(x) = (int64) rint(x * ONE) for x in [0, 1].
 *
 * Rows and cells are those of taoamd_track_association; L_g and F_d are the
 * tracks' frame counts.
 *   eligible    g whose gt_flags lacks TAOAMD_GT_IGNORE: the ground truths that
 *               take part.
 *   kept        d with dt_keep[d] != 0 (uint8[n_dt]; NULL: every d): the detection
 *               tracks that take part.  The class layer passes the `kept` column
 *               of taoamd_track_identity_assign, so HOTA and IDF1 are computed
 *               over the same tracks and the set-aside rules are stated once.
 *   frame group (cell, timeline position p): Gp = the eligible ground truths of
 *               the cell with a frame at p, Dp = the kept detection tracks of the
 *               cell with a frame at p, both in ascending row.
 *   s, c(s)     s = box_iou(d's box at p, g's box at p), the bits of taoamd_bb_iou;
 *               c(s) = 0 unless s > 0 (a NaN is 0), else min(s, 1).
 * ALIGN.  In double, each sum added in ascending row from 0.0 (so whichever lane
 * forms it gets the same bits): rowsum_g = the sum of c(s) over d in Dp, colsum_d
 * = the sum of c(s) over g in Gp, den = (rowsum_g + colsum_d) - c(s), a = den >
 * 2^-52 ? min(c(s) / den, 1) : 0.  pot[cell_iou_off[cell] + d_local * G + g_local]
 * int64 = the sum over the group's positions of q(a): only the integer q(a) is
 * accumulated across frames.  0 for every pair of an ignored g or a d not kept.
 * GLOBAL ALIGNMENT.  P = (double) pot / ONE; gas = pot > 0 ? P / ((L_g + F_d) - P)
 * : 0, read as 0 where it is not positive and as 1 above 1 (no table of the align
 * call gives either).
 * MATCH, per frame group.  w(g, d) = q(gas * c(s)) <= 2^30.  Rows and columns
 * without a positive w drop out; the smaller side becomes the solver's rows (the
 * ground truths when equal); the assignment maximises the sum of w, a unique
 * integer; a pair with w = 0 is unassigned.  Equal minima go to the lowest column,
 * as in the identity's solver (the same code): the assignment returned is a
 * function of the input alone.  It is made ONCE per frame, not once per alpha.
 *   alphas      double[n_alpha] (HOST memory), strictly ascending, 1 <= n_alpha <=
 *               TAOAMD_TRACK_HOTA_ALPHAS; the caller has subtracted TrackEval's eps.
 *   mc, lc      for an assigned pair and every a with c(s) >= alphas[a]:
 *               mc[a][pair] += 1 (int32[n_alpha][n_iou]), lc[a][pair] += q(c(s))
 *               (int64[n_alpha][n_iou]).
 *   match       int32[n_gt_frames]: the in-cell index of the assigned d, or -1;
 *               match_iou double[n_gt_frames] (may be NULL): its s, or 0.0.
 *   status      int32 (device): 0; 1 if a loop bound of the solver ran out (then
 *               that group's frames stay at -1).  Weights of at most 2^30 and fewer
 *               than 2^31 rows cannot overflow 64-bit potentials.
 * REDUCE, per category (gt_cat) and alpha over the pairs of eligible g with m =
 * mc[a][pair] > 0: tp += m; loc += lc[a][pair]; ass[0] += q'(m * r(m, (L_g + F_d)
 * - m)); ass[1] += q'(m * r(m, L_g)); ass[2] += q'(m * r(m, F_d)), with r(m, x) =
 * x > 0 ? min(m / x, 1) : 0 and q'(x) = (int64) rint(x * ONE).  tp int64[n_cat]
 * [n_alpha], loc int64[n_cat][n_alpha], ass int64[n_cat][n_alpha][3]; categories
 * outside [0, n_cat) count nowhere.  With all sizes inside int32, a category's m
 * add up to fewer than 2^31 frames and every term is at most m * ONE: every sum
 * stays below 2^62.
 * The caller forms the ratios: FN = gt_frames - tp, FP = dt_frames - tp (the frame
 * counts of taoamd_track_identity_assign's cat_counts); DetA = tp / max(1, tp + FN
 * + FP), DetRe = tp / max(1, tp + FN), DetPr = tp / max(1, tp + FP); AssA = ass[0]
 * / ONE / max(1, tp), AssRe and AssPr from ass[1] and ass[2]; LocA = loc / ONE /
 * tp; HOTA = sqrt(DetA * AssA).
 *
 * Three calls, so that each kernel can be driven alone; one workspace size
 * (taoamd_track_hota_workspace answers 0 to sizes it refuses; any base address,
 * contents need not be initialised, nothing is carried from call to call).
 * taoamd_track_hota_align zeroes and fills pot.  taoamd_track_hota_match reads pot
 * (any int64 table in that layout; a negative word reads 0) and zeroes / fills
 * mc, lc, match, match_iou and status.  taoamd_track_hota_reduce reads mc and lc
 * (any tables in that layout; mc words <= 0 are skipped) and zeroes / fills tp,
 * loc and ass.  There is no size limit and no TAOAMD_ERR_TOO_LARGE; every loop
 * has a bound known at entry; nothing spins.
 * TAOAMD_ERR_ARG: a size below 0 or beyond int32, n_cat <= 0, n_alpha outside [1,
 * 32], alphas that do not strictly ascend or hold a NaN, a missing table;
 * TAOAMD_ERR_WORKSPACE: fewer bytes than the size reported.  Both are answered
 * before the first device call.  Rows and frames named by the tables that lie
 * outside them are skipped, never dereferenced; n_gt == 0 returns after the
 * zeroing. */
#define TAOAMD_HOTA_ONE 1073741824          /* 2^30: the fixed point of the HOTA sums */
#define TAOAMD_TRACK_HOTA_ALPHAS 32         /* localisation thresholds, at most */
size_t taoamd_track_hota_workspace(int64_t n_dt, int64_t n_gt, int64_t n_gt_frames);
int taoamd_track_hota_align(int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou,
                            int64_t n_dt_frames, int64_t n_gt_frames,
                            const int32_t *cell_dt_off, const int32_t *cell_gt_off,
                            const int64_t *cell_iou_off, const uint8_t *gt_flags,
                            const uint8_t *dt_keep, const int32_t *dt_frame_off,
                            const int32_t *dt_frame_pos, const double *dt_frame_box,
                            const int32_t *gt_frame_off, const int32_t *gt_frame_pos,
                            const double *gt_frame_box, int64_t *pot, void *workspace,
                            size_t workspace_bytes, void *stream);
int taoamd_track_hota_match(int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou,
                            int64_t n_dt_frames, int64_t n_gt_frames, int32_t n_alpha,
                            const double *alphas, const int32_t *cell_dt_off,
                            const int32_t *cell_gt_off, const int64_t *cell_iou_off,
                            const uint8_t *gt_flags, const uint8_t *dt_keep,
                            const int32_t *dt_frame_off, const int32_t *dt_frame_pos,
                            const double *dt_frame_box, const int32_t *gt_frame_off,
                            const int32_t *gt_frame_pos, const double *gt_frame_box,
                            const int64_t *pot, int32_t *mc, int64_t *lc, int32_t *match,
                            double *match_iou, int32_t *status, void *workspace,
                            size_t workspace_bytes, void *stream);
int taoamd_track_hota_reduce(int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou,
                             int64_t n_dt_frames, int64_t n_gt_frames, int32_t n_cat,
                             int32_t n_alpha, const int32_t *cell_dt_off,
                             const int32_t *cell_gt_off, const int64_t *cell_iou_off,
                             const int32_t *gt_cat, const uint8_t *gt_flags,
                             const int32_t *dt_frame_off, const int32_t *gt_frame_off,
                             const int32_t *mc, const int64_t *lc, int64_t *tp, int64_t *loc,
                             int64_t *ass, void *workspace, size_t workspace_bytes,
                             void *stream);

/* ---- track-level CLEAR: MOTA / MOTP / IDSW (csrc/track_clear.hip) --------------------
 * The third of the measures printed beside Track-AP (Bernardin & Stiefelhagen,
 * 2008): a ONE-TO-ONE assignment per frame, as HOTA's, but each frame's weights
 * depend on the frame before -- the pair matched a step ago gets a bonus -- and an
 * ID switch is scored against the last match however long ago it was.  The
 * frames of a cell are a serial chain.  The reference has no counterpart; the
 * definition is this library's, after TrackEval's CLEAR class; it is not
 * TrackEval's TAO number, for the reasons given for HOTA (no preprocessing of the
 * TAO kind).  Track level, boxes.
 *
 * Rows, cells, frame lists, `eligible`, `kept` (dt_keep, NULL: every d), s, c(s)
 * and q are those of track-level HOTA above: MOTA, IDF1 and HOTA are computed over
 * the same tracks and the same gt_frames / dt_frames.
 *   candidate   at a timeline position p the pair (eligible g, kept d) of one cell,
 *               both with a frame at p, with s >= frame_thr and q(c(s)) > 0.  A NaN
 *               is no candidate.  frame_thr: any double in (0, 1].
 *   step        a position of a cell at which at least one eligible ground truth
 *               AND at least one kept detection track of the cell have a frame
 *               (candidates are not required).  A cell's steps are taken in
 *               ascending position.  A position that is no step changes no state
 *               (TrackEval `continue`s there before it touches anything): a track
 *               with holes, or a position without any detection frame of the
 *               cell, does not reset continuity.
 *   state       per eligible g of the cell, both none at first: prev[g], its match
 *               at the cell's previous step; last[g], its most recent match at
 *               any earlier step.
 * A STEP.  w(g, d) = q(c(s)) + (d == prev[g] ? 1000 * 2^30 : 0) for a candidate, 0
 * (no edge) otherwise; a weight is below 2^41.  The step's match is the one-to-one
 * set of pairs with w > 0 that maximises the sum of w, a unique integer.  Among
 * equal sums the solver's choice holds, a function of the input alone, and it
 * feeds later steps, so it is stated: the ROWS are the ground truths of the step
 * with at least one candidate, in ascending row; the COLUMNS are the detection
 * rows those candidates name, in ascending row; the smaller side becomes the
 * solver's rows (the ground truths when equal); shortest augmenting paths, a row
 * at a time in that order, equal minima to the lowest column (assign_solve.hpp,
 * the code of the identity and HOTA).  One row needs no solver: the candidate
 * equal to prev if there is one, else the greatest q, the first of the list among
 * equals -- which is what the solver returns for it.
 * For a matched (g, d): an ID switch is counted (and sw set at the frame) if
 * last[g] is not none and last[g] != d; then last[g] = d.  For EVERY eligible g of
 * the cell, present at the step or not, prev[g] becomes its match at this step or
 * none; started[g] is incremented where prev[g] was none and now is not.
 * Per ground-truth track, gt_clear int32[n_gt][4] = {present, matched, idsw,
 * started}: present = its frames (all of them, steps or not), matched = its
 * matched frames; zeros for an ignored row.  frag = max(started - 1, 0); mostly
 * tracked iff 5 * matched > 4 * present, partly tracked iff not mostly tracked and
 * 5 * matched >= present, mostly lost otherwise (TrackEval's > 0.8 and >= 0.2).
 * Per category (gt_cat), cat_counts int64[n_cat][7] = {tp, idsw, frag, mt, pt, ml,
 * motp_sum} over the eligible tracks: tp = the matched frames, motp_sum = the sum
 * of q(c(s)) over the matches.  The caller forms fn = gt_frames - tp, fp =
 * dt_frames - tp (the frame counts of taoamd_track_identity_assign's cat_counts;
 * positions without a ground truth need no visit), MOTA = (tp - fp - idsw) /
 * max(1, tp + fn), MOTP = motp_sum / 2^30 / max(1, tp).
 * By visibility, vis_counts int64[n_vis][n_cat][4] = {frames, matched, idsw,
 * q sum}: the association's windows -- n_vis <= 8 closed windows vis_rng
 * double[n_vis][2] (device), they may overlap, a NaN visibility lies in none --
 * over the eligible tracks' frames: the frames in the window, the matched ones,
 * those with sw set, the q of those matches.  Categories outside [0, n_cat)
 * count nowhere.
 *
 * Three stages, each of which can be driven alone; one workspace size
 * (taoamd_track_clear_workspace answers 0 to sizes it refuses; any base address,
 * contents need not be initialised, nothing is carried from call to call).
 * CANDIDATES, in parallel, count then fill.  taoamd_track_clear_count fills the
 * whole of cand_off int64[n_gt_frames + 1], the exclusive prefix sum of the
 * frames' candidate counts (cand_off[n_gt_frames] = n_cand), and step
 * uint8[n_gt_frames]: 1 where some kept detection track of the cell has a frame
 * at the position of the (eligible track's) frame -- the step bit; a frame of an
 * ignored track has no candidates and no bit.  taoamd_track_clear_fill, with the
 * same tables, stores per candidate, at the frame's place and in ascending row,
 * cand_row int32 (the in-cell detection row), cand_q int32 (q(c(s)), in (0, 2^30])
 * and, if not NULL, cand_iou double (s); nothing at or beyond entry n_cand.
 * WALK.  taoamd_track_clear_walk reads the cell tables, the ground-truth frame
 * lists' offsets and positions, the step bits and the candidate store (any tables
 * in that layout: a row outside the cell or a q <= 0 is no candidate, a q above
 * 2^30 reads 2^30; lists are taken to ascend in row), never a box.  It fills
 * match int32[n_gt_frames] (the in-cell detection row or -1), match_iou
 * double[n_gt_frames] (may be NULL; the cand_iou of the match, 0.0 where
 * unmatched or cand_iou is NULL), sw uint8[n_gt_frames], gt_clear and one int32
 * *status (device): 0; 1 if a loop bound of the solver ran out (that step is
 * left unmatched); 2 if a cell's smaller side exceeds
 * TAOAMD_TRACK_CLEAR_NMAX = 2^18 -- below it the 64-bit potentials, sums of at
 * most n weights below 2^41 of which the search adds three, stay under 2^61 --:
 * such a cell is not walked, nothing else is computed in its place.
 * REDUCE.  taoamd_track_clear_reduce reads gt_clear (tp, idsw, frag, mt / pt /
 * ml), match, sw, the frames' visibility and the store (motp_sum and the windows'
 * q: the q of the list entry whose row is the match) and zeroes / fills
 * cat_counts and vis_counts.  n_vis = 0 with vis_rng, gt_frame_vis and vis_counts
 * NULL is allowed.  Integer adds only.
 * Every output is zeroed / filled by its call; every loop has a bound known at
 * entry; nothing spins.  TAOAMD_ERR_ARG: frame_thr outside (0, 1] (a NaN
 * included), n_vis outside [0, 8], windows without visibilities, a size below 0
 * or beyond int32, n_cat <= 0, a missing table; TAOAMD_ERR_WORKSPACE: fewer bytes
 * than the size reported.  Both are answered before the first device call and
 * leave every output untouched.  Rows, frames and candidates named by the
 * tables that lie outside them are skipped, never dereferenced. */
#define TAOAMD_TRACK_CLEAR_BONUS 1000       /* times 2^30: the weight of continuity */
#define TAOAMD_TRACK_CLEAR_NMAX 262144      /* 2^18: the smaller side of a cell, at most */
size_t taoamd_track_clear_workspace(int64_t n_dt, int64_t n_gt, int64_t n_gt_frames);
int taoamd_track_clear_count(int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_dt_frames,
                             int64_t n_gt_frames, double frame_thr, const int32_t *cell_dt_off,
                             const int32_t *cell_gt_off, const uint8_t *gt_flags,
                             const uint8_t *dt_keep, const int32_t *dt_frame_off,
                             const int32_t *dt_frame_pos, const double *dt_frame_box,
                             const int32_t *gt_frame_off, const int32_t *gt_frame_pos,
                             const double *gt_frame_box, int64_t *cand_off, uint8_t *step,
                             void *workspace, size_t workspace_bytes, void *stream);
int taoamd_track_clear_fill(int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_dt_frames,
                            int64_t n_gt_frames, double frame_thr, const int32_t *cell_dt_off,
                            const int32_t *cell_gt_off, const uint8_t *gt_flags,
                            const uint8_t *dt_keep, const int32_t *dt_frame_off,
                            const int32_t *dt_frame_pos, const double *dt_frame_box,
                            const int32_t *gt_frame_off, const int32_t *gt_frame_pos,
                            const double *gt_frame_box, const int64_t *cand_off, int64_t n_cand,
                            int32_t *cand_row, int32_t *cand_q, double *cand_iou,
                            void *workspace, size_t workspace_bytes, void *stream);
int taoamd_track_clear_walk(int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_gt_frames,
                            int64_t n_cand, const int32_t *cell_dt_off,
                            const int32_t *cell_gt_off, const uint8_t *gt_flags,
                            const int32_t *gt_frame_off, const int32_t *gt_frame_pos,
                            const int64_t *cand_off, const int32_t *cand_row,
                            const int32_t *cand_q, const double *cand_iou, const uint8_t *step,
                            int32_t *match, double *match_iou, uint8_t *sw, int32_t *gt_clear,
                            int32_t *status, void *workspace, size_t workspace_bytes,
                            void *stream);
int taoamd_track_clear_reduce(int64_t n_dt, int64_t n_gt, int64_t n_gt_frames, int64_t n_cand,
                              int32_t n_cat, int32_t n_vis, const int32_t *gt_cat,
                              const uint8_t *gt_flags, const int32_t *gt_frame_off,
                              const double *gt_frame_vis, const double *vis_rng,
                              const int64_t *cand_off, const int32_t *cand_row,
                              const int32_t *cand_q, const int32_t *match, const uint8_t *sw,
                              const int32_t *gt_clear, int64_t *cat_counts,
                              int64_t *vis_counts, void *workspace, size_t workspace_bytes,
                              void *stream);

/* ---- track-level score thresholds (csrc/track_identity.hip) --------------------------
 * The track tables hold every detection track up to the max_dets cut, whatever
 * its score: Track-AP integrates over the ranking.  The identity, HOTA and CLEAR
 * need an operating point -- "the tracks at or above a score".  WHOLE tracks are
 * thresholded, by the score Track-AP ranks them by; a box is never dropped from
 * a track.  The reference has no counterpart; the definition is this library's.
 *
 * The pass rule.  The score of detection track d is dt_score[d], the column of
 * the track table (the mean the table build forms).  A threshold table is
 * thr double[n_thr][n_cat] (device), 1 <= n_thr <= TAOAMD_TRACK_SCORE_THRS; a row
 * is a LAYER.  d passes layer t iff
 *     0 <= dt_cat[d] < n_cat,
 *     dt_score[d] >= thr[t][dt_cat[d]]   (an IEEE comparison: a NaN on either
 *                                         side does not pass, -inf passes every
 *                                         score that is not a NaN, -0.0 >= 0.0
 *                                         passes), and
 *     base is NULL or base[d] != 0       (uint8[n_dt]: a column to AND with, as
 *                                         the identity's kept column).
 * taoamd_track_score_pass fills pass uint8[n_thr][n_dt] with 0 or 1 and writes
 * nothing else; a lane per (layer, track).  n_dt = 0 is allowed (nothing is
 * launched).  TAOAMD_ERR_ARG, before any device call: n_dt below 0 or beyond
 * int32, n_cat <= 0, n_thr outside [1, TAOAMD_TRACK_SCORE_THRS], thr NULL, or
 * n_dt > 0 and dt_score, dt_cat or pass NULL.  A layer of pass is a dt_keep
 * column of taoamd_track_hota_* and taoamd_track_clear_*.
 *
 * The layered identity assignment.  taoamd_track_identity_assign_at takes the
 * arguments of taoamd_track_identity_assign, n_thr after n_cat and dt_pass
 * uint8[n_thr][n_dt] after dt_flags, and its outputs gain a leading layer axis:
 * cat_counts int64[n_thr][n_cat][6], gt_ident int32[n_thr][n_gt][2] (may be
 * NULL: not written), dt_ident int32[n_thr][n_dt][2].  Layer t is the
 * identity's assignment over the detection tracks with dt_pass[t][d] != 0: a
 * track that does not pass is neither a candidate nor counted, and its dt_ident
 * is {-1, 0}.  The set-aside rules (a) and (b) read a track's OWN shares alone,
 * so the tracks kept at layer t are those kept without a threshold AND passing:
 *     kept_t[d] = kept[d] && dt_pass[t][d] != 0;
 * the eligible ground truths and gt_tracks / gt_frames are the same in every
 * layer.  EXACTLY: layer t is, word for word in cat_counts, gt_ident and
 * dt_ident, what taoamd_track_identity_assign writes for the input in which the
 * share rows of the tracks with dt_pass[t][d] == 0 are zeroed and
 * TAOAMD_DT_IGNORE_UNMATCHED is set in their dt_flags (rule (b) sets them
 * aside).  Word for word, not only in the counts, because rows without a
 * positive share are compacted away before the solver runs: both inputs hand it
 * the same rows and columns in the same order.
 * The kernel is that of taoamd_track_identity_assign with the layer as the
 * launch's second index: a wavefront per (cell, layer), the same LDS state per
 * wavefront; the cells whose larger side exceeds 256 have a slice of the search
 * store per layer, and every cell a slice of the index lists per layer.
 * taoamd_track_identity_assign is the one-layer instance without a mask.  One
 * int32 *status holds the GREATEST code any (cell, layer) stored (an atomic
 * max), 0 otherwise.  No size limit, no TAOAMD_ERR_TOO_LARGE; every loop has a
 * bound known at entry, and nothing spins.  share is read, never written: one
 * taoamd_track_identity_share serves every layer.
 * TAOAMD_ERR_ARG: what taoamd_track_identity_assign refuses (gt_ident excepted),
 * n_thr outside [1, TAOAMD_TRACK_SCORE_THRS], n_dt > 0 and dt_pass NULL;
 * TAOAMD_ERR_WORKSPACE: fewer bytes than
 * taoamd_track_identity_layers_workspace(n_dt, n_gt, n_gt_frames, n_thr) (the
 * identity's workspace with n_thr slices of the 40 + 4 bytes per row; it answers
 * 0 to sizes it refuses, and for n_thr = 1 what taoamd_track_identity_workspace
 * answers).  Both are answered before the first device call, with every output
 * untouched. */
#define TAOAMD_TRACK_SCORE_THRS 64          /* layers of a threshold table, at most */
int taoamd_track_score_pass(int64_t n_dt, int32_t n_cat, int32_t n_thr, const double *dt_score,
                            const int32_t *dt_cat, const double *thr, const uint8_t *base,
                            uint8_t *pass, void *stream);
size_t taoamd_track_identity_layers_workspace(int64_t n_dt, int64_t n_gt, int64_t n_gt_frames,
                                              int32_t n_thr);
int taoamd_track_identity_assign_at(int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou,
                                    int64_t n_dt_frames, int64_t n_gt_frames, int32_t n_cat,
                                    int32_t n_thr, const int32_t *cell_dt_off,
                                    const int32_t *cell_gt_off, const int64_t *cell_iou_off,
                                    const int32_t *gt_cat, const uint8_t *gt_flags,
                                    const int32_t *dt_cat, const uint8_t *dt_flags,
                                    const uint8_t *dt_pass, const int32_t *dt_frame_off,
                                    const int32_t *gt_frame_off, const int32_t *share,
                                    int64_t *cat_counts, int32_t *gt_ident, int32_t *dt_ident,
                                    int32_t *status, void *workspace, size_t workspace_bytes,
                                    void *stream);

/* ---- multi-GPU result exchange (category-partitioned evaluation) -------------------
 * No reference counterpart (the reference is single-process); these carry the
 * tables of taoamd_accumulate_compact between ranks and end in the layout of
 * taoamd_finalize, i.e. of `eval["precision"]` / `eval["recall"]`
 * (lvis_amodal/eval.py:366-371,420-426, tao_amodal/eval.py:521-526,576-584).
 * Rank b owns the categories [b * block_cats, (b+1) * block_cats); a row is a
 * (category, range) pair, global row = category * n_rng + range.
 *
 * A chunk holds one rank's share: the num_gt, level offset and rec of its rows and, per row
 * with num_gt > 0 and per IoU threshold, the distinct runs ("levels") of the
 * 101 recall columns -- a row with n ground truths has at most min(n,100)+1
 * of them, and which columns coincide follows from n alone, so receivers
 * rebuild the map from the chunk header.  Chunks of all ranks have
 * taoamd_exchange_chunk_bytes(block_cats, n_rng, capacity) bytes and sit
 * back to back in `chunks` (one in-place all-gather moves them).
 *  _sizes   levels needed by every block (device int64[world]) from the
 *           gathered num_gt[world * block_cats][n_rng]; capacity = their max
 *  _pack    own rows of val / rec / num_gt (tables addressed by GLOBAL row,
 *           as written by taoamd_accumulate_compact) -> `chunk` (this rank's)
 *  _unpack  all chunks -> precision[T][R][n_cat][n_rng], recall[T][n_cat][n_rng]
 *           (-1 fill) and optionally the assembled num_gt[n_cat][n_rng]
 * *overflow (device int32, may be NULL) is OR-ed with 1 if a block needs more
 * than `capacity` levels (the excess is dropped, results are then invalid).
 * maps_ready != 0: the run maps and level offsets of ALL rows are already in
 * the workspace -- a _sizes call on the num_gt of all rows earlier in the
 * pass (a rank of the by-video partition knows them from its all-reduce, long
 * before the sweep ends) -- so _pack / _unpack start their copy at once.
 * Workspace: taoamd_exchange_workspace(block_cats, n_rng, world). */
size_t taoamd_exchange_chunk_bytes(int32_t block_cats, int32_t n_rng, int64_t capacity);
size_t taoamd_exchange_workspace(int32_t block_cats, int32_t n_rng, int32_t world);
int taoamd_exchange_sizes(int32_t block_cats, int32_t n_rng, int32_t world,
                          const int32_t *num_gt, int64_t *totals, void *workspace,
                          size_t workspace_bytes, void *stream);
int taoamd_exchange_pack(int32_t n_cat, int32_t n_rng, int32_t block_cats,
                         int32_t world, int32_t rank, const int32_t *num_gt,
                         const double *val, const double *rec, void *chunk,
                         int64_t capacity, int32_t *overflow, void *workspace,
                         size_t workspace_bytes, int32_t maps_ready, void *stream);
int taoamd_exchange_unpack(int32_t n_cat, int32_t n_rng, int32_t block_cats,
                           int32_t world, const void *chunks, int64_t capacity,
                           int32_t *num_gt_out, double *precision, double *recall,
                           int32_t *overflow, void *workspace,
                           size_t workspace_bytes, int32_t maps_ready, void *stream);

/* By-video partition, owner side (round 5: in two messages).  A rank's records
 * lie at their sorted place (category, -score): the sort gives the place, the
 * match writes a detection's (matched, ignored) pairs there.  The merged input
 * of an owner is, for source s, the rows [src_base[s], src_base[s + 1]) -- the
 * wire buffer = what the all_to_all delivered, the sources' rows back to back
 * WITHOUT those of `own_rank` (>= 0), which never travel: they are read where
 * the rank's own sort / match wrote them (own_rank < 0: every source's rows
 * are in the wire buffer).  A record carries no category, the run it lies in
 * says it: run_off[s * (block_cats + 1) + kb] = offset of the run of the
 * block's category kb inside source s's rows; cat_base[kb] = first row of that
 * category in the merged layout.
 *  _scores     out[dst[i]] = score[i] (bit patterns): the first message, ready
 *              when the local sort is;
 *  _positions  pos[i] = row of record i in the reference's order (stable -score
 *              sort of the sources' concatenation in rank order,
 *              L/eval.py:353-361): one binary search per other source over the
 *              exchanged scores instead of a radix sort -- needs the scores
 *              alone, so it runs beside the match;
 *  _place      the second message's 16-byte (matched, ignored) pairs scattered
 *              to out[pos[i] * n_words + w]: the paired table the sweep reads
 *              (out, out + 1 as taoamd_accumulate*'s matched / ignored). */
int taoamd_exchange_scores(int64_t n, const int32_t *dst, const double *score,
                           int64_t *out, void *stream);
int taoamd_exchange_positions(int64_t n_recv, int32_t world, int32_t block_cats,
                              const int64_t *scores, const int64_t *own_scores,
                              int32_t own_rank, const int64_t *src_base,
                              const int64_t *run_off, const int64_t *cat_base,
                              int32_t *pos, void *stream);
int taoamd_exchange_place(int64_t n_recv, int32_t world, int32_t n_words,
                          const uint64_t *rows, const uint64_t *own_rows,
                          int32_t own_rank, const int64_t *src_base,
                          const int32_t *pos, uint64_t *out, void *stream);

/* ---------------------------------------------------------------------------
 * The prediction file read on the device (csrc/json_ingest.hip): replaces the
 * reference's json.load of prediction.json (lvis_amodal/results.py:29-30,
 * tools/eval_on_tao_amodal.py:127-128) for the six keys of a prediction.
 *
 * taoamd_json_pred_open copies the file's text into HBM, finds the list's
 * objects (string state, bracket depth and object count of 16 KB blocks, three
 * prefix sums) and checks the list's shape.  *status: TAOAMD_OK (a handle is
 * returned); TAOAMD_JSON_FALLBACK -- the file holds something this reader leaves
 * to the host's (a backslash, an element that is not an object, text around the
 * list, an empty file): call the host reader (include/tao_amodal_ingest.h),
 * whose results and error messages are the contract; TAOAMD_ERR_ARG -- the file
 * cannot be opened (err says so); TAOAMD_ERR_HIP.  `work` (optional, device
 * memory of taoamd_json_pred_workspace(file size) bytes, the caller's until
 * taoamd_json_pred_close): the text, the tables and the objects' offsets live
 * there instead of in memory the call allocates -- for callers with a pool.
 *
 * taoamd_json_pred_convert converts the objects (one thread each; decimal ->
 * double correctly rounded, csrc/decfloat.hpp) into the caller's DEVICE arrays of
 * taoamd_json_pred_count() rows (bbox: 4 doubles a row) and returns when they
 * are written; taoamd_json_pred_read does the same into HOST arrays.
 * Objects left to the host reader -- literals, numbers of more than 19
 * digits, ids that are not plain integers, missing keys, unexpected syntax --
 * are listed (HOST arrays): flag[k] = the object's number, flag_at[k] = the byte
 * offset of its '{' in the file, for the first flag_cap of *n_flagged; their
 * rows are not written (taoamd_pred_patch of the host library fills them in
 * host arrays or reports the error).  More than flag_cap: use the host reader
 * for the file. */
size_t taoamd_json_pred_workspace(size_t file_bytes);
void *taoamd_json_pred_open(const char *path, void *work, size_t work_bytes,
                            int32_t *status, char *err, size_t errlen, void *stream);
int64_t taoamd_json_pred_count(void *handle);
int taoamd_json_pred_convert(void *handle, int64_t *image_id, int64_t *category_id,
                             double *bbox, double *score, int64_t *track_id,
                             int64_t *video_id, int64_t *flag, int64_t *flag_at,
                             int32_t flag_cap, int32_t *n_flagged);
int taoamd_json_pred_read(void *handle, int64_t *image_id, int64_t *category_id,
                          double *bbox, double *score, int64_t *track_id,
                          int64_t *video_id, int64_t *flag, int64_t *flag_at,
                          int32_t flag_cap, int32_t *n_flagged);
void taoamd_json_pred_close(void *handle);

#ifdef __cplusplus
}
#endif
#endif

// Image-level error breakdown per visibility range (gfx950): WHY a detection is
// no true positive.  The reference has no such table (pycocotools users reach
// for TIDE, Bolya et al., ECCV 2020); the definition below is this library's,
// stated again in include/tao_amodal_hip.h and DESIGN.md section 8.
//
// One call = one IoU threshold slot t of the calling thread's iou_thrs
// (tf = min(iou_thrs[t], 1 - 1e-10), the clamp of the match), one background
// threshold tb (0 <= tb < tf), all n_rng <= 8 ranges.  Rows are those of the
// use_cats = 1 cell table.  For detection d (image u, category c), range a:
//   E_a(u) = ground truths of image u, ANY category, with gt_rng bit a clear
//   s      = max box_iou(d, g) over g in E_a(u) of category c, 0 if none;
//            its argmax = the lowest ground-truth row among equal IoUs
//   o      = the same maximum over the other categories
// and exactly one type, the first rule that applies:
//   0 TP       match_gt[d][a * 10 + t] >= 0, that ground truth evaluated in a
//   1 IGNORED  matched to a ground truth ignored in a, or unmatched with
//              TAOAMD_DT_IGNORE_UNMATCHED
//   2 DUP      unmatched, s >= tf
//   3 LOC      unmatched, tb <= s < tf
//   4 CLS      unmatched, o >= tf
//   5 BOTH     unmatched, tb <= o < tf
//   6 BKG      otherwise
// Per (ground truth, range) with the bit clear: evaluated; missed = no
// detection's match_gt names it at (a, t); missed_loc = missed and the
// same-category argmax of at least one LOC detection of range a.
//
//   err_pair_kernel   workgroup = image, lane = detection; the image's ground
//                     truths of every category pass through LDS in tiles of
//                     TAOAMD_ERROR_TYPES_TILE, each IoU is computed once and
//                     folded into the per-range (s, argmax, o) in registers;
//                     writes the type bytes and the ground-truth marks
//   err_count_kernel  lane = detection in TABLE order (category-major: the 64
//                     rows of a wavefront share one or two categories, where
//                     the lanes of an image are spread over all of them): the
//                     counts per (range, category, type) from the type bytes
//   err_tally_kernel  lane = ground truth: the three counts per (range,
//                     category) from the two byte tables the pair kernel marks
// Counts are integers, marks are stores of 1: nothing depends on an order.
// taoamd_error_types_links is the same pass with the pair kernel's LINKS form:
// it also keeps the argmax of o and stores both argmaxes per (detection, range)
// and the held marks in the caller's tables, for error_impact.hip.
#include "common.hpp"
#include "workspace.hpp"

using namespace taoamd;

#define ERR_TILE TAOAMD_ERROR_TYPES_TILE   // ground truths per LDS tile = lanes of a workgroup
#define ERR_RMAX TAOAMD_ERROR_TYPES_MAX_RNG

struct ErrArgs {
    int64_t n_dt, n_gt;
    int32_t n_img, n_cat, n_rng, slot;
    double tf, tb;
    const int32_t *dt_cat;
    const double *dt_box;
    const uint8_t *dt_flags;
    const int32_t *dt_gt0;       // first ground-truth row of the row's cell
    const int32_t *match_gt;
    int64_t match_stride;
    const int32_t *gt_cat;
    const double *gt_box;
    const uint32_t *gt_rng;
    const int32_t *img_gt_off, *img_gt, *img_dt_off, *img_dt;
    unsigned long long *dt_counts;   // [n_rng][n_cat][7]
    unsigned long long *gt_counts;   // [n_rng][n_cat][3]
    uint8_t *types;                  // [n_dt][n_rng]: the caller's dt_type, else the workspace's
    uint8_t *ws_types;
    uint8_t *gt_hit, *gt_loc;        // [n_rng][n_gt]
    int32_t *link_same, *link_other; // [n_dt][n_rng], taoamd_error_types_links only
};

// LINKS: the argmax of o under the rule of s, and both argmaxes stored per
// (detection, range) -- what a fix would hand the detection (error_impact.hip)
template <bool LINKS>
__global__ __launch_bounds__(ERR_TILE) void err_pair_kernel(ErrArgs a)
{
    __shared__ double4 s_box[ERR_TILE];
    __shared__ int4 s_meta[ERR_TILE];      // {category, range mask, row, -}
    const int u = blockIdx.x;
    const int tid = threadIdx.x;
    // (offsets clamped to the tables: a bad CSR reads wrong rows, never past an end)
    const int64_t g_lo = min(max((int64_t)a.img_gt_off[u], (int64_t)0), a.n_gt);
    const int64_t g_hi = min(max((int64_t)a.img_gt_off[u + 1], g_lo), a.n_gt);
    const int64_t d_lo = min(max((int64_t)a.img_dt_off[u], (int64_t)0), a.n_dt);
    const int64_t d_hi = min(max((int64_t)a.img_dt_off[u + 1], d_lo), a.n_dt);
    const uint32_t all = 0xffffffffu >> (32 - a.n_rng);

    for (int64_t d0 = d_lo; d0 < d_hi; d0 += ERR_TILE) {
        int64_t d = d0 + tid < d_hi ? (int64_t)a.img_dt[d0 + tid] : -1;
        if (d >= a.n_dt) d = -1;
        const bool valid = d >= 0;
        double dx = 0, dy = 0, dw = 0, dh = 0;
        int32_t cat = 0, gt0 = 0;
        uint32_t flags = 0;
        int32_t m[ERR_RMAX];
#pragma unroll
        for (int r = 0; r < ERR_RMAX; r++) m[r] = -1;
        if (valid) {
            const double4 B = reinterpret_cast<const double4 *>(a.dt_box)[d];
            dx = B.x; dy = B.y; dw = B.z; dh = B.w;
            cat = a.dt_cat[d];
            gt0 = a.dt_gt0[d];
            flags = a.dt_flags[d];
            const int32_t *row = a.match_gt + d * a.match_stride + a.slot;
#pragma unroll
            for (int r = 0; r < ERR_RMAX; r++)
                if (r < a.n_rng) m[r] = row[r * N_THR];
        }
        double s[ERR_RMAX], o[ERR_RMAX];
        int32_t arg[ERR_RMAX];
        int32_t arg_o[LINKS ? ERR_RMAX : 1];
#pragma unroll
        for (int r = 0; r < ERR_RMAX; r++) { s[r] = 0.0; o[r] = 0.0; arg[r] = -1; }
        if (LINKS) {
#pragma unroll
            for (int r = 0; r < ERR_RMAX; r++) arg_o[LINKS ? r : 0] = -1;
        }

        for (int64_t g0 = g_lo; g0 < g_hi; g0 += ERR_TILE) {
            const int ng = (int)min((int64_t)ERR_TILE, g_hi - g0);
            __syncthreads();                       // the tile before is read
            if (tid < ng) {
                const int32_t row = a.img_gt[g0 + tid];
                const bool ok = row >= 0 && row < a.n_gt;
                // (a row outside the table: ignored in every range)
                s_box[tid] = ok ? reinterpret_cast<const double4 *>(a.gt_box)[row]
                                : make_double4(0, 0, 0, 0);
                s_meta[tid] = make_int4(ok ? a.gt_cat[row] : -1,
                                        (int32_t)(ok ? a.gt_rng[row] : all), row, 0);
            }
            __syncthreads();
            // (a short image leaves whole wavefronts without a detection)
            if (__ballot(valid) == 0) continue;                // (uniform; the barriers stay outside)
            for (int g = 0; g < ng; g++) {
                const double4 G = s_box[g];
                const int4 M = s_meta[g];
                const uint32_t open = ~(uint32_t)M.y & all;   // ranges that evaluate g
                if (open == 0) continue;                       // (uniform)
                const double v = box_iou(dx, dy, dw, dh, G.x, G.y, G.z, G.w);
                const bool same = M.x == cat;
#pragma unroll
                for (int r = 0; r < ERR_RMAX; r++) {
                    const bool in = (open >> r) & 1u;
                    const bool up_s = in && same &&
                        (v > s[r] || (v == s[r] && (uint32_t)M.z < (uint32_t)arg[r]));
                    bool up_o = in && !same && v > o[r];
                    if (LINKS) {
                        const int q = LINKS ? r : 0;
                        up_o = up_o || (in && !same && v == o[r] &&
                                        (uint32_t)M.z < (uint32_t)arg_o[q]);
                        arg_o[q] = up_o ? M.z : arg_o[q];
                    }
                    s[r] = up_s ? v : s[r];
                    arg[r] = up_s ? M.z : arg[r];
                    o[r] = up_o ? v : o[r];
                }
            }
        }

        // ---- classify, mark
#pragma unroll
        for (int r = 0; r < ERR_RMAX; r++) {
            if (r >= a.n_rng) continue;                        // (uniform)
            int ty = ERR_BKG;
            const int64_t grow = (int64_t)gt0 + m[r];
            if (valid && m[r] >= 0 && grow >= 0 && grow < a.n_gt) {
                ty = ((a.gt_rng[grow] >> r) & 1u) ? ERR_IGNORED : ERR_TP;
                a.gt_hit[(int64_t)r * a.n_gt + grow] = 1;
            } else if (flags & TAOAMD_DT_IGNORE_UNMATCHED) {
                ty = ERR_IGNORED;
            } else if (s[r] >= a.tf) {
                ty = ERR_DUP;
            } else if (s[r] >= a.tb) {
                ty = ERR_LOC;
                if (valid && arg[r] >= 0) a.gt_loc[(int64_t)r * a.n_gt + arg[r]] = 1;
            } else if (o[r] >= a.tf) {
                ty = ERR_CLS;
            } else if (o[r] >= a.tb) {
                ty = ERR_BOTH;
            }
            if (valid) a.types[d * a.n_rng + r] = (uint8_t)ty;
            if (LINKS && valid) {
                a.link_same[d * a.n_rng + r] = arg[r];
                a.link_other[d * a.n_rng + r] = arg_o[LINKS ? r : 0];
            }
        }
    }
}

__global__ __launch_bounds__(256) void err_count_kernel(ErrArgs a)
{
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = d < a.n_dt;
    const int32_t cat = valid ? a.dt_cat[d] : 0;
    const bool ok = valid && cat >= 0 && cat < a.n_cat;
#pragma unroll
    for (int r = 0; r < ERR_RMAX; r++) {
        if (r >= a.n_rng) continue;                            // (uniform)
        const int ty = valid ? a.types[d * a.n_rng + r] : 0;
        // (a row no image lists keeps whatever byte the table held)
        wave_count(a.dt_counts + (int64_t)r * a.n_cat * ERR_NTYPE, ok && ty < ERR_NTYPE,
                   cat * ERR_NTYPE + ty);
    }
}

__global__ __launch_bounds__(256) void err_tally_kernel(ErrArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = g < a.n_gt;
    const int32_t cat = valid ? a.gt_cat[g] : 0;
    const uint32_t rng = valid ? a.gt_rng[g] : 0xffffffffu;
    const bool ok = valid && cat >= 0 && cat < a.n_cat;
#pragma unroll
    for (int r = 0; r < ERR_RMAX; r++) {
        if (r >= a.n_rng) continue;                            // (uniform)
        const bool ev = ok && !((rng >> r) & 1u);
        const bool miss = ev && a.gt_hit[(int64_t)r * a.n_gt + g] == 0;
        const bool loc = miss && a.gt_loc[(int64_t)r * a.n_gt + g] != 0;
        unsigned long long *base = a.gt_counts + (int64_t)r * a.n_cat * ERR_NGT;
        wave_count(base, ev, cat * ERR_NGT);
        wave_count(base, miss, cat * ERR_NGT + 1);
        wave_count(base, loc, cat * ERR_NGT + 2);
    }
}

// The tables of the pass, in buffer order: a function of (n_dt, n_gt, n_rng)
static void err_layout(Carve &c, int64_t n_dt, int64_t n_gt, int32_t n_rng, ErrArgs &a)
{
    a.ws_types = c.take<uint8_t>((size_t)n_dt * n_rng);
    a.gt_hit = c.take<uint8_t>((size_t)n_gt * n_rng);
    a.gt_loc = c.take<uint8_t>((size_t)n_gt * n_rng);
}

extern "C" size_t taoamd_error_types_workspace(int64_t n_dt, int64_t n_gt, int32_t n_rng)
{
    if (n_dt < 0 || n_dt > 0x7fffffff || n_gt < 0 || n_gt > 0x7fffffff || n_rng < 1 || n_rng > ERR_RMAX) return 0;
    ErrArgs a;
    return measure([&](Carve &c) { err_layout(c, n_dt, n_gt, n_rng, a); });
}

static int err_run(int64_t n_dt, int64_t n_gt, int32_t n_img, int32_t n_cat,
                   int32_t n_rng, int32_t slot, double bg_thr,
                   const int32_t *dt_cat, const double *dt_box,
                   const uint8_t *dt_flags, const int32_t *dt_gt0,
                   const int32_t *match_gt, int64_t match_stride,
                   const int32_t *gt_cat, const double *gt_box,
                   const uint32_t *gt_rng, const int32_t *img_gt_off,
                   const int32_t *img_gt, const int32_t *img_dt_off,
                   const int32_t *img_dt, int64_t *dt_counts,
                   int64_t *gt_counts, uint8_t *dt_type, int32_t *link_same,
                   int32_t *link_other, uint8_t *held, void *workspace,
                   size_t workspace_bytes, void *stream)
{
    const bool links = link_same != nullptr;
    if (n_dt < 0 || n_dt > 0x7fffffff || n_gt < 0 || n_gt > 0x7fffffff || n_img < 0 ||
        n_cat <= 0 || n_rng < 1 || n_rng > ERR_RMAX || slot < 0 || slot >= N_THR)
        return TAOAMD_ERR_ARG;
    IouThr thr = iou_thr();
    const double tf = thr.v[slot] < 1 - 1e-10 ? thr.v[slot] : 1 - 1e-10;
    if (!(bg_thr >= 0) || !(bg_thr < tf)) return TAOAMD_ERR_ARG;
    if (!dt_counts || !gt_counts || !workspace || !img_gt_off || !img_dt_off)
        return TAOAMD_ERR_ARG;
    if (n_dt > 0 && (!dt_cat || !dt_box || !dt_flags || !dt_gt0 || !match_gt || !img_dt ||
                     match_stride < (int64_t)n_rng * N_THR))
        return TAOAMD_ERR_ARG;
    if (n_gt > 0 && (!gt_cat || !gt_box || !gt_rng || !img_gt)) return TAOAMD_ERR_ARG;
    Carve c(workspace);
    ErrArgs a;
    err_layout(c, n_dt, n_gt, n_rng, a);
    if (!c.fits(workspace, workspace_bytes)) return TAOAMD_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    a.n_dt = n_dt; a.n_gt = n_gt; a.n_img = n_img; a.n_cat = n_cat; a.n_rng = n_rng;
    a.slot = slot; a.tf = tf; a.tb = bg_thr;
    a.dt_cat = dt_cat; a.dt_box = dt_box; a.dt_flags = dt_flags; a.dt_gt0 = dt_gt0;
    a.match_gt = match_gt; a.match_stride = match_stride;
    a.gt_cat = gt_cat; a.gt_box = gt_box; a.gt_rng = gt_rng;
    a.img_gt_off = img_gt_off; a.img_gt = img_gt; a.img_dt_off = img_dt_off; a.img_dt = img_dt;
    a.dt_counts = (unsigned long long *)dt_counts;
    a.gt_counts = (unsigned long long *)gt_counts;
    a.types = dt_type ? dt_type : a.ws_types;
    a.link_same = link_same; a.link_other = link_other;
    if (links) a.gt_hit = held;      // the marks of the pair kernel, in the caller's table
    const size_t cells = (size_t)n_rng * n_cat;
    TAO_HIP(hipMemsetAsync(dt_counts, 0, cells * ERR_NTYPE * sizeof(int64_t), s));
    TAO_HIP(hipMemsetAsync(gt_counts, 0, cells * ERR_NGT * sizeof(int64_t), s));
    if (n_gt > 0) {
        TAO_HIP(hipMemsetAsync(a.gt_hit, 0, (size_t)n_gt * n_rng, s));
        TAO_HIP(hipMemsetAsync(a.gt_loc, 0, (size_t)n_gt * n_rng, s));
    }
    if (links && n_dt > 0) {
        // (a row no image lists links nothing)
        TAO_HIP(hipMemsetAsync(link_same, 0xff, (size_t)n_dt * n_rng * sizeof(int32_t), s));
        TAO_HIP(hipMemsetAsync(link_other, 0xff, (size_t)n_dt * n_rng * sizeof(int32_t), s));
    }
    if (n_dt > 0 && n_img > 0) {
        if (links)
            TAO_TIMED("err_pair_links_kernel", s,
                      err_pair_kernel<true><<<(unsigned)n_img, ERR_TILE, 0, s>>>(a));
        else
            TAO_TIMED("err_pair_kernel", s,
                      err_pair_kernel<false><<<(unsigned)n_img, ERR_TILE, 0, s>>>(a));
    }
    if (n_dt > 0)
        TAO_TIMED("err_count_kernel", s,
                  err_count_kernel<<<(unsigned)((n_dt + 255) / 256), 256, 0, s>>>(a));
    if (n_gt > 0)
        TAO_TIMED("err_tally_kernel", s,
                  err_tally_kernel<<<(unsigned)((n_gt + 255) / 256), 256, 0, s>>>(a));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

extern "C" int taoamd_error_types(int64_t n_dt, int64_t n_gt, int32_t n_img, int32_t n_cat,
                                  int32_t n_rng, int32_t slot, double bg_thr,
                                  const int32_t *dt_cat, const double *dt_box,
                                  const uint8_t *dt_flags, const int32_t *dt_gt0,
                                  const int32_t *match_gt, int64_t match_stride,
                                  const int32_t *gt_cat, const double *gt_box,
                                  const uint32_t *gt_rng, const int32_t *img_gt_off,
                                  const int32_t *img_gt, const int32_t *img_dt_off,
                                  const int32_t *img_dt, int64_t *dt_counts,
                                  int64_t *gt_counts, uint8_t *dt_type, void *workspace,
                                  size_t workspace_bytes, void *stream)
{
    return err_run(n_dt, n_gt, n_img, n_cat, n_rng, slot, bg_thr, dt_cat, dt_box, dt_flags,
                   dt_gt0, match_gt, match_stride, gt_cat, gt_box, gt_rng, img_gt_off, img_gt,
                   img_dt_off, img_dt, dt_counts, gt_counts, dt_type, nullptr, nullptr, nullptr,
                   workspace, workspace_bytes, stream);
}

// The same pass with the links of every (detection, range) and the held marks
// stored for taoamd_error_impact; counts and types are those of
// taoamd_error_types, the workspace is its workspace.
extern "C" int taoamd_error_types_links(int64_t n_dt, int64_t n_gt, int32_t n_img,
                                        int32_t n_cat, int32_t n_rng, int32_t slot,
                                        double bg_thr, const int32_t *dt_cat,
                                        const double *dt_box, const uint8_t *dt_flags,
                                        const int32_t *dt_gt0, const int32_t *match_gt,
                                        int64_t match_stride, const int32_t *gt_cat,
                                        const double *gt_box, const uint32_t *gt_rng,
                                        const int32_t *img_gt_off, const int32_t *img_gt,
                                        const int32_t *img_dt_off, const int32_t *img_dt,
                                        int64_t *dt_counts, int64_t *gt_counts, uint8_t *dt_type,
                                        int32_t *link_same, int32_t *link_other, uint8_t *held,
                                        void *workspace, size_t workspace_bytes, void *stream)
{
    if (!link_same || !link_other || !held) return TAOAMD_ERR_ARG;
    return err_run(n_dt, n_gt, n_img, n_cat, n_rng, slot, bg_thr, dt_cat, dt_box, dt_flags,
                   dt_gt0, match_gt, match_stride, gt_cat, gt_box, gt_rng, img_gt_off, img_gt,
                   img_dt_off, img_dt, dt_counts, gt_counts, dt_type, link_same, link_other, held,
                   workspace, workspace_bytes, stream);
}

// Track-level error breakdown per (area, time) range (gfx950): WHY a detection
// track is no true positive.  The reference has no such table; the definition
// is this library's, the image level's (error_types.hip) rule for rule, stated
// in include/tao_amodal_hip.h and DESIGN.md section 8.
//
// One call = one IoU threshold slot t (tf = min(iou_thrs[t], 1 - 1e-10)), one
// background threshold tb (0 <= tb < tf), all n_rng <= TAOAMD_TAO_RNG ranges.
// Rows are those of the use_cats = 1 track table.  For detection track d
// (video v, category c), range a:
//   E_a(v) = ground-truth tracks of video v, ANY category, gt_rng bit a clear
//   s      = max over g in E_a(v) of category c of the pass's own IoU matrix
//            (the row of d in its cell), 0 if none; argmax = the lowest row
//   o      = the same maximum over the other categories, of the 3D IoU the
//            plan-less taoamd_track_iou gives the pair
// and the type is the first of TP, IGNORED (matched to an ignored ground truth,
// or unmatched with dt_rng bit a set), DUP (s >= tf), LOC (tb <= s), CLS
// (o >= tf), BOTH (tb <= o), BKG.
//
//   trk_err_pair_kernel   the cross-category 3D IoUs, never stored: workgroup =
//                         video, lane = detection track.  The video's ground-
//                         truth tracks pass through LDS in tiles of TE_G tracks
//                         x TE_P timeline positions (two buffers, one barrier a
//                         chunk); every lane reads the same entry (a broadcast)
//                         and walks its own frames in ascending position; the
//                         (i, u) sums of the tile's TE_G pairs stay in
//                         registers.  A frame a track does not have is a clear
//                         presence bit and a select, no in-band box: coordinates
//                         may be any double.  Each pair's IoU is folded at once
//                         into two range masks per row (o >= tf, o >= tb).
//   trk_err_class_kernel  lane = detection track in TABLE order: s and its
//                         argmax from the row of the IoU matrix, the rule table,
//                         the ground-truth marks, and the counts per (range,
//                         category, type) by wavefront ballots
//   trk_err_tally_kernel  lane = ground-truth track: the three counts per
//                         (range, category) from the two byte tables
// The additions of a pair come in the plan-less kernel's order (ascending
// position over the union of the two tracks' frames) and the file is compiled
// with the same -ffp-contract=off: the IoUs equal taoamd_track_iou's bit for bit.
// taoamd_track_error_types_links is the same pass with the LINKS form of the
// pair and class kernels: the pair kernel also keeps the argmax of o per range
// (lane-major LDS columns, folded once a tile where the masks are), the class
// kernel stores the argmax of s it has anyway, and the ground-truth marks land
// in the caller's table, for taoamd_track_error_impact (error_impact.hip).
#include "common.hpp"
#include "workspace.hpp"

using namespace taoamd;

#define TE_G TAOAMD_TRACK_ERROR_TYPES_TILE   // ground-truth tracks per LDS tile
#define TE_P 8                               // timeline positions per chunk
#define TE_LANES 256                         // detection tracks per round of a video
#define TE_RMAX TAOAMD_TAO_RNG

static_assert(TE_G * TE_P <= TE_LANES && (TE_G * TE_P) % WAVE == 0, "whole wavefronts stage a chunk");

struct TrkErrArgs {
    int64_t n_dt, n_gt, n_iou, n_cells;
    int32_t n_vid, n_cat, n_rng, slot;
    double tf, tb;
    const int32_t *dt_cat;
    const uint32_t *dt_rng;
    const int4 *dt_group;            // {first GT row of the cell, GTs, place in the cell, cell}
    const int64_t *cell_iou_off;
    const double *iou;
    const int32_t *match_gt;
    int64_t match_stride;
    const int32_t *gt_cat;
    const uint32_t *gt_rng;
    const int32_t *dfoff, *dfpos;
    const double4 *dfbox;
    const int32_t *gfoff, *gfpos;
    const double4 *gfbox;
    const int32_t *vid_gt_off, *vid_gt, *vid_dt_off, *vid_dt;
    unsigned long long *dt_counts;   // [n_rng][n_cat][7]
    unsigned long long *gt_counts;   // [n_rng][n_cat][3]
    uint8_t *dt_type;                // [n_dt][n_rng] or null
    uint32_t *dt_over;               // [n_dt][2] or null
    uint32_t *over;                  // [n_dt][2]: what the pair kernel found
    uint8_t *gt_hit, *gt_loc;        // [n_rng][n_gt]
    int32_t *link_same, *link_other; // [n_dt][n_rng], taoamd_track_error_types_links only
};

// A lane's own track: the current frame and the one behind it in registers, so
// that the step to the next frame does not wait for the load it issues.
struct OwnTrack {
    const int32_t *pos;
    const double4 *box;
    int32_t q, e, p0, p1;
    double4 b0, b1;
    __device__ __forceinline__ void load(int32_t k, int32_t &p, double4 &b) const
    {
        if (k < e) { p = pos[k]; b = box[k]; } else { p = INT32_MAX; }
    }
    __device__ __forceinline__ void init(const int32_t *pos_, const double4 *box_, int32_t s, int32_t e_)
    {
        pos = pos_; box = box_; q = s; e = e_;
        b0 = b1 = make_double4(0, 0, 0, 0);
        load(q, p0, b0);
        load(q + 1, p1, b1);
    }
    __device__ __forceinline__ void advance()
    {
        q++;
        p0 = p1; b0 = b1;
        load(q + 1, p1, b1);
    }
};

// LINKS: the argmax of o per range under the rule of s (the greatest IoU, the
// lowest table row among equal ones, a NaN is no overlap), kept in one LDS
// column per lane: [r][tid] is the lane's own word, read and written by no
// other lane, so the columns need no barrier and their banks never conflict.
// 72 520 B of LDS a workgroup leave two workgroups a CU, the two wavefronts a
// SIMD of the plain form; LINKS asks for them, since the allocator left alone
// takes 256 VGPRs + 28 AGPRs, one wavefront.  The plain form asks for nothing:
// it stays the kernel it was (219 VGPRs).
template <bool LINKS>
__global__ __launch_bounds__(TE_LANES, LINKS ? 2 : 1) void trk_err_pair_kernel(TrkErrArgs a)
{
    // a ground-truth frame parked as (x1, y1, x2 = x + w, y2 = y + h, area = w * h)
    __shared__ double s_fr[2][TE_G][TE_P][5];
    __shared__ uint32_t s_pres[2][TE_G];     // bit j: the track has a frame at position j of the chunk
    __shared__ int32_t s_cat[TE_G], s_cur[TE_G], s_end[TE_G], s_first[TE_G], s_last[TE_G];
    __shared__ uint32_t s_open[TE_G];        // ranges that evaluate the track
    __shared__ int32_t s_span[2];            // first, last position of the round's detection tracks
    // LINKS: o of (range, lane), its table row (-1: none); the tile's table rows
    __shared__ double s_best[LINKS ? TE_RMAX : 1][LINKS ? TE_LANES : 1];
    __shared__ int32_t s_arg[LINKS ? TE_RMAX : 1][LINKS ? TE_LANES : 1];
    __shared__ int32_t s_row[LINKS ? TE_G : 1];

    const int v = blockIdx.x;
    const int tid = threadIdx.x;
    // (offsets clamped to the tables: a bad CSR reads wrong rows, never past an end)
    const int64_t g_lo = min(max((int64_t)a.vid_gt_off[v], (int64_t)0), a.n_gt);
    const int64_t g_hi = min(max((int64_t)a.vid_gt_off[v + 1], g_lo), a.n_gt);
    const int64_t d_lo = min(max((int64_t)a.vid_dt_off[v], (int64_t)0), a.n_dt);
    const int64_t d_hi = min(max((int64_t)a.vid_dt_off[v + 1], d_lo), a.n_dt);
    const uint32_t all = 0xffffffffu >> (32 - a.n_rng);
    if (g_lo == g_hi) return;                // no ground truth: the masks stay 0

    for (int64_t d0 = d_lo; d0 < d_hi; d0 += TE_LANES) {
        int64_t d = d0 + tid < d_hi ? (int64_t)a.vid_dt[d0 + tid] : -1;
        if (d >= a.n_dt) d = -1;
        const bool valid = d >= 0;
        const int32_t cat = valid ? a.dt_cat[d] : 0;
        // does any range evaluate a ground-truth track of another category?
        bool need = false;
        if (valid)
            for (int64_t k = g_lo; k < g_hi && !need; k++) {
                const int32_t row = a.vid_gt[k];
                if (row >= 0 && row < a.n_gt)
                    need = a.gt_cat[row] != cat && (~a.gt_rng[row] & all) != 0;
            }
        // (uniform: a video whose evaluated ground truths all share the round's
        // category stages nothing)
        if (!__syncthreads_or(need)) continue;
        int32_t fs = 0, fe = 0;
        if (need) { fs = a.dfoff[d]; fe = a.dfoff[d + 1]; }
        if (tid == 0) { s_span[0] = INT32_MAX; s_span[1] = -1; }
        __syncthreads();
        if (fe > fs) {
            atomicMin(&s_span[0], a.dfpos[fs]);
            atomicMax(&s_span[1], a.dfpos[fe - 1]);
        }
        uint32_t hi = 0, lo = 0;
        if constexpr (LINKS) {
            for (int r = 0; r < a.n_rng; r++) { s_best[r][tid] = 0.0; s_arg[r][tid] = -1; }
        }

        for (int64_t g0 = g_lo; g0 < g_hi; g0 += TE_G) {
            const int ng = (int)min((int64_t)TE_G, g_hi - g0);
            __syncthreads();                       // the tile before is read, s_span is complete
            if (tid < TE_G) {
                const int32_t row = tid < ng ? a.vid_gt[g0 + tid] : -1;
                const bool ok = row >= 0 && row < a.n_gt;
                // (a row outside the table: ignored in every range)
                const uint32_t open = ok ? ~a.gt_rng[row] & all : 0u;
                int32_t s = 0, e = 0;
                if (open) { s = a.gfoff[row]; e = a.gfoff[row + 1]; }
                s_cat[tid] = ok ? a.gt_cat[row] : -1;
                s_open[tid] = open;
                if constexpr (LINKS) s_row[tid] = row;
                s_cur[tid] = s;
                s_end[tid] = e;
                s_first[tid] = e > s ? a.gfpos[s] : INT32_MAX;
                s_last[tid] = e > s ? a.gfpos[e - 1] : -1;
            }
            __syncthreads();
            int32_t p_lo = s_span[0], p_hi = s_span[1];
            bool mine = false;
#pragma unroll
            for (int g = 0; g < TE_G; g++) {
                p_lo = min(p_lo, s_first[g]);
                p_hi = max(p_hi, s_last[g]);
                mine = mine || (s_open[g] != 0 && s_cat[g] != cat);
            }
            mine = mine && need;
            // (uniform) nothing of this tile is evaluated for any lane, or no frame anywhere
            // (LINKS: pairs without a frame have IoU 0, and an IoU of 0 can be the argmax)
            if (!__syncthreads_or(mine) || (!LINKS && p_hi < p_lo)) continue;
            const bool frames = p_hi >= p_lo;
            const bool wave_mine = __ballot(mine) != 0;

            double si[TE_G], su[TE_G];
#pragma unroll
            for (int g = 0; g < TE_G; g++) { si[g] = 0.0; su[g] = 0.0; }
            OwnTrack own;
            own.init(a.dfpos, a.dfbox, fs, mine ? fe : fs);

            // lane (g, j) of the first TE_G * TE_P threads parks the j-th frame of
            // track g that lies at or behind the chunk's start, if it is in the chunk
            auto stage = [&](int32_t p0, int b) {
                if (tid >= TE_G * TE_P) return;        // (whole wavefronts)
                const int g = tid / TE_P, j = tid % TE_P;
                const int32_t k = s_cur[g] + j;
                const int32_t p = k < s_end[g] ? a.gfpos[k] : INT32_MAX;
                const bool in = p >= p0 && p < p0 + TE_P;
                uint32_t m = in ? 1u << (p - p0) : 0u;
                if (in) {
                    const double4 B = a.gfbox[k];
                    double *e = s_fr[b][g][p - p0];
                    e[0] = B.x;
                    e[1] = B.y;
                    e[2] = B.x + B.z;
                    e[3] = B.y + B.w;
                    e[4] = B.z * B.w;
                }
                m |= (uint32_t)__shfl_xor((int)m, 1);
                m |= (uint32_t)__shfl_xor((int)m, 2);
                m |= (uint32_t)__shfl_xor((int)m, 4);
                if (j == 0) {
                    s_pres[b][g] = m;
                    s_cur[g] += __popc(m);           // (read above by this wavefront alone)
                }
            };

            const int32_t c_lo = p_lo >> 3, c_hi = !LINKS || frames ? p_hi >> 3 : c_lo - 1;
            static_assert(TE_P == 8, "chunk of a position = position >> 3");
            if (!LINKS || frames) stage(c_lo * TE_P, 0);
            for (int32_t c = c_lo; c <= c_hi; c++) {
                const int b = (c - c_lo) & 1;
                const int32_t p0 = c * TE_P;
                __syncthreads();                   // chunk c is parked, chunk c - 1 is read
                if (c < c_hi) stage(p0 + TE_P, b ^ 1);
                if (!wave_mine) continue;              // (the barriers stay outside)
                uint32_t pr[TE_G], any_g = 0;
#pragma unroll
                for (int g = 0; g < TE_G; g++) {
                    pr[g] = __builtin_amdgcn_readfirstlane(s_pres[b][g]);
                    any_g |= pr[g];
                }
                for (int j = 0; j < TE_P; j++) {
                    const bool hasd = own.p0 == p0 + j;
                    if (!((any_g >> j) & 1u) && __ballot(hasd) == 0) continue;   // (uniform)
                    const double4 B = own.b0;
                    const double dx2 = B.x + B.z, dy2 = B.y + B.w, da = B.z * B.w;
#pragma unroll
                    for (int g = 0; g < TE_G; g++) {
                        if ((pr[g] >> j) & 1u) {       // (uniform)
                            const double *e = s_fr[b][g][j];
                            const double ga = e[4];
                            // the per-frame terms of track_iou_kernel
                            double w = raw_fmin(dx2, e[2]) - raw_fmax(B.x, e[0]);
                            double h = raw_fmin(dy2, e[3]) - raw_fmax(B.y, e[1]);
                            w = w > 0 ? w : 0.0;
                            h = h > 0 ? h : 0.0;
                            const double i_ = w * h;
                            const double u_ = da + ga - i_;
                            si[g] = hasd ? si[g] + i_ : si[g];
                            su[g] = su[g] + (hasd ? u_ : ga);
                        } else {
                            su[g] = hasd ? su[g] + da : su[g];
                        }
                    }
                    if (hasd) own.advance();
                }
            }

#pragma unroll
            for (int g = 0; g < TE_G; g++) {
                const double iou = su[g] > 0 ? si[g] / su[g] : 0.0;
                const uint32_t open = mine && s_cat[g] != cat ? s_open[g] : 0u;
                // (a NaN IoU compares false: no overlap)
                hi |= iou >= a.tf ? open : 0u;
                lo |= iou >= a.tb ? open : 0u;
                if constexpr (LINKS) {
                    // the ranges that evaluate the track, one LDS read-compare-write each
                    const bool take = open != 0;
                    if (__ballot(take) == 0) continue;         // (uniform)
                    const int32_t row = s_row[g];
                    uint32_t left = __builtin_amdgcn_readfirstlane(s_open[g]);
                    while (left) {
                        const int r = __builtin_ctz(left);
                        left &= left - 1;
                        if (take) {
                            const double b = s_best[r][tid];
                            // (row numbers decide a tie, not the order of the video's list)
                            if (iou > b || (iou == b && (uint32_t)row < (uint32_t)s_arg[r][tid])) {
                                s_best[r][tid] = iou;
                                s_arg[r][tid] = row;
                            }
                        }
                    }
                }
            }
        }
        if (valid) {
            a.over[2 * d] = hi;
            a.over[2 * d + 1] = lo;
            if constexpr (LINKS) {
                for (int r = 0; r < a.n_rng; r++) a.link_other[d * a.n_rng + r] = s_arg[r][tid];
            }
        }
    }
}

// LINKS: the argmax of s, as a table row, stored per (detection track, range)
template <bool LINKS>
__global__ __launch_bounds__(256) void trk_err_class_kernel(TrkErrArgs a)
{
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = d < a.n_dt;
    const uint32_t all = 0xffffffffu >> (32 - a.n_rng);
    int32_t cat = 0, gt0 = 0, G = 0;
    uint32_t drng = 0, hi = 0, lo = 0;
    int64_t base = 0;
    if (valid) {
        cat = a.dt_cat[d];
        drng = a.dt_rng[d];
        hi = a.over[2 * d];
        // (the empty maximum is 0, and 0 >= tb when tb is 0)
        lo = a.tb == 0.0 ? all : a.over[2 * d + 1];
        if (a.dt_over) {
            a.dt_over[2 * d] = hi;
            a.dt_over[2 * d + 1] = lo;
        }
        const int4 grp = a.dt_group[d];
        gt0 = grp.x;
        // (a row whose cell lies outside the tables has no same-category ground truth)
        if (grp.w >= 0 && grp.w < a.n_cells && grp.y > 0 && grp.z >= 0 && grp.x >= 0 &&
            (int64_t)grp.x + grp.y <= a.n_gt) {
            base = a.cell_iou_off[grp.w] + (int64_t)grp.z * grp.y;
            if (base >= 0 && base + grp.y <= a.n_iou) G = grp.y;
        }
    }
    // s >= tf, s >= tb and the argmax of s per range
    double s[TE_RMAX];
    int32_t arg[TE_RMAX];
#pragma unroll
    for (int r = 0; r < TE_RMAX; r++) { s[r] = 0.0; arg[r] = -1; }
    for (int32_t g = 0; g < G; g++) {
        const double v = a.iou[base + g];
        const uint32_t open = ~a.gt_rng[gt0 + g] & all;
#pragma unroll
        for (int r = 0; r < TE_RMAX; r++) {
            // (ascending rows: an equal IoU never replaces the argmax; a NaN compares false)
            const bool up = ((open >> r) & 1u) && (v > s[r] || (v == s[r] && arg[r] < 0));
            s[r] = up ? v : s[r];
            arg[r] = up ? g : arg[r];
        }
    }
    const bool ok = valid && cat >= 0 && cat < a.n_cat;
#pragma unroll
    for (int r = 0; r < TE_RMAX; r++) {
        if (r >= a.n_rng) continue;                            // (uniform)
        int ty = ERR_BKG;
        const int32_t m = valid ? a.match_gt[d * a.match_stride + (int64_t)r * N_THR + a.slot] : -1;
        const int64_t grow = (int64_t)gt0 + m;
        if (m >= 0 && grow >= 0 && grow < a.n_gt) {
            ty = ((a.gt_rng[grow] >> r) & 1u) ? ERR_IGNORED : ERR_TP;
            a.gt_hit[(int64_t)r * a.n_gt + grow] = 1;
        } else if ((drng >> r) & 1u) {
            ty = ERR_IGNORED;
        } else if (s[r] >= a.tf) {
            ty = ERR_DUP;
        } else if (s[r] >= a.tb) {
            ty = ERR_LOC;
            if (arg[r] >= 0) a.gt_loc[(int64_t)r * a.n_gt + gt0 + arg[r]] = 1;
        } else if ((hi >> r) & 1u) {
            ty = ERR_CLS;
        } else if ((lo >> r) & 1u) {
            ty = ERR_BOTH;
        }
        if (valid && a.dt_type) a.dt_type[d * a.n_rng + r] = (uint8_t)ty;
        if constexpr (LINKS) {
            if (valid) a.link_same[d * a.n_rng + r] = arg[r] >= 0 ? gt0 + arg[r] : -1;
        }
        wave_count(a.dt_counts + (int64_t)r * a.n_cat * ERR_NTYPE, ok, cat * ERR_NTYPE + ty);
    }
}

__global__ __launch_bounds__(256) void trk_err_tally_kernel(TrkErrArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = g < a.n_gt;
    const int32_t cat = valid ? a.gt_cat[g] : 0;
    const uint32_t rng = valid ? a.gt_rng[g] : 0xffffffffu;
    const bool ok = valid && cat >= 0 && cat < a.n_cat;
    for (int r = 0; r < a.n_rng; r++) {
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
static void trk_err_layout(Carve &c, int64_t n_dt, int64_t n_gt, int32_t n_rng, TrkErrArgs &a)
{
    a.over = c.take<uint32_t>((size_t)n_dt * 2);
    a.gt_hit = c.take<uint8_t>((size_t)n_gt * n_rng);
    a.gt_loc = c.take<uint8_t>((size_t)n_gt * n_rng);
}

extern "C" size_t taoamd_track_error_types_workspace(int64_t n_dt, int64_t n_gt, int32_t n_rng)
{
    if (n_dt < 0 || n_dt > 0x7fffffff || n_gt < 0 || n_gt > 0x7fffffff || n_rng < 1 || n_rng > TE_RMAX) return 0;
    TrkErrArgs a;
    return measure([&](Carve &c) { trk_err_layout(c, n_dt, n_gt, n_rng, a); });
}

static int trk_err_run(
    int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou, int32_t n_vid, int32_t n_cat,
    int32_t n_rng, int32_t slot, double bg_thr, const int32_t *dt_cat, const uint32_t *dt_rng,
    const int32_t *dt_group, const int64_t *cell_iou_off, const double *iou,
    const int32_t *match_gt, int64_t match_stride, const int32_t *gt_cat, const uint32_t *gt_rng,
    const int32_t *dt_frame_off, const int32_t *dt_frame_pos, const double *dt_frame_box,
    const int32_t *gt_frame_off, const int32_t *gt_frame_pos, const double *gt_frame_box,
    const int32_t *vid_gt_off, const int32_t *vid_gt, const int32_t *vid_dt_off,
    const int32_t *vid_dt, int64_t *dt_counts, int64_t *gt_counts, uint8_t *dt_type,
    uint32_t *dt_over, int32_t *link_same, int32_t *link_other, uint8_t *held, void *workspace,
    size_t workspace_bytes, void *stream)
{
    const bool links = link_same != nullptr;
    if (n_dt < 0 || n_dt > 0x7fffffff || n_gt < 0 || n_gt > 0x7fffffff || n_cells < 0 ||
        n_iou < 0 || n_vid < 0 || n_cat <= 0 || n_rng < 1 || n_rng > TE_RMAX || slot < 0 ||
        slot >= N_THR)
        return TAOAMD_ERR_ARG;
    IouThr thr = iou_thr();
    const double tf = thr.v[slot] < 1 - 1e-10 ? thr.v[slot] : 1 - 1e-10;
    if (!(bg_thr >= 0) || !(bg_thr < tf)) return TAOAMD_ERR_ARG;
    if (!dt_counts || !gt_counts || !workspace || !vid_gt_off || !vid_dt_off)
        return TAOAMD_ERR_ARG;
    if (n_dt > 0 && (!dt_cat || !dt_rng || !dt_group || !cell_iou_off || !match_gt || !vid_dt ||
                     !dt_frame_off || match_stride < (int64_t)n_rng * N_THR))
        return TAOAMD_ERR_ARG;
    if (n_gt > 0 && (!gt_cat || !gt_rng || !vid_gt || !gt_frame_off)) return TAOAMD_ERR_ARG;
    if (n_iou > 0 && !iou) return TAOAMD_ERR_ARG;
    Carve c(workspace);
    TrkErrArgs a;
    trk_err_layout(c, n_dt, n_gt, n_rng, a);
    if (!c.fits(workspace, workspace_bytes)) return TAOAMD_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    a.n_dt = n_dt; a.n_gt = n_gt; a.n_iou = n_iou; a.n_cells = n_cells;
    a.n_vid = n_vid; a.n_cat = n_cat; a.n_rng = n_rng; a.slot = slot; a.tf = tf; a.tb = bg_thr;
    a.dt_cat = dt_cat; a.dt_rng = dt_rng; a.dt_group = reinterpret_cast<const int4 *>(dt_group);
    a.cell_iou_off = cell_iou_off; a.iou = iou;
    a.match_gt = match_gt; a.match_stride = match_stride;
    a.gt_cat = gt_cat; a.gt_rng = gt_rng;
    a.dfoff = dt_frame_off; a.dfpos = dt_frame_pos;
    a.dfbox = reinterpret_cast<const double4 *>(dt_frame_box);
    a.gfoff = gt_frame_off; a.gfpos = gt_frame_pos;
    a.gfbox = reinterpret_cast<const double4 *>(gt_frame_box);
    a.vid_gt_off = vid_gt_off; a.vid_gt = vid_gt; a.vid_dt_off = vid_dt_off; a.vid_dt = vid_dt;
    a.dt_counts = (unsigned long long *)dt_counts;
    a.gt_counts = (unsigned long long *)gt_counts;
    a.dt_type = dt_type; a.dt_over = dt_over;
    a.link_same = link_same; a.link_other = link_other;
    if (links) a.gt_hit = held;      // the marks of the class kernel, in the caller's table
    const size_t cells = (size_t)n_rng * n_cat;
    TAO_HIP(hipMemsetAsync(dt_counts, 0, cells * ERR_NTYPE * sizeof(int64_t), s));
    TAO_HIP(hipMemsetAsync(gt_counts, 0, cells * ERR_NGT * sizeof(int64_t), s));
    if (n_gt > 0) {
        TAO_HIP(hipMemsetAsync(a.gt_hit, 0, (size_t)n_gt * n_rng, s));
        TAO_HIP(hipMemsetAsync(a.gt_loc, 0, (size_t)n_gt * n_rng, s));
    }
    if (n_dt > 0) {
        // (a row no video lists, or whose video has nothing to compare it with: no overlap)
        TAO_HIP(hipMemsetAsync(a.over, 0, (size_t)n_dt * 2 * sizeof(uint32_t), s));
        // (and links no ground truth of another category; every link_same is written
        // by the class kernel)
        if (links)
            TAO_HIP(hipMemsetAsync(link_other, 0xff, (size_t)n_dt * n_rng * sizeof(int32_t), s));
        const unsigned row_blocks = (unsigned)((n_dt + 255) / 256);
        if (links) {
            if (n_vid > 0 && n_gt > 0)
                TAO_TIMED("trk_err_pair_links_kernel", s,
                          trk_err_pair_kernel<true><<<(unsigned)n_vid, TE_LANES, 0, s>>>(a));
            TAO_TIMED("trk_err_class_links_kernel", s,
                      trk_err_class_kernel<true><<<row_blocks, 256, 0, s>>>(a));
        } else {
            if (n_vid > 0 && n_gt > 0)
                TAO_TIMED("trk_err_pair_kernel", s,
                          trk_err_pair_kernel<false><<<(unsigned)n_vid, TE_LANES, 0, s>>>(a));
            TAO_TIMED("trk_err_class_kernel", s,
                      trk_err_class_kernel<false><<<row_blocks, 256, 0, s>>>(a));
        }
    }
    if (n_gt > 0)
        TAO_TIMED("trk_err_tally_kernel", s,
                  trk_err_tally_kernel<<<(unsigned)((n_gt + 255) / 256), 256, 0, s>>>(a));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

extern "C" int taoamd_track_error_types(
    int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou, int32_t n_vid, int32_t n_cat,
    int32_t n_rng, int32_t slot, double bg_thr, const int32_t *dt_cat, const uint32_t *dt_rng,
    const int32_t *dt_group, const int64_t *cell_iou_off, const double *iou,
    const int32_t *match_gt, int64_t match_stride, const int32_t *gt_cat, const uint32_t *gt_rng,
    const int32_t *dt_frame_off, const int32_t *dt_frame_pos, const double *dt_frame_box,
    const int32_t *gt_frame_off, const int32_t *gt_frame_pos, const double *gt_frame_box,
    const int32_t *vid_gt_off, const int32_t *vid_gt, const int32_t *vid_dt_off,
    const int32_t *vid_dt, int64_t *dt_counts, int64_t *gt_counts, uint8_t *dt_type,
    uint32_t *dt_over, void *workspace, size_t workspace_bytes, void *stream)
{
    return trk_err_run(n_dt, n_gt, n_cells, n_iou, n_vid, n_cat, n_rng, slot, bg_thr, dt_cat,
                       dt_rng, dt_group, cell_iou_off, iou, match_gt, match_stride, gt_cat, gt_rng,
                       dt_frame_off, dt_frame_pos, dt_frame_box, gt_frame_off, gt_frame_pos,
                       gt_frame_box, vid_gt_off, vid_gt, vid_dt_off, vid_dt, dt_counts, gt_counts,
                       dt_type, dt_over, nullptr, nullptr, nullptr, workspace, workspace_bytes,
                       stream);
}

// The same pass with the links of every (detection track, range) and the held
// marks stored for taoamd_track_error_impact; counts, types and masks are those
// of taoamd_track_error_types, the workspace is its workspace.
extern "C" int taoamd_track_error_types_links(
    int64_t n_dt, int64_t n_gt, int64_t n_cells, int64_t n_iou, int32_t n_vid, int32_t n_cat,
    int32_t n_rng, int32_t slot, double bg_thr, const int32_t *dt_cat, const uint32_t *dt_rng,
    const int32_t *dt_group, const int64_t *cell_iou_off, const double *iou,
    const int32_t *match_gt, int64_t match_stride, const int32_t *gt_cat, const uint32_t *gt_rng,
    const int32_t *dt_frame_off, const int32_t *dt_frame_pos, const double *dt_frame_box,
    const int32_t *gt_frame_off, const int32_t *gt_frame_pos, const double *gt_frame_box,
    const int32_t *vid_gt_off, const int32_t *vid_gt, const int32_t *vid_dt_off,
    const int32_t *vid_dt, int64_t *dt_counts, int64_t *gt_counts, uint8_t *dt_type,
    uint32_t *dt_over, int32_t *link_same, int32_t *link_other, uint8_t *held, void *workspace,
    size_t workspace_bytes, void *stream)
{
    if (!link_same || !link_other || !held) return TAOAMD_ERR_ARG;
    return trk_err_run(n_dt, n_gt, n_cells, n_iou, n_vid, n_cat, n_rng, slot, bg_thr, dt_cat,
                       dt_rng, dt_group, cell_iou_off, iou, match_gt, match_stride, gt_cat, gt_rng,
                       dt_frame_off, dt_frame_pos, dt_frame_box, gt_frame_off, gt_frame_pos,
                       gt_frame_box, vid_gt_off, vid_gt, vid_dt_off, vid_dt, dt_counts, gt_counts,
                       dt_type, dt_over, link_same, link_other, held, workspace, workspace_bytes,
                       stream);
}

// Which category pairs the CLS and BOTH errors confuse (gfx950): a sparse
// histogram of (range a, predicted category c, ground-truth category c') over
// the tables of an error breakdown with links.  Level-agnostic like the error
// impact: it reads type bytes, links and scores, no boxes and no images.  The
// definition is this library's, stated in include/tao_amodal_hip.h
// ("confusion") and DESIGN.md section 8; in short, a CLS or BOTH row of c whose
// link_other is a ground truth of c' adds to the pair (a, c, c'): cls, both,
// unheld (CLS rows whose ground truth is missed) and adopted (the CLS row that
// is the WINNER of its missed ground truth: the row the impact's CLS fix adopts).
//
//   conf_best_kernel   lane = (row, range): atomic max of the score key of every
//   conf_win_kernel    CLS claim, then atomic min of the row among the rows that
//                      hold it -- the impact's rule, from winner.hpp
//   conf_hist_kernel   workgroup = (category c, range a): the rows of c add into
//                      an LDS table hist[c' - tile base][4]; the non-zero entries
//                      of a tile are counted (COUNT) or, ranked by a wavefront
//                      ballot, stored in ascending c' (FILL).  More categories
//                      than a tile holds: the rows are walked once per tile.
//   conf_scan_kernel   one workgroup: the counts of the (a, c) rows -> ent_off
// The ranges of a category are consecutive workgroups of one XCD (xcd_block):
// they read the same byte rows dt_type[d][*] / link_other[d][*] at a stride.
// Everything is integer and every entry has one place: the result is exact and
// the same bytes from run to run.
#include "common.hpp"
#include "winner.hpp"
#include "workspace.hpp"

using namespace taoamd;

#define CONF_TILE TAOAMD_CONFUSION_TILE
#define CONF_THREADS 256
#define CONF_MAX_BLOCKS (1u << 20)      // (a, c) rows beyond that many: a grid-stride loop

static_assert(CONF_TILE * 16 <= 32768, "the LDS table of a tile stays within 32 KB");
static_assert(CONF_TILE % CONF_THREADS == 0, "a tile is emitted in whole steps");

struct ConfArgs {
    int64_t n_dt, n_gt;
    int32_t n_cat, n_rng;
    const int32_t *cat_off;
    const double *score;
    const int32_t *dt_cat;
    const uint8_t *dt_type;                  // [n_dt][n_rng]
    const int32_t *link_other;               // [n_dt][n_rng]
    const int32_t *gt_cat;
    const uint8_t *held;                     // [n_rng][n_gt]
    unsigned long long *best;                // [n_rng][n_gt] greatest key of a CLS claim, 0: none
    uint32_t *win;                           // [n_rng][n_gt] lowest row with that key
    int32_t *nnz;                            // [n_rng][n_cat] entries of the (a, c) row
    const int64_t *ent_off;                  // FILL: [n_rng * n_cat + 1]
    int64_t cap;
    int32_t *ent_gt_cat;                     // [cap]
    int4 *ent_counts;                        // [cap]
};

__device__ __forceinline__ bool conf_claim(const ConfArgs &a, int64_t d, int r, int64_t &slot)
{
    const ClaimTabs t = {a.n_gt, a.n_cat, a.n_rng, a.dt_cat, a.dt_type, nullptr, a.link_other,
                         a.held};
    int tab;
    int64_t g;
    if (!claim_of(t, d, r, tab, g)) return false;     // (no link_same: CLS claims only)
    slot = (int64_t)r * a.n_gt + g;
    return true;
}

__global__ __launch_bounds__(256) void conf_best_kernel(ConfArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_dt * a.n_rng) return;
    const int64_t d = i / a.n_rng;
    int64_t slot;
    if (!conf_claim(a, d, (int)(i - d * a.n_rng), slot)) return;
    claim_best(a.best, slot, a.score[d]);
}

__global__ __launch_bounds__(256) void conf_win_kernel(ConfArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_dt * a.n_rng) return;
    const int64_t d = i / a.n_rng;
    int64_t slot;
    if (!conf_claim(a, d, (int)(i - d * a.n_rng), slot)) return;
    claim_win(a.best, a.win, slot, a.score[d], d);
}

template <bool FILL>
__global__ __launch_bounds__(CONF_THREADS) void conf_hist_kernel(ConfArgs a)
{
    __shared__ int4 s_hist[CONF_TILE];
    __shared__ int32_t s_wave[CONF_THREADS / WAVE];
    int32_t *hist = (int32_t *)s_hist;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t n_rows = (int64_t)a.n_cat * a.n_rng;
    for (int64_t b = xcd_block(blockIdx.x, gridDim.x); b < n_rows; b += gridDim.x) {
        const int32_t c = (int32_t)(b / a.n_rng);
        const int r = (int)(b - (int64_t)c * a.n_rng);
        const int64_t row = (int64_t)r * a.n_cat + c;          // the CSR row of (a, c)
        // rows of category c, clamped to the table
        const int64_t lo = min(max((int64_t)a.cat_off[c], (int64_t)0), a.n_dt);
        const int64_t hi = min(max((int64_t)a.cat_off[c + 1], lo), a.n_dt);
        int64_t start = 0, end = 0;
        bool write = false;
        if (FILL) {
            // the whole (a, c) row lies below cap, or none of it is stored
            start = a.ent_off[row];
            end = a.ent_off[row + 1];
            write = start >= 0 && start <= end && end <= a.cap;
            if (!write) continue;
        }
        if (lo == hi) {
            if (!FILL && tid == 0) a.nnz[row] = 0;
            continue;
        }
        int64_t pos = start;
        for (int64_t base = 0; base < a.n_cat; base += CONF_TILE) {
            const int tn = (int)min((int64_t)CONF_TILE, a.n_cat - base);
            for (int j = tid; j < tn; j += CONF_THREADS) s_hist[j] = make_int4(0, 0, 0, 0);
            __syncthreads();
            for (int64_t d = lo + tid; d < hi; d += CONF_THREADS) {
                if (a.dt_cat[d] != c) continue;
                const int ty = a.dt_type[d * a.n_rng + r];
                if (ty != ERR_CLS && ty != ERR_BOTH) continue;
                const int64_t g = a.link_other[d * a.n_rng + r];
                if (g < 0 || g >= a.n_gt) continue;
                const int64_t k = (int64_t)a.gt_cat[g] - base;
                if (a.gt_cat[g] < 0 || a.gt_cat[g] >= a.n_cat || k < 0 || k >= tn) continue;
                if (ty == ERR_BOTH) {
                    atomicAdd(hist + 4 * k + 1, 1);
                    continue;
                }
                atomicAdd(hist + 4 * k, 1);
                const int64_t slot = (int64_t)r * a.n_gt + g;
                if (a.held[slot]) continue;
                atomicAdd(hist + 4 * k + 2, 1);
                if (a.win[slot] == (uint32_t)d) atomicAdd(hist + 4 * k + 3, 1);
            }
            __syncthreads();
            // the tile's non-zero entries in ascending c'
            for (int j0 = 0; j0 < tn; j0 += CONF_THREADS) {
                const int j = j0 + tid;
                const int4 h = j < tn ? s_hist[j] : make_int4(0, 0, 0, 0);
                const bool nz = h.x + h.y > 0;
                const uint64_t vote = __ballot(nz);
                if (lane_id() == 0) s_wave[wave] = __popcll(vote);
                __syncthreads();
                int32_t before = 0, total = 0;
#pragma unroll
                for (int w = 0; w < CONF_THREADS / WAVE; w++) {
                    const int32_t t = s_wave[w];
                    if (w < wave) before += t;
                    total += t;
                }
                if (FILL && nz) {
                    const int64_t p = pos + before + __popcll(vote & ((1ull << lane_id()) - 1));
                    if (p < end) {                 // (an ent_off of other tables: not past its row)
                        a.ent_gt_cat[p] = (int32_t)(base + j);
                        a.ent_counts[p] = h;       // one 16-byte store
                    }
                }
                pos += total;
                __syncthreads();                   // s_wave is read
            }
        }
        if (!FILL && tid == 0) a.nnz[row] = (int32_t)(pos - start);
    }
}

// ent_off[i] = the sum of nnz[0 .. i), ent_off[n] the total; one workgroup
__global__ __launch_bounds__(1024) void conf_scan_kernel(const int32_t *__restrict__ nnz,
                                                         int64_t *__restrict__ ent_off, int64_t n)
{
    __shared__ long long s_w[1024 / WAVE];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    long long carry = 0;
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + tid;
        const long long v = i < n ? nnz[i] : 0;
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
        if (i < n) ent_off[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();                           // s_w is read
    }
    if (tid == 0) ent_off[n] = carry;
}

// The tables of the pass, in buffer order: a function of (n_dt, n_gt, n_cat, n_rng)
static void conf_layout(Carve &c, int64_t n_gt, int32_t n_cat, int32_t n_rng, ConfArgs &a)
{
    a.best = c.take<unsigned long long>((size_t)n_rng * n_gt);
    a.win = c.take<uint32_t>((size_t)n_rng * n_gt);
    a.nnz = c.take<int32_t>((size_t)n_rng * n_cat);
}

static bool conf_sizes_ok(int64_t n_dt, int64_t n_gt, int32_t n_cat, int32_t n_rng)
{
    return n_dt >= 0 && n_dt <= 0x7fffffff && n_gt >= 0 && n_gt <= 0x7fffffff && n_cat > 0 &&
           n_rng >= 1 && n_rng <= TAOAMD_TAO_RNG;
}

extern "C" size_t taoamd_confusion_workspace(int64_t n_dt, int64_t n_gt, int32_t n_cat,
                                             int32_t n_rng)
{
    if (!conf_sizes_ok(n_dt, n_gt, n_cat, n_rng)) return 0;
    ConfArgs a;
    return measure([&](Carve &c) { conf_layout(c, n_gt, n_cat, n_rng, a); });
}

// What the two entry points share: the refusals and the carved workspace
static int conf_args(ConfArgs &a, int64_t n_dt, int64_t n_gt, int32_t n_cat, int32_t n_rng,
                     const int32_t *cat_off, const double *score, const int32_t *dt_cat,
                     const uint8_t *dt_type, const int32_t *link_other, const int32_t *gt_cat,
                     const uint8_t *held, const int64_t *ent_off, void *workspace,
                     size_t workspace_bytes)
{
    if (!conf_sizes_ok(n_dt, n_gt, n_cat, n_rng)) return TAOAMD_ERR_ARG;
    if (!cat_off || !ent_off || !workspace) return TAOAMD_ERR_ARG;
    if (n_dt > 0 && (!score || !dt_cat || !dt_type || !link_other)) return TAOAMD_ERR_ARG;
    if (n_gt > 0 && (!gt_cat || !held)) return TAOAMD_ERR_ARG;
    Carve c(workspace);
    conf_layout(c, n_gt, n_cat, n_rng, a);
    if (!c.fits(workspace, workspace_bytes)) return TAOAMD_ERR_WORKSPACE;
    a.n_dt = n_dt; a.n_gt = n_gt; a.n_cat = n_cat; a.n_rng = n_rng;
    a.cat_off = cat_off; a.score = score; a.dt_cat = dt_cat; a.dt_type = dt_type;
    a.link_other = link_other; a.gt_cat = gt_cat; a.held = held;
    a.ent_off = ent_off; a.cap = 0; a.ent_gt_cat = nullptr; a.ent_counts = nullptr;
    return TAOAMD_OK;
}

static unsigned conf_blocks(const ConfArgs &a)
{
    const int64_t n_rows = (int64_t)a.n_cat * a.n_rng;
    return n_rows < (int64_t)CONF_MAX_BLOCKS ? (unsigned)n_rows : CONF_MAX_BLOCKS;
}

extern "C" int taoamd_confusion_count(int64_t n_dt, int64_t n_gt, int32_t n_cat, int32_t n_rng,
                                      const int32_t *cat_off, const double *score,
                                      const int32_t *dt_cat, const uint8_t *dt_type,
                                      const int32_t *link_other, const int32_t *gt_cat,
                                      const uint8_t *held, int64_t *ent_off, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    ConfArgs a;
    const int st = conf_args(a, n_dt, n_gt, n_cat, n_rng, cat_off, score, dt_cat, dt_type,
                             link_other, gt_cat, held, ent_off, workspace, workspace_bytes);
    if (st != TAOAMD_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_rows = (int64_t)n_cat * n_rng;
    if (n_dt == 0 || n_gt == 0) {                  // no link names a ground truth
        TAO_HIP(hipMemsetAsync(ent_off, 0, (size_t)(n_rows + 1) * sizeof(int64_t), s));
        return TAOAMD_OK;
    }
    const size_t claims = (size_t)n_rng * n_gt;
    TAO_HIP(hipMemsetAsync(a.best, 0, claims * sizeof(unsigned long long), s));
    TAO_HIP(hipMemsetAsync(a.win, 0xff, claims * sizeof(uint32_t), s));
    const unsigned row_blocks = (unsigned)((n_dt * n_rng + 255) / 256);
    TAO_TIMED("conf_best_kernel", s, conf_best_kernel<<<row_blocks, 256, 0, s>>>(a));
    TAO_TIMED("conf_win_kernel", s, conf_win_kernel<<<row_blocks, 256, 0, s>>>(a));
    TAO_TIMED("conf_count_kernel", s,
              conf_hist_kernel<false><<<conf_blocks(a), CONF_THREADS, 0, s>>>(a));
    TAO_TIMED("conf_scan_kernel", s, conf_scan_kernel<<<1, 1024, 0, s>>>(a.nnz, ent_off, n_rows));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

extern "C" int taoamd_confusion_fill(int64_t n_dt, int64_t n_gt, int32_t n_cat, int32_t n_rng,
                                     const int32_t *cat_off, const double *score,
                                     const int32_t *dt_cat, const uint8_t *dt_type,
                                     const int32_t *link_other, const int32_t *gt_cat,
                                     const uint8_t *held, const int64_t *ent_off, int64_t cap,
                                     int32_t *ent_gt_cat, int32_t *ent_counts, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    ConfArgs a;
    if (cap < 0) return TAOAMD_ERR_ARG;
    const int st = conf_args(a, n_dt, n_gt, n_cat, n_rng, cat_off, score, dt_cat, dt_type,
                             link_other, gt_cat, held, ent_off, workspace, workspace_bytes);
    if (st != TAOAMD_OK) return st;
    // (the counts of an entry leave as one 16-byte store)
    if (cap > 0 && (!ent_gt_cat || !ent_counts || ((uintptr_t)ent_counts & 15)))
        return TAOAMD_ERR_ARG;
    if (n_dt == 0 || n_gt == 0 || cap == 0) return TAOAMD_OK;      // no entry to store
    hipStream_t s = (hipStream_t)stream;
    a.cap = cap; a.ent_gt_cat = ent_gt_cat; a.ent_counts = (int4 *)ent_counts;
    TAO_TIMED("conf_fill_kernel", s,
              conf_hist_kernel<true><<<conf_blocks(a), CONF_THREADS, 0, s>>>(a));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

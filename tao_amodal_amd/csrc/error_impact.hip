// The AP each error type costs (gfx950): TIDE's dAP (Bolya et al., ECCV 2020)
// on the tables of the error breakdown.  Level-agnostic: it reads type bytes,
// links, scores and the sort's order[], no boxes and no images.  The definition
// is this library's, stated in include/tao_amodal_hip.h ("error impact") and
// DESIGN.md section 8; in short, per (category k, range a) the rows of k in
// sweep order are a list of true positives (type TP) and false positives (DUP
// to BKG), IGNORED rows dropped, and nine variants of that list get the
// precision at every recall threshold with the arithmetic of taoamd_accumulate:
//   BASE  the list as it is
//   CLS   CLS rows leave; per missed ground truth the best CLS row linking it
//         (link_other) joins the list of the ground truth's category as a TP
//   LOC   LOC rows whose link_same is held leave; per missed ground truth the
//         best LOC row linking it becomes a TP at its place, the others leave
//   BOTH, DUP, BKG   rows of the type leave;  FP  every false positive leaves
//   MISS  num_gt less the missed ground truths no LOC / CLS row links
//   FN    num_gt less the missed ground truths
//
//   imp_best_kernel    lane = (row, range): atomic max of the score key of every
//                      LOC / CLS row into best[table][range][its link], where
//                      the link is no held ground truth
//   imp_win_kernel     the rows whose key is the maximum: atomic min of the row
//   imp_adopt_kernel   a CLS winner: its place in the target category by binary
//                      search over the category's sorted scores, one add to the
//                      count of that insertion slot
//   imp_gt_kernel      lane = ground truth: evaluated / missed / missed and
//                      unlinked per (category, range)
//   imp_sweep_kernel   workgroup = (category, range), IMP_CHUNK insertion slots +
//                      rows per step, the running (tp, n) of the seven distinct
//                      row lists carried from step to step
// The sweep uses that the envelope of precision only peaks on true positives:
// precision at a threshold is the maximum of tp_j / (n_j + eps) over the
// true-positive rows j with tp_j >= c, c the smallest count whose recall
// reaches the threshold (recall_crossing; c = 0: every row).  A true positive
// with count tp serves the first J thresholds, J = #{c <= tp} (the thresholds
// ascend); it raises bucket[J - 1] in LDS, and the suffix maxima of the buckets
// are the precisions.  Values are doubles computed by the reference's
// expression; a maximum of doubles depends on no order.
#include "common.hpp"
#include "winner.hpp"
#include "workspace.hpp"

using namespace taoamd;

#define IMP_CHUNK TAOAMD_ERROR_IMPACT_CHUNK
#define IMP_NVAR TAOAMD_ERROR_IMPACT_FIXES
#define IMP_NLIST 7            // distinct row lists: MISS and FN sweep BASE's
#define IMP_RMAX 8             // ranges of the image level; the track level has TAOAMD_TAO_RNG

enum { V_BASE = 0, V_CLS, V_LOC, V_BOTH, V_DUP, V_BKG, V_MISS, V_FP, V_FN };

struct ImpArgs {
    int64_t n_dt, n_gt;
    int32_t n_cat, n_rng;
    const int32_t *cat_off, *order;
    const double *score;
    const int32_t *dt_cat;
    const uint8_t *dt_type;                  // [n_dt][n_rng]
    const int32_t *link_same, *link_other;   // [n_dt][n_rng]
    const int32_t *gt_cat;
    const uint32_t *gt_rng;
    const uint8_t *held;                     // [n_rng][n_gt]
    double *precision;                       // [9][N_REC][n_cat][n_rng]
    int32_t *num_gt;                         // [9][n_cat][n_rng]
    unsigned long long *best;                // [2][n_rng][n_gt] greatest score key, 0: none
    uint32_t *win;                           // [2][n_rng][n_gt] lowest row with that key
    uint32_t *adopt;                         // [n_rng][n_dt + n_cat] adopted rows per insertion slot
    uint32_t *cnt;                           // [3][n_cat][n_rng] evaluated, missed and unlinked, missed
};

// The claim of (row d, range r), by the rule winner.hpp shares with
// confusion.hip: its table (0 LOC, 1 CLS) and its slot in best[] / win[]
__device__ __forceinline__ bool imp_claim(const ImpArgs &a, int64_t d, int r, int &tab,
                                          int64_t &slot)
{
    const ClaimTabs t = {a.n_gt, a.n_cat, a.n_rng, a.dt_cat, a.dt_type,
                         a.link_same, a.link_other, a.held};
    int64_t g;
    if (!claim_of(t, d, r, tab, g)) return false;
    slot = ((int64_t)tab * a.n_rng + r) * a.n_gt + g;
    return true;
}

__global__ __launch_bounds__(256) void imp_best_kernel(ImpArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_dt * a.n_rng) return;
    const int64_t d = i / a.n_rng;
    int tab;
    int64_t slot;
    if (!imp_claim(a, d, (int)(i - d * a.n_rng), tab, slot)) return;
    claim_best(a.best, slot, a.score[d]);
}

__global__ __launch_bounds__(256) void imp_win_kernel(ImpArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_dt * a.n_rng) return;
    const int64_t d = i / a.n_rng;
    int tab;
    int64_t slot;
    if (!imp_claim(a, d, (int)(i - d * a.n_rng), tab, slot)) return;
    claim_win(a.best, a.win, slot, a.score[d], d);
}

// rows of category k in order[]: [lo, hi), clamped to the table
__device__ __forceinline__ void imp_segment(const ImpArgs &a, int32_t k, int64_t &lo, int64_t &hi)
{
    lo = min(max((int64_t)a.cat_off[k], (int64_t)0), a.n_dt);
    hi = min(max((int64_t)a.cat_off[k + 1], lo), a.n_dt);
}

__global__ __launch_bounds__(256) void imp_adopt_kernel(ImpArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_dt * a.n_rng) return;
    const int64_t d = i / a.n_rng;
    const int r = (int)(i - d * a.n_rng);
    int tab;
    int64_t slot;
    if (!imp_claim(a, d, r, tab, slot) || tab != 1 || a.win[slot] != (uint32_t)d) return;
    const int32_t k = a.gt_cat[slot - ((int64_t)a.n_rng + r) * a.n_gt];
    if (k < 0 || k >= a.n_cat) return;
    int64_t lo, hi;
    imp_segment(a, k, lo, hi);
    // rows of k whose score is >= this one's: keys ascend along the segment
    const uint64_t key = score_desc_key(a.score[d]);
    int64_t l = lo, h = hi;
    while (l < h) {
        const int64_t mid = (l + h) >> 1;
        const int64_t row = a.order[mid];
        // (a row outside the table: as if its score were a NaN)
        const uint64_t km = row >= 0 && row < a.n_dt ? score_desc_key(a.score[row])
                                                     : 0xfff8000000000000ull;
        if (km <= key) l = mid + 1; else h = mid;
    }
    atomicAdd(a.adopt + (int64_t)r * (a.n_dt + a.n_cat) + l + k, 1u);
}

template <int RMAX>
__global__ __launch_bounds__(256) void imp_gt_kernel(ImpArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = g < a.n_gt;
    const int32_t cat = valid ? a.gt_cat[g] : 0;
    const bool ok = valid && cat >= 0 && cat < a.n_cat;
    const uint32_t rng = ok ? a.gt_rng[g] : 0xffffffffu;
    const int64_t plane = (int64_t)a.n_cat * a.n_rng;
#pragma unroll
    for (int r = 0; r < RMAX; r++) {
        if (r >= a.n_rng) continue;                            // (uniform)
        const bool ev = ok && !((rng >> r) & 1u);
        const int64_t at = (int64_t)r * a.n_gt + g;
        const bool missed = ev && a.held[at] == 0;
        const bool lone = missed && a.best[at] == 0 && a.best[(int64_t)a.n_rng * a.n_gt + at] == 0;
        const int32_t key = cat * a.n_rng + r;
        wave_count(a.cnt, ev, key);
        wave_count(a.cnt + plane, lone, key);
        wave_count(a.cnt + 2 * plane, missed, key);
    }
}

// inclusive scan over the wavefront of a packed (tp << 32 | n) pair
__device__ __forceinline__ unsigned long long imp_wave_scan(unsigned long long v)
{
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const unsigned long long u = __shfl_up(v, off, WAVE);
        if (lane_id() >= off) v += u;
    }
    return v;
}

__global__ __launch_bounds__(IMP_CHUNK) void imp_sweep_kernel(ImpArgs a, RecThr rec)
{
    __shared__ int32_t s_c[3][N_REC];
    __shared__ unsigned long long s_bucket[IMP_NVAR][N_REC];
    __shared__ unsigned long long s_wave[IMP_CHUNK / WAVE][IMP_NLIST];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int32_t k = (int32_t)(blockIdx.x / a.n_rng);
    const int r = (int)(blockIdx.x - (unsigned)k * a.n_rng);
    const int64_t plane = (int64_t)a.n_cat * a.n_rng;
    const int64_t kr = (int64_t)k * a.n_rng + r;
    // num_gt' of the three recall scales: the lists', MISS's, FN's
    const int32_t ev = (int32_t)a.cnt[kr];
    const int32_t ng3[3] = {ev, ev - (int32_t)a.cnt[plane + kr], ev - (int32_t)a.cnt[2 * plane + kr]};
    for (int i = tid; i < 3 * N_REC; i += IMP_CHUNK) {
        const int q = i / N_REC;
        s_c[q][i - q * N_REC] = ng3[q] > 0 ? recall_crossing(rec.v[i - q * N_REC], ng3[q]) : 0;
    }
    for (int i = tid; i < IMP_NVAR * N_REC; i += IMP_CHUNK) (&s_bucket[0][0])[i] = 0;
    __syncthreads();

    int64_t lo, hi;
    imp_segment(a, k, lo, hi);
    const int64_t len = hi - lo;
    const uint32_t *adopt = a.adopt + (int64_t)r * (a.n_dt + a.n_cat) + lo + k;
    const unsigned long long ONE_FP = 1ull, ONE_TP = (1ull << 32) | 1ull;
    // variant of each list
    const int var_of[IMP_NLIST] = {V_BASE, V_CLS, V_LOC, V_BOTH, V_DUP, V_BKG, V_FP};
    unsigned long long carry[IMP_NLIST];
#pragma unroll
    for (int L = 0; L < IMP_NLIST; L++) carry[L] = 0;

    // position p <= len: the rows adopted into insertion slot p, then row p
    for (int64_t base = 0; base <= len; base += IMP_CHUNK) {
        const int64_t p = base + tid;
        const uint32_t m = p <= len ? adopt[p] : 0;
        int ty = 255;
        int64_t d = -1;
        if (p < len) {
            d = a.order[lo + p];
            if (d >= 0 && d < a.n_dt) ty = a.dt_type[d * a.n_rng + r];
        }
        const bool kept = ty == ERR_TP || (ty >= ERR_DUP && ty <= ERR_BKG);
        const unsigned long long row = !kept ? 0 : (ty == ERR_TP ? ONE_TP : ONE_FP);
        unsigned long long inc[IMP_NLIST], own[IMP_NLIST];
        own[0] = row;
        own[1] = ty == ERR_CLS ? 0 : row;
        own[2] = row;
        if (ty == ERR_LOC) {
            const int64_t g = a.link_same[d * a.n_rng + r];
            if (g >= 0 && g < a.n_gt) {
                const int64_t at = (int64_t)r * a.n_gt + g;
                own[2] = !a.held[at] && a.win[at] == (uint32_t)d ? ONE_TP : 0;
            }
        }
        own[3] = ty == ERR_BOTH ? 0 : row;
        own[4] = ty == ERR_DUP ? 0 : row;
        own[5] = ty == ERR_BKG ? 0 : row;
        own[6] = ty == ERR_TP ? row : 0;
#pragma unroll
        for (int L = 0; L < IMP_NLIST; L++) inc[L] = own[L];
        inc[1] += ((unsigned long long)m << 32) | m;

        unsigned long long pre[IMP_NLIST];
#pragma unroll
        for (int L = 0; L < IMP_NLIST; L++) {
            pre[L] = imp_wave_scan(inc[L]);
            if (lane_id() == WAVE - 1) s_wave[wave][L] = pre[L];
        }
        __syncthreads();
#pragma unroll
        for (int L = 0; L < IMP_NLIST; L++) {
            unsigned long long before = carry[L], total = carry[L];
#pragma unroll
            for (int w = 0; w < IMP_CHUNK / WAVE; w++) {
                const unsigned long long t = s_wave[w][L];
                if (w < wave) before += t;
                total += t;
            }
            pre[L] += before;
            carry[L] = total;
        }
        __syncthreads();                               // s_wave is read

        // the last true positive at this position serves the thresholds its count reaches
#pragma unroll
        for (int L = 0; L < IMP_NLIST; L++) {
            unsigned long long c = 0;
            if (own[L] >> 32) c = pre[L];
            else if (L == 1 && m > 0) c = pre[L] - own[L];     // the adopted rows come before the row
            if (c == 0) continue;
            const uint32_t tp = (uint32_t)(c >> 32), n = (uint32_t)c;
            const double val = (double)tp / ((double)n + ACC_EPS);
            const unsigned long long bits = (unsigned long long)__double_as_longlong(val);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                if (q > 0 && L != 0) continue;
                if (ng3[q] <= 0) continue;
                int l = 0, h = N_REC;                  // J = #{j: c_j <= tp}
                while (l < h) {
                    const int mid = (l + h) >> 1;
                    if (s_c[q][mid] <= (int32_t)tp) l = mid + 1; else h = mid;
                }
                if (l > 0) atomicMax(&s_bucket[q == 0 ? var_of[L] : (q == 1 ? V_MISS : V_FN)][l - 1], bits);
            }
        }
    }
    __syncthreads();
    if (tid < IMP_NVAR) {
        unsigned long long run = 0;
        for (int j = N_REC - 1; j >= 0; j--) {
            run = max(run, s_bucket[tid][j]);
            s_bucket[tid][j] = run;
        }
        const int32_t ng = tid == V_MISS ? ng3[1] : (tid == V_FN ? ng3[2] : ng3[0]);
        a.num_gt[(int64_t)tid * plane + kr] = ng;
    }
    __syncthreads();
    for (int i = tid; i < IMP_NVAR * N_REC; i += IMP_CHUNK) {
        const int v = i / N_REC;
        const int32_t ng = v == V_MISS ? ng3[1] : (v == V_FN ? ng3[2] : ng3[0]);
        a.precision[(int64_t)i * plane + kr] =
            ng > 0 ? __longlong_as_double((long long)(&s_bucket[0][0])[i]) : -1.0;
    }
}

// The tables of the pass, in buffer order: a function of (n_dt, n_gt, n_cat, n_rng)
static void imp_layout(Carve &c, int64_t n_dt, int64_t n_gt, int32_t n_cat, int32_t n_rng,
                       ImpArgs &a)
{
    a.best = c.take<unsigned long long>((size_t)2 * n_rng * n_gt);
    a.win = c.take<uint32_t>((size_t)2 * n_rng * n_gt);
    a.adopt = c.take<uint32_t>((size_t)n_rng * (n_dt + n_cat));
    a.cnt = c.take<uint32_t>((size_t)3 * n_cat * n_rng);
}

static bool imp_sizes_ok(int64_t n_dt, int64_t n_gt, int32_t n_cat, int32_t n_rng, int32_t cap)
{
    return n_dt >= 0 && n_dt <= 0x7fffffff && n_gt >= 0 && n_gt <= 0x7fffffff && n_cat > 0 &&
           n_rng >= 1 && n_rng <= cap;
}

static size_t imp_workspace(int64_t n_dt, int64_t n_gt, int32_t n_cat, int32_t n_rng, int32_t cap)
{
    if (!imp_sizes_ok(n_dt, n_gt, n_cat, n_rng, cap)) return 0;
    ImpArgs a;
    return measure([&](Carve &c) { imp_layout(c, n_dt, n_gt, n_cat, n_rng, a); });
}

extern "C" size_t taoamd_error_impact_workspace(int64_t n_dt, int64_t n_gt, int32_t n_cat,
                                                int32_t n_rng)
{
    return imp_workspace(n_dt, n_gt, n_cat, n_rng, IMP_RMAX);
}

extern "C" size_t taoamd_track_error_impact_workspace(int64_t n_dt, int64_t n_gt, int32_t n_cat,
                                                      int32_t n_rng)
{
    return imp_workspace(n_dt, n_gt, n_cat, n_rng, TAOAMD_TAO_RNG);
}

// cap: the most ranges the entry point takes (IMP_RMAX or TAOAMD_TAO_RNG); only
// imp_gt_kernel's unrolled loop is sized by it, every other kernel indexes by n_rng
static int imp_run(int32_t cap, int64_t n_dt, int64_t n_gt, int32_t n_cat, int32_t n_rng,
                   const int32_t *cat_off, const int32_t *order, const double *score,
                   const int32_t *dt_cat, const uint8_t *dt_type, const int32_t *link_same,
                   const int32_t *link_other, const int32_t *gt_cat, const uint32_t *gt_rng,
                   const uint8_t *held, double *precision, int32_t *num_gt, void *workspace,
                   size_t workspace_bytes, void *stream)
{
    if (!imp_sizes_ok(n_dt, n_gt, n_cat, n_rng, cap)) return TAOAMD_ERR_ARG;
    if (!cat_off || !precision || !num_gt || !workspace) return TAOAMD_ERR_ARG;
    if (n_dt > 0 && (!order || !score || !dt_cat || !dt_type || !link_same || !link_other))
        return TAOAMD_ERR_ARG;
    if (n_gt > 0 && (!gt_cat || !gt_rng || !held)) return TAOAMD_ERR_ARG;
    Carve c(workspace);
    ImpArgs a;
    imp_layout(c, n_dt, n_gt, n_cat, n_rng, a);
    if (!c.fits(workspace, workspace_bytes)) return TAOAMD_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    a.n_dt = n_dt; a.n_gt = n_gt; a.n_cat = n_cat; a.n_rng = n_rng;
    a.cat_off = cat_off; a.order = order; a.score = score; a.dt_cat = dt_cat;
    a.dt_type = dt_type; a.link_same = link_same; a.link_other = link_other;
    a.gt_cat = gt_cat; a.gt_rng = gt_rng; a.held = held;
    a.precision = precision; a.num_gt = num_gt;
    const size_t claims = (size_t)2 * n_rng * n_gt;
    if (n_gt > 0) {
        TAO_HIP(hipMemsetAsync(a.best, 0, claims * sizeof(unsigned long long), s));
        TAO_HIP(hipMemsetAsync(a.win, 0xff, claims * sizeof(uint32_t), s));
    }
    TAO_HIP(hipMemsetAsync(a.adopt, 0, (size_t)n_rng * (n_dt + n_cat) * sizeof(uint32_t), s));
    TAO_HIP(hipMemsetAsync(a.cnt, 0, (size_t)3 * n_cat * n_rng * sizeof(uint32_t), s));
    const unsigned row_blocks = (unsigned)((n_dt * n_rng + 255) / 256);
    if (n_dt > 0 && n_gt > 0) {
        TAO_TIMED("imp_best_kernel", s, imp_best_kernel<<<row_blocks, 256, 0, s>>>(a));
        TAO_TIMED("imp_win_kernel", s, imp_win_kernel<<<row_blocks, 256, 0, s>>>(a));
        TAO_TIMED("imp_adopt_kernel", s, imp_adopt_kernel<<<row_blocks, 256, 0, s>>>(a));
    }
    if (n_gt > 0) {
        const unsigned gt_blocks = (unsigned)((n_gt + 255) / 256);
        if (cap <= IMP_RMAX)
            TAO_TIMED("imp_gt_kernel", s, imp_gt_kernel<IMP_RMAX><<<gt_blocks, 256, 0, s>>>(a));
        else
            TAO_TIMED("imp_gt_kernel", s,
                      imp_gt_kernel<TAOAMD_TAO_RNG><<<gt_blocks, 256, 0, s>>>(a));
    }
    TAO_TIMED("imp_sweep_kernel", s,
              imp_sweep_kernel<<<(unsigned)((int64_t)n_cat * n_rng), IMP_CHUNK, 0, s>>>(a, rec_thr()));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

extern "C" int taoamd_error_impact(int64_t n_dt, int64_t n_gt, int32_t n_cat, int32_t n_rng,
                                   const int32_t *cat_off, const int32_t *order,
                                   const double *score, const int32_t *dt_cat,
                                   const uint8_t *dt_type, const int32_t *link_same,
                                   const int32_t *link_other, const int32_t *gt_cat,
                                   const uint32_t *gt_rng, const uint8_t *held,
                                   double *precision, int32_t *num_gt, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    return imp_run(IMP_RMAX, n_dt, n_gt, n_cat, n_rng, cat_off, order, score, dt_cat, dt_type,
                   link_same, link_other, gt_cat, gt_rng, held, precision, num_gt, workspace,
                   workspace_bytes, stream);
}

// The same sweep on the tables of the track level (taoamd_track_error_types_links):
// up to TAOAMD_TAO_RNG ranges.
extern "C" int taoamd_track_error_impact(int64_t n_dt, int64_t n_gt, int32_t n_cat, int32_t n_rng,
                                         const int32_t *cat_off, const int32_t *order,
                                         const double *score, const int32_t *dt_cat,
                                         const uint8_t *dt_type, const int32_t *link_same,
                                         const int32_t *link_other, const int32_t *gt_cat,
                                         const uint32_t *gt_rng, const uint8_t *held,
                                         double *precision, int32_t *num_gt, void *workspace,
                                         size_t workspace_bytes, void *stream)
{
    return imp_run(TAOAMD_TAO_RNG, n_dt, n_gt, n_cat, n_rng, cat_off, order, score, dt_cat,
                   dt_type, link_same, link_other, gt_cat, gt_rng, held, precision, num_gt,
                   workspace, workspace_bytes, stream);
}

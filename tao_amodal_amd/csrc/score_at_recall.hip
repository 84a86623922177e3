// eval["scores"]: the detection score at the row where recall first reaches
// each recall threshold (gfx950).  pycocotools' cocoeval.py keeps it beside the
// precision table (ss[ri] = dtScoresSorted[pi]); the reference's accumulate
// computes the very index it is read at and drops the array
// (lvis_amodal/eval.py:406-417 == tao_amodal/eval.py:562-573).
//
// For category k, range a, IoU threshold t and recall threshold j, with
// c = cj[k][a][j] the smallest TP count whose recall reaches rec_thrs[j]
// (recall_crossing, the table the sweeps of accumulate.hip use):
//   pi    = first sorted row of the category whose inclusive TP count is >= c
//           (c == 0: the category's first row, TP or not),
//   value = score of row pi; 0 where the category has no such row (the
//           reference's bare `except`); -1 where num_gt[k][a] == 0.
// No floating-point operation touches a value: it is a copy of an input score.
//
// Shaped like the chunked sweep of accumulate.hip: lane = (range, threshold)
// combo, rows 64 at a time through the 64 x 64 bit transpose, a category cut
// into chunks of SAR_CH rows so that a long one spreads over the chip:
//
//   sar_chunks    chunk table from cat_off (block scan)
//   sar_cj        the crossings cj[k][a][j] (recall_crossing)
//   sar_count     per (chunk, word): transposed TP words, TP count per combo
//   sar_prefix    per (category, word): exclusive prefix of the chunk counts
//   sar_select    per (chunk, word): every threshold whose c lies in
//                 (pre, pre + cnt] -> the (c - pre)-th set bit of the chunk's
//                 transposed words -> place[k][a][t][j] = that sorted row
//   sar_finalize  place -> scores[T][R][n_cat][n_rng]: the score gathered, the
//                 -1 / 0 fills, LDS-tiled so that both sides are coalesced
#include "common.hpp"
#include "transpose64.hpp"
#include "workspace.hpp"

using namespace taoamd;

#define SAR_CH 256                 // rows of a chunk
#define SAR_BLK (SAR_CH / WAVE)    // 64-row blocks per chunk
#define SAR_RMAX 8                 // ranges that can overlap one 64-combo word

struct SarArgs {
    int32_t n_cat, n_rng, n_words;
    int32_t paired;          // rows are (matched, ignored) pairs: ignored == matched + 1
    int32_t wide;            // ... 16-byte aligned: one load per pair
    const int32_t *cat_off;
    const uint64_t *matched;
    const uint64_t *ignored;
    const int32_t *order;    // optional: sorted position -> row of matched / ignored
    const int32_t *score_at; // sorted position -> element of score (null: the position itself)
    const double *score;
    const int32_t *num_gt;
    int32_t *cat_chunk_off;  // [n_cat + 1]
    uint32_t *cnt, *pre;     // [chunk][word][64] TP count of the chunk / of the chunks before it
    uint64_t *t_tp;          // [chunk][word][SAR_BLK][64] transposed TP words
    int32_t *cj;             // [n_cat][n_rng][N_REC] TP count crossing each recall threshold
    int32_t *place;          // [n_cat][n_rng][N_THR][N_REC] sorted row pi; -1: never reached
    double *scores;          // [N_THR][N_REC][n_cat][n_rng]
};

__global__ __launch_bounds__(256) void sar_chunks_kernel(SarArgs a)
{
    __shared__ int32_t part[256];
    const int per = (a.n_cat + 255) / 256;
    const int lo = min((int)threadIdx.x * per, a.n_cat), hi = min(lo + per, a.n_cat);
    auto chunks_of = [&](int k) {
        return (a.cat_off[k + 1] - a.cat_off[k] + SAR_CH - 1) / SAR_CH;
    };
    int32_t s = 0;
    for (int k = lo; k < hi; k++) s += chunks_of(k);
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        int32_t v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int32_t run = part[threadIdx.x] - s;
    for (int k = lo; k < hi; k++) {
        a.cat_chunk_off[k] = run;
        run += chunks_of(k);
    }
    if (threadIdx.x == 255) a.cat_chunk_off[a.n_cat] = part[255];
}

// cj[k][r][j] (np.searchsorted(rc, rec_thrs, side="left") on rc = tp / num_gt,
// reference lvis_amodal/eval.py:386,406-408); 0 where the range has no ground truth
__global__ void sar_cj_kernel(SarArgs a, RecThr rec)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)a.n_cat * a.n_rng * N_REC) return;
    const int64_t kr = i / N_REC;
    const int32_t ng = a.num_gt[kr];
    a.cj[i] = ng > 0 ? recall_crossing(rec.v[i - kr * N_REC], ng) : 0;
}

struct SarChunk {
    int32_t k, c, word, len;
    int64_t start;
    bool first, valid;
};

// wavefront = (chunk, word); the category owning the chunk: last k with
// cat_chunk_off[k] <= c (uniform)
__device__ __forceinline__ SarChunk sar_chunk(const SarArgs &a)
{
    SarChunk ci;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t item = (int64_t)blockIdx.x * 4 + wave;
    ci.c = (int32_t)(item / a.n_words);
    ci.word = (int32_t)(item - (int64_t)ci.c * a.n_words);
    ci.valid = ci.c < a.cat_chunk_off[a.n_cat];
    if (!ci.valid) return ci;
    int32_t lo = 0, hi = a.n_cat;
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (a.cat_chunk_off[mid] <= ci.c) lo = mid; else hi = mid;
    }
    ci.k = lo;
    const int32_t j = ci.c - a.cat_chunk_off[lo];
    ci.start = (int64_t)a.cat_off[lo] + (int64_t)j * SAR_CH;
    ci.len = (int32_t)min((int64_t)SAR_CH, (int64_t)a.cat_off[lo + 1] - ci.start);
    ci.first = j == 0;
    return ci;
}

// TP words (matched & ~ignored) of the chunk's rows, lane = row of a 64-row
// block.  Every load ahead of the first use; a lane past the chunk's rows
// re-reads the chunk's first row and drops it.
__device__ __forceinline__ void sar_load(const SarArgs &a, const SarChunk &ci, int lane,
                                         uint64_t (&tpw)[SAR_BLK])
{
    int64_t at[SAR_BLK];
#pragma unroll
    for (int blk = 0; blk < SAR_BLK; blk++) {
        const int i = blk * WAVE + lane;
        const int64_t p = ci.start + (i < ci.len ? i : 0);
        at[blk] = a.order ? (int64_t)a.order[p] : p;
    }
    uint64_t m[SAR_BLK], ig[SAR_BLK];
#pragma unroll
    for (int blk = 0; blk < SAR_BLK; blk++) {
        const int64_t e = at[blk] * a.n_words + ci.word;
        if (a.wide) {
            const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(a.matched + 2 * e);
            m[blk] = v.x;
            ig[blk] = v.y;
        } else if (a.paired) {
            m[blk] = a.matched[2 * e];
            ig[blk] = a.matched[2 * e + 1];
        } else {
            m[blk] = a.matched[e];
            ig[blk] = a.ignored[e];
        }
    }
#pragma unroll
    for (int blk = 0; blk < SAR_BLK; blk++)
        tpw[blk] = blk * WAVE + lane < ci.len ? m[blk] & ~ig[blk] : 0;
}

__global__ __launch_bounds__(256) void sar_count_kernel(SarArgs a)
{
    const SarChunk ci = sar_chunk(a);
    if (!ci.valid) return;
    const int lane = lane_id();
    uint64_t tpw[SAR_BLK];
    sar_load(a, ci, lane, tpw);
    const int64_t o = ((int64_t)ci.c * a.n_words + ci.word) * WAVE + lane;
    uint32_t tp = 0;
#pragma unroll
    for (int blk = 0; blk < SAR_BLK; blk++) {
        // (blocks past the chunk's rows: zero words)
        const uint64_t T = blk * WAVE < ci.len ? transpose64(tpw[blk], lane) : 0;
        a.t_tp[(o - lane) * SAR_BLK + blk * WAVE + lane] = T;
        tp += (uint32_t)__popcll(T);
    }
    a.cnt[o] = tp;
}

// one workgroup per (category, word): the four wavefronts scan a quarter of the
// category's chunks each, the quarters are stitched through LDS
__global__ __launch_bounds__(256) void sar_prefix_kernel(SarArgs a)
{
    __shared__ uint32_t s_tp[4][WAVE];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int32_t k = (int32_t)(blockIdx.x / a.n_words);
    const int word = (int)(blockIdx.x % a.n_words);
    const int lane = lane_id();
    const int32_t c0 = a.cat_chunk_off[k], c1 = a.cat_chunk_off[k + 1];
    const int32_t q = (c1 - c0 + 3) / 4;
    const int32_t lo = min(c1, c0 + wave * q), hi = min(c1, lo + q);
    uint32_t tp = 0;
    // eight chunks per step: their loads in flight together, then the stores
    for (int32_t c = lo; c < hi; c += 8) {
        uint32_t t_[8];
#pragma unroll
        for (int u = 0; u < 8; u++)
            t_[u] = a.cnt[((int64_t)min(c + u, hi - 1) * a.n_words + word) * WAVE + lane];
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (c + u < hi) {
                a.pre[((int64_t)(c + u) * a.n_words + word) * WAVE + lane] = tp;
                tp += t_[u];
            }
    }
    s_tp[wave][lane] = tp;
    __syncthreads();
    uint32_t before = 0;                           // the earlier quarters
    for (int w = 0; w < wave; w++) before += s_tp[w][lane];
    if (wave > 0 && __ballot(before) != 0)
        for (int32_t c = lo; c < hi; c++)
            a.pre[((int64_t)c * a.n_words + word) * WAVE + lane] += before;
}

// position of the r-th set bit of w, r in [1, popcount(w)]: the half that holds
// it by the popcount of the lower half, six times
__device__ __forceinline__ int select64(uint64_t w, uint32_t r)
{
    uint32_t x = (uint32_t)w;
    int pos = 0;
    uint32_t c = (uint32_t)__popc(x);
    if (r > c) { r -= c; pos = 32; x = (uint32_t)(w >> 32); }
    c = (uint32_t)__popc(x & 0xffffu);
    if (r > c) { r -= c; pos += 16; x >>= 16; }
    c = (uint32_t)__popc(x & 0xffu);
    if (r > c) { r -= c; pos += 8; x >>= 8; }
    c = (uint32_t)__popc(x & 0xfu);
    if (r > c) { r -= c; pos += 4; x >>= 4; }
    c = (uint32_t)__popc(x & 0x3u);
    if (r > c) { r -= c; pos += 2; x >>= 2; }
    if (r > (x & 1u)) pos += 1;
    return pos;
}

__global__ __launch_bounds__(256) void sar_select_kernel(SarArgs a)
{
    __shared__ int32_t s_cj[4][SAR_RMAX][N_REC];
    const SarChunk ci = sar_chunk(a);
    if (!ci.valid) return;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int combo = ci.word * WAVE + lane;
    const bool active = combo < a.n_rng * N_THR;
    const int r = active ? combo / N_THR : 0;
    const int t = active ? combo - r * N_THR : 0;
    const int r_lo = (ci.word * WAVE) / N_THR;
    const int r_hi = min(a.n_rng - 1, (ci.word * WAVE + WAVE - 1) / N_THR);
    const int64_t o = ((int64_t)ci.c * a.n_words + ci.word) * WAVE + lane;
    const uint32_t tp0 = a.pre[o], cnt = a.cnt[o];
    uint64_t T[SAR_BLK];
#pragma unroll
    for (int blk = 0; blk < SAR_BLK; blk++) T[blk] = a.t_tp[(o - lane) * SAR_BLK + blk * WAVE + lane];
    // crossings of the ranges this word overlaps -> LDS (one copy per wavefront)
    for (int q = 0; q <= r_hi - r_lo; q++) {
        const int32_t *src = a.cj + ((int64_t)ci.k * a.n_rng + r_lo + q) * N_REC;
        s_cj[wave][q][lane] = src[lane];
        if (lane + WAVE < N_REC) s_cj[wave][q][lane + WAVE] = src[lane + WAVE];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const int64_t kr = (int64_t)ci.k * a.n_rng + r;
    if (!active || a.num_gt[kr] <= 0) return;
    const int32_t *__restrict__ cj = s_cj[wave][r - r_lo];
    int32_t *__restrict__ out = a.place + (kr * N_THR + t) * N_REC;
    // thresholds crossed at TP count 0 sit on the category's first row
    if (ci.first)
        for (int j = 0; j < N_REC && cj[j] == 0; j++) out[j] = (int32_t)ci.start;
    // first threshold not reached before this chunk: cj is non-decreasing in j
    int j = 0;
    {
        int lo = 0, hi = N_REC;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cj[mid] <= (int32_t)tp0) lo = mid + 1; else hi = mid;
        }
        j = lo;
    }
    const uint32_t end = tp0 + cnt;
    uint32_t c = j < N_REC ? (uint32_t)cj[j] : 0xffffffffu;
    if (c > end) return;
    uint32_t base = tp0;                           // TP count before the block
#pragma unroll
    for (int blk = 0; blk < SAR_BLK; blk++) {
        const uint32_t pc = (uint32_t)__popcll(T[blk]);
        while (c <= base + pc) {                   // (c > base: the blocks before are done)
            out[j] = (int32_t)(ci.start + blk * WAVE + select64(T[blk], c - base));
            j++;
            c = j < N_REC ? (uint32_t)cj[j] : 0xffffffffu;
        }
        base += pc;
    }
}

// place[KR][T * R] -> scores[T * R][KR]: one workgroup = 64 (k, r) rows x 64
// (t, j) columns.  Read side lane = column (coalesced places, the scores
// gathered), write side lane = row.  Rows without evaluated ground truth are
// never read.
#define SAR_TILE 64

__global__ __launch_bounds__(256) void sar_finalize_kernel(SarArgs a)
{
    __shared__ double tile[SAR_TILE][SAR_TILE + 1];
    const int64_t KR = (int64_t)a.n_cat * a.n_rng;
    const int64_t COLS = (int64_t)N_THR * N_REC;
    const int64_t row0 = (int64_t)blockIdx.x * SAR_TILE;
    const int64_t col0 = (int64_t)blockIdx.y * SAR_TILE;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ncol = (int)min((int64_t)SAR_TILE, COLS - col0);
    for (int i = wave; i < SAR_TILE; i += 4) {
        const int64_t row = row0 + i;
        if (row >= KR || a.num_gt[row] <= 0) continue;         // (uniform)
        double v = 0.0;
        if (lane < ncol) {
            const int32_t p = a.place[row * COLS + col0 + lane];
            if (p >= 0) v = a.score[a.score_at ? (int64_t)a.score_at[p] : (int64_t)p];
        }
        tile[i][lane] = v;
    }
    __syncthreads();
    const int64_t orow = row0 + lane;
    if (orow >= KR) return;
    const bool live = a.num_gt[orow] > 0;
    for (int c = wave; c < ncol; c += 4)
        a.scores[(col0 + c) * KR + orow] = live ? tile[lane][c] : -1.0;
}

static int32_t sar_max_chunks(int64_t n_dt, int32_t n_cat)
{
    return (int32_t)((n_dt + SAR_CH - 1) / SAR_CH + n_cat);
}

// The tables of the pass, in buffer order: a function of (n_dt, n_cat, n_rng)
static void sar_layout(Carve &c, int64_t n_dt, int32_t n_cat, int32_t n_rng, SarArgs &a)
{
    a.n_words = (n_rng * N_THR + 63) / 64;
    const size_t nw = (size_t)a.n_words, nc = (size_t)sar_max_chunks(n_dt, n_cat);
    a.cat_chunk_off = c.take<int32_t>((size_t)n_cat + 1);
    a.cnt = c.take<uint32_t>(nc * nw * WAVE);
    a.pre = c.take<uint32_t>(nc * nw * WAVE);
    a.t_tp = c.take<uint64_t>(nc * nw * SAR_BLK * WAVE);
    a.cj = c.take<int32_t>((size_t)n_cat * n_rng * N_REC);
    a.place = c.take<int32_t>((size_t)n_cat * n_rng * N_THR * N_REC);
}

extern "C" size_t taoamd_score_at_recall_workspace(int64_t n_dt, int32_t n_cat, int32_t n_rng)
{
    if (n_dt < 0 || n_cat <= 0 || n_rng < 1 || n_rng > 32) return 0;
    SarArgs a;
    return measure([&](Carve &c) { sar_layout(c, n_dt, n_cat, n_rng, a); });
}

extern "C" int taoamd_score_at_recall(int64_t n_dt, int32_t n_cat, int32_t n_rng,
                                      const int32_t *cat_off, const int32_t *order,
                                      const uint64_t *matched, const uint64_t *ignored,
                                      const double *score, const int32_t *score_order,
                                      const int32_t *num_gt,
                                      double *scores, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    if (n_dt < 0 || n_dt > 0x7fffffff || n_cat <= 0 || n_rng < 1 || n_rng > 32)
        return TAOAMD_ERR_ARG;
    if (!cat_off || !num_gt || !scores || !workspace) return TAOAMD_ERR_ARG;
    if (n_dt > 0 && (!matched || !ignored || !score)) return TAOAMD_ERR_ARG;
    Carve c(workspace);
    SarArgs a;
    sar_layout(c, n_dt, n_cat, n_rng, a);
    if (!c.fits(workspace, workspace_bytes)) return TAOAMD_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    a.n_cat = n_cat; a.n_rng = n_rng;
    a.cat_off = cat_off; a.matched = matched; a.ignored = ignored; a.order = order;
    a.paired = matched != nullptr && ignored == matched + 1;
    a.wide = a.paired && ((uintptr_t)matched & 15) == 0;
    a.score = score; a.score_at = score_order ? score_order : order; a.num_gt = num_gt; a.scores = scores;
    const size_t nw = (size_t)a.n_words, nc = (size_t)sar_max_chunks(n_dt, n_cat);
    const int64_t n_cj = (int64_t)n_cat * n_rng * N_REC;
    const unsigned chunk_blocks = (unsigned)((nc * nw + 3) / 4);
    // a threshold no chunk reaches keeps -1: all bits set
    TAO_HIP(hipMemsetAsync(a.place, 0xff, (size_t)n_cj * N_THR * sizeof(int32_t), s));
    TAO_TIMED("sar_chunks_kernel", s, sar_chunks_kernel<<<1, 256, 0, s>>>(a));
    TAO_TIMED("sar_cj_kernel", s, sar_cj_kernel<<<(unsigned)((n_cj + 255) / 256), 256, 0, s>>>(a, rec_thr()));
    TAO_TIMED("sar_count_kernel", s, sar_count_kernel<<<chunk_blocks, 256, 0, s>>>(a));
    TAO_TIMED("sar_prefix_kernel", s, sar_prefix_kernel<<<(unsigned)((size_t)n_cat * nw), 256, 0, s>>>(a));
    TAO_TIMED("sar_select_kernel", s, sar_select_kernel<<<chunk_blocks, 256, 0, s>>>(a));
    const int64_t KR = (int64_t)n_cat * n_rng;
    dim3 grid((unsigned)((KR + SAR_TILE - 1) / SAR_TILE),
              (unsigned)((N_THR * N_REC + SAR_TILE - 1) / SAR_TILE));
    TAO_TIMED("sar_finalize_kernel", s, sar_finalize_kernel<<<grid, 256, 0, s>>>(a));
    TAO_LAUNCH_CHECK();
    return TAOAMD_OK;
}

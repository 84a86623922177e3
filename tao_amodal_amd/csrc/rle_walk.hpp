// Device code shared by the two run-length IoU kernels: rle_iou.hip (mask
// pairs of an image-level cell) and track_mask_iou.hip (the shared frames of
// a pair of mask tracks).  The method is described at the head of rle_iou.hip:
// per mask, once, E[r] = pixels up to the end of run r and P[r] = ones up to
// the end of run r; |A & B| is then a signed sum over A's run boundaries of
// F_B(E_A[i]), dealt to the lanes of a wavefront, RLE_RPT CONSECUTIVE
// boundaries per lane.
#pragma once
#include "common.hpp"
#include "workspace.hpp"

#define RLE_RPT 8               // run boundaries of A a lane keeps in registers (even)

// one wavefront per mask: inclusive scans of the run lengths and of the
// lengths of the odd-numbered runs (the ones)
// (detections are only ever the "A" of a pair: their P is not stored.  Summing
// their boundaries inside the IoU kernel instead, lazily for the detections
// that have a pair to walk, was measured slower: 0.56 vs 0.54 ms.)
template <bool WITH_P>
__global__ __launch_bounds__(256) void rle_prefix_kernel(int64_t n,
                                                         const int64_t *off,
                                                         const uint32_t *runs,
                                                         void *out, uint32_t *ones)
{
    const int lane = taoamd::lane_id();
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= n) return;
    const int64_t b = off[m], k = off[m + 1] - b;
    uint32_t carry_e = 0, carry_p = 0;
    for (int64_t base = 0; base < k; base += WAVE) {
        const int64_t i = base + lane;
        const uint32_t c = i < k ? runs[b + i] : 0;
        uint32_t e = c, p = (i & 1) ? c : 0;
#pragma unroll
        for (int s = 1; s < WAVE; s <<= 1) {
            const uint32_t ue = __shfl_up(e, s, WAVE), up = __shfl_up(p, s, WAVE);
            if (lane >= s) { e += ue; p += up; }
        }
        e += carry_e;
        p += carry_p;
        if (i < k) {
            if (WITH_P) ((uint2 *)out)[b + i] = make_uint2(e, p);
            else ((uint32_t *)out)[b + i] = e;
        }
        carry_e = __shfl(e, WAVE - 1, WAVE);
        carry_p = __shfl(p, WAVE - 1, WAVE);
    }
    if (lane == 0) ones[m] = carry_p;
}

// The workspace of both IoU stages: the tables rle_prefix_kernel writes for the
// n_dt / n_gt masks of dt_runs / gt_runs runs (A: RleArgs, TrackMaskArgs)
template <class A>
static void rle_layout(taoamd::Carve &c, int64_t n_dt, int64_t dt_runs, int64_t n_gt,
                       int64_t gt_runs, A &a)
{
    a.dt_end = c.take<uint32_t>((size_t)dt_runs);
    a.gt_pre = c.take<uint2>((size_t)gt_runs);
    a.dt_ones = c.take<uint32_t>((size_t)n_dt);
    a.gt_ones = c.take<uint32_t>((size_t)n_gt);
}

// A's run boundaries of one piece (RLE_RPT * 64 of them) into the lane's
// registers: the lane owns i = piece base + lane*RPT + q (RLE_RPT is even: the
// parity of i is q's).  An even one (start of a run of ones) only counts when
// that run exists.  Past the end: 0, a boundary that makes the walk stand still.
__device__ __forceinline__ void rle_load_piece(uint32_t piece, int lane,
                                               const uint32_t *__restrict__ a_end,
                                               uint32_t ka, uint32_t (&xq)[RLE_RPT],
                                               bool (&use)[RLE_RPT])
{
#pragma unroll
    for (int q = 0; q < RLE_RPT; q++) {
        const uint32_t i = piece * (RLE_RPT * WAVE) + (uint32_t)lane * RLE_RPT + q;
        use[q] = i < ka && ((i & 1) || i + 1 < ka);
        xq[q] = i < ka ? a_end[i] : 0u;
    }
}

// Adds the lane's signed share of |A & B| (modulo 2^32) for the boundaries it
// holds against B's (E, P) table of kb >= 1 runs with ones_b ones in all.
__device__ __forceinline__ void rle_lane_walk(const uint32_t (&xq)[RLE_RPT],
                                              const bool (&use)[RLE_RPT],
                                              const uint2 *__restrict__ tab,
                                              uint32_t kb, uint32_t ones_b,
                                              uint32_t &acc)
{
    // one binary search per lane, for its first boundary
    // (branch-free: ceil(log2(kb + 1)) halvings) ...
    uint32_t lo = 0, hi = kb;
    for (uint32_t span = kb; span != 0; span >>= 1) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint32_t e = tab[min(mid, kb - 1)].x;
        const bool open = lo < hi, right = e <= xq[0];
        lo = (open && right) ? mid + 1 : lo;
        hi = (open && !right) ? mid : hi;
    }
    // ... then B's runs are followed while the lane's own
    // boundaries rise: both lists are sorted, so all of it is
    // one merge of ~RLE_RPT * (1 + kb / ka) steps per lane.
    // (Searching every boundary on its own costs ~10 rounds
    // x 12 VALU instructions each: measured 4x slower, the
    // kernel is bound by instruction issue, not by the LDS.)
    uint32_t r = lo;
    uint2 cur = tab[min(r, kb - 1)];
#pragma unroll
    for (int q = 0; q < RLE_RPT; q++) {
        if (!use[q]) continue;      // (also the trailing run of zeros)
        const uint32_t x = xq[q];
        // a few steps usually do; a long stretch of B inside
        // one run of A (A in two distant parts, A's last run)
        // is crossed by bisection instead
        for (int step = 0; step < 4 && r < kb && cur.x <= x; step++) {
            r++;
            cur = tab[min(r, kb - 1)];
        }
        if (r < kb && cur.x <= x) {
            uint32_t l2 = r + 1, h2 = kb;
            while (l2 < h2) {
                const uint32_t mid = (l2 + h2) >> 1;
                if (tab[mid].x <= x) l2 = mid + 1; else h2 = mid;
            }
            r = l2;
            cur = tab[min(r, kb - 1)];
        }
        const uint32_t part = (r & 1) ? cur.x - x : 0u;
        const uint32_t f = r < kb ? cur.y - part : ones_b;
        acc += (q & 1) ? f : 0u - f;
    }
}

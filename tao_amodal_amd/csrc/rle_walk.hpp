// Device code shared by the two run-length IoU kernels: rle_iou.hip (mask
// pairs of an image-level cell) and track_mask_iou.hip (the shared frames of
// a pair of mask tracks).  The method is described at the head of rle_iou.hip:
// per mask, once, E[r] = pixels up to the end of run r and P[r] = ones up to
// the end of run r; |A & B| is then a signed sum over A's run boundaries of
// F_B(E_A[i]), dealt to the lanes of a wavefront, RLE_RPT CONSECUTIVE
// boundaries per lane.
//
// That sum counts every pixel of the frame.  The reference's two-cursor loops
// (rleIou, rleMerge) end when the pixels left in the two current runs add up
// to 0 as C unsigned ints, and that also happens before the frame's end:
//   - both cursors finish a run at the same pixel and the next run of each
//     mask is empty (both then hold 0);
//   - the two current runs have 2^32 pixels left between them (frames of 2^31
//     pixels and more).
// The reference ignores every pixel from there on, and so must the kernels.
// Both cases are rare and recognised before a pair is walked (a flag per
// ground truth, the frame's size, then rle_stops_early: a superset); such a pair is walked with the two cursors themselves
// (rle_two_cursors), every other pair by the sum above.
//
// Outside the domain: run lists whose lengths add up to 2^32 or more (the
// prefix sums cannot hold them; taoamd_rle_add_counts / _string refuse them),
// lists that do not add up to height * width (the frame size stands for the
// totals where the second case is looked for), and a pair whose two lists add up to different totals -- on such a pair the
// reference's loop never returns (c = umin(0, cb) = 0 for ever); the kernels
// return some number.
#pragma once
#include "common.hpp"
#include "workspace.hpp"

#define RLE_RPT 8               // run boundaries of A a lane keeps in registers (even)

// one wavefront per mask: inclusive scans of the run lengths and of the
// lengths of the odd-numbered runs (the ones)
// (detections are only ever the "A" of a pair: their P is not stored.  Summing
// their boundaries inside the IoU kernel instead, lazily for the detections
// that have a pair to walk, was measured slower: 0.56 vs 0.54 ms.)
// P of run 0 is 0 for every mask (run 0 holds zeros): with WITH_P that word
// keeps the mask's flag "a run other than the first is empty" instead -- 1
// sends all pairs of the mask to rle_two_cursors, which never reads the table.
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
    bool empty_run = false;
    for (int64_t base = 0; base < k; base += WAVE) {
        const int64_t i = base + lane;
        const uint32_t c = i < k ? runs[b + i] : 0;
        empty_run |= i >= 1 && i < k && c == 0;
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
    if (WITH_P) {
        const bool any = __ballot(empty_run) != 0;
        if (lane == 0 && k > 0 && any) ((uint2 *)out)[b].y = 1u;   // (after this lane's own store of entry 0)
    }
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
    // (`<=` here and in the bisection below, `<` would give the same sums: F_B
    // is continuous at a run's end, and the follow loop steps over a tie)
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

// Whether the reference's loop may stop before the frame's end on this pair (a
// superset, wavefront-uniform; ka, kb >= 1).  Callers ask only for the rare
// pair whose ground truth carries the flag of rle_prefix_kernel (b_flag: the
// P word of its table entry 0) or whose frame has 2^31 pixels or more
// (rle_big_frame): without an empty run the loop stops early only on 2^32
// pixels left in two runs, which takes two lists of 2^32 pixels between them
// whose longest runs add up to that.
__device__ __forceinline__ bool rle_big_frame(int32_t h, int32_t w)
{
    return (uint64_t)(uint32_t)h * (uint32_t)w >= (1ull << 31);
}

__device__ __forceinline__ bool rle_stops_early(int lane, const uint32_t *__restrict__ ra,
                                                uint32_t ka, const uint32_t *__restrict__ rb,
                                                uint32_t kb, uint32_t b_flag)
{
    if (b_flag != 0) return true;
    uint32_t ma = 0, mb = 0;
    for (uint32_t i = lane; i < ka; i += WAVE) ma = max(ma, ra[i]);
    for (uint32_t i = lane; i < kb; i += WAVE) mb = max(mb, rb[i]);
#pragma unroll
    for (int s = WAVE / 2; s > 0; s >>= 1) {
        ma = max(ma, (uint32_t)__shfl_xor(ma, s, WAVE));
        mb = max(mb, (uint32_t)__shfl_xor(mb, s, WAVE));
    }
    return (uint64_t)ma + mb >= (1ull << 32);
}

// |A & B| and |A | B| as the reference's loop counts them (maskApi.c:85-92,
// and the areas of rleMerge's two results): ka, kb >= 1 raw run lengths.
// Every lane does the same steps and returns the same numbers.  The loop takes
// at most ka + kb + 1 steps on lists of one total; the bound ends it on a
// pair of unequal totals, where the reference's never returns.
__device__ __forceinline__ void rle_two_cursors(const uint32_t *__restrict__ ra, uint32_t ka,
                                                const uint32_t *__restrict__ rb, uint32_t kb,
                                                uint32_t &inter, uint32_t &uni)
{
    uint32_t ca = ra[0], cb = rb[0], a = 1, b = 1, ct = 1, i = 0, u = 0;
    bool va = false, vb = false;
    for (uint64_t step = 0; ct > 0 && step < (uint64_t)ka + kb + 2; step++) {
        const uint32_t c = min(ca, cb);
        if (va || vb) {
            u += c;
            if (va && vb) i += c;
        }
        ct = 0;
        ca -= c;
        if (!ca && a < ka) { ca = ra[a++]; va = !va; }
        ct += ca;
        cb -= c;
        if (!cb && b < kb) { cb = rb[b++]; vb = !vb; }
        ct += cb;
    }
    inter = i;
    uni = u;
}

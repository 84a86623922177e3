// The WINNER rule of the error impact (include/tao_amodal_hip.h, "error impact"),
// shared by error_impact.hip and confusion.hip so that the two cannot drift
// apart: the key whose maximum is the best claim, and which (row, range) pairs
// claim a ground truth at all.
#pragma once
#include "common.hpp"

namespace taoamd {

// Greater key = better claim: greater score, -0.0 == 0.0, a NaN below every
// number; never 0.
__device__ __forceinline__ unsigned long long imp_key(double s)
{
    return ~score_desc_key(s);
}

// The tables a claim reads
struct ClaimTabs {
    int64_t n_gt;
    int32_t n_cat, n_rng;
    const int32_t *dt_cat;
    const uint8_t *dt_type;                  // [n_dt][n_rng]
    const int32_t *link_same, *link_other;   // [n_dt][n_rng]; link_same may be null: no LOC claims
    const uint8_t *held;                     // [n_rng][n_gt]
};

// The claim of (row d, range r): which table (0 LOC by link_same, 1 CLS by
// link_other) and which ground truth g; false where the row claims nothing
__device__ __forceinline__ bool claim_of(const ClaimTabs &t, int64_t d, int r, int &tab, int64_t &g)
{
    const int32_t cat = t.dt_cat[d];
    if (cat < 0 || cat >= t.n_cat) return false;
    const int ty = t.dt_type[d * t.n_rng + r];
    if (ty != ERR_LOC && ty != ERR_CLS) return false;
    tab = ty == ERR_CLS;
    if (!tab && !t.link_same) return false;
    g = tab ? t.link_other[d * t.n_rng + r] : t.link_same[d * t.n_rng + r];
    if (g < 0 || g >= t.n_gt) return false;
    return !t.held[(int64_t)r * t.n_gt + g];
}

// Two passes over the claimants of a slot leave win[slot] = the winner: the
// atomic max of the key, then among the rows that hold it the atomic min of the
// row.  best[] starts at 0 (no claim), win[] at 0xffffffff.
__device__ __forceinline__ void claim_best(unsigned long long *best, int64_t slot, double score)
{
    atomicMax(best + slot, imp_key(score));
}
__device__ __forceinline__ void claim_win(const unsigned long long *best, uint32_t *win,
                                          int64_t slot, double score, int64_t d)
{
    if (best[slot] == imp_key(score)) atomicMin(win + slot, (uint32_t)d);
}

}  // namespace taoamd

// 64 x 64 bit-matrix transpose across a wavefront (gfx950), shared by the
// sweeps of accumulate.hip and score_at_recall.hip.
#pragma once
#include "common.hpp"

// value of lane (i ^ S): CDNA4 lane permutes that need neither an address VGPR
// nor a round trip through the LDS crossbar queue (what __shfl_xor compiles to,
// ds_bpermute_b32): v_permlane32_swap / v_permlane16_swap for the two widest
// strides, DPP row_ror:8 and quad_perm for 8 / 2 / 1, ds_swizzle for 4
template <int S>
__device__ __forceinline__ uint32_t xor_lane(uint32_t x, int lane)
{
    if constexpr (S == 32) {
        auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
        return (lane & 32) ? r[0] : r[1];
    } else if constexpr (S == 16) {
        auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
        return (lane & 16) ? r[0] : r[1];
    } else if constexpr (S == 8) {
        return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x128, 0xf, 0xf, false);   // row_ror:8
    } else if constexpr (S == 4) {
        return (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, 0x101f);                // xor 4
    } else if constexpr (S == 2) {
        return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4e, 0xf, 0xf, false);    // [2,3,0,1]
    } else {
        return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xb1, 0xf, 0xf, false);    // [1,0,3,2]
    }
}

// 64 x 64 bit-matrix transpose across the wavefront: in: lane i holds row i
// (bit j = element (i, j)); out: lane j holds column j (bit i = element (i, j)).
// Stage S swaps the off-diagonal S x S blocks between lanes i and i ^ S.
//
// Round 4: ~30 VALU instructions instead of ~100 (the ternaries of the first
// version compiled to exec-masked branches, both sides executed; the sweep is
// bound by VALU issue -- a wave64 instruction occupies its SIMD for four
// cycles -- and the transposes were 0.12 ms of chip time at 21 M rows):
//   S = 32  the two words change places between the wave's halves: ONE
//           v_permlane32_swap (lower lanes' hi <-> upper lanes' lo);
//   S = 16  half words move: see transpose64 (one v_permlane16_swap for both
//           words, four v_perm_b32 with constant selectors);
//   S = 8   whole bytes move: the partner's word (DPP row_ror:8) and ONE
//           v_perm_b32 with a per-lane selector;
//   S = 4, 2, 1  the partner's word rotated so that the bits it hands over
//           sit where they go (v_alignbit, per-lane amount) and ONE v_bfi.
struct TransposeConsts {
    uint32_t sel8;                 // v_perm_b32 selector
    uint32_t keep4, keep2, keep1;  // bits of my own word that stay
    uint32_t rot4, rot2, rot1;     // right-rotation of the partner's word
};
__device__ __forceinline__ TransposeConsts transpose_consts(int lane)
{
    TransposeConsts c;
    // lower lane of a pair keeps the low part and takes the partner's low part
    // into its high part; the upper lane the other way round
    c.sel8 = (lane & 8) ? 0x03070105u : 0x06020400u;
    c.keep4 = (lane & 4) ? 0xf0f0f0f0u : 0x0f0f0f0fu;
    c.keep2 = (lane & 2) ? 0xccccccccu : 0x33333333u;
    c.keep1 = (lane & 1) ? 0xaaaaaaaau : 0x55555555u;
    c.rot4 = (lane & 4) ? 4 : 28;      // upper: partner >> S; lower: partner << S
    c.rot2 = (lane & 2) ? 2 : 30;
    c.rot1 = (lane & 1) ? 1 : 31;
    return c;
}
template <int S>
__device__ __forceinline__ uint32_t transpose_bits(uint32_t x, int lane, uint32_t keep,
                                                   uint32_t rot)
{
    const uint32_t y = xor_lane<S>(x, lane);
    const uint32_t r = __builtin_amdgcn_alignbit(y, y, rot);
    return (x & keep) | (r & ~keep);                       // v_bfi_b32
}
__device__ __forceinline__ uint64_t transpose64(uint64_t x, int lane, const TransposeConsts &c)
{
    uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    {
        // vdst lanes 32..63 <-> src lanes 0..31
        auto r = __builtin_amdgcn_permlane32_swap(lo, hi, false, false);
        lo = r[0];
        hi = r[1];
    }
    {
        // S = 16 (round 6): the halves that change lanes gathered into ONE
        // register first -- P = the low halves of (lo, hi), Q = the high ones;
        // the lower lane of a pair keeps P and needs its partner's P, the upper
        // one keeps Q and needs its partner's Q -- so that a single
        // v_permlane16_swap (odd rows of P <-> even rows of Q) serves both
        // words and both directions, and the two words are put together again
        // with the same selectors in every lane: 5 instructions for the stage
        // instead of 8 (a copy, a swap, a per-lane select and a v_perm a word).
        const uint32_t p = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
        const uint32_t q = __builtin_amdgcn_perm(hi, lo, 0x07060302u);
        auto r = __builtin_amdgcn_permlane16_swap(p, q, false, false);
        lo = __builtin_amdgcn_perm(r[1], r[0], 0x05040100u);
        hi = __builtin_amdgcn_perm(r[1], r[0], 0x07060302u);
    }
    lo = __builtin_amdgcn_perm(xor_lane<8>(lo, lane), lo, c.sel8);
    hi = __builtin_amdgcn_perm(xor_lane<8>(hi, lane), hi, c.sel8);
    lo = transpose_bits<4>(lo, lane, c.keep4, c.rot4);
    hi = transpose_bits<4>(hi, lane, c.keep4, c.rot4);
    lo = transpose_bits<2>(lo, lane, c.keep2, c.rot2);
    hi = transpose_bits<2>(hi, lane, c.keep2, c.rot2);
    lo = transpose_bits<1>(lo, lane, c.keep1, c.rot1);
    hi = transpose_bits<1>(hi, lane, c.keep1, c.rot1);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t transpose64(uint64_t x, int lane)
{
    return transpose64(x, lane, transpose_consts(lane));
}

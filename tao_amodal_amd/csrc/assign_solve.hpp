// The wavefront assignment solver of the track analyses: a maximum-weight
// bipartite assignment by shortest augmenting paths (Hungarian in the Jonker-
// Volgenant form, on cost = -weight), one wavefront a problem.  The identity
// (track_identity.hip: a cell's tracks, weight share * (n + 1) + (share > 0)),
// HOTA (track_hota.hip: a frame's boxes, weight w) and CLEAR (track_clear.hip: a
// step's stored candidates, weight q + the bonus of continuity) share it; the
// weight is a functor, computed on the fly, so no matrix is stored.
//
// A row a time; a step scans the free columns, lanes striding them (ceil(m / 64)
// a lane), the minimum (value, column) by a wavefront reduction -- the lowest
// column among equal values, so the result is one function of the input;
// potentials in 64 bits (the caller sees to it that n weights fit).  Every loop
// has a bound known at entry: n rows, at most m + 1 steps an augmentation, at
// most m + 1 edges of a path; a bound that runs out returns false.
// The wavefront is the workgroup, so __syncthreads() is the fence between its
// lanes' stores and loads of the search state, in LDS and in global memory alike;
// all control flow around it is uniform.
//
// Around the solver, what its three users share: where the search state lives
// (SearchLds in LDS, SearchStore in the workspace), which side becomes the rows
// (assign_sides) and the walk over the assigned pairs (assign_pairs).  The weight
// functors and what becomes of a pair are each kernel's own.
#pragma once
#include "common.hpp"
#include "workspace.hpp"

namespace taoamd {

#define ASSIGN_INF 0x1fffffffffffffffll

// The search state: column arrays of m entries, u of n, the index lists
struct Search {
    long long *u, *v, *minv;
    int32_t *p, *way, *used;
    const int32_t *ridx, *cidx;      // what the weight functor is told of row i / column j
};

// The state of a cell (a tile) whose sides are at most N, declared __shared__ by
// the kernel, and two index lists beside it
template <int N> struct SearchLds {
    long long u[N], v[N], minv[N];
    int32_t p[N], way[N], used[N], idx0[N], idx1[N];
    __device__ __forceinline__ Search search()
    {
        return {u, v, minv, p, way, used, nullptr, nullptr};
    }
};

// The state of the cells beyond LDS: six workspace arrays of n = n_dt + n_gt
// entries; cell c owns [base, the next cell's), base = cell_dt_off[c] +
// cell_gt_off[c], and one wavefront walks it
struct SearchStore {
    long long *u, *v, *minv;
    int32_t *p, *way, *used;
    void layout(Carve &c, size_t n)
    {
        u = c.take<long long>(n);
        v = c.take<long long>(n);
        minv = c.take<long long>(n);
        p = c.take<int32_t>(n);
        way = c.take<int32_t>(n);
        used = c.take<int32_t>(n);
    }
    __device__ __forceinline__ Search at(int64_t base) const
    {
        return {u + base, v + base, minv + base, p + base, way + base, used + base, nullptr,
                nullptr};
    }
};

// The smaller of two sides becomes the rows (n <= m), the FIRST where they are
// equal.  The solver breaks ties by the lowest column, so that choice is part of
// the result: HOTA and CLEAR pass the ground truths first.  (The identity takes
// the detections when equal; its kernel has the choice written out.)
struct Sides {
    bool first;                      // the rows are the first side's entries
    int n, m;
    const int32_t *rows, *cols;      // the two lists, for Search::ridx and cidx
};
__device__ __forceinline__ Sides assign_sides(const int32_t *first, int n_first,
                                              const int32_t *second, int n_second)
{
    Sides r;
    r.first = n_first <= n_second;
    r.n = r.first ? n_first : n_second;
    r.m = r.first ? n_second : n_first;
    r.rows = r.first ? first : second;
    r.cols = r.first ? second : first;
    return r;
}

// Rows 1 .. n, columns 1 .. m, n <= m; p[j - 1] = the row of column j, 0: free;
// way[j - 1] = the column before j on the path, 0: the root (the new row).
// weight(ridx[i], cidx[j]) >= 0 is the weight of the pair (row i, column j).
// Returns false if a bound ran out (then p is not an assignment).
template <class Weight>
__device__ __forceinline__ bool assign_solve(const Weight &weight, const Search &s, int n, int m)
{
    const int lane = lane_id();
    for (int j = lane; j < m; j += WAVE) {
        s.v[j] = 0;
        s.p[j] = 0;
    }
    for (int i = lane; i < n; i += WAVE) s.u[i] = 0;
    __syncthreads();
    for (int i = 1; i <= n; i++) {
        for (int j = lane; j < m; j += WAVE) {
            s.minv[j] = ASSIGN_INF;
            s.used[j] = 0;
            s.way[j] = 0;
        }
        __syncthreads();
        int j0 = 0, i0 = i;
        bool found = false;
        for (int step = 0; step <= m; step++) {
            const long long ui = s.u[i0 - 1];
            const int64_t r = s.ridx[i0 - 1];
            long long best = ASSIGN_INF;
            int bj = 0x7fffffff;
            for (int j = lane; j < m; j += WAVE) {
                if (s.used[j]) continue;
                const int64_t c = s.cidx[j];
                const long long cur = -weight(r, c) - ui - s.v[j];
                long long mv = s.minv[j];
                if (cur < mv) {
                    mv = cur;
                    s.minv[j] = cur;
                    s.way[j] = j0;
                }
                if (mv < best) {             // (ascending j: the lowest among equal values)
                    best = mv;
                    bj = j;
                }
            }
#pragma unroll
            for (int o = WAVE / 2; o > 0; o >>= 1) {
                const long long ob = __shfl_xor(best, o);
                const int oj = __shfl_xor(bj, o);
                if (ob < best || (ob == best && oj < bj)) {
                    best = ob;
                    bj = oj;
                }
            }
            if (bj == 0x7fffffff) return false;     // no free column: n <= m rules it out
            for (int j = lane; j < m; j += WAVE) {
                if (s.used[j]) {
                    s.u[s.p[j] - 1] += best;         // (distinct columns hold distinct rows)
                    s.v[j] -= best;
                } else {
                    s.minv[j] -= best;
                }
            }
            if (lane == 0) s.u[i - 1] += best;       // the root's row
            if ((bj & (WAVE - 1)) == lane) s.used[bj] = 1;
            __syncthreads();
            j0 = bj + 1;
            i0 = s.p[bj];
            if (i0 == 0) {
                found = true;
                break;
            }
        }
        if (!found) return false;
        // the path back to the root; every lane walks it and stores the same words
        for (int step = 0; step <= m && j0; step++) {
            const int j1 = s.way[j0 - 1];
            s.p[j0 - 1] = j1 ? s.p[j1 - 1] : i;
            j0 = j1;
        }
        if (j0) return false;
        __syncthreads();
    }
    return true;
}

// The assigned pairs of a solved search, a lane a column: take(has, a, b) with
// the pair's entry of the first and of the second side.  Every lane of the
// wavefront calls take in every pass (has = false: no pair), so take may hold
// wavefront operations.
template <class Take>
__device__ __forceinline__ void assign_pairs(const Search &s, const Sides &sd, Take take)
{
    for (int jb = 0; jb < sd.m; jb += WAVE) {
        const int j = jb + lane_id();
        const int i = j < sd.m ? s.p[j] : 0;
        int64_t r = 0, c = 0;
        if (i > 0) {
            r = s.ridx[i - 1];
            c = s.cidx[j];
        }
        take(i > 0, sd.first ? r : c, sd.first ? c : r);
    }
}

}  // namespace taoamd

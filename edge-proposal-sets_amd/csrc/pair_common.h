// Helpers shared by the pair-scoring kernels (generic and column-run), gfx950.
#pragma once
#include "eps_common.h"

// Number of elements of the ascending array a[0..n) that are < t.  Same trip count in every
// lane (n is wave-uniform), no divergent branches.
template <typename P>
__device__ __forceinline__ int lower_bound_uniform(P a, int n, int t)
{
    int pos = 0;
    for (int step = 1 << (31 - __builtin_clz(n)); step > 0; step >>= 1) {
        int np = pos + step;
        int idx = (np < n ? np : n) - 1;
        int x = a[idx];
        if (np <= n && x < t) pos = np;
    }
    return pos;
}

// One common neighbour t of (u, v), stored at es in the shorter row and at el in the longer (swapped: the shorter row is v's):
// its A[u,t] * A[v,t] and its weighted product, added to the lane's sums.
template <bool HAS_VAL, bool HAS_W, typename WT>
__device__ __forceinline__ void pair_products(const float *__restrict__ val, const WT *__restrict__ node_w, int64_t es, int64_t el,
                                              bool swapped, int t, float &acc_cn, WT &acc_ws)
{
    if (!HAS_VAL && !HAS_W) return;
    float vs = 1.0f, vl = 1.0f;
    if (HAS_VAL) { vs = val[es]; vl = val[el]; }
    const float va = swapped ? vl : vs, vbv = swapped ? vs : vl;  // va = A[u,w], vbv = A[v,w]
    if (HAS_VAL) acc_cn += va * vbv;
    if (HAS_W) acc_ws += (WT)va * ((WT)vbv * node_w[t]);  // A_ entry rounded first (adamic_utils.py:17)
}

// Buffer resource over one adjacency row (eps_raw_rsrc: entries past the row's end read as 0)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const int32_t *row, int32_t len) { return eps_raw_rsrc(row, len * 4); }

// Sum over the (few) lanes whose flag is set, in ascending lane order: deterministic, and cheaper than a
// 6-step butterfly when 1-3 lanes hold a contribution (mean CN of a candidate pair is ~1.3).
__device__ __forceinline__ int lane_get(int x, int l) { return __builtin_amdgcn_readlane(x, l); }
__device__ __forceinline__ float lane_get(float x, int l)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l));
}
__device__ __forceinline__ double lane_get(double x, int l)
{
    return __builtin_bit_cast(double, eps_bcast64(__builtin_bit_cast(int64_t, x), l));
}
template <typename T>
__device__ __forceinline__ T sparse_lane_sum(uint64_t mask, T x)
{
    T tot = 0;
    while (mask) {
        const int l = __builtin_ctzll(mask);
        mask &= mask - 1;
        tot += lane_get(x, l);
    }
    return tot;
}

// Lower bound over a sorted LDS array of 2^lg entries (padded with INT_MAX): fully unrolled, branch-free steps,
// trip count selected by a wave-uniform switch.  Returns pos in [0, 2^lg - 1]; the caller tests L[pos] == t.
__device__ __forceinline__ int lb_pow2(const int32_t *L, int lg, int t)
{
    int pos = 0;
    switch (lg) {
    case 10: pos += (L[pos + 511] < t) ? 512 : 0; [[fallthrough]];
    case 9: pos += (L[pos + 255] < t) ? 256 : 0; [[fallthrough]];
    case 8: pos += (L[pos + 127] < t) ? 128 : 0; [[fallthrough]];
    case 7: pos += (L[pos + 63] < t) ? 64 : 0; [[fallthrough]];
    case 6: pos += (L[pos + 31] < t) ? 32 : 0; [[fallthrough]];
    case 5: pos += (L[pos + 15] < t) ? 16 : 0; [[fallthrough]];
    case 4: pos += (L[pos + 7] < t) ? 8 : 0; [[fallthrough]];
    case 3: pos += (L[pos + 3] < t) ? 4 : 0; [[fallthrough]];
    case 2: pos += (L[pos + 1] < t) ? 2 : 0; [[fallthrough]];
    case 1: pos += (L[pos] < t) ? 1 : 0; [[fallthrough]];
    default: break;
    }
    return pos;
}

// INT_MAX in the elements of a staged 16-byte group that lie past the end of the row (n entries)
__device__ __forceinline__ v4i pad_tail(v4i x, int idx, int n)
{
    const int big = 0x7fffffff;
    x.x = idx + 0 < n ? x.x : big;
    x.y = idx + 1 < n ? x.y : big;
    x.z = idx + 2 < n ? x.z : big;
    x.w = idx + 3 < n ? x.w : big;
    return x;
}

// Two idioms of the model kernels (Katz pairs and columns, PPR push, local-community degrees), gfx950.  Only these pieces are
// shared: what a kernel does per item, and what it keeps in its table, is its own loop.
//
//   * ROWS LAID END TO END over a wave's lanes, 64 rows per wave step: eps_wave_excl_scan (eps_common.h) over the rows' lengths,
//     the exclusive prefix parked in the wave's LDS between two lds_wave_sync, then every lane takes item t = t0 + lane of the
//     step's total and finds the row it belongs to with flat_owner -- so short rows leave no lane idle.
//   * A NODE TABLE: open addressing keyed by node id (empty = -1), 2^lg slots, in LDS or in a workgroup's region of a workspace.
//     atomicCAS decides the slot a key lands in, so that depends on the order; nothing read from the table does.
#pragma once
#include "eps_common.h"

struct EpsCsr {
    const int64_t *__restrict__ rp;
    const int32_t *__restrict__ col;
    const float *__restrict__ val;
};

// The row that item t of a wave step belongs to: the last k of 0..63 with excl[k] <= t.  excl holds 64 ascending entries (the
// exclusive prefix of the rows' lengths, so excl[0] == 0) and 0 <= t.  Of equal prefixes the last wins, so empty rows are
// skipped: for t below the step's total the owner has at least one entry, and t - excl[k] is the item's place in its row.
template <typename T>
__device__ __forceinline__ int flat_owner(const T *excl, T t)
{
    int k = 0;
#pragma unroll
    for (int step = 32; step > 0; step >>= 1)
        if (excl[k + step] <= t) k += step;
    return k;
}

// The last column of [lo, hi] whose segment starts at or before slot p (colptr ascends; colptr[lo] <= p).
__device__ __forceinline__ int64_t column_of(const int64_t *__restrict__ colptr, int64_t lo, int64_t hi, int64_t p)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (colptr[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- the node table ------------------------------------------------------------------------------------------------------
// A global table is written with atomics (they execute in L2) and read back by other waves of the workgroup: every access
// goes to L2 (agent scope), never through a vector-L1 line that an earlier use of the region left behind.
template <bool IN_LDS, typename T>
__device__ __forceinline__ T tbl_ld(const T *p)
{
    if (IN_LDS) return *p;
    return __hip_atomic_load((T *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool IN_LDS, typename T>
__device__ __forceinline__ void tbl_st(T *p, T x)
{
    if (IN_LDS) *p = x;
    else __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t tbl_hash(int32_t w, int lg) { return ((uint32_t)w * 2654435761u) >> (32 - lg); }
// 2^lg - 1 (lg <= 31), spelled so that the compiler sees its top bit clear: a slot is never negative as an int, and a caller's
// `slot < 0` is a test of the miss paths alone.
__device__ __forceinline__ uint32_t tbl_mask(int lg) { return 0x7fffffffu >> (31 - lg); }

// The slot of key w (inserted if new: *won), or -1 when every slot holds another key.
__device__ __forceinline__ int tbl_insert(int32_t *keys, int lg, int32_t w, bool *won)
{
    const uint32_t mask = tbl_mask(lg);
    uint32_t h = tbl_hash(w, lg);
    for (uint32_t t = 0; t <= mask; ++t) {
        const int32_t prev = atomicCAS(&keys[h], -1, w);
        if (prev == -1 || prev == w) {
            *won = prev == -1;
            return (int)h;
        }
        h = (h + 1) & mask;
    }
    *won = false;
    return -1;
}

// The slot of key w, or -1 when it is not in the table.
template <bool IN_LDS>
__device__ __forceinline__ int tbl_find_slot(const int32_t *keys, int lg, int32_t w)
{
    const uint32_t mask = tbl_mask(lg);
    uint32_t h = tbl_hash(w, lg);
    for (uint32_t t = 0; t <= mask; ++t) {
        const int32_t k = tbl_ld<IN_LDS>(keys + h);
        if (k == w) return (int)h;
        if (k < 0) return -1;
        h = (h + 1) & mask;
    }
    return -1;
}

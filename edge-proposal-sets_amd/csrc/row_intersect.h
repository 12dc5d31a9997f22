// N(a) & N(b) of two ascending CSR rows by one wave, gfx950: the walk shared by the pair-score, common-neighbour-list and cosine
// backward kernels (and, its staging half, by the local-community degrees).  What a kernel does per match is its visitor.
//
//   * The LONGER row is staged in the wave's LDS slice, ROW_CAP entries per pass, and the SHORTER row is spread one element per
//     lane; every lane runs lb_pow2 -- unrolled, branch-free -- over the staged entries.  A pass's 16-byte raw buffer loads are ALL
//     issued before its first LDS write, so their latencies overlap instead of chaining; dwords past the row's end read 0 and are
//     replaced by INT_MAX up to the next power of two (no bounds branch).  The short row's first 64-entry slice is loaded between
//     the issue and the commit: the pair then costs one memory round trip, not two (most short rows ARE one slice).
//   * A long row takes several passes.  Both rows ascend, so the passes co-iterate with the short row like a merge: a pass settles
//     the short elements <= its own last entry -- a prefix of what is left -- and a cursor marks the first one not yet settled;
//     everything stops when the short row is used up.  Matches therefore arrive in the short row's order, pass after pass.
//   * Very lopsided pairs (long > ROW_CAP and long >= ROW_INPLACE_RATIO * short) skip the staging: lower_bound_uniform in the long
//     row where it lies (L2-resident), log2(long) probes per short element instead of a full read of a degree-100k hub.
// Ids and bounds are the caller's business: the walk reads col[sbase .. sbase + slen) and col[lbase .. lbase + llen), nothing else.
#pragma once
#include "pair_common.h"

#define ROW_CAP 1024          // long-row entries staged per wave and pass (4 KiB of LDS per wave): lb_pow2's largest table (lg = 10)
#define ROW_INPLACE_RATIO 32  // long row searched in place when long > ROW_CAP && long >= ratio * short

// The wave's next ticket off one device word (lane 0 draws, every lane gets it).
__device__ __forceinline__ int64_t take_chunk(unsigned int *next_chunk, int lane)
{
    unsigned int t = 0;
    if (lane == 0) t = atomicAdd(next_chunk, 1u);
    return (int64_t)(unsigned int)__builtin_amdgcn_readfirstlane((int)t);
}

// Stage row[0 .. n), n <= ROW_CAP, as P = 2^lg >= n ascending LDS entries: one, two or four 16-byte loads per lane ...
struct StagedRow { v4i x0, x1, x2, x3; };
__device__ __forceinline__ StagedRow stage_issue(const int32_t *row, int n, int lg, int lane)
{
    const __amdgpu_buffer_rsrc_t lrs = row_rsrc(row, n);
    const int P = 1 << lg;
    StagedRow r;
    r.x0 = __builtin_amdgcn_raw_buffer_load_b128(lrs, lane * 16, 0, 0);
    if (P > 256) r.x1 = __builtin_amdgcn_raw_buffer_load_b128(lrs, lane * 16 + 1024, 0, 0);
    if (P > 512) {
        r.x2 = __builtin_amdgcn_raw_buffer_load_b128(lrs, lane * 16 + 2048, 0, 0);
        r.x3 = __builtin_amdgcn_raw_buffer_load_b128(lrs, lane * 16 + 3072, 0, 0);
    }
    return r;
}
// ... then, once whoever read the slice's previous contents is done (the leading barrier), the stores.
__device__ __forceinline__ void stage_commit(int32_t *L, const StagedRow &r, int n, int lg, int lane)
{
    const int P = 1 << lg;
    __builtin_amdgcn_wave_barrier();
    *reinterpret_cast<v4i *>(&L[4 * lane]) = pad_tail(r.x0, 4 * lane, n);
    if (P > 256) *reinterpret_cast<v4i *>(&L[256 + 4 * lane]) = pad_tail(r.x1, 256 + 4 * lane, n);
    if (P > 512) {
        *reinterpret_cast<v4i *>(&L[512 + 4 * lane]) = pad_tail(r.x2, 512 + 4 * lane, n);
        *reinterpret_cast<v4i *>(&L[768 + 4 * lane]) = pad_tail(r.x3, 768 + 4 * lane, n);
    }
    lds_wave_sync();
}
__device__ __forceinline__ int stage_lg(int n) { return n > 1 ? 32 - __builtin_clz(n - 1) : 0; }

// hit(found, t, si, li, staged), called by the whole wave once per 64-entry slice of the short row: t = the lane's short-row id
// (0 past the row's end), si its index in the short row, li the match's index in the long row (meaningful where found).
template <typename Hit>
__device__ __forceinline__ void intersect_rows_inplace(const int32_t *__restrict__ col, int64_t sbase, int32_t slen, int64_t lbase,
                                                       int32_t llen, int lane, Hit &&hit)
{
    const int32_t *__restrict__ lcol = col + lbase;
    for (int s0 = 0; s0 < slen; s0 += 64) {
        const int si = s0 + lane;
        const bool act = si < slen;
        const int t = act ? col[sbase + si] : 0;
        const int pos = lower_bound_uniform(lcol, llen, t);
        const int pc = pos < llen ? pos : llen - 1;
        hit(act && pos < llen && lcol[pc] == t, t, si, pc, false);
    }
}

// Returns whether the pair was staged in L (CAP entries of LDS, this wave's) -- false: searched in place.  slen <= llen, both > 0.
template <int CAP, int RATIO, typename Hit>
__device__ __forceinline__ bool intersect_rows(const int32_t *__restrict__ col, int64_t sbase, int32_t slen, int64_t lbase,
                                               int32_t llen, int32_t *L, int lane, Hit &&hit)
{
    static_assert(CAP == ROW_CAP, "stage_issue / lb_pow2 cover 2^10 entries per pass");
    if (llen > CAP && (int64_t)llen >= (int64_t)slen * RATIO) {
        intersect_rows_inplace(col, sbase, slen, lbase, llen, lane, hit);
        return false;
    }
    int s_cursor = 0;
    const __amdgpu_buffer_rsrc_t srs = row_rsrc(col + sbase, slen);
    for (int l0 = 0; l0 < llen && s_cursor < slen; l0 += CAP) {
        const int n = (llen - l0) < CAP ? (llen - l0) : CAP;
        const int lg = stage_lg(n);
        const StagedRow regs = stage_issue(col + lbase + l0, n, lg, lane);
        const int t_first = __builtin_amdgcn_raw_buffer_load_b32(srs, (s_cursor + lane) * 4, 0, 0);
        const int s_first = s_cursor;
        stage_commit(L, regs, n, lg, lane);
        const int last = llen > CAP ? __builtin_amdgcn_readfirstlane(L[n - 1]) : 0x7fffffff;
        for (int s0 = s_cursor; s0 < slen; s0 += 64) {
            const int si = s0 + lane;
            const int t = s0 == s_first ? t_first : __builtin_amdgcn_raw_buffer_load_b32(srs, si * 4, 0, 0);
            const bool mine = si < slen && t <= last;        // a prefix of the lanes (sorted row)
            const int n_mine = __popcll(__ballot(mine));
            s_cursor = s0 + n_mine;
            const int pos = lb_pow2(L, lg, t);
            hit(mine && L[pos] == t, t, si, l0 + pos, true);
            if (n_mine < 64) s0 = slen;                      // the rest of the short row belongs to later passes
        }
    }
    return true;
}

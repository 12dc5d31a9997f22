// Local-community indices (Cannistraci, Alanis-Lobato, Ravasi: "From link-prediction in brain connectomes and protein interactomes
// to the local-community-paradigm in complex networks", Sci. Rep. 3:1613), gfx950.
//
// For a pair (u, v) with L = the ascending list of its common STORED neighbours (csrc/pair_cn_list.hip), c = |L|, a and b the
// stored entries of rows u and v, d_w those of row w:
//   gamma(w) = |{z in L : z != w, z stored in row w}|      the local-community degree of w (a self loop never counts)
//   G = sum of gamma over L (an integer; twice the links among the common neighbours on a symmetric pattern),  LCL = G / 2
//   car c LCL    cpa ((a - c) + CAR)((b - c) + CAR)    caa sum gamma(w) / log2 d_w    cra sum gamma(w) / d_w    cjc CAR / (a + b - c)
// A term with gamma(w) == 0 is skipped (so d_w = 1 never divides by log2 1), cjc over 0 is 0.  float64 arithmetic on the
// integers, ONE rounding to float32 -- lc_score, shared by every path.
//
// eps_local_community_degrees: the hot kernel, a SECOND intersection pass -- the sorted row N(w) against the sorted list that
//   holds w -- for every listed w.  Chunks of up to 64 segments go to waves by ticket (pair_cn_list.hip's hand-out; a launch
//   of few segments uses smaller chunks, so that its longer lists spread over the device); a wave then runs
//   * SHORT lists (up to LC_SHORT entries: what a filter's candidates have) all together: the ordered (i, j) pairs of all the
//     chunk's short lists are dealt over the lanes, a lane answers "is z_j stored in row w_i" by a lower bound in the row, and
//     gamma_i is a segmented count (ballot, popcount of the lanes of one (list, i), one LDS add per group and step);
//   * longer lists one after the other: the list staged in the wave's LDS slice by row_intersect.h's stage_issue / stage_commit
//     (ROW_CAP entries per pass; a longer list in passes, the partial counts added in gamma itself by the lane that owns the entry),
//     the rows of 64 list members STREAMED one element per lane against it -- the rows laid end to end, so short rows do not
//     idle the wave -- matches by ballot and popcount, the self match dropped;
//   * IN PLACE: a member whose row is ROW_INPLACE_RATIO times the staged entries (a hub between two low-degree nodes) is not
//     streamed; the staged entries are searched in its row, 64 per step.
//   Plain vector stores only; the one global atomic is the ticket.  Integer counts: no float atomics, nothing depends on order.
// eps_local_community_scores: per pair, G (int64) and the float64 sum of the index's terms in a FIXED association of the list
//   positions -- blocks of 64 consecutive entries, a balanced pairwise tree inside a block (x[i] + x[i ^ 1], then ^ 2, ...;
//   positions past the end count 0.0, which adds exactly), the blocks added first to last -- so a score depends on the list
//   alone, not on launch shape, place in the batch, route or orientation.  Lists up to LC_SHORT entries are summed by one lane
//   each (the same tree, written out), longer ones by the whole wave; chunks by ticket, so one 40,000-entry list occupies one
//   wave while the others go on.
#include "flat_rows.h"
#include "row_intersect.h"

#include <math.h>

#define LC_WAVES 4            // waves per workgroup
#define LC_SHORT 8            // lists up to this many entries: ordered pairs dealt over the lanes / one lane per list in the scores
#define LC_INDICES 5

enum { LC_CAR = 0, LC_CPA, LC_CAA, LC_CRA, LC_CJC };

__device__ __forceinline__ float lc_score(int index, int64_t c, int64_t a, int64_t b, int64_t big_gamma, double term_sum)
{
    const double C = (double)c, A = (double)a, B = (double)b;
    const double car = C * ((double)big_gamma * 0.5);
    switch (index) {
    case LC_CAR: return (float)car;
    case LC_CPA: return (float)(((A - C) + car) * ((B - C) + car));
    case LC_CAA:
    case LC_CRA: return (float)term_sum;
    default: {                            // LC_CJC
        const double den = A + B - C;
        return den == 0.0 ? 0.0f : (float)(car / den);
    }
    }
}

// One entry's term of the caa / cra sums (0.0 for the indices that need G alone).
__device__ __forceinline__ double lc_term(int index, int32_t g, int64_t d)
{
    if (g == 0) return 0.0;
    if (index == LC_CAA) return (double)g / log2((double)d);
    if (index == LC_CRA) return (double)g / (double)d;
    return 0.0;
}

__device__ __forceinline__ uint64_t lc_lanes(int lo, int hi) { return (~0ull >> (63 - hi)) & (~0ull << lo); }   // 0 <= lo <= hi <= 63

__device__ __forceinline__ int64_t lc_shfl64(int64_t x, int l)
{
    const int lo = __shfl((int)(x & 0xffffffffll), l), hi = __shfl((int)(x >> 32), l);
    return ((int64_t)hi << 32) | (uint32_t)lo;
}

// Segment p of ptr clamped into [0, total]; `bad` when it had to be.
__device__ __forceinline__ void lc_segment(const int64_t *__restrict__ ptr, int64_t p, int64_t total, int64_t &sb, int64_t &se, bool &bad)
{
    sb = ptr[p];
    se = ptr[p + 1];
    bad = false;
    if (se > total) { se = total; bad = true; }
    if (se < 0) { se = 0; bad = true; }
    if (sb < 0 || sb > se) { sb = se; bad = true; }
    if (se - sb > 0x7fffffffll) { sb = se; bad = true; }
}

__global__ __launch_bounds__(LC_WAVES * 64) void local_community_degrees_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t n_rows, const int64_t *__restrict__ ptr,
    const int32_t *__restrict__ w, int64_t n_pairs, int group, unsigned int *__restrict__ next_chunk, int32_t *__restrict__ gamma,
    int32_t *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) int32_t s_list[LC_WAVES][ROW_CAP];
    __shared__ int32_t s_off[LC_WAVES][64];
    __shared__ int32_t s_acc[LC_WAVES][64];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int32_t *L = s_list[wib];
    int32_t *E = s_off[wib];
    int32_t *ACC = s_acc[wib];
    const int64_t n_chunks = (n_pairs + group - 1) / group;  // `group` segments per chunk (1 .. 64): lanes past it hold none
    const int64_t total = ptr[n_pairs];                      // nothing of w or gamma is touched at or past it, whatever ptr holds

    auto do_chunk = [&](const int64_t chunk) {
        const int64_t p = chunk * group + lane;
        const bool valid = lane < group && p < n_pairs;
        int64_t sb = 0, se = 0;
        bool bad = false;
        if (valid) lc_segment(ptr, p, total, sb, se, bad);
        const int c = (int)(se - sb);

        // ---- the short lists of the chunk, all together -----------------------------------------------------------------
        const bool is_short = c >= 1 && c <= LC_SHORT;
        bool ok = is_short;
        if (is_short) {
            int prev = -1;                                   // strictly ascending from >= 0, below n_rows
            for (int k = 0; k < c; ++k) {
                const int x = w[sb + k];
                ok = ok && x > prev && (int64_t)x < n_rows;
                prev = x;
            }
            if (!ok) bad = true;
        }
        int n_items = 0;
        const int off = eps_wave_excl_scan(ok ? c * (c - 1) : 0, lane, n_items);
        E[lane] = off;
#pragma unroll
        for (int k = 0; k < LC_SHORT; ++k) L[k * 64 + lane] = 0;  // counts of (list s, entry i) at L[s * LC_SHORT + i]
        lds_wave_sync();
        for (int t0 = 0; t0 < n_items; t0 += 64) {
            const int t = t0 + lane;
            const bool act = t < n_items;
            const int s = act ? flat_owner(E, t) : 0;
            const int cs = __shfl(c, s);
            const int64_t bs = lc_shfl64(sb, s);
            const int cm1 = act ? cs - 1 : 1;                // (an owner has c >= 2)
            const int r = act ? t - E[s] : 0;
            const int i = r / cm1, jj = r - i * cm1;
            const int j = jj + (jj >= i ? 1 : 0);            // the other entries of the list, in order
            bool found = false;
            if (act) {
                const int wi = w[bs + i], z = w[bs + j];
                const int64_t rb = rowptr[wi];
                const int d = (int)(rowptr[wi + 1] - rb);
                const int pos = eps_lower_bound(col + rb, 0, d, z);
                found = pos < d && col[rb + pos] == z;
            }
            const uint64_t m = __ballot(found);
            if (act) {                                       // the lanes of (s, i) in this step; the first of them adds their matches
                const int lo = lane - jj > 0 ? lane - jj : 0;
                const int hi = lane - jj + cm1 - 1 < 63 ? lane - jj + cm1 - 1 : 63;
                if (lane == lo) {
                    const int cnt = __popcll(m & lc_lanes(lo, hi));
                    if (cnt) L[s * LC_SHORT + i] += cnt;
                }
            }
            lds_wave_sync();                                   // (a group that straddles two steps is added to by two lanes in turn)
        }
#pragma unroll
        for (int k = 0; k < LC_SHORT; ++k) {
            const int slot = k * 64 + lane;
            const int s = slot / LC_SHORT, i = slot % LC_SHORT;
            const int cs = __shfl(is_short ? c : 0, s);
            const int64_t bs = lc_shfl64(sb, s);
            if (i < cs) gamma[bs + i] = L[slot];             // (a refused list: zeros)
        }
        lds_wave_sync();

        // ---- the longer lists, one after the other ----------------------------------------------------------------------
        for (int j = 0; j < group; ++j) {
            const int cj = __builtin_amdgcn_readlane(c, j);
            if (cj <= LC_SHORT) continue;                    // wave-uniform
            const int64_t bj = eps_bcast64(sb, j);
            const int32_t *__restrict__ seg = w + bj;
            int32_t *__restrict__ gseg = gamma + bj;
            bool seg_bad = false;
            for (int k0 = 0; k0 < cj; k0 += 64) {
                const int k = k0 + lane;
                const bool a = k < cj;
                const int x = a ? seg[k] : 0;
                const int nx = (a && k + 1 < cj) ? seg[k + 1] : 0x7fffffff;
                if (__ballot(a && (x < 0 || (int64_t)x >= n_rows || nx <= x)) != 0ull) {
                    seg_bad = true;
                    break;
                }
            }
            if (seg_bad) {                                   // refused: zeros, no row is read
                for (int k = lane; k < cj; k += 64) gseg[k] = 0;
                if (lane == j) bad = true;
                continue;
            }
            for (int l0 = 0; l0 < cj; l0 += ROW_CAP) {
                const int n = (cj - l0) < ROW_CAP ? (cj - l0) : ROW_CAP;
                const int lg = stage_lg(n);
                stage_commit(L, stage_issue(seg + l0, n, lg, lane), n, lg, lane);
                for (int i0 = 0; i0 < cj; i0 += 64) {        // 64 members of the list, lane m <-> entry i0 + m in every pass
                    const int i = i0 + lane;
                    const bool am = i < cj;
                    const int wi = am ? seg[i] : 0;
                    const int64_t rb = am ? rowptr[wi] : 0;
                    const int d = am ? (int)(rowptr[wi + 1] - rb) : 0;
                    const bool inplace = am && d >= 64 && (int64_t)d >= (int64_t)n * ROW_INPLACE_RATIO;
                    const int fd = inplace ? 0 : d;          // streamed rows, laid end to end (each below 32 * ROW_CAP entries)
                    int n_flat = 0;
                    E[lane] = eps_wave_excl_scan(fd, lane, n_flat);
                    ACC[lane] = 0;
                    lds_wave_sync();
                    for (int t0 = 0; t0 < n_flat; t0 += 64) {
                        const int t = t0 + lane;
                        const bool act = t < n_flat;
                        const int m = act ? flat_owner(E, t) : 0;
                        const int em = E[m];
                        const int dm = __shfl(fd, m);
                        const int wm = __shfl(wi, m);
                        const int64_t rbm = lc_shfl64(rb, m);
                        const int x = act ? col[rbm + (t - em)] : -1;
                        const bool found = act && x != wm && L[lb_pow2(L, lg, x)] == x;   // (the self match dropped)
                        const uint64_t mask = __ballot(found);
                        if (act) {
                            const int lo = em - t0 > 0 ? em - t0 : 0;
                            const int hi = em + dm - 1 - t0 < 63 ? em + dm - 1 - t0 : 63;
                            if (lane == lo) {
                                const int cnt = __popcll(mask & lc_lanes(lo, hi));
                                if (cnt) ACC[m] += cnt;
                            }
                        }
                        lds_wave_sync();
                    }
                    int mine = 0;
                    uint64_t todo = __ballot(inplace);
                    while (todo) {                           // wave-uniform: the staged entries searched in the long row
                        const int m = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
                        todo &= todo - 1;
                        const int dm = __builtin_amdgcn_readlane(d, m);
                        const int wm = __builtin_amdgcn_readlane(wi, m);
                        const int32_t *__restrict__ row = col + eps_bcast64(rb, m);
                        int cnt = 0;
                        for (int k0 = 0; k0 < n; k0 += 64) {
                            const int k = k0 + lane;
                            const bool a = k < n;
                            const int z = a ? L[k] : 0;
                            const int pos = lower_bound_uniform(row, dm, z);
                            const int pc = pos < dm ? pos : dm - 1;
                            cnt += __popcll(__ballot(a && z != wm && pos < dm && row[pc] == z));
                        }
                        if (lane == m) mine = cnt;
                    }
                    if (am) {
                        const int got = ACC[lane] + mine;
                        if (l0 == 0) gseg[i] = got;
                        else gseg[i] += got;                 // (a later pass: the same lane wrote the earlier passes' count)
                    }
                    lds_wave_sync();                           // (the next 64 members overwrite E and ACC)
                }
                __builtin_amdgcn_wave_barrier();             // (the next pass overwrites the staged entries)
            }
        }
        if (valid && bad) *status = 1;
    };
    int64_t chunk = take_chunk(next_chunk, lane);
    while (chunk < n_chunks) {
        const int64_t next = take_chunk(next_chunk, lane);
        do_chunk(chunk);
        chunk = next;
    }
}

// ---- scores --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LC_WAVES * 64) void local_community_scores_kernel(
    const int64_t *__restrict__ rowptr, int64_t n_rows, const int32_t *__restrict__ pu, const int32_t *__restrict__ pv,
    const int64_t *__restrict__ ptr, const int32_t *__restrict__ w, const int32_t *__restrict__ gamma, int64_t n_pairs, int index,
    unsigned int *__restrict__ next_chunk, float *__restrict__ score)
{
    const int lane = threadIdx.x & 63;
    const int64_t n_chunks = (n_pairs + 63) >> 6;
    const int64_t total = ptr[n_pairs];
    const bool listed = w != nullptr;                        // else: closed forms, c from ptr alone
    const bool sums = index == LC_CAA || index == LC_CRA;

    // one entry of a list -> its gamma, and its term of the index's sum (an id outside the graph: nothing is read, term 0)
    auto entry = [&](const int64_t at, int32_t &g) -> double {
        g = gamma[at];
        if (!sums || g == 0) return 0.0;
        const int x = w[at];
        if (x < 0 || (int64_t)x >= n_rows) return 0.0;
        return lc_term(index, g, rowptr[x + 1] - rowptr[x]);
    };
    auto do_chunk = [&](const int64_t chunk) {
        const int64_t p = chunk * 64 + lane;
        const bool valid = p < n_pairs;
        const int32_t nu = valid ? pu[p] : -1, nv = valid ? pv[p] : -1;
        const bool ok = nu >= 0 && nv >= 0 && (int64_t)nu < n_rows && (int64_t)nv < n_rows;
        const int64_t a = ok ? rowptr[nu + 1] - rowptr[nu] : 0, b = ok ? rowptr[nv + 1] - rowptr[nv] : 0;
        int64_t sb = 0, se = 0;
        bool bad = false;
        if (valid) lc_segment(ptr, p, listed ? total : 0x7fffffffffffffffll, sb, se, bad);
        const int64_t c = se - sb;
        int64_t G = 0;
        double S = 0.0;
        const int wide = (listed && c > LC_SHORT) ? (int)c : 0;
        if (listed && c >= 2 && c <= LC_SHORT) {             // one lane: the pairwise tree over 8 places, written out
            double t[LC_SHORT];
#pragma unroll
            for (int k = 0; k < LC_SHORT; ++k) {
                int32_t g = 0;
                t[k] = k < c ? entry(sb + k, g) : 0.0;
                G += g;
            }
            S = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
        }
        for (int j = 0; j < 64; ++j) {                       // the whole wave: blocks of 64 entries, first to last
            const int cj = __builtin_amdgcn_readlane(wide, j);
            if (cj == 0) continue;
            const int64_t bj = eps_bcast64(sb, j);
            int64_t gj = 0;
            double sj = 0.0;
            for (int k0 = 0; k0 < cj; k0 += 64) {
                const int k = k0 + lane;
                int32_t g = 0;
                double x = k < cj ? entry(bj + k, g) : 0.0;
                long long gs = g;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    x += __shfl_xor(x, o);
                    gs += __shfl_xor(gs, o);
                }
                sj += x;
                gj += gs;
            }
            if (lane == j) { G = gj; S = sj; }
        }
        if (valid) score[p] = ok ? lc_score(index, c, a, b, G, S) : __builtin_nanf("");
    };
    int64_t chunk = take_chunk(next_chunk, lane);
    while (chunk < n_chunks) {
        const int64_t next = take_chunk(next_chunk, lane);
        do_chunk(chunk);
        chunk = next;
    }
}

static int64_t lc_blocks(int64_t n_pairs)
{
    const int64_t n_chunks = (n_pairs + 63) / 64;
    int64_t blocks = (n_chunks + LC_WAVES - 1) / LC_WAVES;
    const int64_t max_blocks = (int64_t)eps_num_cus() * 8;  // 32 waves per CU
    return blocks > max_blocks ? max_blocks : blocks;
}

extern "C" int eps_local_community_limits(int32_t *short_max, int32_t *cap, int32_t *inplace_ratio)
{
    if (short_max) *short_max = LC_SHORT;
    if (cap) *cap = ROW_CAP;
    if (inplace_ratio) *inplace_ratio = ROW_INPLACE_RATIO;
    return EPS_OK;
}

extern "C" int eps_local_community_degrees(const int64_t *rowptr, const int32_t *col, int64_t n_rows, const int64_t *ptr,
                                           const int32_t *w, int64_t n_pairs, int32_t *gamma, int32_t *status, void *stream)
{
    EPS_REQUIRE(n_pairs >= 0 && n_rows >= 0 && n_rows < (1ll << 31), "eps_local_community_degrees: bad size (n_rows=%lld n_pairs=%lld)",
                (long long)n_rows, (long long)n_pairs);
    EPS_REQUIRE(status, "eps_local_community_degrees: null status");
    if (hipMemsetAsync(status, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) {
        eps_set_error("eps_local_community_degrees: cannot clear the status word");
        return EPS_ELAUNCH;
    }
    if (n_pairs == 0) return EPS_OK;
    EPS_REQUIRE(ptr && w && gamma && (n_rows == 0 || (rowptr && col)), "eps_local_community_degrees: null pointer");
    // A wave works through the longer lists of its chunk one after the other: a launch of few segments hands them out in
    // smaller groups, so that they spread over the device (the counts do not depend on the grouping).
    int group = 64;
    while (group > 1 && n_pairs / group < (int64_t)eps_num_cus() * 32) group >>= 1;
    const int64_t n_chunks = (n_pairs + group - 1) / group;
    int64_t blocks = (n_chunks + LC_WAVES - 1) / LC_WAVES;
    if (blocks > (int64_t)eps_num_cus() * 8) blocks = (int64_t)eps_num_cus() * 8;
    unsigned int *counter = nullptr;
    const int crc = eps_take_counter(&counter, (hipStream_t)stream, "eps_local_community_degrees");
    if (crc) return crc;
    hipLaunchKernelGGL(local_community_degrees_kernel, dim3((unsigned)blocks), dim3(LC_WAVES * 64), 0, (hipStream_t)stream,
                       rowptr, col, n_rows, ptr, w, n_pairs, group, counter, gamma, status);
    EPS_CHECK_LAUNCH("eps_local_community_degrees");
    return EPS_OK;
}

extern "C" int eps_local_community_scores(const int64_t *rowptr, int64_t n_rows, const int32_t *u, const int32_t *v, const int64_t *ptr,
                                          const int32_t *w, const int32_t *gamma, int64_t n_pairs, int32_t index, float *score,
                                          void *stream)
{
    EPS_REQUIRE(index >= 0 && index < LC_INDICES, "eps_local_community_scores: index=%d must lie in [0, %d)", (int)index, LC_INDICES);
    EPS_REQUIRE(n_pairs >= 0 && n_rows >= 0 && n_rows < (1ll << 31), "eps_local_community_scores: bad size (n_rows=%lld n_pairs=%lld)",
                (long long)n_rows, (long long)n_pairs);
    EPS_REQUIRE((w != nullptr) == (gamma != nullptr), "eps_local_community_scores: w and gamma come together (both null: closed forms)");
    if (n_pairs == 0) return EPS_OK;
    EPS_REQUIRE(rowptr && u && v && ptr && score, "eps_local_community_scores: null pointer");
    unsigned int *counter = nullptr;
    const int crc = eps_take_counter(&counter, (hipStream_t)stream, "eps_local_community_scores");
    if (crc) return crc;
    hipLaunchKernelGGL(local_community_scores_kernel, dim3((unsigned)lc_blocks(n_pairs)), dim3(LC_WAVES * 64), 0, (hipStream_t)stream,
                       rowptr, n_rows, u, v, ptr, w, gamma, n_pairs, (int)index, counter, score);
    EPS_CHECK_LAUNCH("eps_local_community_scores");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void local_community_warm_kernel() {}
extern "C" void eps_warm_local_community(void *stream) { hipLaunchKernelGGL(local_community_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

// Truncated Katz scores at pairs, gfx950: out[p] = c1*A[u,v] + c2*(A^2)[u,v] + c3*(A^3)[u,v] for any square CSR A
// (weighted or unit-valued, symmetric or not), without forming A^2 or A^3.
//
// Replaces the collab branch of train_and_eval.py:272-343 (test_katz): `H = beta*A; H += beta*(A @ H)` twice, i.e.
// H = beta*A + 2*beta^2*A^2 + beta^3*A^3 materialised by SciPy, then read at the evaluation pairs.
//
// Per pair the three-hop walk starts from whichever end is cheaper:
//   * forward (from u): the map M[x] = A[x,v] is row v of A^T.  A[u,v] = M[u]; (A^2)[u,v] = sum_{w in row u} A[u,w] M[w];
//     (A^3)[u,v] = sum_{w in row u} A[u,w] sum_{x in row w} A[w,x] M[x].  Work: the two-paths out of u, paths_out[u].
//   * backward (from v): the same walk over A^T from v with the map built from row u of A; work paths_in[v].
//   The side with the smaller (two-paths + map row) is taken; ties go forward.
// The map is row b of the map matrix, sorted by column (CSR rows are), staged in LDS when it has at most KZ_MAP_CAP entries
// and searched in place in global memory otherwise: a lookup is a binary search with a wave-uniform trip count.
// The two-paths of the walk are flattened over the 64 lanes: for each 64-entry slice of row a, the lanes scan the degrees
// of their w, and every lane then takes one two-path (w, x) per step, so low-degree w leave no lane idle.
//
// Work split: 64-pair chunks are handed to waves dynamically; a wave scores its chunk's pairs one after the other.  A pair
// whose walk exceeds KZ_BIG two-paths is not scored there: it is appended to a list, and a second launch splits its walk
// into up to KZ_NSEG segments of the flat two-path range, one wave each (a collab-like graph has walks of ~50 for random
// negatives and up to ~19 k for hub positives; one wave per such pair would hold the launch).  A third launch adds the
// segments of every listed pair in segment order.
//
// Arithmetic: each lane accumulates its terms in float64, the wave reduces with a fixed butterfly, segments are added in
// a fixed order, and the result is rounded to float32 once.  Which pairs are split, and how, depends on the graph and the
// pair alone, so two launches give bitwise equal outputs (the list's order differs between launches, nothing read from it does).
#include "flat_rows.h"
#include "row_intersect.h"      // (take_chunk; pair_common.h)
#include <math.h>

#define KZ_WAVES 4
#define KZ_MAP_CAP 1024      // map entries staged per wave (8 KiB of LDS: keys + values)
#define KZ_BIG 2048          // walks longer than this (two-paths) are split over several waves
#define KZ_SEG 1024          // target two-paths per segment of a split walk
#define KZ_NSEG 16           // at most this many segments per pair

struct KzLds {
    int32_t key[KZ_WAVES][KZ_MAP_CAP];
    float val[KZ_WAVES][KZ_MAP_CAP];
    int64_t excl[KZ_WAVES][64];    // exclusive prefix of the degrees of the slice's w
    int64_t start[KZ_WAVES][64];   // row start of each w
    float aw[KZ_WAVES][64];        // A[a,w]
};

// Side and walk length of pair (u, v): fwd = walk A from u, else walk A^T from v.
__device__ __forceinline__ void kz_plan(const int64_t *__restrict__ rp, const int64_t *__restrict__ rp_t,
                                        const int64_t *__restrict__ paths_out, const int64_t *__restrict__ paths_in,
                                        int32_t u, int32_t v, bool &fwd, int64_t &walk)
{
    const int64_t cf = paths_out[u] + (rp_t[v + 1] - rp_t[v]);
    const int64_t cb = paths_in[v] + (rp[u + 1] - rp[u]);
    fwd = cf <= cb;
    walk = fwd ? paths_out[u] : paths_in[v];
}

__device__ __forceinline__ int kz_segments(int64_t walk)
{
    const int64_t s = (walk + KZ_SEG - 1) / KZ_SEG;
    return s > KZ_NSEG ? KZ_NSEG : (int)s;
}

// M[x] for a wave-uniform sorted key array of md > 0 entries (LDS or global); 0 when x is not stored.
__device__ __forceinline__ double kz_lookup(const int32_t *keys, const float *vals, int32_t md, int32_t x, bool act)
{
    const int pos = lower_bound_uniform(keys, md, x);
    const int pc = pos < md ? pos : md - 1;
    const bool hit = act && pos < md && keys[pc] == x;
    return hit ? (vals ? (double)vals[pc] : 1.0) : 0.0;
}

// The part of pair (a, b)'s score held by the two-paths [t_lo, t_hi) of the walk over W from a; the map is row b of M
// (M = W^T).  `first` adds the c1 and c2 terms (they belong to the first segment only).  Returns the wave's total in every lane.
__device__ double kz_walk(const EpsCsr W, const EpsCsr M, int32_t a, int32_t b, int64_t t_lo, int64_t t_hi, bool first,
                          double c1, double c2, double c3, KzLds &S, int wib, int lane)
{
    const int64_t mb = M.rp[b];
    const int32_t md = (int32_t)(M.rp[b + 1] - mb);
    const int64_t ab = W.rp[a];
    const int32_t ad = (int32_t)(W.rp[a + 1] - ab);
    if (md == 0 || ad == 0) return 0.0;    // nothing reaches b, or nothing leaves a (and A[a,b] needs both)
    const int32_t *keys = M.col + mb;
    const float *vals = M.val ? M.val + mb : nullptr;
    if (md <= KZ_MAP_CAP) {
        lds_wave_sync();                   // (the previous pair's lookups are done before the map is overwritten)
        for (int i = lane; i < md; i += 64) {
            S.key[wib][i] = keys[i];
            if (vals) S.val[wib][i] = vals[i];
        }
        lds_wave_sync();
        keys = S.key[wib];
        vals = vals ? S.val[wib] : nullptr;
    }
    double acc = 0.0;
    double s1 = 0.0;
    if (first) s1 = kz_lookup(keys, vals, md, a, true);
    int64_t base = 0;                       // flat index of the slice's first two-path
    for (int c0 = 0; c0 < ad && (first || base < t_hi); c0 += 64) {
        const int j = c0 + lane;
        const bool act = j < ad;
        const int32_t w = act ? W.col[ab + j] : 0;
        const float aw = act ? (W.val ? W.val[ab + j] : 1.0f) : 0.0f;
        const int64_t ws = W.rp[w];
        const int64_t wd = act ? W.rp[w + 1] - ws : 0;
        if (first) {
            const double m = kz_lookup(keys, vals, md, w, act);
            acc += c2 * ((double)aw * m);
        }
        int64_t tot;
        const int64_t wex = eps_wave_excl_scan(wd, lane, tot);
        const int64_t lo = t_lo > base ? t_lo - base : 0;
        const int64_t hi = t_hi - base < tot ? t_hi - base : tot;
        if (lo < hi) {
            lds_wave_sync();
            S.excl[wib][lane] = wex;
            S.start[wib][lane] = ws;
            S.aw[wib][lane] = aw;
            lds_wave_sync();
            const int64_t *ex = S.excl[wib];
            for (int64_t t0 = lo; t0 < hi; t0 += 64) {
                const int64_t t = t0 + lane;
                const bool on = t < hi;
                const int k = flat_owner(ex, t);        // t's w (it has degree > 0)
                int32_t x = 0;
                double wx = 0.0;
                if (on) {
                    const int64_t e = S.start[wib][k] + (t - ex[k]);
                    x = W.col[e];
                    wx = (double)S.aw[wib][k] * (double)(W.val ? W.val[e] : 1.0f);
                }
                const double m = kz_lookup(keys, vals, md, x, on);
                acc += c3 * (wx * m);
            }
        }
        base += tot;
    }
    return c1 * s1 + eps_wave_sum(acc);
}

__device__ __forceinline__ int32_t kz_readlane(int32_t x, int l) { return __builtin_amdgcn_readlane(x, l); }

// One wave per pair, 64-pair chunks handed out dynamically; pairs with long walks are listed for katz_split_kernel.
__global__ __launch_bounds__(KZ_WAVES * 64) void katz_pairs_kernel(
    const EpsCsr A, const EpsCsr AT, const int64_t *__restrict__ paths_out, const int64_t *__restrict__ paths_in,
    const int32_t *__restrict__ pu, const int32_t *__restrict__ pv, int64_t n_pairs, double c1, double c2, double c3,
    unsigned int *__restrict__ next_chunk, unsigned int *__restrict__ n_big, int32_t *__restrict__ big_list,
    float *__restrict__ out)
{
    __shared__ KzLds S;
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n_chunks = (n_pairs + 63) >> 6;
    for (;;) {
        const int64_t chunk = take_chunk(next_chunk, lane);
        if (chunk >= n_chunks) break;
        const int64_t p = chunk * 64 + lane;
        const bool valid = p < n_pairs;
        const int32_t u = valid ? pu[p] : 0, v = valid ? pv[p] : 0;
        bool fwd = true;
        int64_t walk = 0;
        if (valid) kz_plan(A.rp, AT.rp, paths_out, paths_in, u, v, fwd, walk);
        const bool big = valid && walk > KZ_BIG;
        if (big) big_list[atomicAdd(n_big, 1u)] = (int32_t)p;
        const uint64_t todo = __ballot(valid && !big);
        const uint64_t fwd_mask = __ballot(fwd);
        float res = 0.0f;
        uint64_t m = todo;
        while (m) {
            const int k = __builtin_ctzll(m);
            m &= m - 1;
            const int32_t uk = kz_readlane(u, k), vk = kz_readlane(v, k);
            const bool fk = (fwd_mask >> k) & 1;
            const double tot = kz_walk(fk ? A : AT, fk ? AT : A, fk ? uk : vk, fk ? vk : uk, 0, INT64_MAX, true, c1, c2, c3, S,
                                       wib, lane);
            if (lane == k) res = (float)tot;
        }
        if (valid && !big) out[p] = res;
    }
}

// One wave per (listed pair, segment): item i is segment i % KZ_NSEG of big_list[i / KZ_NSEG].  Segments past the pair's
// count write 0.
__global__ __launch_bounds__(KZ_WAVES * 64) void katz_split_kernel(
    const EpsCsr A, const EpsCsr AT, const int64_t *__restrict__ paths_out, const int64_t *__restrict__ paths_in,
    const int32_t *__restrict__ pu, const int32_t *__restrict__ pv, double c1, double c2, double c3,
    const unsigned int *__restrict__ n_big, const int32_t *__restrict__ big_list, double *__restrict__ part)
{
    __shared__ KzLds S;
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n_items = (int64_t)*n_big * KZ_NSEG;
    const int64_t n_waves = (int64_t)gridDim.x * KZ_WAVES;
    for (int64_t it = (int64_t)blockIdx.x * KZ_WAVES + wib; it < n_items; it += n_waves) {
        const int64_t p = big_list[it / KZ_NSEG];
        const int s = (int)(it % KZ_NSEG);
        const int32_t u = pu[p], v = pv[p];
        bool fwd;
        int64_t walk;
        kz_plan(A.rp, AT.rp, paths_out, paths_in, u, v, fwd, walk);
        const int nseg = kz_segments(walk);
        double tot = 0.0;
        if (s < nseg) {
            const int64_t len = (walk + nseg - 1) / nseg;
            const int64_t lo = s * len, hi = lo + len < walk ? lo + len : walk;
            tot = kz_walk(fwd ? A : AT, fwd ? AT : A, fwd ? u : v, fwd ? v : u, lo, hi, s == 0, c1, c2, c3, S, wib, lane);
        }
        if (lane == 0) part[it] = tot;
    }
}

__global__ void katz_combine_kernel(const unsigned int *__restrict__ n_big, const int32_t *__restrict__ big_list,
                                    const double *__restrict__ part, float *__restrict__ out)
{
    const int64_t nb = *n_big;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nb; j += (int64_t)gridDim.x * blockDim.x) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < KZ_NSEG; ++k) s += part[j * KZ_NSEG + k];
        out[big_list[j]] = (float)s;
    }
}

// paths[x] = sum_{w in row x} (rowptr[w+1] - rowptr[w]), one thread per node.
__global__ void two_path_counts_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t n,
                                       int64_t *__restrict__ paths)
{
    for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (int64_t)gridDim.x * blockDim.x) {
        int64_t s = 0;
        for (int64_t e = rowptr[x], end = rowptr[x + 1]; e < end; ++e) {
            const int32_t w = col[e];
            s += rowptr[w + 1] - rowptr[w];
        }
        paths[x] = s;
    }
}

static inline int64_t kz_list_bytes(int64_t n_pairs) { return (n_pairs * 4 + 255) / 256 * 256; }

extern "C" int64_t eps_katz_workspace_bytes(int64_t n_pairs)
{
    if (n_pairs < 0) return 0;
    return kz_list_bytes(n_pairs) + n_pairs * KZ_NSEG * (int64_t)sizeof(double);
}

extern "C" int eps_two_path_counts(const int64_t *rowptr, const int32_t *col, int64_t n_nodes, int64_t *paths, void *stream)
{
    EPS_REQUIRE(n_nodes >= 0, "eps_two_path_counts: negative size");
    EPS_REQUIRE(n_nodes == 0 || (rowptr && col && paths), "eps_two_path_counts: null pointer");
    if (n_nodes == 0) return EPS_OK;
    int64_t blocks = (n_nodes + 255) / 256;
    const int64_t max_blocks = (int64_t)eps_num_cus() * 16;
    if (blocks > max_blocks) blocks = max_blocks;
    hipLaunchKernelGGL(two_path_counts_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, col, n_nodes,
                       paths);
    EPS_CHECK_LAUNCH("eps_two_path_counts");
    return EPS_OK;
}

extern "C" int eps_katz_pair_scores(const int64_t *rowptr, const int32_t *col, const float *val, const int64_t *rowptr_t,
                                    const int32_t *col_t, const float *val_t, const int64_t *paths_out,
                                    const int64_t *paths_in, int64_t n_nodes, const int32_t *u, const int32_t *v,
                                    int64_t n_pairs, double c1, double c2, double c3, void *workspace, float *out,
                                    void *stream)
{
    EPS_REQUIRE(n_pairs >= 0 && n_nodes >= 0, "eps_katz_pair_scores: negative size");
    EPS_REQUIRE(isfinite(c1) && isfinite(c2) && isfinite(c3), "eps_katz_pair_scores: non-finite coefficient");
    EPS_REQUIRE(n_pairs == 0 || (rowptr && col && rowptr_t && col_t && paths_out && paths_in && u && v && workspace && out),
                "eps_katz_pair_scores: null pointer");
    EPS_REQUIRE(n_pairs == 0 || n_nodes > 0, "eps_katz_pair_scores: pairs on an empty graph");
    if (n_pairs == 0) return EPS_OK;
    hipStream_t s = (hipStream_t)stream;
    unsigned int *next_chunk = nullptr, *n_big = nullptr;
    int crc = eps_take_counter(&next_chunk, s, "eps_katz_pair_scores");
    if (crc) return crc;
    crc = eps_take_counter(&n_big, s, "eps_katz_pair_scores");
    if (crc) return crc;
    int32_t *big_list = (int32_t *)workspace;
    double *part = (double *)((char *)workspace + kz_list_bytes(n_pairs));
    const EpsCsr A{rowptr, col, val}, AT{rowptr_t, col_t, val_t};
    const int64_t n_chunks = (n_pairs + 63) / 64;
    int64_t blocks = (n_chunks + KZ_WAVES - 1) / KZ_WAVES;
    const int64_t max_blocks = (int64_t)eps_num_cus() * 4;
    if (blocks > max_blocks) blocks = max_blocks;
    hipLaunchKernelGGL(katz_pairs_kernel, dim3((unsigned)blocks), dim3(KZ_WAVES * 64), 0, s, A, AT, paths_out, paths_in, u, v,
                       n_pairs, c1, c2, c3, next_chunk, n_big, big_list, out);
    hipLaunchKernelGGL(katz_split_kernel, dim3((unsigned)max_blocks), dim3(KZ_WAVES * 64), 0, s, A, AT, paths_out, paths_in, u,
                       v, c1, c2, c3, (const unsigned int *)n_big, (const int32_t *)big_list, part);
    hipLaunchKernelGGL(katz_combine_kernel, dim3(64), dim3(256), 0, s, (const unsigned int *)n_big, (const int32_t *)big_list,
                       (const double *)part, out);
    EPS_CHECK_LAUNCH("eps_katz_pair_scores");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void katz_pairs_warm_kernel() {}
extern "C" void eps_warm_katz_pairs(void *stream) { hipLaunchKernelGGL(katz_pairs_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

// The K rows of a filter step from ONE score sort of its re-scored pairs, gfx950 (filter.py:160-161 for the rows rank.py:294 reads).
//
// The declared order is score descending, then (v, u) ascending, and both orientations of a pair carry the pair's score: the (v, u)
// order only matters between rows of EQUAL score.  So the re-scored list (eps_rescore_runs: one entry per unordered pair) is sorted by
// score alone -- half the records of the mirrored list, 32 key bits instead of 40 + 32 (eps_select_topk_rows: nine radix passes over
// 2 m rows) -- and the rows are put in order inside each run of equal scores:
//   1. rocprim::radix_sort_pairs_desc, score -> pair key (library sort; the key halves are exchanged on the way in);
//   2. rbs_cut_kernel: a sorted list holds its own cut -- the k2-th best live score is entry k2 - 1, the counts are positions.  Same
//      definition, same bits as eps_score_hist + eps_score_pick_compact with above = base = bar (score_buckets.h);
//   3. rbs_expand_kernel: independent workgroups over windows of RBS_T sorted pairs write every run's 2 g directed rows at rows
//      [2 s, 2 e) of the proposal tensor, each row at its rank among the run's rows (counted in LDS).  A run longer than RBS_L pairs
//      is not attempted: *flag is set and the caller orders the selection with eps_select_topk_rows_pairs instead.
// No host read, no cooperative launch: n_sel stays on the device.
#include "eps_common.h"
#include "score_buckets.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#define RBS_T 1024              // threads per workgroup = sorted pairs per window of the expansion
#define RBS_L 1024              // longest run of equal scores ordered in the kernel (a window's run reaches at most RBS_L - 1 pairs
                                // beyond the window: window + reach, packed ids and scores, are 24 KB of LDS)

struct rbs_swap_halves {        // u << 32 | v -> v << 32 | u: the form eps_select_topk_rows takes its pairs in
    __host__ __device__ int64_t operator()(int64_t k) const { return (int64_t)(((uint64_t)k << 32) | ((uint64_t)k >> 32)); }
};
using rbs_keys_in = rocprim::transform_iterator<const int64_t *, rbs_swap_halves, int64_t>;

// Entries in front of the first one that fails `pred` in s[0, n), pred holding on a prefix.  Whole workgroup: RBS_T probes a round
// (a one-thread bisection is ~21 dependent loads from memory a search; this is three rounds for 2 M entries).
template <class Pred>
__device__ int64_t rbs_prefix_len(const float *__restrict__ s, int64_t n, Pred pred)
{
    int64_t lo = 0, hi = n;                                   // the answer lies in [lo, hi]
    while (lo < hi) {
        const int64_t step = (hi - lo + RBS_T - 1) / RBS_T, idx = lo + (int64_t)threadIdx.x * step;
        const int c = __syncthreads_count(idx < hi && pred(s[idx]));
        if (c == 0) {
            hi = lo;
        } else {
            const int64_t last = lo + (int64_t)(c - 1) * step;                // (the probes that hold are a prefix of the probes)
            lo = last + 1;
            hi = last + step < hi ? last + step : hi;
        }
    }
    return lo;
}

// s: scores sorted descending.  Live: > *bar and > -inf.  Fewer than k2 live entries (or k2 == 0): *cut = -inf, *n_sel = the live
// count; else *cut = the lower edge of the bucket (of distances to *bar) that holds the k2-th best score, *n_sel = live entries >= it.
__global__ __launch_bounds__(RBS_T) void rbs_cut_kernel(const float *__restrict__ s, int64_t n, const float *__restrict__ bar, uint64_t k2,
                                                        float *__restrict__ cut_out, int64_t *__restrict__ n_sel_out,
                                                        int64_t *__restrict__ flag)
{
    const float floor_v = *bar;
    const int64_t n_live = rbs_prefix_len(s, n, [=](float x) { return x > floor_v && x > -__builtin_inff(); });
    float cut = -__builtin_inff();
    int64_t n_sel = n_live;
    if (k2 != 0 && (uint64_t)n_live >= k2) {
        const uint32_t ob = eps_ordered_bits(floor_v), o = eps_ordered_bits(s[k2 - 1]);
        const uint32_t b = ts_bucket(o > ob ? o - ob : 0u);
        if (b != 0u) {                                        // (bucket 0 also holds what lies below the base: its lower edge is "anything")
            const uint64_t e = (uint64_t)ob + ts_bucket_floor(b);
            cut = eps_unordered_bits(e > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)e);
            n_sel = rbs_prefix_len(s, n_live, [=](float x) { return x >= cut; });
        }
    }
    if (threadIdx.x == 0) {
        *cut_out = cut;
        *n_sel_out = n_sel;
        *flag = 0;
    }
}

// The window [w0, w0 + RBS_T) of the first *n_sel sorted pairs (sk: v << 32 | u in the scanned graph's labels, sv: scores).  A run
// of equal scores belongs to the window it starts in; its pairs beyond the window are fetched too (up to RBS_L of them are probed).
// Ids go through perm first, the smaller mapped id is u of the first orientation (as sel_mirror_kernel).  Row (u, v) of a run sits
// at the run's first row + its rank by (v, u) among the run's 2 g rows; ids are compared as whole 32-bit words.
__global__ __launch_bounds__(RBS_T) void rbs_expand_kernel(const int64_t *__restrict__ sk, const float *__restrict__ sv,
                                                           const int64_t *__restrict__ n_sel_p, const int64_t *__restrict__ perm, int64_t k,
                                                           int64_t *__restrict__ out_pairs, int64_t ld, float *__restrict__ out_vals,
                                                           int64_t *__restrict__ flag)
{
    __shared__ uint64_t lk[RBS_T + RBS_L];                   // smaller id << 32 | larger id, caller's labels
    __shared__ float ls[RBS_T + RBS_L];
    const int64_t n_sel = *n_sel_p;
    const int64_t w0 = (int64_t)blockIdx.x * RBS_T;
    if (w0 >= n_sel) return;
    const int tid = threadIdx.x;
    const int64_t w1 = w0 + RBS_T < n_sel ? w0 + RBS_T : n_sel;
    auto fetch = [&](int64_t j, int slot, float x) {
        const uint64_t key = (uint64_t)sk[j];
        uint64_t a = key & 0xFFFFFFFFull, b = key >> 32;
        if (perm) {
            a = (uint64_t)perm[a];
            b = (uint64_t)perm[b];
        }
        lk[slot] = a < b ? (a << 32) | b : (b << 32) | a;
        ls[slot] = x;
    };
    if (w0 + tid < w1) fetch(w0 + tid, tid, sv[w0 + tid]);
    // how far the window's last run reaches beyond the window: the entries there that equal the window's last score are a prefix
    bool reach = false;
    if (w1 == w0 + RBS_T && w1 + tid < n_sel) {
        const float x = sv[w1 + tid];
        reach = x == sv[w1 - 1];
        if (reach) fetch(w1 + tid, RBS_T + tid, x);
    }
    const int n_reach = __syncthreads_count(reach), lim = (int)(w1 - w0) + n_reach;
    // the two rows of the pair in slot p, each at its rank among the rows of the pair's run
    auto place = [&](int p) {
        const float mine = ls[p];
        int s = p;
        while (s > 0 && ls[s - 1] == mine) --s;
        if (s == 0 && w0 > 0 && sv[w0 - 1] == mine) return;  // the run started in an earlier window
        int e = p + 1;
        while (e < lim && ls[e] == mine) ++e;
        if (e - s > RBS_L) {
            *flag = 1;
            return;
        }
        const uint64_t kb = lk[p], ka = (kb << 32) | (kb >> 32);     // row (u = smaller, v = larger) sorts by ka; its mirror by kb
        int ra = 0, rb = 0;
        for (int q = s; q < e; ++q) {
            const uint64_t cb = lk[q], ca = (cb << 32) | (cb >> 32);
            ra += (int)(ca < ka) + (int)(cb < ka);
            rb += (int)(ca < kb) + (int)(cb < kb);
        }
        const int64_t row0 = 2 * (w0 + s), row_a = row0 + ra, row_b = row0 + rb;
        if (row_a < k) {
            out_pairs[row_a] = (int64_t)(kb >> 32);
            out_pairs[ld + row_a] = (int64_t)(kb & 0xFFFFFFFFull);
            out_vals[row_a] = mine;
        }
        if (row_b < k) {
            out_pairs[row_b] = (int64_t)(kb & 0xFFFFFFFFull);
            out_pairs[ld + row_b] = (int64_t)(kb >> 32);
            out_vals[row_b] = mine;
        }
    };
    if (w0 + tid < w1) place(tid);
    if (tid < n_reach) place(RBS_T + tid);                   // (the pairs of the last run that lie beyond the window: no other window takes them)
}

static size_t rbs_sort_temp_bytes(int64_t n)
{
    size_t b = 0;
    (void)rocprim::radix_sort_pairs_desc((void *)nullptr, b, (const float *)nullptr, (float *)nullptr, rbs_keys_in(nullptr, rbs_swap_halves()),
                                         (int64_t *)nullptr, (size_t)n, 0u, 32u, (hipStream_t)0);
    return b;
}

extern "C" int32_t eps_rows_by_score_max_run(void) { return RBS_L; }
extern "C" int32_t eps_rows_by_score_window(void) { return RBS_T; }

extern "C" int64_t eps_rows_by_score_workspace_bytes(int64_t n)
{
    if (n <= 0) return 256;
    return (int64_t)((rbs_sort_temp_bytes(n) + 255) & ~(size_t)255);
}

extern "C" int eps_rows_by_score(const int64_t *keys_by_u, const float *vals, int64_t n, const float *bar, int64_t k2, int64_t k,
                                 int32_t id_bits, const int64_t *perm_or_null, int64_t *sorted_keys, float *sorted_vals, float *cut,
                                 int64_t *n_sel, int64_t *flag, int64_t *out_pairs, int64_t pairs_ld, float *out_vals, void *workspace,
                                 int64_t workspace_bytes, void *stream)
{
    EPS_REQUIRE(n >= 0 && n < (1ll << 31) && k2 >= 0 && k >= 0 && id_bits >= 1 && id_bits <= 32, "eps_rows_by_score: bad argument");
    EPS_REQUIRE(bar && cut && n_sel && flag, "eps_rows_by_score: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n != 0) {
        EPS_REQUIRE(keys_by_u && vals && sorted_keys && sorted_vals, "eps_rows_by_score: null pointer");
        EPS_REQUIRE(k == 0 || (out_pairs && out_vals && pairs_ld >= (k < 2 * n ? k : 2 * n)), "eps_rows_by_score: out_pairs / pairs_ld too small");
        EPS_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= eps_rows_by_score_workspace_bytes(n),
                    "eps_rows_by_score: needs a 256-byte aligned workspace of eps_rows_by_score_workspace_bytes(n) bytes");
        size_t temp_bytes = (size_t)workspace_bytes;
        if (rocprim::radix_sort_pairs_desc(workspace, temp_bytes, vals, sorted_vals, rbs_keys_in(keys_by_u, rbs_swap_halves()), sorted_keys,
                                           (size_t)n, 0u, 32u, s) != hipSuccess) {
            eps_set_error("eps_rows_by_score: radix sort failed");
            return EPS_ELAUNCH;
        }
    }
    hipLaunchKernelGGL(rbs_cut_kernel, dim3(1), dim3(RBS_T), 0, s, sorted_vals, n, bar, (uint64_t)k2, cut, n_sel, flag);
    if (n != 0 && k != 0)
        hipLaunchKernelGGL(rbs_expand_kernel, dim3((unsigned)((n + RBS_T - 1) / RBS_T)), dim3(RBS_T), 0, s, sorted_keys, sorted_vals, n_sel,
                           perm_or_null, k, out_pairs, pairs_ld, out_vals, flag);
    EPS_CHECK_LAUNCH("eps_rows_by_score");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void rows_by_score_warm_kernel() {}
extern "C" void eps_warm_rows_by_score(void *stream) { hipLaunchKernelGGL(rows_by_score_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

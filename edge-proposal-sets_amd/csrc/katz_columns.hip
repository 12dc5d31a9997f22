// Truncated Katz scores of the candidates of a block of columns, gfx950: for every candidate (u, v) of the column-major list
//   out[p] = c1*A[u,v] + c2*(A^2)[u,v] + c3*(A^3)[u,v]
// for any square CSR A (weighted or unit-valued, symmetric or not) -- the score katz_pairs.hip computes, for the access
// pattern of a FILTER: every candidate of column v shares the two-hop vector y2 = (A^2)[:, v], so it is built once per
// column and candidate u costs one pass over row u, (A^3)[u,v] = sum_{w in row u} A[u,w] * y2[w]: deg(u) table lookups
// instead of the paths_out[u] two-path steps of the pair kernel.
//
// Work units are slices of `chunk` candidates (KC_CHUNK .. KC_CHUNK_BIG by the list's length unless the caller says otherwise)
// of the candidate array, handed to
// workgroups dynamically; a unit walks the columns
// its slice meets, so a column with more candidates than one slice is scored by several units (each builds the column's table
// again) and many light columns share one unit.  Per (column, part of its candidates):
//   1. y2's support is inserted into an open-addressing table keyed by node id (atomicCAS: the slot a key lands in depends on
//      the order, nothing read from the table does).  The support is walked over A^T from v: x in row v of A^T, w in row x
//      of A^T, the two-paths flattened over the lanes (flat_rows.h).  Its size is at most ub = min(paths_in[v], n): the
//      table gets >= 2 ub slots (a power of two), in LDS when ub <= KC_LDS_CAP (KC_LDS_SLOTS slots, load <= 0.5625), else in
//      this workgroup's region of the caller's workspace.
//   2. one owner thread per slot sums y2[w] = sum_x A[w,x] * A[x,v] in ascending x: row w of A against the sorted row v of
//      A^T (staged in LDS up to KC_ROW_CAP entries), iterating the shorter and searching the longer.  A unit-valued graph
//      skips this pass: step 1 counts the two-paths per key with integer atomics, which are exact in any order.
//   3. candidates, 64 per wave step: c1*y1[u] + c2*y2[u] come from one search of row v and one table lookup; the row sum is
//      taken by a team whose size depends on deg(u) alone -- one lane (deg <= 8), 8 lanes (deg <= 128) or the wave -- each lane
//      adding its entries j = l, l + T, ... in order, the team reducing with a fixed butterfly.
// Arithmetic: float64 throughout, rounded to float32 once.  A score therefore depends on the graph, the coefficients and the
// pair alone -- not on the block, the slice, the launch or the workgroup: bitwise reproducible, and equal under any split.
#include "flat_rows.h"
#include "pair_common.h"
#include <math.h>

#define KC_THREADS 512
#define KC_WAVES (KC_THREADS / 64)
#define KC_LDS_LG 13
#define KC_LDS_SLOTS (1 << KC_LDS_LG)   // 96 KiB of LDS: 8-byte values + 4-byte keys
#define KC_LDS_CAP 4608                 // largest support bound whose table stays in LDS
#define KC_ROW_CAP 2048                 // entries of row v of A^T staged in LDS (16 KiB)
#define KC_CHUNK 2048                   // candidates per work unit: the smallest default ...
#define KC_CHUNK_BIG 8192               // ... and the largest: doubled while the list still gives KC_UNITS_MIN units
#define KC_UNITS_MIN 1024               //     (four per CU; fewer rebuilds of split columns' tables -- measured)
#define KC_CHUNK_MAX (1 << 20)          // a caller may ask for any size up to this
#define KC_MAX_GROUPS 256               // workgroups per launch (one per CU: the table takes most of a CU's LDS)
#define KC_WS_BUDGET ((int64_t)2 << 30) // global tables: fewer workgroups rather than more than this much workspace
#define KC_T1_DEG 8                     // rows up to this length: one lane
#define KC_T8_DEG 128                   // ... up to this length: 8 lanes; longer: the wave

struct KcLds {
    unsigned long long val[KC_LDS_SLOTS];   // y2 as float64 bits (a unit-valued graph: the two-path count until step 2)
    int32_t key[KC_LDS_SLOTS];
    int32_t rkey[KC_ROW_CAP];
    float rval[KC_ROW_CAP];
    int64_t excl[KC_WAVES][64];     // insert: exclusive prefix of the in-degrees of the slice's x
    int64_t start[KC_WAVES][64];    // ... and their row starts
    int64_t crs[KC_WAVES][64];      // scoring: row start, degree and c1/c2 part of the slice's candidates
    double cbase[KC_WAVES][64];
    int32_t cdeg[KC_WAVES][64];
    int32_t list[KC_WAVES][64];     // lanes of the slice's 8-lane-team candidates
    unsigned int unit;
    int fail;
};

// y2[w]; 0 when w is not in the table.
template <bool IN_LDS>
__device__ __forceinline__ double kc_find(const int32_t *keys, const unsigned long long *vals, int lg, int32_t w)
{
    const int slot = tbl_find_slot<IN_LDS>(keys, lg, w);
    return slot < 0 ? 0.0 : __builtin_bit_cast(double, tbl_ld<IN_LDS>(vals + slot));
}

// sum over the common keys x of two sorted rows of a[x] * b[x], in ascending x; the shorter row is walked, the longer searched.
__device__ double kc_sorted_dot(const int32_t *ak, const float *av, int na, const int32_t *bk, const float *bv, int nb)
{
    if (na > nb) {
        const int32_t *tk = ak; ak = bk; bk = tk;
        const float *tv = av; av = bv; bv = tv;
        const int tn = na; na = nb; nb = tn;
    }
    double s = 0.0;
    int lo = 0;
    for (int i = 0; i < na && lo < nb; ++i) {
        const int32_t x = ak[i];
        int hi = nb;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (bk[mid] < x) lo = mid + 1; else hi = mid;
        }
        if (lo < nb && bk[lo] == x) s += (double)(av ? av[i] : 1.0f) * (double)(bv ? bv[lo] : 1.0f);
    }
    return s;
}

__device__ __forceinline__ int kc_table_lg(int64_t ub)
{
    int lg = 6;
    while (((int64_t)1 << lg) < 2 * ub) ++lg;
    return lg;
}

// Candidates [p0, p1) of column v (all of them in that column).  Every thread of the workgroup calls this with the same
// arguments; the table is free again when it returns.
template <bool IN_LDS, bool UNIT>
__device__ __forceinline__ void kc_column(const EpsCsr A, const EpsCsr AT, int64_t n, int32_t v, int64_t p0, int64_t p1,
                                          const int32_t *__restrict__ cand_u, double c1, double c2, double c3, KcLds &S,
                                          int32_t *keys, unsigned long long *vals, int lg, float *__restrict__ out)
{
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t mb = AT.rp[v];
    const int32_t md = (int32_t)(AT.rp[v + 1] - mb);
    const float qnan = __builtin_nanf("");
    if (md == 0) {                            // nothing reaches v: every walk count is 0
        for (int64_t p = p0 + tid; p < p1; p += KC_THREADS) {
            const int32_t u = cand_u[p];
            out[p] = (u >= 0 && u < n) ? 0.0f : qnan;
        }
        return;
    }
    const int slots = 1 << lg;
    for (int i = tid; i < slots; i += KC_THREADS) {
        tbl_st<IN_LDS>(keys + i, (int32_t)-1);
        tbl_st<IN_LDS>(vals + i, 0ull);
    }
    const bool staged = md <= KC_ROW_CAP;
    if (staged)
        for (int i = tid; i < md; i += KC_THREADS) {
            S.rkey[i] = AT.col[mb + i];
            if (AT.val) S.rval[i] = AT.val[mb + i];
        }
    if (tid == 0) S.fail = 0;
    __syncthreads();
    const int32_t *rk = staged ? (const int32_t *)S.rkey : AT.col + mb;
    const float *rv = AT.val ? (staged ? (const float *)S.rval : AT.val + mb) : nullptr;

    // 1. the support of y2: w with a two-path w -> x -> v
    for (int c0 = wib * 64; c0 < md; c0 += KC_WAVES * 64) {
        const int j = c0 + lane;
        const bool act = j < md;
        const int32_t x = act ? AT.col[mb + j] : 0;
        const int64_t xs = AT.rp[x];
        const int64_t xd = act ? AT.rp[x + 1] - xs : 0;
        int64_t tot;
        const int64_t xex = eps_wave_excl_scan(xd, lane, tot);
        lds_wave_sync();
        S.excl[wib][lane] = xex;
        S.start[wib][lane] = xs;
        lds_wave_sync();
        const int64_t *ex = S.excl[wib];
        for (int64_t t0 = 0; t0 < tot; t0 += 64) {
            const int64_t t = t0 + lane;
            if (t < tot) {
                const int k = flat_owner(ex, t);           // t's x (it has degree > 0)
                const int32_t w = AT.col[S.start[wib][k] + (t - ex[k])];
                bool won;                      // (not needed: a key's value starts at 0 whoever inserts it)
                const int slot = tbl_insert(keys, lg, w, &won);        // -1: never while the support bound holds
                if (slot < 0) S.fail = 1;
                else if (UNIT) atomicAdd(vals + slot, 1ull);
            }
        }
    }
    __syncthreads();
    if (S.fail) {                              // (a support bound that did not hold: the caller's paths_in is not A^T's)
        for (int64_t p = p0 + tid; p < p1; p += KC_THREADS) out[p] = qnan;
        __syncthreads();
        return;
    }

    // 2. y2 of every key, by the thread that owns its slot
    for (int i = tid; i < slots; i += KC_THREADS) {
        const int32_t w = tbl_ld<IN_LDS>(keys + i);
        if (w < 0) continue;
        double y;
        if (UNIT) {
            y = (double)tbl_ld<IN_LDS>(vals + i);
        } else {
            const int64_t wb = A.rp[w];
            y = kc_sorted_dot(A.col + wb, A.val ? A.val + wb : nullptr, (int)(A.rp[w + 1] - wb), rk, rv, md);
        }
        tbl_st<IN_LDS>(vals + i, __builtin_bit_cast(unsigned long long, y));
    }
    __syncthreads();

    // 3. the candidates
    for (int64_t s0 = p0 + wib * 64; s0 < p1; s0 += KC_WAVES * 64) {
        const int64_t p = s0 + lane;
        const bool valid = p < p1;
        const int32_t u = valid ? cand_u[p] : 0;
        const bool ok = valid && u >= 0 && u < n;
        const int64_t rs = ok ? A.rp[u] : 0;
        const int32_t deg = ok ? (int32_t)(A.rp[u + 1] - rs) : 0;
        double base = 0.0;
        {
            const int pos = lower_bound_uniform(rk, md, ok ? u : 0);
            const int pc = pos < md ? pos : md - 1;
            const bool hit = ok && pos < md && rk[pc] == u;
            const double y1 = hit ? (rv ? (double)rv[pc] : 1.0) : 0.0;
            const double y2 = ok ? kc_find<IN_LDS>(keys, vals, lg, u) : 0.0;
            base = c1 * y1 + c2 * y2;
        }
        const int cls = !ok ? 0 : deg <= KC_T1_DEG ? 1 : deg <= KC_T8_DEG ? 2 : 3;
        const uint64_t m2 = __ballot(cls == 2), m3 = __ballot(cls == 3);
        if (valid && !ok) out[p] = qnan;
        if (cls == 1) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < KC_T1_DEG; ++j)
                if (j < deg) {
                    const int32_t w = A.col[rs + j];
                    const double a = A.val ? (double)A.val[rs + j] : 1.0;
                    acc += a * kc_find<IN_LDS>(keys, vals, lg, w);
                }
            out[p] = (float)(base + c3 * acc);
        }
        if ((m2 | m3) == 0) continue;
        lds_wave_sync();                        // (the previous step's teams are done with the arrays)
        S.crs[wib][lane] = rs;
        S.cdeg[wib][lane] = deg;
        S.cbase[wib][lane] = base;
        if (cls == 2) S.list[wib][__popcll(m2 & ((1ull << lane) - 1))] = lane;
        lds_wave_sync();
        const int n2 = __popcll(m2);
        for (int i0 = 0; i0 < n2; i0 += 8) {
            const int ci = i0 + (lane >> 3);
            const bool on = ci < n2;
            const int src = on ? S.list[wib][ci] : 0;
            const int64_t trs = S.crs[wib][src];
            const int32_t tdeg = on ? S.cdeg[wib][src] : 0;
            double acc = 0.0;
            for (int j = lane & 7; j < tdeg; j += 8) {
                const int32_t w = A.col[trs + j];
                const double a = A.val ? (double)A.val[trs + j] : 1.0;
                acc += a * kc_find<IN_LDS>(keys, vals, lg, w);
            }
            acc += __shfl_xor(acc, 1);
            acc += __shfl_xor(acc, 2);
            acc += __shfl_xor(acc, 4);
            if (on && (lane & 7) == 0) out[s0 + src] = (float)(S.cbase[wib][src] + c3 * acc);
        }
        uint64_t m = m3;
        while (m) {
            const int k = __builtin_ctzll(m);
            m &= m - 1;
            const int64_t trs = S.crs[wib][k];
            const int32_t tdeg = S.cdeg[wib][k];
            double acc = 0.0;
            for (int j = lane; j < tdeg; j += 64) {
                const int32_t w = A.col[trs + j];
                const double a = A.val ? (double)A.val[trs + j] : 1.0;
                acc += a * kc_find<IN_LDS>(keys, vals, lg, w);
            }
            const double tot = eps_wave_sum(acc);
            if (lane == 0) out[s0 + k] = (float)(S.cbase[wib][k] + c3 * tot);
        }
    }
    __syncthreads();
}

template <bool UNIT>
__global__ __launch_bounds__(KC_THREADS) void katz_columns_kernel(
    const EpsCsr A, const EpsCsr AT, const int64_t *__restrict__ paths_in, int64_t n, int64_t v_lo, int64_t n_cols,
    const int64_t *__restrict__ colptr, const int32_t *__restrict__ cand_u, int64_t n_cand, double c1, double c2, double c3,
    int64_t max_support, int64_t chunk, char *__restrict__ tables, int glg, unsigned int *__restrict__ next_unit,
    float *__restrict__ out)
{
    __shared__ KcLds S;
    const int tid = threadIdx.x;
    const int64_t n_units = (n_cand + chunk - 1) / chunk;
    // this workgroup's global table: values, then keys
    unsigned long long *gval = tables ? (unsigned long long *)(tables + (int64_t)blockIdx.x * (((int64_t)12) << glg)) : nullptr;
    int32_t *gkey = tables ? (int32_t *)(gval + ((int64_t)1 << glg)) : nullptr;
    for (;;) {
        __syncthreads();
        if (tid == 0) S.unit = atomicAdd(next_unit, 1u);
        __syncthreads();
        const int64_t unit = S.unit;
        if (unit >= n_units) break;
        int64_t p = unit * chunk;
        const int64_t pe = p + chunk < n_cand ? p + chunk : n_cand;
        int64_t c = column_of(colptr, 0, n_cols - 1, p);
        while (p < pe) {
            while (c + 1 < n_cols && colptr[c + 1] <= p) ++c;      // (columns without candidates)
            const int64_t ce = colptr[c + 1];
            const int64_t q = ce < pe ? ce : pe;
            if (q <= p) break;                 // (column pointers that do not cover the list: nothing is scored past them)
            const int32_t v = (int32_t)(v_lo + c);
            const int64_t pin = paths_in[v];
            const int64_t ub = pin < n ? pin : n;
            if (ub <= KC_LDS_CAP) {
                const int lg = ub > KC_LDS_SLOTS / 2 ? KC_LDS_LG : kc_table_lg(ub);
                kc_column<true, UNIT>(A, AT, n, v, p, q, cand_u, c1, c2, c3, S, S.key, S.val, lg, out);
            } else if (gval && ub <= max_support) {
                kc_column<false, UNIT>(A, AT, n, v, p, q, cand_u, c1, c2, c3, S, gkey, gval, kc_table_lg(ub), out);
            } else {                           // (a column beyond the support the workspace was sized for)
                for (int64_t i = p + tid; i < q; i += KC_THREADS) out[i] = __builtin_nanf("");
            }
            p = q;
        }
    }
}

static inline int kc_global_lg(int64_t max_support)
{
    int lg = 6;
    while (((int64_t)1 << lg) < 2 * max_support) ++lg;
    return lg;
}

// workgroups of a launch whose largest support bound is max_support
static inline int64_t kc_groups(int64_t max_support)
{
    if (max_support <= KC_LDS_CAP) return KC_MAX_GROUPS;
    const int64_t region = (int64_t)12 << kc_global_lg(max_support);
    int64_t g = KC_WS_BUDGET / region;
    return g < 1 ? 1 : g > KC_MAX_GROUPS ? KC_MAX_GROUPS : g;
}

static inline int64_t kc_default_chunk(int64_t n_cand)
{
    int64_t c = KC_CHUNK;
    while (c < KC_CHUNK_BIG && n_cand / (2 * c) >= KC_UNITS_MIN) c *= 2;
    return c;
}

extern "C" int64_t eps_katz_columns_chunk(int64_t n_cand) { return kc_default_chunk(n_cand < 0 ? 0 : n_cand); }

extern "C" int eps_katz_columns_limits(int32_t *lds_capacity, int32_t *chunk)
{
    EPS_REQUIRE(lds_capacity && chunk, "eps_katz_columns_limits: null pointer");
    *lds_capacity = KC_LDS_CAP;
    *chunk = KC_CHUNK;
    return EPS_OK;
}

extern "C" int64_t eps_katz_columns_workspace_bytes(int64_t max_support)
{
    if (max_support <= KC_LDS_CAP) return 0;
    if (max_support > (int64_t)1 << 31) max_support = (int64_t)1 << 31;
    // (256 tables; once those pass the budget, the budget -- kc_groups tables fit it; one table when even that does not)
    const int64_t region = (int64_t)12 << kc_global_lg(max_support);
    if (KC_MAX_GROUPS * region <= KC_WS_BUDGET) return KC_MAX_GROUPS * region;
    return region <= KC_WS_BUDGET ? KC_WS_BUDGET : region;
}

extern "C" int eps_katz_column_scores(const int64_t *rowptr, const int32_t *col, const float *val, const int64_t *rowptr_t,
                                      const int32_t *col_t, const float *val_t, const int64_t *paths_in, int64_t n_nodes,
                                      int64_t v_lo, int64_t v_hi, const int64_t *colptr, const int32_t *cand_u, int64_t n_cand,
                                      double c1, double c2, double c3, int64_t max_support, int32_t chunk, void *workspace,
                                      int64_t workspace_bytes, float *out, void *stream)
{
    EPS_REQUIRE(n_nodes >= 0 && n_cand >= 0 && max_support >= 0 && workspace_bytes >= 0,
                "eps_katz_column_scores: negative size");
    EPS_REQUIRE(n_nodes < (int64_t)1 << 31, "eps_katz_column_scores: node ids are int32");
    EPS_REQUIRE(chunk >= 0 && chunk <= KC_CHUNK_MAX, "eps_katz_column_scores: chunk outside [0, 2^20] (0: the default)");
    const int64_t per_unit = chunk ? chunk : kc_default_chunk(n_cand);
    EPS_REQUIRE((n_cand + per_unit - 1) / per_unit < (int64_t)1 << 31, "eps_katz_column_scores: more than 2^31 work units");
    EPS_REQUIRE(0 <= v_lo && v_lo <= v_hi && v_hi <= n_nodes, "eps_katz_column_scores: columns [v_lo, v_hi) outside the graph");
    EPS_REQUIRE(isfinite(c1) && isfinite(c2) && isfinite(c3), "eps_katz_column_scores: non-finite coefficient");
    EPS_REQUIRE(n_cand == 0 || v_lo < v_hi, "eps_katz_column_scores: candidates in an empty block of columns");
    EPS_REQUIRE(n_cand == 0 || (rowptr && col && rowptr_t && col_t && paths_in && colptr && cand_u && out),
                "eps_katz_column_scores: null pointer");
    EPS_REQUIRE(n_cand == 0 || (val == nullptr) == (val_t == nullptr),
                "eps_katz_column_scores: A and A^T must both carry values or both be unit-valued (null)");
    const int64_t need = eps_katz_columns_workspace_bytes(max_support);
    EPS_REQUIRE(n_cand == 0 || need == 0 || (workspace && workspace_bytes >= need),
                "eps_katz_column_scores: workspace is null or smaller than eps_katz_columns_workspace_bytes(max_support)");
    if (n_cand == 0) return EPS_OK;
    hipStream_t s = (hipStream_t)stream;
    unsigned int *next_unit = nullptr;
    const int crc = eps_take_counter(&next_unit, s, "eps_katz_column_scores");
    if (crc) return crc;
    const EpsCsr A{rowptr, col, val}, AT{rowptr_t, col_t, val_t};
    const int64_t n_units = (n_cand + per_unit - 1) / per_unit;
    int64_t blocks = kc_groups(max_support);
    if (blocks > eps_num_cus()) blocks = eps_num_cus();
    if (blocks > n_units) blocks = n_units;
    char *tables = need ? (char *)workspace : nullptr;
    const int glg = need ? kc_global_lg(max_support) : 0;
    if (val)
        hipLaunchKernelGGL(katz_columns_kernel<false>, dim3((unsigned)blocks), dim3(KC_THREADS), 0, s, A, AT, paths_in, n_nodes,
                           v_lo, v_hi - v_lo, colptr, cand_u, n_cand, c1, c2, c3, max_support, per_unit, tables, glg, next_unit,
                           out);
    else
        hipLaunchKernelGGL(katz_columns_kernel<true>, dim3((unsigned)blocks), dim3(KC_THREADS), 0, s, A, AT, paths_in, n_nodes,
                           v_lo, v_hi - v_lo, colptr, cand_u, n_cand, c1, c2, c3, max_support, per_unit, tables, glg, next_unit,
                           out);
    EPS_CHECK_LAUNCH("eps_katz_column_scores");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void katz_columns_warm_kernel() {}
extern "C" void eps_warm_katz_columns(void *stream) { hipLaunchKernelGGL(katz_columns_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

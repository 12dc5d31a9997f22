// Degree-normalised local similarity indices (Zhou, Lu, Zhang: "Predicting missing links via local information"), gfx950.
//
// With c = the number of common stored neighbours of u and v (the pattern count eps_pair_scores / the expansions produce) and
// a = deg(u), b = deg(v) the numbers of stored entries of their rows (rowptr differences):
//   salton c / sqrt(a b)   jaccard c / (a + b - c)   sorensen 2c / (a + b)   hpi c / min(a, b)   hdi c / max(a, b)
//   lhn c / (a b)          pa a b
// A zero denominator scores 0.  The arithmetic is float64 on the integers (a b < 2^62 rounds once; below 2^53 it is exact),
// then ONE rounding to float32 -- li_score, shared by both entry points.  A score therefore depends on (c, a, b, index) alone:
// score(u, v) == score(v, u) bit for bit, whatever block, slice or launch formed it.
//
// eps_local_index_pairs:   elementwise over an evaluation list (u, v, c).
// eps_local_index_columns: over a column-major block of the filter stage -- candidate p has u = cand_u[p] and
//   v = v_lo + (the column whose segment holds p).  Work is dealt in fixed slices of LI_SLICE slots of the slot array; a slice
//   finds the first and the last column it meets by two searches of colptr (uniform over the workgroup), a thread its own
//   column by a search between those two -- so runs of empty columns and a column longer than a slice are nothing special.
//   In the padded layout (counts given) the slots behind a column's counted entries are neither read nor written.
//   With a bar the kernel reports the slots whose score EXCEEDS *bar, in ascending position: count per slice, one exclusive
//   prefix over the slices, fill -- three launches, each slice's place known before it writes.  No atomics, no workgroup
//   waits on another: the same inputs give the same bits in the same places.
// Both are streaming kernels (4 B id + 4 B count in, 4 B score out per candidate; 16-byte accesses where four consecutive
// slots are live in one column), rowptr is the only gathered table.
#include "flat_rows.h"      // (column_of)

#include <math.h>

#define LI_THREADS 256
#define LI_WAVES (LI_THREADS / 64)
#define LI_VEC 4                          // consecutive slots per thread and step: one 16-byte access per array
#define LI_STEP (LI_THREADS * LI_VEC)     // slots per workgroup step
#define LI_SLICE 4096                     // slots per slice: the unit of work, and of the survivor counts
#define LI_SCAN_THREADS 1024
#define LI_SCAN_WAVES (LI_SCAN_THREADS / 64)
#define LI_INDICES 7

enum { LI_SALTON = 0, LI_JACCARD, LI_SORENSEN, LI_HPI, LI_HDI, LI_LHN, LI_PA };

__device__ __forceinline__ float li_score(int index, int64_t c, int64_t a, int64_t b)
{
    const double C = (double)c, A = (double)a, B = (double)b;
    double num = C, den;
    switch (index) {
    case LI_SALTON: den = sqrt(A * B); break;
    case LI_JACCARD: den = A + B - C; break;
    case LI_SORENSEN: num = 2.0 * C; den = A + B; break;
    case LI_HPI: den = A < B ? A : B; break;
    case LI_HDI: den = A > B ? A : B; break;
    case LI_LHN: den = A * B; break;
    default: return (float)(A * B);      // LI_PA
    }
    return den == 0.0 ? 0.0f : (float)(num / den);
}

// Stored entries of row x; the caller has checked 0 <= x < n_nodes.
__device__ __forceinline__ int64_t li_degree(const int64_t *__restrict__ rowptr, int64_t x) { return rowptr[x + 1] - rowptr[x]; }

// ---- the evaluation list ------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(LI_THREADS) void local_index_pairs_kernel(const int64_t *__restrict__ rowptr, int64_t n_nodes,
                                                                      const int32_t *__restrict__ u, const int32_t *__restrict__ v,
                                                                      const int32_t *__restrict__ cn, int64_t n_pairs, int index,
                                                                      float *__restrict__ score)
{
    const int64_t p0 = ((int64_t)blockIdx.x * LI_THREADS + threadIdx.x) * LI_VEC;
    if (p0 >= n_pairs) return;
    const bool whole = VEC && p0 + LI_VEC <= n_pairs;
    int32_t uu[LI_VEC], vv[LI_VEC], cc[LI_VEC];
    if (whole) {
        const int4 a = *(const int4 *)(u + p0), b = *(const int4 *)(v + p0), c = *(const int4 *)(cn + p0);
        uu[0] = a.x; uu[1] = a.y; uu[2] = a.z; uu[3] = a.w;
        vv[0] = b.x; vv[1] = b.y; vv[2] = b.z; vv[3] = b.w;
        cc[0] = c.x; cc[1] = c.y; cc[2] = c.z; cc[3] = c.w;
    } else {
#pragma unroll
        for (int j = 0; j < LI_VEC; ++j) {
            const bool in = p0 + j < n_pairs;
            uu[j] = in ? u[p0 + j] : 0;
            vv[j] = in ? v[p0 + j] : 0;
            cc[j] = in ? cn[p0 + j] : 0;
        }
    }
    float s[LI_VEC];
#pragma unroll
    for (int j = 0; j < LI_VEC; ++j) {
        const bool ok = uu[j] >= 0 && uu[j] < n_nodes && vv[j] >= 0 && vv[j] < n_nodes;
        const int64_t a = ok ? li_degree(rowptr, uu[j]) : 0, b = ok ? li_degree(rowptr, vv[j]) : 0;
        s[j] = ok ? li_score(index, cc[j], a, b) : __builtin_nanf("");
    }
    if (whole) {
        *(float4 *)(score + p0) = make_float4(s[0], s[1], s[2], s[3]);
    } else {
#pragma unroll
        for (int j = 0; j < LI_VEC; ++j)
            if (p0 + j < n_pairs) score[p0 + j] = s[j];
    }
}

// ---- a block of columns -------------------------------------------------------------------------------------------------
struct LiBlock {
    const int64_t *__restrict__ rowptr;
    int64_t n_nodes, v_lo, n_cols;
    const int64_t *__restrict__ colptr;
    const int64_t *__restrict__ counts;       // or null: segments are [colptr[s], colptr[s + 1])
    const int32_t *__restrict__ cand_u;
    const int32_t *__restrict__ cn_i;         // exactly one of cn_i / cn_f
    const float *__restrict__ cn_f;
    int64_t n_slots;
    int index;
    int vec;                                  // cand_u, the count array and score are 16-byte aligned
    float *__restrict__ score;                // or null
    const float *__restrict__ bar;            // or null
    int64_t capacity;
    int64_t *__restrict__ surv_pos;
    float *__restrict__ surv_score;
    int64_t *__restrict__ slice_ofs;          // [n_slices + 1]: survivors per slice, then their exclusive prefix
};

#define LI_MODE_SCORE 0     // score[] only
#define LI_MODE_COUNT 1     // survivors per slice (and score[] when given)
#define LI_MODE_FILL 2      // the survivors, at their places

template <int MODE, bool F32CN>
__global__ __launch_bounds__(LI_THREADS) void local_index_columns_kernel(const LiBlock B)
{
    __shared__ uint32_t s_w[2][LI_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t slice = blockIdx.x;
    const int64_t s0 = slice * LI_SLICE;
    const int64_t s1 = s0 + LI_SLICE < B.n_slots ? s0 + LI_SLICE : B.n_slots;
    int64_t out_at = 0;
    if (MODE == LI_MODE_FILL) {
        out_at = B.slice_ofs[slice];
        if (B.slice_ofs[slice + 1] == out_at || out_at >= B.capacity) return;     // (uniform: nothing of this slice is listed)
    }
    const float bar = MODE == LI_MODE_SCORE ? 0.0f : *B.bar;
    const float qnan = __builtin_nanf("");
    // the columns this slice meets (the same for every thread)
    const int64_t c_first = column_of(B.colptr, 0, B.n_cols - 1, s0);
    const int64_t c_last = column_of(B.colptr, c_first, B.n_cols - 1, s1 - 1);
    uint32_t n_over = 0;
    int buf = 0;

    for (int64_t base = s0; base < s1; base += LI_STEP) {
        const int64_t p0 = base + (int64_t)tid * LI_VEC;
        float s[LI_VEC] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool live[LI_VEC] = {false, false, false, false};
        bool whole = false;
        if (p0 < s1) {
            int64_t c = column_of(B.colptr, c_first, c_last, p0);
            int64_t next = c + 1 < B.n_cols ? B.colptr[c + 1] : B.n_slots;
            if (next > B.n_slots) next = B.n_slots;
            int64_t end = B.counts ? B.colptr[c] + B.counts[c] : next;      // the counted entries of column c end here
            if (end > next) end = next;
            int64_t v = B.v_lo + c;
            int64_t b = li_degree(B.rowptr, v);
            whole = B.vec && p0 + LI_VEC <= end;
            if (whole) {                                                    // four live slots of one column
                const int4 u4 = *(const int4 *)(B.cand_u + p0);
                const int32_t uu[LI_VEC] = {u4.x, u4.y, u4.z, u4.w};
                int64_t cc[LI_VEC];
                if (F32CN) {
                    const float4 f = *(const float4 *)(B.cn_f + p0);
                    cc[0] = (int64_t)f.x; cc[1] = (int64_t)f.y; cc[2] = (int64_t)f.z; cc[3] = (int64_t)f.w;
                } else {
                    const int4 i = *(const int4 *)(B.cn_i + p0);
                    cc[0] = i.x; cc[1] = i.y; cc[2] = i.z; cc[3] = i.w;
                }
#pragma unroll
                for (int j = 0; j < LI_VEC; ++j) {
                    const bool ok = uu[j] >= 0 && uu[j] < B.n_nodes;
                    const int64_t a = ok ? li_degree(B.rowptr, uu[j]) : 0;
                    s[j] = ok ? li_score(B.index, cc[j], a, b) : qnan;
                    live[j] = true;
                }
            } else {
#pragma unroll
                for (int j = 0; j < LI_VEC; ++j) {
                    const int64_t p = p0 + j;
                    s[j] = 0.0f;
                    if (p >= s1) continue;
                    if (p >= next) {                                        // the next column with a segment at or before p
                        c = column_of(B.colptr, c + 1, c_last, p);
                        next = c + 1 < B.n_cols ? B.colptr[c + 1] : B.n_slots;
                        if (next > B.n_slots) next = B.n_slots;
                        end = B.counts ? B.colptr[c] + B.counts[c] : next;
                        if (end > next) end = next;
                        v = B.v_lo + c;
                        b = li_degree(B.rowptr, v);
                    }
                    if (p >= end) continue;                                 // padding: not read, not written
                    const int32_t u = B.cand_u[p];
                    const int64_t cn = F32CN ? (int64_t)B.cn_f[p] : (int64_t)B.cn_i[p];
                    const bool ok = u >= 0 && u < B.n_nodes;
                    const int64_t a = ok ? li_degree(B.rowptr, u) : 0;
                    s[j] = ok ? li_score(B.index, cn, a, b) : qnan;
                    live[j] = true;
                }
            }
        }
        if (MODE != LI_MODE_FILL && B.score) {
            if (whole) {
                *(float4 *)(B.score + p0) = make_float4(s[0], s[1], s[2], s[3]);
            } else {
#pragma unroll
                for (int j = 0; j < LI_VEC; ++j)
                    if (live[j]) B.score[p0 + j] = s[j];
            }
        }
        if (MODE == LI_MODE_SCORE) continue;
        uint32_t own = 0;
#pragma unroll
        for (int j = 0; j < LI_VEC; ++j) own += (live[j] && s[j] > bar) ? 1u : 0u;
        if (MODE == LI_MODE_COUNT) {
            n_over += own;
            continue;
        }
        // fill: the survivors of this step in slot order -- an exclusive prefix over the workgroup's threads
        const uint32_t incl = eps_wave_incl_scan(own, lane);
        if (lane == 63) s_w[buf][wv] = incl;
        __syncthreads();
        uint32_t front = 0, all = 0;
#pragma unroll
        for (int w = 0; w < LI_WAVES; ++w) {
            if (w < wv) front += s_w[buf][w];
            all += s_w[buf][w];
        }
        buf ^= 1;      // (the next step writes the other buffer: a wave that runs ahead cannot touch counts still being read)
        int64_t at = out_at + front + incl - own;
#pragma unroll
        for (int j = 0; j < LI_VEC; ++j)
            if (live[j] && s[j] > bar) {
                if (at < B.capacity) {
                    B.surv_pos[at] = p0 + j;
                    B.surv_score[at] = s[j];
                }
                ++at;
            }
        out_at += all;
    }
    if (MODE == LI_MODE_COUNT) {
        uint32_t t = n_over;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) t += __shfl_xor(t, o);
        if (lane == 0) s_w[0][wv] = t;
        __syncthreads();
        if (tid == 0) {
            uint32_t all = 0;
#pragma unroll
            for (int w = 0; w < LI_WAVES; ++w) all += s_w[0][w];
            B.slice_ofs[slice] = all;
        }
    }
}

// ofs[0 .. n) -> its exclusive prefix in place, ofs[n] and *n_surv = the total.  One workgroup: the slices are few (one per
// LI_SLICE slots), and a single ordered pass needs no hand-off between workgroups.
__global__ __launch_bounds__(LI_SCAN_THREADS) void local_index_scan_kernel(int64_t *__restrict__ ofs, int64_t n,
                                                                          int64_t *__restrict__ n_surv)
{
    __shared__ int64_t s_w[2][LI_SCAN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int64_t run = 0;
    int buf = 0;
    for (int64_t base = 0; base < n; base += LI_SCAN_THREADS * 4) {
        const int64_t i = base + (int64_t)tid * 4;
        int64_t x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = i + j < n ? ofs[i + j] : 0;
        const int64_t own = x[0] + x[1] + x[2] + x[3];
        const int64_t incl = eps_wave_incl_scan(own, lane);
        if (lane == 63) s_w[buf][wv] = incl;
        __syncthreads();
        int64_t front = 0, all = 0;
#pragma unroll
        for (int w = 0; w < LI_SCAN_WAVES; ++w) {
            if (w < wv) front += s_w[buf][w];
            all += s_w[buf][w];
        }
        buf ^= 1;
        int64_t e = run + front + incl - own;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i + j < n) ofs[i + j] = e;
            e += x[j];
        }
        run += all;
    }
    if (tid == 0) {
        ofs[n] = run;
        *n_surv = run;
    }
}

static inline int64_t li_slices(int64_t n_slots) { return (n_slots + LI_SLICE - 1) / LI_SLICE; }

static inline bool li_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int64_t eps_local_index_columns_workspace_bytes(int64_t n_slots)
{
    return n_slots <= 0 ? 0 : (li_slices(n_slots) + 1) * (int64_t)sizeof(int64_t);
}

extern "C" int eps_local_index_pairs(const int64_t *rowptr, int64_t n_nodes, const int32_t *u, const int32_t *v, const int32_t *cn,
                                     int64_t n_pairs, int32_t index, float *score, void *stream)
{
    EPS_REQUIRE(index >= 0 && index < LI_INDICES, "eps_local_index_pairs: index=%d must lie in [0, %d)", (int)index, LI_INDICES);
    EPS_REQUIRE(n_nodes >= 0 && n_nodes < (1ll << 31), "eps_local_index_pairs: n_nodes=%lld must lie in [0, 2^31)", (long long)n_nodes);
    EPS_REQUIRE(n_pairs >= 0, "eps_local_index_pairs: n_pairs=%lld is negative", (long long)n_pairs);
    if (n_pairs == 0) return EPS_OK;
    EPS_REQUIRE(rowptr && u && v && cn && score, "eps_local_index_pairs: null pointer with n_pairs=%lld", (long long)n_pairs);
    const int64_t blocks = (n_pairs + LI_STEP - 1) / LI_STEP;
    EPS_REQUIRE(blocks < (1ll << 31), "eps_local_index_pairs: n_pairs=%lld is more than one launch takes", (long long)n_pairs);
    hipStream_t s = (hipStream_t)stream;
    if (li_aligned16(u) && li_aligned16(v) && li_aligned16(cn) && li_aligned16(score))
        hipLaunchKernelGGL(local_index_pairs_kernel<true>, dim3((unsigned)blocks), dim3(LI_THREADS), 0, s, rowptr, n_nodes, u, v, cn,
                           n_pairs, (int)index, score);
    else
        hipLaunchKernelGGL(local_index_pairs_kernel<false>, dim3((unsigned)blocks), dim3(LI_THREADS), 0, s, rowptr, n_nodes, u, v, cn,
                           n_pairs, (int)index, score);
    EPS_CHECK_LAUNCH("eps_local_index_pairs");
    return EPS_OK;
}

template <bool F32CN>
static void li_launch_columns(const LiBlock &B, int64_t n_slices, hipStream_t s, int64_t *n_surv)
{
    const dim3 grid((unsigned)n_slices), block(LI_THREADS);
    if (!B.bar) {
        hipLaunchKernelGGL((local_index_columns_kernel<LI_MODE_SCORE, F32CN>), grid, block, 0, s, B);
        return;
    }
    hipLaunchKernelGGL((local_index_columns_kernel<LI_MODE_COUNT, F32CN>), grid, block, 0, s, B);
    hipLaunchKernelGGL(local_index_scan_kernel, dim3(1), dim3(LI_SCAN_THREADS), 0, s, B.slice_ofs, n_slices, n_surv);
    hipLaunchKernelGGL((local_index_columns_kernel<LI_MODE_FILL, F32CN>), grid, block, 0, s, B);
}

extern "C" int eps_local_index_columns(const int64_t *rowptr, int64_t n_nodes, int64_t v_lo, int64_t v_hi, const int64_t *colptr,
                                       const int64_t *counts_or_null, const int32_t *cand_u, int64_t n_slots,
                                       const int32_t *cn_i32_or_null, const float *cn_f32_or_null, int32_t index,
                                       float *score_or_null, const float *bar_or_null, int64_t capacity, int64_t *surv_pos,
                                       float *surv_score, int64_t *n_surv, void *workspace, int64_t workspace_bytes, void *stream)
{
    EPS_REQUIRE(index >= 0 && index < LI_INDICES, "eps_local_index_columns: index=%d must lie in [0, %d)", (int)index, LI_INDICES);
    EPS_REQUIRE((cn_i32_or_null != nullptr) != (cn_f32_or_null != nullptr),
                "eps_local_index_columns: exactly one count form (cn_i32 or cn_f32), got %s",
                cn_i32_or_null ? "both" : "neither");
    EPS_REQUIRE(n_nodes >= 0 && n_nodes < (1ll << 31), "eps_local_index_columns: n_nodes=%lld must lie in [0, 2^31)", (long long)n_nodes);
    EPS_REQUIRE(n_slots >= 0, "eps_local_index_columns: n_slots=%lld is negative", (long long)n_slots);
    EPS_REQUIRE(capacity >= 0, "eps_local_index_columns: capacity=%lld is negative", (long long)capacity);
    EPS_REQUIRE(workspace_bytes >= 0, "eps_local_index_columns: workspace_bytes=%lld is negative", (long long)workspace_bytes);
    EPS_REQUIRE(v_lo >= 0 && v_lo <= v_hi && v_hi <= n_nodes,
                "eps_local_index_columns: columns [v_lo=%lld, v_hi=%lld) must ascend inside [0, n_nodes=%lld]", (long long)v_lo,
                (long long)v_hi, (long long)n_nodes);
    EPS_REQUIRE(!cn_f32_or_null || n_nodes < (1ll << 24),
                "eps_local_index_columns: n_nodes=%lld: a float32 count is exact below 2^24 nodes only (pass cn_i32)",
                (long long)n_nodes);
    EPS_REQUIRE(!bar_or_null || (n_surv && (capacity == 0 || (surv_pos && surv_score))),
                "eps_local_index_columns: a bar without a survivor list (surv_pos / surv_score / n_surv, capacity=%lld)",
                (long long)capacity);
    EPS_REQUIRE(bar_or_null || score_or_null || n_slots == 0, "eps_local_index_columns: neither score nor bar: nothing to compute");
    EPS_REQUIRE(n_slots == 0 || v_lo < v_hi, "eps_local_index_columns: n_slots=%lld in an empty block of columns", (long long)n_slots);
    EPS_REQUIRE(n_slots == 0 || (rowptr && colptr && cand_u), "eps_local_index_columns: null pointer with n_slots=%lld", (long long)n_slots);
    const int64_t n_slices = li_slices(n_slots);
    EPS_REQUIRE(n_slices < (1ll << 31), "eps_local_index_columns: n_slots=%lld is more than one launch takes", (long long)n_slots);
    const int64_t need = bar_or_null ? eps_local_index_columns_workspace_bytes(n_slots) : 0;
    EPS_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0),
                "eps_local_index_columns: workspace is null, misaligned or smaller than "
                "eps_local_index_columns_workspace_bytes(n_slots)=%lld", (long long)need);
    hipStream_t s = (hipStream_t)stream;
    if (n_slots == 0) {
        if (bar_or_null && hipMemsetAsync(n_surv, 0, sizeof(int64_t), s) != hipSuccess) {
            eps_set_error("eps_local_index_columns: cannot clear n_surv");
            return EPS_ELAUNCH;
        }
        return EPS_OK;
    }
    LiBlock B;
    B.rowptr = rowptr; B.n_nodes = n_nodes; B.v_lo = v_lo; B.n_cols = v_hi - v_lo;
    B.colptr = colptr; B.counts = counts_or_null; B.cand_u = cand_u; B.cn_i = cn_i32_or_null; B.cn_f = cn_f32_or_null;
    B.n_slots = n_slots; B.index = (int)index;
    B.vec = li_aligned16(cand_u) && li_aligned16(cn_i32_or_null) && li_aligned16(cn_f32_or_null) && li_aligned16(score_or_null);
    B.score = score_or_null; B.bar = bar_or_null; B.capacity = capacity; B.surv_pos = surv_pos; B.surv_score = surv_score;
    B.slice_ofs = (int64_t *)workspace;
    if (cn_f32_or_null) li_launch_columns<true>(B, n_slices, s, n_surv);
    else li_launch_columns<false>(B, n_slices, s, n_surv);
    EPS_CHECK_LAUNCH("eps_local_index_columns");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void local_index_warm_kernel() {}
extern "C" void eps_warm_local_index(void *stream) { hipLaunchKernelGGL(local_index_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

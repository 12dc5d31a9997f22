// Common-neighbour LISTS per pair, and their transpose, gfx950.
//
// The pair kernels of pair_intersect.hip reduce over N(u) & N(v) (a count, a weighted sum); Neural Common Neighbor (Wang, Yang,
// Zhang) needs the intersection itself: Z = C H with C the sparse [pairs x nodes] incidence "w is a common neighbour of pair b",
// and dH = C^T dZ in the backward.  Both products are eps_spmm_csr; this unit builds C (count, the caller's prefix sum, fill) and
// C^T (a stable sort by w).
//
// Work decomposition: pair_intersect.hip's generic kernel (PART 0) without the sums --
//   * 64-pair chunks are handed to waves by ticket (one device-scope atomic per chunk, drawn one chunk ahead);
//   * lane i fetches pair i's ids, row bounds and (fill) segment bounds; the 64 pairs are then listed one after the other by the
//     whole wave, each by the walk of row_intersect.h;
//   * the matches of a 64-element slice are compacted by ballot + prefix popcount, so a slice is written in the short row's
//     order; the walk delivers the slices in the short row's order too, pass after pass, so the whole segment ascends in w
//     whichever row is the short one: list(u, v) and list(v, u) are the same array.
// COUNT and FILL are the two modes of ONE template: the same walk decides what is a match in both.  The fill writes plain vector
// stores at ptr[b] + rank, never at or past ptr[b + 1] (nor past ptr[n_pairs]), and reports a segment whose length is not the
// pair's match count in *status.  No atomics on global memory but the ticket.
// HBM traffic: both rows once, 4 bytes per match, 24 (count) / 32 (fill) bytes of header per pair.
#include "row_intersect.h"

#include <rocprim/device/device_radix_sort.hpp>

#define CL_WAVES 4            // waves per workgroup

template <bool FILL>
__global__ __launch_bounds__(CL_WAVES * 64) void pair_cn_list_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t n_rows, const int32_t *__restrict__ pu,
    const int32_t *__restrict__ pv, int64_t n_pairs, unsigned int *__restrict__ next_chunk, int32_t *__restrict__ out_count,
    const int64_t *__restrict__ ptr, int32_t *__restrict__ out_w, int32_t *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) int32_t s_rows[CL_WAVES][ROW_CAP];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int32_t *L = s_rows[wib];
    const int64_t n_chunks = (n_pairs + 63) >> 6;
    const int64_t total = FILL ? ptr[n_pairs] : 0;           // no store at or past the end of out_w, whatever ptr holds

    auto do_chunk = [&](const int64_t chunk) {
        const int64_t p = chunk * 64 + lane;
        const bool valid = p < n_pairs;
        const int32_t nu = valid ? pu[p] : -1, nv = valid ? pv[p] : -1;
        // an id outside the graph contributes nothing and reads nothing
        const bool ok = nu >= 0 && nv >= 0 && (int64_t)nu < n_rows && (int64_t)nv < n_rows;
        const int64_t ub = ok ? rowptr[nu] : 0, vb = ok ? rowptr[nv] : 0;
        const int32_t du = ok ? (int32_t)(rowptr[nu + 1] - ub) : 0;
        const int32_t dv = ok ? (int32_t)(rowptr[nv + 1] - vb) : 0;
        int64_t seg_b = 0, seg_e = 0;
        if (FILL && valid) {
            seg_b = ptr[p];
            seg_e = ptr[p + 1];
            if (seg_e > total) seg_e = total;
            if (seg_b < 0 || seg_b > seg_e) seg_b = seg_e;   // (a ptr that does not ascend from 0: an empty segment, reported below)
        }
        int32_t my_count = 0;

        for (int j = 0; j < 64; ++j) {
            const int32_t dju = __builtin_amdgcn_readlane(du, j);
            const int32_t djv = __builtin_amdgcn_readlane(dv, j);
            if (dju <= 0 || djv <= 0) continue;              // wave-uniform (also: lanes past the end of the list, ids out of range)
            const int64_t bju = eps_bcast64(ub, j), bjv = eps_bcast64(vb, j);
            const int64_t ob = FILL ? eps_bcast64(seg_b, j) : 0, oe = FILL ? eps_bcast64(seg_e, j) : 0;
            const bool swapped = dju > djv;                  // short row = v
            const int32_t slen = swapped ? djv : dju, llen = swapped ? dju : djv;
            const int64_t sbase = swapped ? bjv : bju, lbase = swapped ? bju : bjv;
            int cnt = 0;                                     // wave-uniform: matches of this pair so far
            // one slice of the short row: t per lane, `found` where it is a common neighbour
            auto emit = [&](const bool found, const int t, int, int, bool) {
                const uint64_t m = __ballot(found);
                if (m == 0ull) return;
                if (FILL) {
                    const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
                    const int64_t at = ob + cnt + below;
                    if (found && at < oe) out_w[at] = t;     // never at or past the segment's end
                }
                cnt += __popcll(m);
            };
            intersect_rows<ROW_CAP, ROW_INPLACE_RATIO>(col, sbase, slen, lbase, llen, L, lane, emit);
            if (lane == j) my_count = cnt;
        }
        if (valid) {
            if (FILL) {
                // a segment that would overflow (clamped above) or stays short: the count this ptr came from was not this list's
                if ((int64_t)my_count != ptr[p + 1] - ptr[p] || ptr[p] < 0 || ptr[p + 1] > total) *status = 1;
            } else {
                out_count[p] = my_count;
            }
        }
    };
    int64_t chunk = take_chunk(next_chunk, lane);
    while (chunk < n_chunks) {
        const int64_t next = take_chunk(next_chunk, lane);
        do_chunk(chunk);
        chunk = next;
    }
}

template <bool FILL>
static int launch_cn_list(const char *who, const int64_t *rowptr, const int32_t *col, int64_t n_rows, const int32_t *u,
                          const int32_t *v, int64_t n_pairs, int32_t *count, const int64_t *ptr, int32_t *out_w, int32_t *status,
                          hipStream_t stream)
{
    const int64_t n_chunks = (n_pairs + 63) / 64;
    int64_t blocks = (n_chunks + CL_WAVES - 1) / CL_WAVES;
    const int64_t max_blocks = (int64_t)eps_num_cus() * 8;  // 32 waves per CU
    if (blocks > max_blocks) blocks = max_blocks;
    unsigned int *counter = nullptr;
    const int crc = eps_take_counter(&counter, stream, who);
    if (crc) return crc;
    hipLaunchKernelGGL((pair_cn_list_kernel<FILL>), dim3((unsigned)blocks), dim3(CL_WAVES * 64), 0, stream, rowptr, col, n_rows, u, v,
                       n_pairs, counter, count, ptr, out_w, status);
    EPS_CHECK_LAUNCH(who);
    return EPS_OK;
}

extern "C" int eps_pair_cn_list_limits(int32_t *cap, int32_t *inplace_ratio)
{
    if (cap) *cap = ROW_CAP;
    if (inplace_ratio) *inplace_ratio = ROW_INPLACE_RATIO;
    return EPS_OK;
}

extern "C" int eps_pair_cn_list_count(const int64_t *rowptr, const int32_t *col, int64_t n_rows, const int32_t *u, const int32_t *v,
                                      int64_t n_pairs, int32_t *count, void *stream)
{
    EPS_REQUIRE(n_pairs >= 0 && n_rows >= 0 && n_rows < (1ll << 31), "eps_pair_cn_list_count: bad size (n_rows=%lld n_pairs=%lld)",
                (long long)n_rows, (long long)n_pairs);
    if (n_pairs == 0) return EPS_OK;
    EPS_REQUIRE(u && v && count && (n_rows == 0 || (rowptr && col)), "eps_pair_cn_list_count: null pointer");
    return launch_cn_list<false>("eps_pair_cn_list_count", rowptr, col, n_rows, u, v, n_pairs, count, nullptr, nullptr, nullptr,
                                 (hipStream_t)stream);
}

extern "C" int eps_pair_cn_list_fill(const int64_t *rowptr, const int32_t *col, int64_t n_rows, const int32_t *u, const int32_t *v,
                                     int64_t n_pairs, const int64_t *ptr, int32_t *out_w, int32_t *status, void *stream)
{
    EPS_REQUIRE(n_pairs >= 0 && n_rows >= 0 && n_rows < (1ll << 31), "eps_pair_cn_list_fill: bad size (n_rows=%lld n_pairs=%lld)",
                (long long)n_rows, (long long)n_pairs);
    EPS_REQUIRE(status, "eps_pair_cn_list_fill: null status");
    if (hipMemsetAsync(status, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) {
        eps_set_error("eps_pair_cn_list_fill: cannot clear the status word");
        return EPS_ELAUNCH;
    }
    if (n_pairs == 0) return EPS_OK;
    EPS_REQUIRE(u && v && ptr && out_w && (n_rows == 0 || (rowptr && col)), "eps_pair_cn_list_fill: null pointer");
    return launch_cn_list<true>("eps_pair_cn_list_fill", rowptr, col, n_rows, u, v, n_pairs, nullptr, ptr, out_w, status,
                                (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------- transpose
// The same incidence by node: entry i of the list belongs to pair b(i) = the segment of ptr that holds i; a STABLE radix sort of
// (w, b) by w (rocPRIM, least significant digit first: equal keys keep their order, and the list is ascending in b) gives tb, and
// tptr[w] is the first place of w in the sorted keys.  A function of the input alone: no atomics.
__global__ void cn_list_pair_ids_kernel(const int64_t *__restrict__ ptr, int64_t n_pairs, int64_t m, int32_t *__restrict__ b_of)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        int64_t lo = 0, hi = n_pairs;                        // the last b with ptr[b] <= i (empty segments are skipped)
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (ptr[mid] <= i) lo = mid;
            else hi = mid;
        }
        b_of[i] = (int32_t)lo;
    }
}

__global__ void cn_list_tptr_kernel(const int32_t *__restrict__ w_sorted, int64_t m, int64_t n_rows, int64_t *__restrict__ tptr)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w <= n_rows; w += stride) {
        const int64_t below = eps_lower_bound(w_sorted, (int64_t)0, m, w);      // entries of w_sorted below w
        tptr[w] = w == n_rows ? m : below;
    }
}

static size_t cl_align(size_t x) { return (x + 255) & ~(size_t)255; }

static unsigned cl_key_bits(int64_t n_rows)
{
    unsigned bits = 1;
    while (bits < 31 && (1ll << bits) < n_rows) ++bits;
    return bits;
}

static size_t cl_sort_temp_bytes(int64_t m, int64_t n_rows)
{
    size_t a = 0;
    (void)rocprim::radix_sort_pairs((void *)nullptr, a, (const int32_t *)nullptr, (int32_t *)nullptr, (const int32_t *)nullptr,
                                    (int32_t *)nullptr, (size_t)m, 0u, cl_key_bits(n_rows), (hipStream_t)0);
    return a;
}

static unsigned cl_blocks(int64_t n)
{
    int64_t blocks = (n + 255) / 256;
    const int64_t cap = (int64_t)eps_num_cus() * 8;
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

extern "C" int64_t eps_cn_list_transpose_workspace_bytes(int64_t m, int64_t n_rows)
{
    if (m <= 0 || n_rows <= 0 || m >= (1ll << 31) || n_rows >= (1ll << 31)) return 256;
    return (int64_t)(2 * cl_align((size_t)m * 4) + cl_align(cl_sort_temp_bytes(m, n_rows)) + 256);   // (pair ids, sorted w, rocPRIM's)
}

extern "C" int eps_cn_list_transpose(const int64_t *ptr, const int32_t *out_w, int64_t m, int64_t n_pairs, int64_t n_rows,
                                     int64_t *tptr, int32_t *tb, void *workspace, int64_t workspace_bytes, void *stream)
{
    EPS_REQUIRE(m >= 0 && m < (1ll << 31) && n_pairs >= 0 && n_pairs < (1ll << 31) && n_rows >= 0 && n_rows < (1ll << 31),
                "eps_cn_list_transpose: bad size (m=%lld n_pairs=%lld n_rows=%lld)", (long long)m, (long long)n_pairs, (long long)n_rows);
    EPS_REQUIRE(tptr, "eps_cn_list_transpose: null tptr");
    EPS_REQUIRE(m == 0 || (n_pairs > 0 && n_rows > 0), "eps_cn_list_transpose: m=%lld entries without pairs or nodes", (long long)m);
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) {                                            // nothing listed: every node's segment is empty, nothing is read
        if (hipMemsetAsync(tptr, 0, (size_t)(n_rows + 1) * sizeof(int64_t), s) != hipSuccess) {
            eps_set_error("eps_cn_list_transpose: cannot clear tptr");
            return EPS_ELAUNCH;
        }
        return EPS_OK;
    }
    EPS_REQUIRE(ptr && out_w && tb, "eps_cn_list_transpose: null pointer");
    EPS_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= eps_cn_list_transpose_workspace_bytes(m, n_rows),
                "eps_cn_list_transpose: needs a 256-byte aligned workspace of eps_cn_list_transpose_workspace_bytes(m, n_rows) bytes");
    int32_t *b_of = (int32_t *)workspace;
    int32_t *w_sorted = (int32_t *)((char *)workspace + cl_align((size_t)m * 4));
    void *temp = (char *)workspace + 2 * cl_align((size_t)m * 4);
    size_t temp_bytes = (size_t)workspace_bytes - 2 * cl_align((size_t)m * 4);
    hipLaunchKernelGGL(cn_list_pair_ids_kernel, dim3(cl_blocks(m)), dim3(256), 0, s, ptr, n_pairs, m, b_of);
    if (rocprim::radix_sort_pairs(temp, temp_bytes, out_w, w_sorted, (const int32_t *)b_of, tb, (size_t)m, 0u, cl_key_bits(n_rows), s) !=
        hipSuccess) {
        eps_set_error("eps_cn_list_transpose: radix sort failed");
        return EPS_ELAUNCH;
    }
    hipLaunchKernelGGL(cn_list_tptr_kernel, dim3(cl_blocks(n_rows + 1)), dim3(256), 0, s, (const int32_t *)w_sorted, m, n_rows, tptr);
    EPS_CHECK_LAUNCH("eps_cn_list_transpose");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void pair_cn_list_warm_kernel() {}
extern "C" void eps_warm_pair_cn_list(void *stream) { hipLaunchKernelGGL(pair_cn_list_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

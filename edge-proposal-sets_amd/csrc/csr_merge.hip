// Adding a sorted batch of edges to a resident CSR graph: a merge per row, not a sort of the whole edge list (gfx950).
//
// rank.py:28-36 rebuilds its adjacency at every sweep point: the training edges and the k best proposals are concatenated,
// coalesced and symmetrised (graph.add_edges: two torch.unique calls over every stored entry).  The training graph does not
// change between points and is already a sorted, coalesced, symmetric CSR in HBM; what a point adds is a small batch.  With the
// batch as SORTED keys x[p] = row << 32 | col (mirrored by the caller, duplicates allowed) every output position follows from
// two counts -- the base entries in front of it and the NEW keys in front of it:
//   flag[p]  = 1 where x[p] is the first of its run of equal keys and its column is absent from the base row,
//   G        = the exclusive prefix of flag over the whole batch (G[m] = all new entries; rocPRIM scan, int32),
//   new_deg[r] = deg(r) + G[xe] - G[xs],  [xs, xe) = row r's keys, found by two lower-bound searches on x,
//   base entry i of row r, column c  ->  i + G[lower_bound(x, r << 32 | c)]   (inside the row: its index + the row's new keys
//                                        with a smaller column),
//   new key p, column c              ->  lower_bound(base row, c) + G[p]      (inside the row: its rank among the row's new
//                                        keys + the base entries with a smaller column),
// and the values are val + (length of the run of equal keys) resp. that length: whole numbers, added once per output entry.
// No atomics on the data path, no order dependence: the same inputs give the same bits.
//
// Work split.  The keys are handled one per thread (flag, new entries): nothing about a key depends on its neighbours but the
// run test against x[p - 1].  The base entries -- all the bytes -- are split FLAT OVER THE ENTRIES OF A BLOCK OF ROWS: a
// workgroup takes up to 255 consecutive rows, one thread per row finds the row's first key (the only search on the whole batch,
// once per row, never per entry) and parks it in LDS with the row's old and new offsets; the block's entries are contiguous in
// col[], so the 256 threads then stream them 256 at a time, coalesced, each finding its row by a search over the <= 256 offsets
// in LDS.  Rows of 10 entries (collab) fill the lanes as well as rows of 74 (ppa), a row nobody adds to costs one subtraction
// per entry, and a hub row is shared by four waves instead of serialising one.  One wave per row would run collab's rows at
// 10 / 64 lanes and pay the two searches on the batch per row and wave; a fully flat split would pay them per entry.
#include "eps_common.h"

#include <rocprim/device/device_scan.hpp>

#define CM_THREADS 256
#define CM_MAX_ROWS 255          // rows of a block: their CM_MAX_ROWS + 1 offsets are searched by one thread each

#define CM_BAD_RANGE 1u          // status bits (eps_abi.h)
#define CM_BAD_ORDER 2u

static unsigned cm_blocks(int64_t n, int per_block)
{
    int64_t blocks = (n + per_block - 1) / per_block;
    const int64_t cap = (int64_t)eps_num_cus() * 16;
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

// (The searches below are eps_lower_bound.  Over col[] the key is a uint32_t, so ids compare as unsigned: a column taken from
// a key may be any 32 bits.)

// end of the run of keys equal to x[p] == key inside [p, hi): doubling steps, then a search between the last two probes (a
// pair that occurs once costs one load; every probe stays below hi whatever the keys hold)
__device__ __forceinline__ int64_t cm_run_end(const int64_t *__restrict__ x, int64_t p, int64_t hi, int64_t key)
{
    int64_t q = p + 1, step = 1;
    while (q + step <= hi && x[q + step - 1] == key) {
        q += step;
        step <<= 1;
    }
    int64_t lo = q, end = q + step - 1 < hi ? q + step - 1 : hi;
    while (lo < end) {
        const int64_t mid = (lo + end) >> 1;
        if (x[mid] == key) lo = mid + 1; else end = mid;
    }
    return lo;
}

// per key: range and order into the status word; flag = first of its run and absent from the base row
__global__ __launch_bounds__(CM_THREADS) void cm_flag_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                            int64_t n, const int64_t *__restrict__ x, int64_t m,
                                                            int32_t *__restrict__ flag, int32_t *__restrict__ xrank,
                                                            unsigned int *__restrict__ status)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += stride) {
        const int64_t key = x[p], row = key >> 32;
        const uint32_t c = (uint32_t)key;
        const int64_t prev = p ? x[p - 1] : key;
        unsigned bad = 0;
        if (row < 0 || row >= n || (int64_t)c >= n) bad |= CM_BAD_RANGE;
        if (prev > key) bad |= CM_BAD_ORDER;
        int32_t f = 0;
        if (!(bad & CM_BAD_RANGE) && (p == 0 || prev != key)) {
            const int64_t b = rowptr[row], e = rowptr[row + 1];
            const int64_t at = eps_lower_bound(col, b, e, c);
            f = !(at < e && (uint32_t)col[at] == c);
        }
        flag[p] = f;
        if (p == 0) xrank[0] = 0;
        if (bad) atomicOr(status, bad);          // (a refused batch only: nothing is added on the data path)
    }
}

// per row: its keys are [xs, xe) by two lower-bound searches; new_deg = deg + the new keys among them
__global__ __launch_bounds__(CM_THREADS) void cm_count_kernel(const int64_t *__restrict__ rowptr, int64_t n,
                                                             const int64_t *__restrict__ x, int64_t m,
                                                             const int32_t *__restrict__ xrank, int64_t *__restrict__ new_deg)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        int64_t d = rowptr[r + 1] - rowptr[r];
        if (m > 0) {
            const int64_t xs = eps_lower_bound(x, (int64_t)0, m, r << 32);
            const int64_t xe = eps_lower_bound(x, xs, m, (r + 1) << 32);
            d += xrank[xe] - xrank[xs];
        }
        new_deg[r] = d;
    }
}

// the base entries, a block of `rows_per_block` (<= CM_MAX_ROWS) consecutive rows per workgroup, flat over the block's entries
__global__ __launch_bounds__(CM_THREADS) void cm_fill_base_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                 const float *__restrict__ val, int64_t n,
                                                                 const int64_t *__restrict__ x, int64_t m,
                                                                 const int32_t *__restrict__ xrank,
                                                                 const int64_t *__restrict__ new_rowptr, int64_t new_nnz,
                                                                 int rows_per_block, int32_t *__restrict__ new_col,
                                                                 float *__restrict__ new_val)
{
    __shared__ int64_t s_b[CM_MAX_ROWS + 1];     // first entry of every row of the block, and the end of the last
    __shared__ int64_t s_nb[CM_MAX_ROWS + 1];    // ... in the new graph
    __shared__ int64_t s_xs[CM_MAX_ROWS + 1];    // first key of every row, and the end of the last row's
    const int tid = threadIdx.x;
    const int64_t n_blocks = (n + rows_per_block - 1) / rows_per_block;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t r0 = blk * rows_per_block;
        const int nr = (int)(n - r0 < rows_per_block ? n - r0 : rows_per_block);
        if (tid <= nr) {
            const int64_t r = r0 + tid;
            s_b[tid] = rowptr[r];
            s_nb[tid] = new_rowptr[r];
            s_xs[tid] = m > 0 ? eps_lower_bound(x, (int64_t)0, m, r << 32) : 0;
        }
        __syncthreads();
        const int64_t i_end = s_b[nr];
        for (int64_t i = s_b[0] + tid; i < i_end; i += CM_THREADS) {
            const int k = eps_lower_bound(s_b + 1, 0, nr - 1, i + 1);     // the row of entry i: the first k with s_b[k + 1] > i
            const int32_t c = col[i];
            float v = val ? val[i] : 1.0f;
            int64_t dest = s_nb[k] + (i - s_b[k]);
            const int64_t xs = s_xs[k], xe = s_xs[k + 1];
            if (xe > xs) {                       // the row receives keys: the new ones among those with a smaller column go in front
                const int64_t key = ((r0 + k) << 32) | (int64_t)(uint32_t)c;
                const int64_t p = eps_lower_bound(x, xs, xe, key);
                dest += xrank[p] - xrank[xs];
                if (new_val && p < xe && x[p] == key) v += (float)(cm_run_end(x, p, xe, key) - p);
            }
            if (dest >= 0 && dest < new_nnz) {   // (holds for the prefix of eps_csr_merge_count's degrees; anything else writes nothing)
                new_col[dest] = c;
                if (new_val) new_val[dest] = v;
            }
        }
        __syncthreads();
    }
}

// the new entries, one key per thread
__global__ __launch_bounds__(CM_THREADS) void cm_fill_new_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                int64_t n, const int64_t *__restrict__ x, int64_t m,
                                                                const int32_t *__restrict__ xrank,
                                                                const int64_t *__restrict__ new_rowptr, int64_t new_nnz,
                                                                int32_t *__restrict__ new_col, float *__restrict__ new_val)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += stride) {
        const int32_t g = xrank[p];
        if (xrank[p + 1] == g) continue;         // a repeat, or a pair the base row holds: its base entry took the multiplicity
        const int64_t key = x[p], row = key >> 32;
        if (row < 0 || row >= n) continue;
        const uint32_t c = (uint32_t)key;
        const int64_t dest = eps_lower_bound(col, rowptr[row], rowptr[row + 1], c) + g;
        if (dest < 0 || dest < new_rowptr[row] || dest >= new_rowptr[row + 1] || dest >= new_nnz) continue;
        new_col[dest] = (int32_t)c;
        if (new_val) new_val[dest] = (float)(cm_run_end(x, p, m, key) - p);
    }
}

static size_t cm_align(size_t b) { return (b + 255) & ~(size_t)255; }

static size_t cm_scan_temp(int64_t m)
{
    size_t t = 0;
    (void)rocprim::inclusive_scan((void *)nullptr, t, (const int32_t *)nullptr, (int32_t *)nullptr, (size_t)m, rocprim::plus<int32_t>(),
                                  (hipStream_t)0);
    return t;
}

extern "C" int64_t eps_csr_merge_workspace_bytes(int64_t m)
{
    if (m <= 0 || m >= (1ll << 31) - 1) return 256;
    return (int64_t)(cm_align((size_t)m * 4) + cm_align(cm_scan_temp(m)));
}

extern "C" int eps_csr_merge_count(const int64_t *rowptr, const int32_t *col, int64_t n, const int64_t *xkeys, int64_t m,
                                   int64_t *new_deg, int32_t *xrank, int32_t *status, void *workspace, int64_t workspace_bytes,
                                   void *stream)
{
    EPS_REQUIRE(n >= 0 && n < (1ll << 31), "eps_csr_merge_count: n=%lld must lie in [0, 2^31)", (long long)n);
    EPS_REQUIRE(m >= 0 && m < (1ll << 31) - 1, "eps_csr_merge_count: m=%lld must lie in [0, 2^31 - 1)", (long long)m);
    EPS_REQUIRE(rowptr, "eps_csr_merge_count: rowptr is null");
    EPS_REQUIRE(status, "eps_csr_merge_count: status is null");
    EPS_REQUIRE(n == 0 || new_deg, "eps_csr_merge_count: new_deg is null");
    EPS_REQUIRE(m == 0 || (xkeys && xrank && col), "eps_csr_merge_count: xkeys / xrank / col is null with m=%lld", (long long)m);
    EPS_REQUIRE(m == 0 || (workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= eps_csr_merge_workspace_bytes(m)),
                "eps_csr_merge_count: needs a 256-byte aligned workspace of eps_csr_merge_workspace_bytes(m) bytes");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) {
        eps_set_error("eps_csr_merge_count: cannot clear the status word");
        return EPS_ELAUNCH;
    }
    if (m > 0) {                                 // (m == 0: nothing below reads xkeys)
        int32_t *flag = (int32_t *)workspace;
        void *temp = (char *)workspace + cm_align((size_t)m * 4);
        size_t temp_bytes = cm_scan_temp(m);
        hipLaunchKernelGGL(cm_flag_kernel, dim3(cm_blocks(m, CM_THREADS)), dim3(CM_THREADS), 0, s, rowptr, col, n, xkeys, m, flag, xrank,
                           (unsigned int *)status);
        if (rocprim::inclusive_scan(temp, temp_bytes, flag, xrank + 1, (size_t)m, rocprim::plus<int32_t>(), s) != hipSuccess) {
            eps_set_error("eps_csr_merge_count: prefix sum failed");
            return EPS_ELAUNCH;
        }
    }
    if (n > 0)
        hipLaunchKernelGGL(cm_count_kernel, dim3(cm_blocks(n, CM_THREADS)), dim3(CM_THREADS), 0, s, rowptr, n, xkeys, m, xrank, new_deg);
    EPS_CHECK_LAUNCH("eps_csr_merge_count");
    return EPS_OK;
}

extern "C" int eps_csr_merge_fill(const int64_t *rowptr, const int32_t *col, const float *val_or_null, int64_t n,
                                  const int64_t *xkeys, int64_t m, const int32_t *xrank, const int64_t *new_rowptr, int64_t new_nnz,
                                  int32_t *new_col, float *new_val_or_null, void *stream)
{
    EPS_REQUIRE(n >= 0 && n < (1ll << 31), "eps_csr_merge_fill: n=%lld must lie in [0, 2^31)", (long long)n);
    EPS_REQUIRE(m >= 0 && m < (1ll << 31) - 1, "eps_csr_merge_fill: m=%lld must lie in [0, 2^31 - 1)", (long long)m);
    EPS_REQUIRE(new_nnz >= 0, "eps_csr_merge_fill: new_nnz=%lld is negative", (long long)new_nnz);
    EPS_REQUIRE(rowptr, "eps_csr_merge_fill: rowptr is null");
    EPS_REQUIRE(new_rowptr, "eps_csr_merge_fill: new_rowptr is null");
    EPS_REQUIRE(m == 0 || (xkeys && xrank), "eps_csr_merge_fill: xkeys / xrank is null with m=%lld", (long long)m);
    if (n == 0 || new_nnz == 0) return EPS_OK;
    EPS_REQUIRE(col && new_col, "eps_csr_merge_fill: col / new_col is null");
    hipStream_t s = (hipStream_t)stream;
    // rows per workgroup: about eight workgroups per CU when the graph has the rows for it
    int64_t rows = (n + (int64_t)eps_num_cus() * 8 - 1) / ((int64_t)eps_num_cus() * 8);
    if (rows > CM_MAX_ROWS) rows = CM_MAX_ROWS;
    int64_t blocks = (n + rows - 1) / rows;
    if (blocks > (1ll << 20)) blocks = 1ll << 20;
    hipLaunchKernelGGL(cm_fill_base_kernel, dim3((unsigned)blocks), dim3(CM_THREADS), 0, s, rowptr, col, val_or_null, n, xkeys, m, xrank,
                       new_rowptr, new_nnz, (int)rows, new_col, new_val_or_null);
    if (m > 0)
        hipLaunchKernelGGL(cm_fill_new_kernel, dim3(cm_blocks(m, CM_THREADS)), dim3(CM_THREADS), 0, s, rowptr, col, n, xkeys, m, xrank,
                           new_rowptr, new_nnz, new_col, new_val_or_null);
    EPS_CHECK_LAUNCH("eps_csr_merge_fill");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void csr_merge_warm_kernel() {}
extern "C" void eps_warm_csr_merge(void *stream) { hipLaunchKernelGGL(csr_merge_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

// Subgraph sketches (ELPH / BUDDY, Chamberlain et al., ICLR 2023), gfx950: a HyperLogLog (256 one-byte registers) and a MinHash
// (128 uint32 words) sketch per node and hop, and the pair statistics read off four such rows.  All arithmetic is integer: the
// tables and the statistics are functions of the sets alone and are held to a numpy restatement bit for bit.
//
//   own        one wave per id: lane l writes register dword l and the words l and 64 + l (768 B per id, plain stores).
//   propagate  out[v] = union of in[w] over the stored entries w of row v (byte-wise max / word-wise min), a gather of 768-B rows:
//              one wave per destination, lane l holds register dword l and the words 2l, 2l + 1; the ids of 64 entries are fetched
//              by one load, then four neighbour rows are in flight per wave.  A row longer than SK_ROW_CHUNK entries does not run
//              on one wave: the ENTRY array is cut at the multiples of SK_ROW_CHUNK, the wave of a cut piece reduces the part(s)
//              of long rows inside it into a partial table (two slots per piece: a long row's tail and the next one's head), and
//              the row's own wave then unions its slots instead of its neighbours.  The union is idempotent and order-free, so
//              the result does not depend on the cut; every slot is written in full by exactly one wave before it is read.  No
//              atomics.
//   pair stats sixteen lanes per pair, four pairs per wave: a lane loads 16 B of each register row and 2 x 16 B of each word row,
//              forms its share of S = sum 2^(33 - M_r), Z = #{M_r == 0} and the word matches for the K^2 hop combinations as ONE
//              packed int64 each (S bits 0..41, Z 42..50, matches 51..58: no field can carry into the next), and K^2 sixteen-lane
//              DPP reductions finish the pair.
#include "eps_common.h"

#define SK_REGS 256           // HyperLogLog registers per sketch, one byte each
#define SK_WORDS 128          // MinHash words per sketch
#define SK_ROW_CHUNK 512      // entries per cut piece: rows longer than this are reduced piecewise by separate waves
#define SK_PAIRS_PER_WAVE 4   // sixteen lanes per pair
#define SK_WAVES 4            // waves per workgroup
#define SK_MAX_RANK 33

typedef unsigned short sk_u16x2 __attribute__((ext_vector_type(2)));

__host__ __device__ static inline uint64_t sk_mix64(uint64_t x)   // the splitmix64 finaliser
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// byte-wise unsigned max of two dwords: there is no packed byte max, so the even and the odd bytes go through one u16x2 max each
__device__ __forceinline__ uint32_t sk_bytemax(uint32_t a, uint32_t b)
{
    const sk_u16x2 e = __builtin_elementwise_max(__builtin_bit_cast(sk_u16x2, a & 0x00FF00FFu), __builtin_bit_cast(sk_u16x2, b & 0x00FF00FFu));
    const sk_u16x2 o = __builtin_elementwise_max(__builtin_bit_cast(sk_u16x2, (a >> 8) & 0x00FF00FFu),
                                                 __builtin_bit_cast(sk_u16x2, (b >> 8) & 0x00FF00FFu));
    return __builtin_bit_cast(uint32_t, e) | (__builtin_bit_cast(uint32_t, o) << 8);
}

// ------------------------------------------------------------------------------------------------------------------ own sketches
__global__ __launch_bounds__(SK_WAVES * 64) void sketch_own_kernel(int64_t first_id, int64_t n, uint32_t *__restrict__ hll,
                                                                   uint32_t *__restrict__ mh)
{
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * SK_WAVES;
    for (int64_t i = (int64_t)blockIdx.x * SK_WAVES + (threadIdx.x >> 6); i < n; i += n_waves) {
        const uint64_t x = (uint64_t)(first_id + i);
        const uint64_t h = sk_mix64(x);
        const int idx = (int)(h >> 56);
        const uint32_t w = (uint32_t)(h >> 24);
        const uint32_t rank = w == 0 ? SK_MAX_RANK : (uint32_t)__builtin_clz(w) + 1u;
        hll[i * (SK_REGS / 4) + lane] = (idx >> 2) == lane ? rank << (8 * (idx & 3)) : 0u;
        mh[i * SK_WORDS + lane] = (uint32_t)sk_mix64(x ^ ((uint64_t)(lane + 1) << 32));
        mh[i * SK_WORDS + 64 + lane] = (uint32_t)sk_mix64(x ^ ((uint64_t)(lane + 65) << 32));
    }
}

// -------------------------------------------------------------------------------------------------------------------- propagate
struct SkAcc {
    uint32_t h;               // register dword `lane`
    uint2 m;                  // words 2 lane, 2 lane + 1
};

__device__ __forceinline__ void sk_merge(SkAcc &a, const uint32_t h, const uint2 m)
{
    a.h = sk_bytemax(a.h, h);
    a.m.x = a.m.x < m.x ? a.m.x : m.x;
    a.m.y = a.m.y < m.y ? a.m.y : m.y;
}

// union of up to four rows (ids r[0..3], wave-uniform; an id outside [0, n_tab) is skipped and nothing is read for it) into acc:
// the loads of all four are issued before the first is merged
__device__ __forceinline__ void sk_gather4(SkAcc &acc, const uint32_t *__restrict__ th, const uint2 *__restrict__ tm, const int64_t n_tab,
                                           const int64_t r0, const int64_t r1, const int64_t r2, const int64_t r3, const int lane)
{
    const int64_t r[4] = {r0, r1, r2, r3};
    uint32_t h[4];
    uint2 m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        h[k] = 0u;
        m[k] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        if (r[k] >= 0 && r[k] < n_tab) {                      // wave-uniform
            h[k] = th[r[k] * (SK_REGS / 4) + lane];
            m[k] = tm[r[k] * (SK_WORDS / 2) + lane];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) sk_merge(acc, h[k], m[k]);
}

// union of in[w] over the entries col[beg .. end) into acc
__device__ __forceinline__ void sk_gather_entries(SkAcc &acc, const int32_t *__restrict__ col, const int64_t beg, const int64_t end,
                                                  const uint32_t *__restrict__ th, const uint2 *__restrict__ tm, const int64_t n_tab,
                                                  const int lane)
{
    for (int64_t e0 = beg; e0 < end; e0 += 64) {
        const int cnt = end - e0 < 64 ? (int)(end - e0) : 64;
        const int32_t mine = lane < cnt ? col[e0 + lane] : -1;
        for (int j = 0; j < cnt; j += 4)                      // (lanes past cnt hold -1: skipped)
            sk_gather4(acc, th, tm, n_tab, __builtin_amdgcn_readlane(mine, j), __builtin_amdgcn_readlane(mine, j + 1),
                       __builtin_amdgcn_readlane(mine, j + 2), __builtin_amdgcn_readlane(mine, j + 3), lane);
    }
}

__device__ __forceinline__ int64_t sk_clamp(int64_t x, int64_t hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

// the last row r in [0, n_rows] with rowptr[r] <= e (rowptr ascends from 0; an inconsistent rowptr only moves the answer)
__device__ __forceinline__ int64_t sk_row_of(const int64_t *__restrict__ rowptr, const int64_t n_rows, const int64_t e)
{
    int64_t lo = 0, hi = n_rows + 1;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (rowptr[mid] <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

// one wave per cut piece j of the entry array: the part(s) of LONG rows inside [j RC, (j + 1) RC) go to the partial slots 2 j (a
// row that began in an earlier piece) and 2 j + 1 (a row that begins in this one)
__global__ __launch_bounds__(SK_WAVES * 64) void sketch_propagate_pieces_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t n_rows, int64_t nnz, const uint32_t *__restrict__ hin,
    const uint2 *__restrict__ min_, uint32_t *__restrict__ part_h, uint2 *__restrict__ part_m, int64_t n_pieces)
{
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * SK_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (j >= n_pieces) return;
    const int64_t lo = j * SK_ROW_CHUNK, hi = lo + SK_ROW_CHUNK < nnz ? lo + SK_ROW_CHUNK : nnz;
    const int64_t v0 = sk_row_of(rowptr, n_rows, lo), v1 = sk_row_of(rowptr, n_rows, hi - 1);
    for (int side = 0; side < 2; ++side) {
        const int64_t v = side ? v1 : v0;
        if (v >= n_rows || (side && v1 == v0)) continue;
        const int64_t b = sk_clamp(rowptr[v], nnz), e = sk_clamp(rowptr[v + 1], nnz);
        if (e - b <= SK_ROW_CHUNK) continue;                  // a short row is its own wave's work
        const int64_t pb = b > lo ? b : lo, pe = e < hi ? e : hi;
        if (pb >= pe) continue;
        const int64_t slot = 2 * j + (b >= lo ? 1 : 0);
        SkAcc acc = {0u, make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu)};
        sk_gather_entries(acc, col, pb, pe, hin, min_, n_rows, lane);
        part_h[slot * (SK_REGS / 4) + lane] = acc.h;
        part_m[slot * (SK_WORDS / 2) + lane] = acc.m;
    }
}

// one wave per destination row: its neighbours, or for a long row its partial slots
__global__ __launch_bounds__(SK_WAVES * 64) void sketch_propagate_rows_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t n_rows, int64_t nnz, const uint32_t *__restrict__ hin,
    const uint2 *__restrict__ min_, uint32_t *__restrict__ hout, uint2 *__restrict__ mout, int keep_own,
    const uint32_t *__restrict__ part_h, const uint2 *__restrict__ part_m, int64_t n_pieces)
{
    const int lane = threadIdx.x & 63;
    const int64_t v = (int64_t)blockIdx.x * SK_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (v >= n_rows) return;
    const int64_t b = sk_clamp(rowptr[v], nnz), e = sk_clamp(rowptr[v + 1], nnz);
    SkAcc acc = {0u, make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu)};
    if (keep_own) {
        acc.h = hin[v * (SK_REGS / 4) + lane];
        acc.m = min_[v * (SK_WORDS / 2) + lane];
    }
    if (e - b <= SK_ROW_CHUNK) {
        sk_gather_entries(acc, col, b, e, hin, min_, n_rows, lane);
    } else {
        const int64_t j0 = b / SK_ROW_CHUNK, j1 = (e - 1) / SK_ROW_CHUNK;
        for (int64_t j = j0; j <= j1; j += 4) {
            const int64_t s0 = 2 * j + (j == j0 ? 1 : 0);     // (the piece the row begins in; every later one holds its tail slot)
            sk_gather4(acc, part_h, part_m, 2 * n_pieces, s0, j + 1 <= j1 ? 2 * (j + 1) : -1, j + 2 <= j1 ? 2 * (j + 2) : -1,
                       j + 3 <= j1 ? 2 * (j + 3) : -1, lane);
        }
    }
    hout[v * (SK_REGS / 4) + lane] = acc.h;
    mout[v * (SK_WORDS / 2) + lane] = acc.m;
}

// ------------------------------------------------------------------------------------------------------------------- pair stats
__device__ __forceinline__ uint64_t sk_sum16(uint64_t x)        // all sixteen lanes of a DPP row receive the row's total
{
#define SK_STEP(CTRL)                                                                                       \
    x += ((uint64_t)(uint32_t)eps_dpp_i<CTRL>((int)(uint32_t)(x >> 32)) << 32) | (uint32_t)eps_dpp_i<CTRL>((int)(uint32_t)x);
    SK_STEP(0xB1)    // quad_perm [1,0,3,2]
    SK_STEP(0x4E)    // quad_perm [2,3,0,1]
    SK_STEP(0x141)   // row_half_mirror
    SK_STEP(0x140)   // row_mirror
#undef SK_STEP
    return x;
}

// a lane's share of one hop combination: sixteen registers and eight words of each side, packed
__device__ __forceinline__ uint64_t sk_share(const uint4 hu, const uint4 hv, const uint4 mu0, const uint4 mu1, const uint4 mv0,
                                             const uint4 mv1)
{
    const uint32_t a[4] = {hu.x, hu.y, hu.z, hu.w}, b[4] = {hv.x, hv.y, hv.z, hv.w};
    uint64_t s = 0;
    uint32_t z = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t M = sk_bytemax(a[d], b[d]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t m = (M >> (8 * k)) & 0xFFu;
            z += m == 0u;
            s += m <= SK_MAX_RANK ? 1ull << (SK_MAX_RANK - m) : 0ull;   // (a register above 33 is no rank: it adds nothing)
        }
    }
    const uint32_t match = (mu0.x == mv0.x) + (mu0.y == mv0.y) + (mu0.z == mv0.z) + (mu0.w == mv0.w) + (mu1.x == mv1.x) +
                           (mu1.y == mv1.y) + (mu1.z == mv1.z) + (mu1.w == mv1.w);
    return s | ((uint64_t)z << 42) | ((uint64_t)match << 51);
}

template <int K>
__global__ __launch_bounds__(SK_WAVES * 64) void sketch_pair_stats_kernel(const uint8_t *__restrict__ hll, const uint32_t *__restrict__ mh,
                                                                          int64_t n_rows, const int32_t *__restrict__ pu,
                                                                          const int32_t *__restrict__ pv, int64_t n_pairs,
                                                                          int64_t *__restrict__ stat)
{
    const int g = threadIdx.x & 15;
    const int64_t n_groups = (int64_t)gridDim.x * (SK_WAVES * SK_PAIRS_PER_WAVE);
    for (int64_t p = (int64_t)blockIdx.x * (SK_WAVES * SK_PAIRS_PER_WAVE) + (threadIdx.x >> 4); p < n_pairs; p += n_groups) {
        const int64_t nu = pu[p], nv = pv[p];
        if (nu < 0 || nv < 0 || nu >= n_rows || nv >= n_rows) {   // (uniform over the pair's sixteen lanes) reads nothing
            if (g < K * K) stat[p * (K * K) + g] = -1;
            continue;
        }
        uint4 hu[K], hv[K], mu[K][2], mv[K][2];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint4 *ru = reinterpret_cast<const uint4 *>(hll + ((int64_t)k * n_rows + nu) * SK_REGS);
            const uint4 *rv = reinterpret_cast<const uint4 *>(hll + ((int64_t)k * n_rows + nv) * SK_REGS);
            const uint4 *wu = reinterpret_cast<const uint4 *>(mh + ((int64_t)k * n_rows + nu) * SK_WORDS);
            const uint4 *wv = reinterpret_cast<const uint4 *>(mh + ((int64_t)k * n_rows + nv) * SK_WORDS);
            hu[k] = ru[g]; hv[k] = rv[g];
            mu[k][0] = wu[g]; mu[k][1] = wu[16 + g];          // (a sixteen-lane group reads contiguous 256-B pieces)
            mv[k][0] = wv[g]; mv[k][1] = wv[16 + g];
        }
        uint64_t mine = 0;
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint64_t t = sk_sum16(sk_share(hu[i], hv[j], mu[i][0], mu[i][1], mv[j][0], mv[j][1]));
                if (g == i * K + j) mine = t;
            }
        if (g < K * K) stat[p * (K * K) + g] = (int64_t)mine;
    }
}

// ------------------------------------------------------------------------------------------------------------------ entry points
static unsigned sk_blocks(int64_t items, int64_t per_block)
{
    int64_t blocks = (items + per_block - 1) / per_block;
    const int64_t cap = 1ll << 22;                            // (the grid-stride kernels take the rest in further trips)
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

static bool sk_overlap(const void *a, int64_t a_bytes, const void *b, int64_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    if (a0 == b0) return true;
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

extern "C" int eps_sketch_limits(int32_t *row_chunk, int32_t *pairs_per_wave)
{
    if (row_chunk) *row_chunk = SK_ROW_CHUNK;
    if (pairs_per_wave) *pairs_per_wave = SK_PAIRS_PER_WAVE;
    return EPS_OK;
}

extern "C" int eps_sketch_own(int64_t first_id, int64_t n, uint8_t *hll, uint32_t *mh, void *stream)
{
    EPS_REQUIRE(hll && mh, "eps_sketch_own: null pointer");
    EPS_REQUIRE(n >= 0 && first_id >= 0 && first_id <= (1ll << 31) && n <= (1ll << 31) - first_id,
                "eps_sketch_own: ids must lie in [0, 2^31) (first_id=%lld n=%lld)", (long long)first_id, (long long)n);
    EPS_REQUIRE(((uintptr_t)hll & 15) == 0 && ((uintptr_t)mh & 15) == 0, "eps_sketch_own: the tables must be 16-byte aligned");
    if (n == 0) return EPS_OK;
    hipLaunchKernelGGL(sketch_own_kernel, dim3(sk_blocks(n, SK_WAVES)), dim3(SK_WAVES * 64), 0, (hipStream_t)stream, first_id, n,
                       reinterpret_cast<uint32_t *>(hll), mh);
    EPS_CHECK_LAUNCH("eps_sketch_own");
    return EPS_OK;
}

static int64_t sk_pieces(int64_t nnz) { return nnz <= 0 ? 0 : (nnz + SK_ROW_CHUNK - 1) / SK_ROW_CHUNK; }

extern "C" int64_t eps_sketch_propagate_workspace_bytes(int64_t nnz)
{
    return 2 * sk_pieces(nnz) * (int64_t)(SK_REGS + 4 * SK_WORDS) + 256;   // (two partial slots per cut piece)
}

extern "C" int eps_sketch_propagate(const int64_t *rowptr, const int32_t *col, int64_t n_rows, int64_t nnz, const uint8_t *hll_in,
                                    const uint32_t *mh_in, uint8_t *hll_out, uint32_t *mh_out, int keep_own, void *workspace,
                                    int64_t workspace_bytes, void *stream)
{
    EPS_REQUIRE(rowptr && hll_in && mh_in && hll_out && mh_out && (nnz <= 0 || col), "eps_sketch_propagate: null pointer");
    EPS_REQUIRE(n_rows >= 0 && n_rows <= (1ll << 31) && nnz >= 0, "eps_sketch_propagate: bad size (n_rows=%lld nnz=%lld)",
                (long long)n_rows, (long long)nnz);
    EPS_REQUIRE(!sk_overlap(hll_out, n_rows * SK_REGS, hll_in, n_rows * SK_REGS) &&
                    !sk_overlap(mh_out, n_rows * SK_WORDS * 4, mh_in, n_rows * SK_WORDS * 4),
                "eps_sketch_propagate: hll_out / mh_out must not alias their inputs (a row is read after other rows are written)");
    EPS_REQUIRE((((uintptr_t)hll_in | (uintptr_t)mh_in | (uintptr_t)hll_out | (uintptr_t)mh_out) & 15) == 0,
                "eps_sketch_propagate: the tables must be 16-byte aligned");
    const int64_t n_pieces = sk_pieces(nnz);
    EPS_REQUIRE(n_pieces == 0 || (workspace && ((uintptr_t)workspace & 255) == 0 &&
                                  workspace_bytes >= eps_sketch_propagate_workspace_bytes(nnz)),
                "eps_sketch_propagate: needs a 256-byte aligned workspace of eps_sketch_propagate_workspace_bytes(nnz) bytes");
    if (n_rows == 0) return EPS_OK;
    hipStream_t s = (hipStream_t)stream;
    uint32_t *part_h = (uint32_t *)workspace;
    uint2 *part_m = (uint2 *)((char *)workspace + 2 * n_pieces * SK_REGS);
    const uint32_t *hin = reinterpret_cast<const uint32_t *>(hll_in);
    const uint2 *min_ = reinterpret_cast<const uint2 *>(mh_in);
    EPS_REQUIRE((n_pieces + SK_WAVES - 1) / SK_WAVES < (1ll << 31), "eps_sketch_propagate: nnz=%lld is beyond one launch", (long long)nnz);
    if (n_pieces)
        hipLaunchKernelGGL(sketch_propagate_pieces_kernel, dim3((unsigned)((n_pieces + SK_WAVES - 1) / SK_WAVES)), dim3(SK_WAVES * 64), 0, s,
                           rowptr, col, n_rows, nnz, hin, min_, part_h, part_m, n_pieces);
    hipLaunchKernelGGL(sketch_propagate_rows_kernel, dim3((unsigned)((n_rows + SK_WAVES - 1) / SK_WAVES)), dim3(SK_WAVES * 64), 0, s, rowptr,
                       col, n_rows, nnz, hin, min_, reinterpret_cast<uint32_t *>(hll_out), reinterpret_cast<uint2 *>(mh_out), keep_own,
                       (const uint32_t *)part_h, (const uint2 *)part_m, n_pieces);
    EPS_CHECK_LAUNCH("eps_sketch_propagate");
    return EPS_OK;
}

extern "C" int eps_sketch_pair_stats(const uint8_t *hll, const uint32_t *mh, int K, int64_t n_rows, const int32_t *u, const int32_t *v,
                                     int64_t n_pairs, int64_t *stat, void *stream)
{
    EPS_REQUIRE(hll && mh && u && v && stat, "eps_sketch_pair_stats: null pointer");
    EPS_REQUIRE(K == 1 || K == 2, "eps_sketch_pair_stats: K=%d hops: 1 or 2", K);
    EPS_REQUIRE(n_rows >= 0 && n_rows <= (1ll << 31) && n_pairs >= 0, "eps_sketch_pair_stats: bad size (n_rows=%lld n_pairs=%lld)",
                (long long)n_rows, (long long)n_pairs);
    EPS_REQUIRE((((uintptr_t)hll | (uintptr_t)mh) & 15) == 0, "eps_sketch_pair_stats: the tables must be 16-byte aligned");
    if (n_pairs == 0) return EPS_OK;
    const unsigned blocks = sk_blocks(n_pairs, SK_WAVES * SK_PAIRS_PER_WAVE);
    if (K == 1)
        hipLaunchKernelGGL(sketch_pair_stats_kernel<1>, dim3(blocks), dim3(SK_WAVES * 64), 0, (hipStream_t)stream, hll, mh, n_rows, u, v,
                           n_pairs, stat);
    else
        hipLaunchKernelGGL(sketch_pair_stats_kernel<2>, dim3(blocks), dim3(SK_WAVES * 64), 0, (hipStream_t)stream, hll, mh, n_rows, u, v,
                           n_pairs, stat);
    EPS_CHECK_LAUNCH("eps_sketch_pair_stats");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void sketch_warm_kernel() {}
extern "C" void eps_warm_sketch(void *stream) { hipLaunchKernelGGL(sketch_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

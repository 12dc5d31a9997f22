// Exact re-scoring of the screened survivors, gfx950: the few candidates that pass the one-pass scan's screening sums
// (scan_pieces.hip: K of 10^10) get the exact score of filter_scan.hip / expand_score.hip -- the final list is bit-identical.
//
// The survivors of a scan are pairs of hubs: a few thousand nodes u recur in hundreds of pairs each.  The list comes sorted by
// (u, v) as keys (u << 32) | v; a workgroup takes 256 consecutive pairs, and for every run of equal u inside them turns N(u)
// into an LDS bitmap over the id space (windows of RS_BITS ids when the space is wider), streams the short rows N(v) of the
// run against it -- one wave per pair, coalesced -- and sums the exact weights of the hits in float64.  The weights are
// multiples of 2^-40 below 2^12, so the float64 sum is exact whatever the order: (float)sum is eps_filter_scan's score, bit
// for bit (adamic_utils.py:13-25 / train_and_eval.py:195-216 / models.py:536-542 with the engine's fixed-point definition).
#include "eps_common.h"

#define RS_THREADS 1024
#define RS_CHUNK 256
#define RS_BITS (1 << 20)       // ids per bitmap window: 128 KiB of LDS
#define RS_SHORT 512            // rows up to this long go through rescore_short_kernel
#define RS_GROUP 128            // consecutive 256-pair chunks that go to the same XCD (32 k pairs: most of a block of 2^9 v)
#define RS_MINW 8               // waves per SIMD the kernel is compiled for: 8 = two 1024-thread workgroups per CU (<= 64 VGPRs)
#define RS_NB 8                 // entries of N(v) a lane takes per trip: two 16-byte row loads issued together, then eight bitmap
                                // words read together (the survivors' rows are long, ~1100 entries on the ppa-like graph: 2.3 G
                                // entries to stream for 2 M pairs)

// One trip of a lane: the eight entries of its two row loads against the bitmap of N(u), the weights of the hits summed.
//  * The eight bitmap words are read unconditionally, all before the first wait: an entry beyond the row's end or outside the id
//    window reads some valid word and its predicate drops the bit.  (The empty asm keeps the word index and the scaled add of the
//    LDS address apart: shift + v_lshl_add, where the compiler otherwise makes shift, mask and add of them.)
//  * A weight is loaded only by the lanes that hit, each entry under its own exec mask, and nothing waits before the last of the
//    eight is issued: the adds come at the end.  The straight-line form -- every lane loads, a lane without a hit from an offset
//    beyond the descriptor -- measured 340 us SLOWER per call on the bench graph (1645 against 1305 us; NOTES, "Re-scoring
//    trips"): it seems a buffer load whose lanes are all out of range still costs its slot in the vector-memory pipeline, and
//    most of a trip's entries do not hit.
//  * rem = the entries the row has left from the lane's first one.  A lane beyond the end got zeros from the col descriptor,
//    i.e. id 0 -- the heaviest hub, which IS in most N(u) -- so rem stays in the hit.
//  * fix_rs: a descriptor over the weights of the id window, so a hit's byte offset is x * 8 < 2^23 whatever n_nodes is.
// WIN = the id space is wider than one window (otherwise x = w, and the window subtraction, clamp and test are dead).
template <bool WIN>
static __device__ __forceinline__ long long rs_trip(const uint32_t *bm, __amdgpu_buffer_rsrc_t fix_rs, int32_t wlo, v4i w0, v4i w1,
                                                    int rem)
{
    uint32_t x[RS_NB], word[RS_NB];
#pragma unroll
    for (int b = 0; b < RS_NB; ++b) {
        const int32_t w = b < 4 ? w0[b & 3] : w1[b & 3];
        x[b] = WIN ? (uint32_t)(w - wlo) : (uint32_t)w;
        const uint32_t xa = WIN ? (x[b] < (uint32_t)RS_BITS ? x[b] : (uint32_t)RS_BITS - 1u) : x[b];
        uint32_t wi = xa >> 5;
        asm("" : "+v"(wi));                // (see above: not volatile, it only pins the value)
        word[b] = bm[wi];
    }
    typedef int v2i __attribute__((ext_vector_type(2)));
    v2i add[RS_NB];
#pragma unroll
    for (int b = 0; b < RS_NB; ++b) {
        bool hit = (((word[b] >> (x[b] & 31u)) & 1u) != 0u) & (rem > (b >> 2) * 128 + (b & 3));
        if (WIN) hit &= x[b] < (uint32_t)RS_BITS;
        add[b] = v2i{0, 0};
        if (hit) add[b] = __builtin_amdgcn_raw_buffer_load_b64(fix_rs, (int)(x[b] * 8u), 0, 0);
    }
    long long acc = 0ll;
#pragma unroll
    for (int b = 0; b < RS_NB; ++b) acc += (long long)(((unsigned long long)(uint32_t)add[b][1] << 32) | (uint32_t)add[b][0]);
    return acc;
}

// A lane's 16-byte row load at byte offset ofs of col[], if the row has entries left there (otherwise zeros, no bytes moved).
static __device__ __forceinline__ v4i rs_row_load(__amdgpu_buffer_rsrc_t col_rs, uint32_t ofs, bool inside)
{
    return __builtin_amdgcn_raw_buffer_load_b128(col_rs, (int)(inside ? ofs : 0xFFFFFFF0u), 0, 0);
}

template <bool WIN>
__global__ __launch_bounds__(RS_THREADS, RS_MINW) void rescore_runs_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                 const int64_t *__restrict__ fixw, int32_t n_nodes,
                                                                 const int64_t *__restrict__ keys, int64_t n,
                                                                 float *__restrict__ out, unsigned int *__restrict__ next_chunk,
                                                                 const int64_t *__restrict__ n_dev)
{
    if (n_dev) {                 // (r06: the list's length lives on the device -- the sorts in front read it there too)
        const int64_t c = *n_dev;
        n = c < 0 ? 0 : (c < n ? c : n);
    }
    extern __shared__ __attribute__((aligned(16))) uint32_t bm[];          // RS_BITS / 32 words
    __shared__ unsigned long long s_starts[RS_CHUNK / 64];
    __shared__ long long s_sum[RS_CHUNK];
    __shared__ uint32_t s_vb[RS_CHUNK], s_vl[RS_CHUNK];                    // the chunk's rows N(v): first entry, length
    __shared__ unsigned int s_c;
    const int tid = threadIdx.x, lane = tid & 63, wib = tid >> 6;
    constexpr int W = RS_THREADS / 64;
    const int words = (n_nodes < RS_BITS ? (n_nodes + 31) >> 5 : RS_BITS >> 5);
    // (one descriptor over all of col[]: 16-byte loads at 4-byte-aligned offsets, out-of-range lanes read zeros at a far offset)
    const __amdgpu_buffer_rsrc_t col_rs = eps_raw_rsrc(col, (int)(uint32_t)(rowptr[n_nodes] * 4));
    for (int i = tid; i < words; i += RS_THREADS) bm[i] = 0u;
    const int64_t n_chunks = (n + RS_CHUNK - 1) / RS_CHUNK;
    // XCD-aware hand-out (r05).  The pairs come sorted by (block of 2^9 consecutive v, u, v): neighbouring chunks stream the rows of
    // the same few hundred v -- 2 MB, which an XCD's 4 MB of L2 holds, if the workgroups of that XCD work on the same chunks.  So
    // groups of RS_GROUP consecutive chunks are dealt round-robin over the eight XCDs, each XCD draws from ITS counter (the id from
    // HW_REG_XCC_ID: blockIdx says which blocks share an XCD, not which), and an XCD that runs out helps the next one.  Placement is
    // speed only: any workgroup may score any chunk.
    unsigned int xcc = 0;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcc &= 7u;
    for (;;) {
        if (tid == 0) {
            unsigned int got = 0xFFFFFFFFu;
            for (unsigned int j = 0; j < 8u; ++j) {
                const unsigned int y = (xcc + j) & 7u;
                const unsigned int t = atomicAdd(&next_chunk[y], 1u);
                const unsigned long long c = ((unsigned long long)(t / RS_GROUP) * 8ull + y) * RS_GROUP + t % RS_GROUP;
                if (c < (unsigned long long)n_chunks) {
                    got = (unsigned int)c;
                    break;
                }
            }
            s_c = got;
        }
        __syncthreads();
        const int64_t c = s_c == 0xFFFFFFFFu ? n_chunks : (int64_t)s_c;
        if (c >= n_chunks) break;
        const int64_t c0 = c * RS_CHUNK;
        const int cn = (int)(n - c0 < RS_CHUNK ? n - c0 : RS_CHUNK);
        // The chunk's descriptors, once: thread t loads key t and the rowptr words of its v and its u -- 256 chains of two
        // latencies side by side -- and leaves (first entry, length) of N(v) in LDS, so that a pair's first row load starts from
        // two LDS words.  The same key gives the run starts, and the thread remembers whether its pair is this kernel's.
        bool my_long = false;
        if (tid < RS_CHUNK) {
            s_sum[tid] = 0ll;
            const bool have = tid < cn;
            const int64_t key = keys[c0 + (have ? tid : 0)];
            const int32_t u = (int32_t)(key >> 32), v = (int32_t)(key & 0xFFFFFFFFll);
            int32_t pu = __shfl_up(u, 1);                    // (the wave's first lane reads its predecessor's key itself)
            if (lane == 0 && tid > 0 && have) pu = (int32_t)(keys[c0 + tid - 1] >> 32);
            const bool start = have && (tid == 0 || u != pu);
            uint32_t vb = 0u, vl = 0u;
            if (have) {
                // (32-bit entry indices: nnz < 2^30)
                vb = (uint32_t)rowptr[v];
                vl = (uint32_t)rowptr[v + 1] - vb;
                my_long = rowptr[u + 1] - rowptr[u] > RS_SHORT;
            }
            s_vb[tid] = vb;
            s_vl[tid] = vl;
            const unsigned long long m = __ballot(start);
            if (lane == 0) s_starts[wib] = m;
        }
        __syncthreads();
        int s = 0;
        while (s < cn) {
            // end of the run that starts at s: the next start bit after s
            int e = cn;
            for (int q = s >> 6; q < RS_CHUNK / 64; ++q) {
                unsigned long long m = s_starts[q];
                if (q == (s >> 6)) m &= (s & 63) == 63 ? 0ull : ~0ull << ((s & 63) + 1);
                if (m) {
                    e = q * 64 + __builtin_ctzll(m);
                    break;
                }
            }
            if (e > cn) e = cn;
            const int32_t u = (int32_t)(keys[c0 + s] >> 32);
            const int64_t ub = rowptr[u], ue = rowptr[u + 1];
            if (ue - ub <= RS_SHORT) {        // a short row: its pairs are rescore_short_kernel's (no bitmap, no barriers)
                s = e;
                continue;
            }
            for (int32_t wlo = 0; wlo < (WIN ? n_nodes : 1); wlo += RS_BITS) {
                // N(u) inside the id window -> bits (rows ascend; a plain scan of the row is cheap next to the pairs)
                for (uint32_t i = (uint32_t)ub + tid; i < (uint32_t)ue; i += RS_THREADS) {     // (nnz < 2^30)
                    const uint32_t x = (uint32_t)(col[i] - wlo);
                    if (!WIN || x < (uint32_t)RS_BITS) atomicOr(&bm[x >> 5], 1u << (x & 31));
                }
                __syncthreads();
                // (the window's weights: at most RS_BITS * 8 bytes)
                const int32_t wn = n_nodes - wlo < RS_BITS ? n_nodes - wlo : RS_BITS;
                const __amdgpu_buffer_rsrc_t fix_rs = eps_raw_rsrc(fixw + wlo, wn * 8);
                // two pairs per wave, one per half: a half wave covers 256 entries of its row N(v) per trip -- two 16-byte loads a
                // lane (a quarter of the vector-memory instructions of one-entry loads for the same bytes: the rows are what this
                // kernel streams, 8.8 GB per step on the bench graph) -- and the trip count is the longer row's, wave-uniform.
                // A trip is three dependent latencies (rows, bitmap words, weights); the other waves of the CU hide them.  Loading
                // the next trip's rows under the current trip's look-ups needs more than 64 VGPRs without scratch, and measured
                // slower where it was tried (NOTES, "Re-scoring trips").
                for (int p0 = s + 2 * wib; p0 < e; p0 += 2 * W) {
                    const int pi = p0 + (lane >> 5);
                    const bool live = pi < e;
                    const int hl = lane & 31;
                    const uint32_t vb = s_vb[live ? pi : s], vl = live ? s_vl[pi] : 0u;
                    // (the longer of the wave's two rows, as a scalar: the trip loop is a uniform one and says so to the compiler)
                    const uint32_t vl_a = (uint32_t)__builtin_amdgcn_readlane((int)vl, 0), vl_b = (uint32_t)__builtin_amdgcn_readlane((int)vl, 32);
                    const uint32_t longest = vl_a > vl_b ? vl_a : vl_b;
                    // rem: entries the row has from this lane's first one of the trip on; ofs: that entry's byte offset in col[]
                    int rem = (int)vl - 4 * hl;
                    uint32_t ofs = (vb + 4u * (uint32_t)hl) * 4u;
                    long long acc = 0ll;
                    for (uint32_t off = 0; off < longest; off += 32 * RS_NB) {     // (uniform trip count over the wave)
                        const v4i w0 = rs_row_load(col_rs, ofs, rem > 0), w1 = rs_row_load(col_rs, ofs + 512u, rem > 128);
                        __builtin_amdgcn_sched_barrier(0);     // (both loads issue before the first one's look-ups start)
                        acc += rs_trip<WIN>(bm, fix_rs, wlo, w0, w1, rem);
                        rem -= 32 * RS_NB;
                        ofs += 32 * RS_NB * 4;
                    }
#pragma unroll
                    for (int d = 16; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
                    if (hl == 0 && live) s_sum[pi] += acc;
                }
                __syncthreads();
                for (uint32_t i = (uint32_t)ub + tid; i < (uint32_t)ue; i += RS_THREADS) {
                    const uint32_t x = (uint32_t)(col[i] - wlo);
                    if (!WIN || x < (uint32_t)RS_BITS) bm[x >> 5] = 0u;
                }
                __syncthreads();
            }
            s = e;
        }
        if (tid < cn && my_long) out[c0 + tid] = (float)((double)s_sum[tid] * (1.0 / (double)(1ll << 40)));
        __syncthreads();
    }
}

// The pairs whose u has at most RS_SHORT entries (most distinct u have few survivors each: a bitmap per run would cost three
// workgroup barriers for a handful of pairs).  Under hubs-first labels v is the lighter endpoint, so both rows are short: a
// wave stages the shorter row in its own 2 KiB of LDS (no barrier: wave-private), spreads the other row over its lanes and
// looks every entry up by a binary search in LDS.  Same exact float64 sums.
#define RSS_THREADS 256
#define RSS_TRIPS 4             // windows of 64 keys a wave is given, where the list is long enough (the grid is sized from this)

// One short pair by the whole wave (u, v wave-uniform; stage = the wave's RS_SHORT words of LDS) -> its score, in every lane.
static __device__ __forceinline__ float rss_score_pair(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                       const int64_t *__restrict__ fixw, int32_t *stage, int lane, int32_t u, int32_t v)
{
    const int64_t ub = rowptr[u], ue = rowptr[u + 1];
    const int64_t vb = rowptr[v], ve = rowptr[v + 1];
    const bool u_short = ue - ub <= ve - vb;
    const int64_t sb = u_short ? ub : vb, se = u_short ? ue : ve;       // staged (the shorter: <= RS_SHORT entries)
    const int64_t lb = u_short ? vb : ub, le = u_short ? ve : ue;       // spread over the lanes
    const int ns = (int)(se - sb);
    int pow2 = 1;
    while (pow2 < ns) pow2 <<= 1;
    for (int i = lane; i < pow2; i += 64) stage[i] = i < ns ? col[sb + i] : 0x7fffffff;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    long long acc = 0ll;
    for (int64_t i0 = lb; i0 < le; i0 += 64) {
        const int64_t i = i0 + lane;
        const int32_t w = i < le ? col[i] : -1;
        int lo = 0;                                           // last position with stage[pos] <= w
        for (int step = pow2 >> 1; step >= 1; step >>= 1)
            if (stage[lo + step] <= w) lo += step;
        if (w >= 0 && ns > 0 && stage[lo] == w) acc += (long long)fixw[w];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (the next pair overwrites the staged row)
    return (float)((double)acc * (1.0 / (double)(1ll << 40)));
}

// The search for the short pairs, 64 keys a trip: every lane loads ITS key and the two rowptr words of its u -- 64 chains of two
// dependent latencies in flight at once -- a ballot says which lanes hold a short pair, and the wave scores those one after the
// other (the body is wave-cooperative: u and v come from the owning lane).  One key a trip, read wave-uniformly, was 173 us of
// bare latency per call on the bench graph: the survivors of a K = 4 M scan are pairs of hubs, NONE of its 2 M pairs is short,
// and the pass is a filter over 16 MB of keys.  Waves are independent: no barrier, no atomics.
__global__ __launch_bounds__(RSS_THREADS) void rescore_short_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                  const int64_t *__restrict__ fixw, const int64_t *__restrict__ keys,
                                                                  int64_t n, float *__restrict__ out, const int64_t *__restrict__ n_dev)
{
    if (n_dev) {
        const int64_t c = *n_dev;
        n = c < 0 ? 0 : (c < n ? c : n);
    }
    __shared__ int32_t s_stage[RSS_THREADS / 64][RS_SHORT];
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    int32_t *stage = s_stage[wib];
    const int64_t wave = (int64_t)blockIdx.x * (RSS_THREADS / 64) + wib;
    const int64_t n_waves = (int64_t)gridDim.x * (RSS_THREADS / 64);
    for (int64_t p0 = wave * 64; p0 < n; p0 += n_waves * 64) {
        int32_t my_u = 0, my_v = 0;
        bool is_short = false;
        if (p0 + lane < n) {
            const int64_t key = keys[p0 + lane];
            my_u = (int32_t)(key >> 32);
            my_v = (int32_t)(key & 0xFFFFFFFFll);
            is_short = rowptr[my_u + 1] - rowptr[my_u] <= RS_SHORT;       // (the others are rescore_runs_kernel's)
        }
        for (unsigned long long todo = __ballot(is_short); todo; todo &= todo - 1) {
            const int owner = __builtin_ctzll(todo);
            const int32_t u = __builtin_amdgcn_readlane(my_u, owner), v = __builtin_amdgcn_readlane(my_v, owner);
            const float score = rss_score_pair(rowptr, col, fixw, stage, lane, u, v);
            if (lane == 0) out[p0 + owner] = score;
        }
    }
}

// A weighted pair: term = (A[u,w] * A[v,w]) * node_w[w] in float32 (the association eps_expand_fill uses: symmetric in u, v),
// converted to 2^-40 fixed point and summed in int64.  One wave per pair: the shorter row spread over the lanes, each entry
// looked up in the longer row by a binary search in global memory (the lists of weighted graphs -- collab -- are short).
__global__ __launch_bounds__(256) void rescore_weighted_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                              const float *__restrict__ val, const float *__restrict__ node_w,
                                                              const int64_t *__restrict__ keys, int64_t n, float *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t pi = wave; pi < n; pi += n_waves) {
        const int64_t key = keys[pi];
        const int32_t u = (int32_t)(key >> 32), v = (int32_t)(key & 0xFFFFFFFFll);
        const int64_t ub = rowptr[u], ue = rowptr[u + 1], vb = rowptr[v], ve = rowptr[v + 1];
        const bool u_short = ue - ub <= ve - vb;
        const int64_t sb = u_short ? ub : vb, se = u_short ? ue : ve, lb = u_short ? vb : ub, le = u_short ? ve : ue;
        long long acc = 0ll;
        for (int64_t i = sb + lane; i < se; i += 64) {
            const int32_t w = col[i];
            const int64_t lo = eps_lower_bound(col, lb, le, w);
            if (lo < le && col[lo] == w) {
                const float term = (val[i] * val[lo]) * node_w[w];
                acc += __double2ll_rn((double)term * (double)(1ll << 40));
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
        if (lane == 0) out[pi] = (float)((double)acc * (1.0 / (double)(1ll << 40)));
    }
}

// keys: (u << 32) | v sorted ascending (runs of equal u); fixw[i] = the 2^-40 fixed-point weight of node i (eps_fixed_weights);
// out[i] = score of pair i as float32 of the exact sum.  Unit-valued adjacency.
static int rescore_runs_launch(const int64_t *rowptr, const int32_t *col, const int64_t *fixw, int64_t n_nodes, const int64_t *keys,
                               int64_t n, const int64_t *n_dev, float *out, void *stream)
{
    EPS_REQUIRE(n >= 0 && n_nodes >= 0 && n_nodes < (1ll << 31), "eps_rescore_runs: bad size");      // (col[] is addressed with 32-bit byte offsets: nnz < 2^30, like eps_scan_screen)
    if (n == 0) return EPS_OK;
    EPS_REQUIRE(rowptr && col && fixw && keys && out, "eps_rescore_runs: null pointer");
    hipStream_t s = (hipStream_t)stream;
    unsigned int *counter = nullptr;
    const int rc = eps_take_counters8(&counter, s, "eps_rescore_runs");
    if (rc) return rc;
    const size_t lds = (size_t)(n_nodes < RS_BITS ? ((n_nodes + 31) >> 5) : (RS_BITS >> 5)) * 4 + 16;
    // (two instantiations: an id space of one bitmap window needs no window arithmetic per entry)
    auto kernel = n_nodes > RS_BITS ? rescore_runs_kernel<true> : rescore_runs_kernel<false>;
    if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        eps_set_error("eps_rescore_runs: cannot reserve %zu bytes of LDS", lds);
        return EPS_ELAUNCH;
    }
    int64_t blocks = (n + RS_CHUNK - 1) / RS_CHUNK;
    // workgroups the LDS lets a CU hold: next to the bitmap a workgroup has 4.2 KB of its own (sums, chunk descriptors, run starts)
    const int64_t per_cu = (160 * 1024 - 2048) / (int64_t)(lds + 4608);
    const int64_t cap = (int64_t)eps_num_cus() * (per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu));
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(RS_THREADS), lds, s, rowptr, col, fixw, (int32_t)n_nodes, keys, n, out, counter,
                       n_dev);
    {
        // (a wave per RSS_TRIPS windows of 64 keys: a short list does not start waves that find no window)
        const int64_t per_block = (int64_t)(RSS_THREADS / 64) * 64 * RSS_TRIPS;
        int64_t sb = (n + per_block - 1) / per_block;
        const int64_t scap = (int64_t)eps_num_cus() * 8;
        if (sb > scap) sb = scap;
        hipLaunchKernelGGL(rescore_short_kernel, dim3((unsigned)sb), dim3(RSS_THREADS), 0, s, rowptr, col, fixw, keys, n, out, n_dev);
    }
    EPS_CHECK_LAUNCH("eps_rescore_runs");
    return EPS_OK;
}

extern "C" int eps_rescore_limits(int32_t *window_bits, int32_t *short_max, int32_t *chunk)
{
    if (window_bits) *window_bits = RS_BITS;
    if (short_max) *short_max = RS_SHORT;
    if (chunk) *chunk = RS_CHUNK;
    return EPS_OK;
}

extern "C" int eps_rescore_runs(const int64_t *rowptr, const int32_t *col, const int64_t *fixw, int64_t n_nodes,
                                const int64_t *keys, int64_t n, float *out, void *stream)
{
    return rescore_runs_launch(rowptr, col, fixw, n_nodes, keys, n, nullptr, out, stream);
}

// The same with the list's length read on the DEVICE: min(*n_dev, n_max) pairs (the grid is sized for n_max).
extern "C" int eps_rescore_runs_dev(const int64_t *rowptr, const int32_t *col, const int64_t *fixw, int64_t n_nodes,
                                    const int64_t *keys, int64_t n_max, const int64_t *n_dev, float *out, void *stream)
{
    EPS_REQUIRE(n_dev, "eps_rescore_runs_dev: null count");
    return rescore_runs_launch(rowptr, col, fixw, n_nodes, keys, n_max, n_dev, out, stream);
}

// The same for an adjacency with stored values (any order of the keys).
extern "C" int eps_rescore_weighted(const int64_t *rowptr, const int32_t *col, const float *val, const float *node_w,
                                    int64_t n_nodes, const int64_t *keys, int64_t n, float *out, void *stream)
{
    EPS_REQUIRE(n >= 0 && n_nodes >= 0, "eps_rescore_weighted: bad size");
    if (n == 0) return EPS_OK;
    EPS_REQUIRE(rowptr && col && val && node_w && keys && out, "eps_rescore_weighted: null pointer");
    int64_t blocks = (n + 3) / 4;
    const int64_t cap = (int64_t)eps_num_cus() * 8;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(rescore_weighted_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, col, val, node_w, keys,
                       n, out);
    EPS_CHECK_LAUNCH("eps_rescore_weighted");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void rescore_warm_kernel() {}
extern "C" void eps_warm_rescore(void *stream) { hipLaunchKernelGGL(rescore_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

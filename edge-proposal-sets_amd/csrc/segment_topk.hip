// Segmented top-k: for every segment of a score array, the positions of its k best entries (gfx950).
//
// The list kernels deliver a block's candidates column-major -- column v, u ascending, one score each -- so "node v's k best
// proposals" (filter.py --keep_per_node k) is a top-k per SEGMENT of the block's score array.  The order is the declared one:
// eps_ordered_bits(score) descending (csrc/eps_common.h: -0.0 ties +0.0, NaN where its bit pattern puts it), then position ascending.
//
// Selection by threshold, not by heap, so no resource depends on k:
//   1. the k-th largest key T of the segment by radix select (four rounds of a 256-bin LDS histogram over the keys that still
//      match the prefix found so far; a wave holding a short segment in registers finds T bit by bit with ballots instead),
//      which also leaves t = how many entries EQUAL to T belong to the k best;
//   2. entry p is kept when key(p) > T, or key(p) == T and fewer than t equal entries precede it -- the FIRST t ties;
//   3. its place is outptr[s] + (kept entries in front of it) = gt_before(p) + min(eq_before(p), t): a running count over
//      ordered chunks of the segment, so positions come out ascending and do not depend on the launch shape.
// A segment of at most k entries keeps all of them.  No atomics on global memory at all (the histograms are LDS integer
// counters); the same inputs give the same bits.
//
// Work distribution.  Three shapes, one launch each, every launch walks `order` (the caller's heaviest-first list of segments;
// NULL = as numbered) and takes the segments of its own class -- the classes partition the lengths, so every segment is written
// by exactly one launch whatever `order` holds; its order only decides the balance:
//   wave   len <= SEG_WAVE_MAX: one wave per segment, keys in registers (SEG_WAVE_MAX / 64 per lane), no LDS, no barrier;
//   lds    len <= SEG_LDS_MAX:  one workgroup, the keys converted once into LDS, every later pass reads LDS;
//   stream longer:              one workgroup, the segment streamed from memory once per radix round and once to compact
//                               (a hub column of a few hundred thousand candidates is L2-resident between the passes).
// Workgroup b owns the items i = b, b + G, b + 2G, ... of `order`: with the list sorted by length the heavy segments are dealt
// round-robin over the grid and start first.
#include "eps_common.h"

#define SEG_THREADS 256
#define SEG_WAVES (SEG_THREADS / 64)
#define SEG_WAVE_MAX 256         // one wave, SEG_WAVE_U keys per lane
#define SEG_WAVE_U (SEG_WAVE_MAX / 64)
#define SEG_LDS_MAX 8192         // one workgroup, keys in LDS (32 KiB: four workgroups per CU)
#define SEG_CHUNK (SEG_THREADS * 4)   // entries per compaction step: four consecutive ones per thread

struct seg_range {
    int64_t start, len, out, room;
};

// segment s: [start, start + len) of the arrays, its kept positions go to [out, out + room)
__device__ __forceinline__ seg_range seg_get(const int64_t *__restrict__ colptr, const int64_t *__restrict__ counts,
                                             const int64_t *__restrict__ outptr, int64_t s)
{
    seg_range r;
    r.start = colptr[s];
    r.len = counts ? counts[s] : colptr[s + 1] - r.start;
    if (r.len < 0) r.len = 0;
    r.out = outptr[s];
    r.room = outptr[s + 1] - r.out;
    return r;
}

// ---- one wave per short segment ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(SEG_THREADS) void seg_wave_kernel(const int64_t *__restrict__ colptr, const int64_t *__restrict__ counts,
                                                              const float *__restrict__ score, int64_t n_seg, uint32_t k,
                                                              const int64_t *__restrict__ outptr, const int32_t *__restrict__ order,
                                                              int64_t *__restrict__ out_pos)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * SEG_THREADS + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * SEG_THREADS) >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;       // the lanes in front of this one
    // a wave looks at 64 items of the list at a time (one per lane) and serves those of its class one after the other
    for (int64_t i0 = wave * 64; i0 < n_seg; i0 += n_waves * 64) {
        const int64_t i = i0 + lane;
        int64_t s = -1;
        bool mine = false;
        if (i < n_seg) {
            s = order ? (int64_t)order[i] : i;
            if (s >= 0 && s < n_seg) {
                const int64_t len = counts ? counts[s] : colptr[s + 1] - colptr[s];
                mine = len <= SEG_WAVE_MAX;
            }
        }
        unsigned long long todo = __ballot(mine);
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const int64_t seg = __shfl(s, src);
            const seg_range r = seg_get(colptr, counts, outptr, seg);
            const int len = (int)r.len;
            if ((uint32_t)len <= k) {                              // everything is kept
#pragma unroll
                for (int j = 0; j < SEG_WAVE_U; ++j) {
                    const int p = j * 64 + lane;
                    if (p < len && p < r.room) out_pos[r.out + p] = r.start + p;
                }
                continue;
            }
            uint32_t key[SEG_WAVE_U];
            bool live[SEG_WAVE_U];
#pragma unroll
            for (int j = 0; j < SEG_WAVE_U; ++j) {
                const int p = j * 64 + lane;
                live[j] = p < len;
                key[j] = live[j] ? eps_ordered_bits(score[r.start + p]) : 0u;
            }
            // the k-th largest key, bit by bit from the top: how many live keys carry the prefix found so far with this bit set
            uint32_t prefix = 0u, t = k;
#pragma unroll 1
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t cand = prefix | (1u << bit), high = ~((1u << bit) - 1u);
                uint32_t c = 0u;
#pragma unroll
                for (int j = 0; j < SEG_WAVE_U; ++j) c += (uint32_t)__popcll(__ballot(live[j] && (key[j] & high) == cand));
                if (c >= t) prefix = cand; else t -= c;
            }
            // (prefix is the k-th largest key now and t, 1 <= t <= its multiplicity, the ties that belong to the k best)
            uint32_t gt_run = 0u, eq_run = 0u;
#pragma unroll
            for (int j = 0; j < SEG_WAVE_U; ++j) {
                const bool gt = live[j] && key[j] > prefix, eq = live[j] && key[j] == prefix;
                const unsigned long long mg = __ballot(gt), me = __ballot(eq);
                const uint32_t gb = gt_run + (uint32_t)__popcll(mg & below), eb = eq_run + (uint32_t)__popcll(me & below);
                if (gt || (eq && eb < t)) {
                    const int64_t at = (int64_t)gb + (int64_t)(eb < t ? eb : t);
                    if (at < r.room) out_pos[r.out + at] = r.start + j * 64 + lane;
                }
                gt_run += (uint32_t)__popcll(mg);
                eq_run += (uint32_t)__popcll(me);
            }
        }
    }
}

// ---- one workgroup per segment: keys in LDS, or streamed --------------------------------------------------------------
// (a wave whose live lanes agree on the bin adds their count once: the leading digits of a column's scores are nearly
//  constant, and 64 LDS atomics on one address run one after the other -- the same step as kth_hist_kernel's)
__device__ __forceinline__ void seg_hist_add(uint32_t *h, bool live, uint32_t bin, int lane)
{
    const unsigned long long m = __ballot(live);
    if (m) {
        const int first = __builtin_ctzll(m);
        const uint32_t b0 = (uint32_t)__shfl((int)bin, first);
        if (__ballot(live && bin == b0) == m) {
            if (lane == first) atomicAdd(&h[b0], (uint32_t)__popcll(m));
        } else if (live) {
            atomicAdd(&h[bin], 1u);
        }
    }
}

template <bool STREAM>
__global__ __launch_bounds__(SEG_THREADS) void seg_group_kernel(const int64_t *__restrict__ colptr, const int64_t *__restrict__ counts,
                                                               const float *__restrict__ score, int64_t n_seg, uint32_t k,
                                                               const int64_t *__restrict__ outptr, const int32_t *__restrict__ order,
                                                               int64_t *__restrict__ out_pos)
{
    __shared__ uint32_t s_key[STREAM ? 4 : SEG_LDS_MAX];
    __shared__ uint32_t s_hist[256];
    __shared__ int64_t s_list[SEG_THREADS];
    __shared__ uint32_t s_wcnt[2][SEG_WAVES];   // per wave: items of the class / packed (gt | eq << 16) of a chunk, two buffers in turn
    __shared__ uint32_t s_prefix, s_mask, s_t;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    for (int64_t m0 = 0; m0 * gridDim.x + blockIdx.x < n_seg; m0 += SEG_THREADS) {
        // this workgroup's next SEG_THREADS items of the list, one per thread; those of the class are queued in list order
        const int64_t i = (m0 + tid) * gridDim.x + blockIdx.x;
        int64_t s = -1;
        bool mine = false;
        if (i < n_seg) {
            s = order ? (int64_t)order[i] : i;
            if (s >= 0 && s < n_seg) {
                const int64_t len = counts ? counts[s] : colptr[s + 1] - colptr[s];
                mine = STREAM ? len > SEG_LDS_MAX : (len > SEG_WAVE_MAX && len <= SEG_LDS_MAX);
            }
        }
        const unsigned long long mm = __ballot(mine);
        if (lane == 0) s_wcnt[0][wv] = (uint32_t)__popcll(mm);
        __syncthreads();
        uint32_t before = 0u, n_list = 0u;
#pragma unroll
        for (int w = 0; w < SEG_WAVES; ++w) {
            if (w < wv) before += s_wcnt[0][w];
            n_list += s_wcnt[0][w];
        }
        if (mine) s_list[before + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull))] = s;
        __syncthreads();

        for (uint32_t q = 0; q < n_list; ++q) {
            const seg_range r = seg_get(colptr, counts, outptr, s_list[q]);
            const int64_t len = r.len;
            if ((uint64_t)len <= (uint64_t)k) {                    // (cannot happen for k < SEG_WAVE_MAX: a long segment kept whole)
                for (int64_t p = tid; p < len; p += SEG_THREADS)
                    if (p < r.room) out_pos[r.out + p] = r.start + p;
                continue;
            }
            const float *__restrict__ x = score + r.start;
            // ---- radix select: four rounds of eight bits over the keys that match the prefix so far
            uint32_t prefix = 0u, mask = 0u, t = k;
#pragma unroll 1
            for (int round = 0; round < 4; ++round) {
                const int shift = 24 - 8 * round;
                s_hist[tid] = 0u;                                  // (SEG_THREADS == 256 bins)
                __syncthreads();
                // (whole waves run the loop: the ballots of seg_hist_add need every lane)
                for (int64_t base = 0; base < len; base += SEG_CHUNK) {
                    uint32_t key[4];
                    bool live[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int64_t p = base + j * SEG_THREADS + tid;
                        live[j] = p < len;
                        if (STREAM) {
                            key[j] = live[j] ? eps_ordered_bits(x[p]) : 0u;
                        } else if (round == 0) {
                            key[j] = live[j] ? eps_ordered_bits(x[p]) : 0u;
                            if (live[j]) s_key[p] = key[j];
                        } else {
                            key[j] = live[j] ? s_key[p] : 0u;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        seg_hist_add(s_hist, live[j] && (key[j] & mask) == prefix, (key[j] >> shift) & 255u, lane);
                }
                __syncthreads();
                if (wv == 0) {
                    // lane l owns the bins 255 - 4 l .. 252 - 4 l (from the top); the first lane whose running total reaches t
                    // holds the bin of the t-th largest.  The matching keys number at least t (the round before counted them).
                    uint32_t c[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) c[j] = s_hist[255 - 4 * lane - j];
                    const uint32_t own = c[0] + c[1] + c[2] + c[3];
                    const uint32_t incl = eps_wave_incl_scan(own, lane);
                    const unsigned long long reach = __ballot(incl >= t);
                    const int owner = reach ? __builtin_ctzll(reach) : 63;
                    if (lane == owner) {
                        uint32_t t2 = t - (incl - own);
                        int b = 255 - 4 * lane;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if (j == 3 || t2 <= c[j]) break;
                            t2 -= c[j];
                            --b;
                        }
                        s_t = t2;
                        s_prefix = prefix | ((uint32_t)b << shift);
                        s_mask = mask | (255u << shift);
                    }
                }
                __syncthreads();
                prefix = s_prefix;
                mask = s_mask;
                t = s_t;
            }
            // ---- compaction in ordered chunks: thread `tid` holds the entries base + 4 tid .. + 3 of a chunk
            uint32_t gt_run = 0u, eq_run = 0u;
            int buf = 0;
            uint32_t cur[4], nxt[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t p = 4 * tid + j;
                cur[j] = p < len ? (STREAM ? eps_ordered_bits(x[p]) : s_key[p]) : 0u;
            }
            for (int64_t base = 0; base < len; base += SEG_CHUNK) {
                if (STREAM) {                                      // (the next chunk's loads are under way while this one is placed)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int64_t p = base + SEG_CHUNK + 4 * tid + j;
                        nxt[j] = p < len ? eps_ordered_bits(x[p]) : 0u;
                    }
                }
                uint32_t own = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool in = base + 4 * tid + j < len;
                    own += (in && cur[j] > prefix ? 1u : 0u) + (in && cur[j] == prefix ? 1u << 16 : 0u);
                }
                const uint32_t incl = eps_wave_incl_scan(own, lane);   // (a chunk holds 1024 entries: both halves stay below 2^16)
                if (lane == 63) s_wcnt[buf][wv] = incl;
                __syncthreads();
                uint32_t front = 0u, whole = 0u;
#pragma unroll
                for (int w = 0; w < SEG_WAVES; ++w) {
                    if (w < wv) front += s_wcnt[buf][w];
                    whole += s_wcnt[buf][w];
                }
                buf ^= 1;      // (the next chunk writes the other buffer: a wave that runs ahead cannot touch counts still being read)
                const uint32_t ahead = front + incl - own;
                uint32_t gb = gt_run + (ahead & 0xFFFFu), eb = eq_run + (ahead >> 16);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t p = base + 4 * tid + j;
                    if (p < len) {
                        if (cur[j] > prefix) {
                            const int64_t at = (int64_t)gb + (int64_t)(eb < t ? eb : t);
                            if (at < r.room) out_pos[r.out + at] = r.start + p;
                            ++gb;
                        } else if (cur[j] == prefix) {
                            if (eb < t && (int64_t)gb + eb < r.room) out_pos[r.out + gb + eb] = r.start + p;
                            ++eb;
                        }
                    }
                }
                gt_run += whole & 0xFFFFu;
                eq_run += whole >> 16;
                if (gt_run + (eq_run < t ? eq_run : t) >= k) break;          // all k are placed (uniform over the workgroup)
                if (STREAM) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int64_t p = base + SEG_CHUNK + 4 * tid + j;
                        cur[j] = p < len ? s_key[p] : 0u;
                    }
                }
            }
            __syncthreads();   // (s_key, s_hist and the chunk counts are free for the next segment)
        }
        __syncthreads();       // (... and s_list for the next items)
    }
}

extern "C" int64_t eps_segment_topk_class_max(int32_t cls)
{
    return cls == 0 ? SEG_WAVE_MAX : (cls == 1 ? SEG_LDS_MAX : -1);
}

extern "C" int eps_segment_topk(const int64_t *colptr, const int64_t *counts_or_null, const float *score, int64_t n_seg, int64_t k,
                                const int64_t *outptr, const int32_t *order_or_null, int64_t *out_pos, void *stream)
{
    EPS_REQUIRE(k >= 1 && k < (1ll << 31), "eps_segment_topk: k=%lld must lie in [1, 2^31)", (long long)k);
    EPS_REQUIRE(n_seg >= 0 && n_seg < (1ll << 31), "eps_segment_topk: n_seg=%lld must lie in [0, 2^31)", (long long)n_seg);
    if (n_seg == 0) return EPS_OK;
    EPS_REQUIRE(colptr, "eps_segment_topk: colptr is null with n_seg=%lld", (long long)n_seg);
    EPS_REQUIRE(score && outptr && out_pos, "eps_segment_topk: score / outptr / out_pos is null with n_seg=%lld", (long long)n_seg);
    hipStream_t s = (hipStream_t)stream;
    const int64_t cus = eps_num_cus();
    // stream / lds: a workgroup per item of the list up to four (LDS: 34 KiB each) resp. eight per CU; wave: 64 items per wave
    int64_t g_stream = n_seg < cus * 8 ? n_seg : cus * 8, g_lds = n_seg < cus * 4 ? n_seg : cus * 4;
    int64_t g_wave = (n_seg + 64 * SEG_WAVES - 1) / (64 * SEG_WAVES);
    if (g_wave > cus * 8) g_wave = cus * 8;
    hipLaunchKernelGGL(seg_group_kernel<true>, dim3((unsigned)g_stream), dim3(SEG_THREADS), 0, s, colptr, counts_or_null, score, n_seg,
                       (uint32_t)k, outptr, order_or_null, out_pos);
    hipLaunchKernelGGL(seg_group_kernel<false>, dim3((unsigned)g_lds), dim3(SEG_THREADS), 0, s, colptr, counts_or_null, score, n_seg,
                       (uint32_t)k, outptr, order_or_null, out_pos);
    hipLaunchKernelGGL(seg_wave_kernel, dim3((unsigned)g_wave), dim3(SEG_THREADS), 0, s, colptr, counts_or_null, score, n_seg,
                       (uint32_t)k, outptr, order_or_null, out_pos);
    EPS_CHECK_LAUNCH("eps_segment_topk");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void segment_topk_warm_kernel() {}
extern "C" void eps_warm_segment_topk(void *stream) { hipLaunchKernelGGL(segment_topk_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

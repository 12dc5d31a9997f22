// Pair scores (Common Neighbours / Adamic-Adar / Resource Allocation) by CSR neighbour-list
// intersection, gfx950.
//
// Replaces, per pair (u,v):  np.sum(A[src].multiply(A_[dst]), 1)   adamic_utils.py:22,
// train_and_eval.py:212 and  adj[e0] (.) adj[e1] -> sparse row-sum   models.py:536-542.
//
// This file: the GENERIC kernel (any pair list: the eval sets of train_and_eval.py:108-136, random negatives) and the
// per-node weight table.  pair_grouped.hip holds the column-run kernel for lists in the reference's candidate order.
//
// Work decomposition (wave = 64 lanes):
//   * 64-pair chunks are handed to waves dynamically (one device-scope atomic per chunk, drawn one chunk ahead):
//     pair costs are heavy-tailed, a static split leaves the slowest wave running long after the others.
//   * lane i fetches pair i's (u,v) and the four rowptr words in parallel -- one coalesced metadata fetch per 64
//     pairs instead of a dependent scalar chain per pair -- and lane i finally stores pair i's results (coalesced).
//   * the 64 pairs are then scored one after the other by the whole wave, each by the walk of row_intersect.h (the longer row
//     staged in LDS or, for very lopsided pairs, searched in place).  Matches are counted with ballot+popcount; for unit-weight
//     graphs the node_w gathers of the hits are queued in LDS and resolved once per 64 pairs (no dependent global load on a
//     pair's critical path); weighted graphs / float64 weights accumulate inline and reduce with a DPP butterfly.
// HBM traffic is the algorithmic minimum: both rows once, coalesced; rowptr/pair/outputs once.
#include "row_intersect.h"

#define PI_WAVES 4           // waves per workgroup
#define PI_QCAP 256          // per-wave hit queue (1 KiB): deferred node_w gathers
#define PI_TICKET 4          // consecutive 64-pair chunks per ticket of the launch that scores the longer pairs (PART 2)
#define PI_SMALL 128         // pairs whose LONGER row has at most this many entries are scored four at a time (16 lanes each).
                             // r06, 2^24 pairs of the ppa-like graph, uniform / stored edges: 64: 3.55 / 10.64 ms, 128: 3.33 / 10.41, 256: 5.20 / 11.81
#define PI_SMALL_LG (PI_SMALL == 256 ? 8 : PI_SMALL == 128 ? 7 : 6)

typedef int v4i_a4 __attribute__((ext_vector_type(4), aligned(4)));

// PART (r06): 0 = every pair, one at a time per wave (stored values, float64 weights); 1 = the SMALL pairs only, four at a time;
// 2 = everything but the small pairs.  r05 had the small-pair path inside the one kernel: its 16 staging registers took the
// unit-valued float32 instantiations from 62 to 96 VGPRs = 8 -> 5 waves per SIMD, and the lists whose longer rows exceed 256
// entries paid for it (stored-edge positives 4.37 -> 5.73 ms, the R-MAT-24 share 0.64 -> 0.70 s: VERDICT r05 weak #8).  Two
// launches over the same list now: part 1 at its own register count, part 2 = the r04 body at 8 waves per SIMD; each writes the
// outputs of ITS pairs only; the list's 48 bytes of header per pair are read twice (3 M pairs: 0.03 ms).
template <bool HAS_VAL, bool HAS_W, typename WT, int PART, int TKC>
__global__ __launch_bounds__(PI_WAVES * 64) void pair_scores_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const WT *__restrict__ node_w, const int32_t *__restrict__ pu, const int32_t *__restrict__ pv,
    int64_t n_pairs, unsigned int *__restrict__ next_chunk, int32_t *__restrict__ out_count,
    float *__restrict__ out_cn, WT *__restrict__ out_ws, const unsigned int *__restrict__ cls)
{
    // (r06) cls = {small pairs, pairs} of a sample of the list (pair_classify_kernel) or NULL: the three launches of a unit-valued
    // float32 list all go out, and each decides here -- the same two words for everyone -- whether it is the one that runs
    if (cls) {
        const bool split = (unsigned long long)cls[0] * 5ull > (unsigned long long)cls[1] * 3ull;      // >= 60 % small pairs
        if (split != (PART != 0)) return;
    }
    constexpr bool DEFER = HAS_W && !HAS_VAL && sizeof(WT) == 4;  // unit weights: node_w gathers resolved per 64 pairs
    __shared__ __attribute__((aligned(16))) int32_t s_rows[PI_WAVES][ROW_CAP];
    __shared__ uint32_t s_q[PI_WAVES][PI_QCAP];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int32_t *L = s_rows[wib];
    uint32_t *q = s_q[wib];
    const int64_t n_chunks = (n_pairs + 63) >> 6;

    // 64-pair chunks are handed out dynamically (pair costs are heavy-tailed); the next ticket is drawn while the
    // current chunk is being scored, so the atomic's round trip is off the critical path.
    // r06: the small pairs (PART 1: bounded cost) are dealt statically -- no tickets at all.  The rest (PART 2) draws tickets of
    // PI_TICKET consecutive chunks: one device word serves
    // ~90 M atomics a second, and after the split most chunks of an evaluation list hold no work for this part -- 262 k
    // single-chunk tickets were 2.9 ms for 2^24 uniform pairs.  The draw stays
    // r04's (one word, the next ticket requested while the current one is scored, its value first looked at when that is done):
    // eight per-XCD counters with a steal loop were tried twice and lost both times -- testing the drawn value at once cost every
    // wave the atomic's round trip per chunk (10.7 vs 8.8 ms on 2^24 stored-edge pairs), and the lazy version's bookkeeping took
    // the kernel from 62 to 71 VGPRs, 8 -> 7 waves per SIMD (11.4 ms): profiles/r06/eval_pairs_variants.txt.
    const int64_t wave_id = (int64_t)blockIdx.x * PI_WAVES + wib, n_waves = (int64_t)gridDim.x * PI_WAVES;
    int64_t static_next = wave_id;
    auto take = [&]() -> int64_t {
        if (PART == 1) {
            const int64_t c = static_next;
            static_next += n_waves;
            return c;
        }
        return take_chunk(next_chunk, lane);
    };
    auto do_chunk = [&](const int64_t chunk) {
        const int64_t p = chunk * 64 + lane;
        const bool valid = p < n_pairs;
        const int32_t nu = valid ? pu[p] : 0, nv = valid ? pv[p] : 0;
        const int64_t ub = rowptr[nu], vb = rowptr[nv];
        const int32_t du = valid ? (int32_t)(rowptr[nu + 1] - ub) : 0;
        const int32_t dv = valid ? (int32_t)(rowptr[nv + 1] - vb) : 0;

        int32_t my_count = 0;
        float my_cn = 0.0f;
        WT my_ws = 0;
        int my_qstart = 0, my_qcnt = 0, qlen = 0;

        auto flush = [&](int open_j, int open_q0) {  // see pair_grouped.hip: one parallel gather, per-lane segment sums
            if (!DEFER) return;
            if (open_j >= 0 && lane == open_j) { my_qstart = open_q0; my_qcnt = qlen - open_q0; }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int t = lane; t < qlen; t += 64) q[t] = __builtin_bit_cast(uint32_t, (float)node_w[q[t]]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            float sacc = 0.0f;
            for (int t = 0; t < my_qcnt; ++t) sacc += __builtin_bit_cast(float, q[my_qstart + t]);
            my_ws += (WT)sacc;
            my_qcnt = 0;
            qlen = 0;
            __builtin_amdgcn_wave_barrier();
        };

        // SMALL pairs, four at a time (r05).  An evaluation list (train_and_eval.py:108-136: uniform negatives, stored edges) is
        // mostly pairs of two short rows; scored one after the other by the whole wave each of them is a memory round trip with
        // a handful of busy lanes -- 0.28 of the HBM roofline on 3 M uniform pairs of the ppa-like graph.  Here a quarter of the
        // wave takes a pair: its 16 lanes stage the longer row (<= 256 entries) in their quarter of the wave's LDS, spread the
        // shorter row over themselves and search; four pairs' loads are in flight together.  Unit-valued graphs, float32 weights.
        int32_t du_left = du, dv_left = dv;
        bool is_small = false;
        if (PART != 0) {
            const int32_t mx = du > dv ? du : dv, mn = du < dv ? du : dv;
            is_small = valid && mn > 0 && mx <= PI_SMALL;
            if (PART == 1 || is_small) du_left = dv_left = 0;                     // (the one-at-a-time loop below skips them)
        }
#if PI_SMALL >= 64
        if (PART == 1) {
            uint64_t small = __ballot(is_small);
            if (!small) return;                                                   // (wave-uniform: a chunk of longer rows is part 2's)
            const int g = lane >> 4, gl = lane & 15;
            while (small) {
                int jg[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    jg[q] = small ? __builtin_ctzll(small) : -1;
                    small &= small - 1ull;
                }
                const int j = g == 0 ? jg[0] : g == 1 ? jg[1] : g == 2 ? jg[2] : jg[3];
                const int js = j < 0 ? 0 : j;
                // (every lane takes part in the shuffles: a group without a pair must still SERVE its lanes' values to the others)
                const int32_t du_j = __shfl(du, js), dv_j = __shfl(dv, js);
                const int64_t bju = __shfl(ub, js), bjv = __shfl(vb, js);
                const int32_t dju = j < 0 ? 0 : du_j, djv = j < 0 ? 0 : dv_j;
                const bool swapped = dju > djv;
                const int32_t slen = swapped ? djv : dju, llen = swapped ? dju : djv;
                const int32_t *__restrict__ srow = col + (swapped ? bjv : bju), *__restrict__ lrow = col + (swapped ? bju : bjv);
                int32_t *Lg = L + g * PI_SMALL;
                // the longer row of each group, every load issued before the first LDS write; INT_MAX beyond its end.
                // (r06: 16-byte loads -- a lane takes four consecutive entries, a group 64 per instruction: a quarter of the vector-memory
                //  instructions of the one-entry loads for the same bytes; one descriptor over all of col[], offsets per lane)
                v4i x[PI_SMALL / 64];
#pragma unroll
                for (int r = 0; r < PI_SMALL / 64; ++r) {
                    const int idx = r * 64 + 4 * gl;
                    const int big = 0x7fffffff;
                    if (idx + 4 <= llen) {
                        x[r] = *reinterpret_cast<const v4i_a4 *>(lrow + idx);      // (4-byte aligned: global_load_dwordx4 takes it)
                    } else {                                                       // (the row's last entries: never past its end)
                        x[r].x = idx < llen ? lrow[idx] : big;
                        x[r].y = idx + 1 < llen ? lrow[idx + 1] : big;
                        x[r].z = idx + 2 < llen ? lrow[idx + 2] : big;
                        x[r].w = big;
                    }
                }
                const int32_t t0 = gl < slen ? srow[gl] : 0;                    // (the first slice of the shorter row rides along)
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int r = 0; r < PI_SMALL / 64; ++r) *reinterpret_cast<v4i *>(&Lg[r * 64 + 4 * gl]) = pad_tail(x[r], r * 64 + 4 * gl, llen);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                int32_t s_max = slen;                                          // rounds: the longest of the four shorter rows
                s_max = max(s_max, __shfl_xor(s_max, 16));
                s_max = max(s_max, __shfl_xor(s_max, 32));
                int cnt = 0;
                float acc = 0.0f;
                for (int s0 = 0; s0 < s_max; s0 += 16) {
                    const int si = s0 + gl;
                    const int32_t t = s0 == 0 ? t0 : (si < slen ? srow[si] : 0);
                    const int pos = lb_pow2(Lg, PI_SMALL_LG, t);
                    if (si < slen && Lg[pos] == t) {
                        ++cnt;
                        if (HAS_W) acc += (float)node_w[t];
                    }
                }
#pragma unroll
                for (int d = 8; d >= 1; d >>= 1) {                              // (within the 16 lanes of a group)
                    cnt += __shfl_xor(cnt, d);
                    acc += __shfl_xor(acc, d);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int cq = __builtin_amdgcn_readlane(cnt, q * 16);
                    const float aq = lane_get(acc, q * 16);
                    if (jg[q] >= 0 && lane == jg[q]) {
                        my_count = cq;
                        my_cn = (float)cq;
                        my_ws = (WT)aq;
                    }
                }
                __builtin_amdgcn_wave_barrier();                               // (the next four overwrite the staged rows)
            }
        }

#endif
        for (int j = 0; PART != 1 && j < 64; ++j) {
            const int32_t dju = __builtin_amdgcn_readlane(du_left, j);
            const int32_t djv = __builtin_amdgcn_readlane(dv_left, j);
            if (dju == 0 || djv == 0) continue;  // wave-uniform (also: lanes past the end of the list)
            const int64_t bju = eps_bcast64(ub, j), bjv = eps_bcast64(vb, j);
            const bool swapped = dju > djv;  // short row = v
            const int32_t slen = swapped ? djv : dju, llen = swapped ? dju : djv;
            const int64_t sbase = swapped ? bjv : bju, lbase = swapped ? bju : bjv;

            int cnt = 0;
            float acc_cn = 0.0f;
            WT acc_ws = 0;
            int q0 = qlen;
            // the slice's matches: counted; unit weights queue their node_w gathers (staged pairs), the rest multiply inline
            const bool staged = intersect_rows<ROW_CAP, ROW_INPLACE_RATIO>(
                col, sbase, slen, lbase, llen, L, lane, [&](const bool found, const int t, const int si, const int li, const bool staged) {
                    const uint64_t m = __ballot(found);
                    if (m == 0ull) return;
                    const int c = __popcll(m);
                    cnt += c;
                    if (DEFER && staged) {
                        if (qlen > PI_QCAP - 64) {
                            flush(j, q0);
                            q0 = 0;
                        }
                        const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
                        if (found) q[qlen + below] = (uint32_t)t;
                        qlen += c;
                    } else if (found) {
                        pair_products<HAS_VAL, HAS_W, WT>(val, node_w, sbase + si, lbase + li, swapped, t, acc_cn, acc_ws);
                    }
                });
            if (DEFER && staged) {
                if (cnt != 0 && lane == j) { my_count = cnt; my_cn = (float)cnt; my_qstart = q0; my_qcnt = qlen - q0; }
                continue;
            }
            if (cnt != 0) {  // wave-uniform
                float r_cn = (float)cnt;
                if (HAS_VAL) r_cn = eps_wave_sum(acc_cn);
                WT r_ws = 0;
                if (HAS_W) r_ws = eps_wave_sum(acc_ws);
                if (lane == j) { my_count = cnt; my_cn = r_cn; my_ws = r_ws; }
            }
        }
        if (PART != 1) flush(-1, 0);
        if (PART == 0 ? valid : valid && is_small == (PART == 1)) {
            if (out_count) out_count[p] = my_count;
            if (out_cn) out_cn[p] = my_cn;
            if (HAS_W && out_ws) out_ws[p] = my_ws;
        }
    };
    if (TKC == 1) {                  // (r04's loop, instruction for instruction: the next ticket is in flight while this chunk is scored)
        int64_t chunk = take();
        while (chunk < n_chunks) {
            const int64_t next = take();
            do_chunk(chunk);
            chunk = next;
        }
    } else {
        int64_t ticket = take();
        while (ticket * TKC < n_chunks) {
            const int64_t next = take();
            for (int64_t chunk = ticket * TKC; chunk < (ticket + 1) * TKC && chunk < n_chunks; ++chunk) do_chunk(chunk);
            ticket = next;
        }
    }
}

// {pairs whose longer row has at most PI_SMALL entries (and a non-empty shorter one), valid pairs} of every PI_CLS_STRIDE-th
// 64-pair chunk of the list -> cls[0], cls[1]: what decides, on the device, which launch shape scores the list.
#define PI_CLS_STRIDE 16
__global__ __launch_bounds__(PI_WAVES * 64) void pair_classify_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ pu,
                                                                      const int32_t *__restrict__ pv, int64_t n_pairs,
                                                                      unsigned int *__restrict__ cls)
{
    const int lane = threadIdx.x & 63;
    const int64_t n_chunks = (n_pairs + 63) >> 6;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    unsigned int small = 0u, all = 0u;
    for (int64_t c = wave * PI_CLS_STRIDE; c < n_chunks; c += n_waves * PI_CLS_STRIDE) {
        const int64_t p = c * 64 + lane;
        const bool valid = p < n_pairs;
        const int32_t nu = valid ? pu[p] : 0, nv = valid ? pv[p] : 0;
        const int32_t du = valid ? (int32_t)(rowptr[nu + 1] - rowptr[nu]) : 0, dv = valid ? (int32_t)(rowptr[nv + 1] - rowptr[nv]) : 0;
        const int32_t mx = du > dv ? du : dv, mn = du < dv ? du : dv;
        small += (unsigned int)__popcll(__ballot(valid && mn > 0 && mx <= PI_SMALL));
        all += (unsigned int)__popcll(__ballot(valid));
    }
    if (lane == 0 && all) {
        atomicAdd(&cls[0], small);
        atomicAdd(&cls[1], all);
    }
}

template <typename WT>
static int launch_pair_scores(const int64_t *rowptr, const int32_t *col, const float *val, const WT *node_w,
                              const int32_t *u, const int32_t *v, int64_t n_pairs, int32_t *count, float *cn,
                              WT *wsum, hipStream_t stream)
{
    if (n_pairs == 0) return EPS_OK;
    const int64_t n_chunks = (n_pairs + 63) / 64;
    int64_t blocks = (n_chunks + PI_WAVES - 1) / PI_WAVES;
    const int64_t max_blocks = (int64_t)eps_num_cus() * 8;  // 32 waves per CU
    if (blocks > max_blocks) blocks = max_blocks;
    unsigned int *counter = nullptr, *counter2 = nullptr, *cls = nullptr;
    int crc = eps_take_counter(&counter, stream, "eps_pair_scores");
    if (crc) return crc;
    dim3 grid((unsigned)blocks), block(PI_WAVES * 64);
    const bool hv = val != nullptr, hw = node_w != nullptr && wsum != nullptr;
    constexpr bool F32 = sizeof(WT) == 4;
    const unsigned int *no_cls = nullptr;
#define PI_LAUNCH(HV, HW, PART, CTR, CLS, TKV) \
    hipLaunchKernelGGL((pair_scores_kernel<HV, HW, WT, PART, TKV>), grid, block, 0, stream, rowptr, col, val, node_w, u, v, \
                       n_pairs, CTR, count, cn, wsum, CLS)
    if (hv && hw) PI_LAUNCH(true, true, 0, counter, no_cls, 1);
    else if (hv) PI_LAUNCH(true, false, 0, counter, no_cls, 1);
    else if (!F32) {
        if (hw) PI_LAUNCH(false, true, 0, counter, no_cls, 1);
        else PI_LAUNCH(false, false, 0, counter, no_cls, 1);
    } else {
        // Unit values, float32 weights (the evaluation lists of train_and_eval.py:108-136).  Which shape wins depends on the list: mostly
        // small pairs (uniform negatives) -> the split (small pairs four at a time in a launch of their own + the rest: 2^24 pairs
        // 3.40 ms against 4.09 for one pair at a time); mostly stored edges (hub-heavy) -> every pair one at a time, r04's body
        // (8.80 ms against 10.2 split).  A sample of the list is classified on the device (every 16th chunk: small pairs / pairs), all
        // three launches go out, and each looks at the two words and runs or returns -- no host read.
        crc = eps_take_counter(&counter2, stream, "eps_pair_scores");
        if (crc) return crc;
        crc = eps_take_counters8(&cls, stream, "eps_pair_scores");
        if (crc) return crc;
        const int64_t sampled = (n_chunks + PI_CLS_STRIDE - 1) / PI_CLS_STRIDE;
        int64_t cb = (sampled + PI_WAVES - 1) / PI_WAVES;
        if (cb > max_blocks) cb = max_blocks;
        hipLaunchKernelGGL(pair_classify_kernel, dim3((unsigned)cb), block, 0, stream, rowptr, u, v, n_pairs, cls);
        // (the split only runs on lists of mostly small pairs, where the launch of the longer pairs finds little to do: tickets of
        //  PI_TICKET chunks whatever the list's length -- 3 M negatives drew 47 k single-chunk tickets for 0.5 of their 1.16 ms)
        if (hw) {
            PI_LAUNCH(false, true, 1, counter, cls, 1);
            PI_LAUNCH(false, true, 2, counter2, cls, PI_TICKET);
            PI_LAUNCH(false, true, 0, counter, cls, 1);
        } else {
            PI_LAUNCH(false, false, 1, counter, cls, 1);
            PI_LAUNCH(false, false, 2, counter2, cls, PI_TICKET);
            PI_LAUNCH(false, false, 0, counter, cls, 1);
        }
    }
#undef PI_LAUNCH
    EPS_CHECK_LAUNCH("eps_pair_scores");
    return EPS_OK;
}

extern "C" int eps_pair_scores_limits(int32_t *small_max, int32_t *cap, int32_t *queue, int32_t *inplace_ratio, int32_t *ticket,
                                      int32_t *cls_stride)
{
    if (small_max) *small_max = PI_SMALL;
    if (cap) *cap = ROW_CAP;
    if (queue) *queue = PI_QCAP;
    if (inplace_ratio) *inplace_ratio = ROW_INPLACE_RATIO;
    if (ticket) *ticket = PI_TICKET;
    if (cls_stride) *cls_stride = PI_CLS_STRIDE;
    return EPS_OK;
}

extern "C" int eps_pair_scores(const int64_t *rowptr, const int32_t *col, const float *val, const float *node_w,
                               int64_t n_nodes, const int32_t *u, const int32_t *v, int64_t n_pairs,
                               int32_t *count, float *cn, float *wsum, void *stream)
{
    EPS_REQUIRE(n_pairs >= 0 && n_nodes >= 0, "eps_pair_scores: negative size");
    EPS_REQUIRE(n_pairs == 0 || (rowptr && col && u && v), "eps_pair_scores: null graph or pair pointer");
    EPS_REQUIRE(!(wsum && !node_w), "eps_pair_scores: wsum requested without node_w");
    EPS_REQUIRE(count || cn || wsum || n_pairs == 0, "eps_pair_scores: no output requested");
    return launch_pair_scores<float>(rowptr, col, val, node_w, u, v, n_pairs, count, cn, wsum, (hipStream_t)stream);
}

extern "C" int eps_pair_scores_f64(const int64_t *rowptr, const int32_t *col, const float *val,
                                   const double *node_w, int64_t n_nodes, const int32_t *u, const int32_t *v,
                                   int64_t n_pairs, int32_t *count, double *wsum, void *stream)
{
    EPS_REQUIRE(n_pairs >= 0 && n_nodes >= 0, "eps_pair_scores_f64: negative size");
    EPS_REQUIRE(n_pairs == 0 || (rowptr && col && u && v), "eps_pair_scores_f64: null graph or pair pointer");
    EPS_REQUIRE(!(wsum && !node_w), "eps_pair_scores_f64: wsum requested without node_w");
    EPS_REQUIRE(count || wsum || n_pairs == 0, "eps_pair_scores_f64: no output requested");
    return launch_pair_scores<double>(rowptr, col, val, node_w, u, v, n_pairs, count, nullptr, wsum,
                                      (hipStream_t)stream);
}

// ---------------------------------------------------------------- K2: node weight table
// Column sums in FLOAT64 atomics: exact -- hence independent of the arrival order -- for integer-valued adjacencies
// (every stored value of the reference's datasets is an integer: unit values, or collab's summed multi-edge counts)
// up to 2^53; the float32 table is the float64 sum rounded once.  (Float32 atomics were exact only below 2^24.)
__global__ void col_sums_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                const float *__restrict__ val, int64_t n_rows, double *__restrict__ colsum)
{
    // one wave per row, lanes stride the row: coalesced col/val reads
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < n_rows; r += n_waves) {
        const int64_t b = rowptr[r], e = rowptr[r + 1];
        for (int64_t k = b + lane; k < e; k += 64) atomicAdd(&colsum[col[k]], val ? (double)val[k] : 1.0);
    }
}

__global__ void round_f32_kernel(const double *__restrict__ x, int64_t n, float *__restrict__ y)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = (float)x[i];
}

template <typename ST, typename WT>
__global__ void node_weights_kernel(const ST *__restrict__ colsum, int64_t n, int mode, WT *__restrict__ w)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const WT s = (WT)colsum[i];
    WT m;
    if (sizeof(WT) == 4) m = (mode == EPS_W_AA) ? (WT)(1.0f / logf((float)s)) : (WT)(1.0f / (float)s);
    else m = (mode == EPS_W_AA) ? (WT)(1.0 / log((double)s)) : (WT)(1.0 / (double)s);
    if (isinf(m)) m = 0;
    w[i] = m;
}

extern "C" int eps_col_sums(const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                            int64_t n_cols, double *colsum_f64, float *colsum_f32, void *stream)
{
    EPS_REQUIRE(n_rows >= 0 && n_cols >= 0, "eps_col_sums: negative size");
    if (n_cols == 0) return EPS_OK;
    EPS_REQUIRE(colsum_f64 && (n_rows == 0 || (rowptr && col)), "eps_col_sums: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(colsum_f64, 0, (size_t)n_cols * sizeof(double), s) != hipSuccess) {
        eps_set_error("eps_col_sums: memset failed");
        return EPS_ELAUNCH;
    }
    if (n_rows > 0) {
        int64_t blocks = (n_rows + 3) / 4;
        const int64_t cap = (int64_t)eps_num_cus() * 16;
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(col_sums_kernel, dim3((unsigned)blocks), dim3(256), 0, s, rowptr, col, val, n_rows, colsum_f64);
    }
    if (colsum_f32)
        hipLaunchKernelGGL(round_f32_kernel, dim3((unsigned)((n_cols + 255) / 256)), dim3(256), 0, s, colsum_f64, n_cols,
                           colsum_f32);
    EPS_CHECK_LAUNCH("eps_col_sums");
    return EPS_OK;
}

extern "C" int eps_node_weights(const float *colsum, int64_t n, int mode, float *w, void *stream)
{
    EPS_REQUIRE(n >= 0 && (mode == EPS_W_AA || mode == EPS_W_RA), "eps_node_weights: bad size or mode");
    if (n == 0) return EPS_OK;
    EPS_REQUIRE(colsum && w, "eps_node_weights: null pointer");
    hipLaunchKernelGGL((node_weights_kernel<float, float>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, colsum, n, mode, w);
    EPS_CHECK_LAUNCH("eps_node_weights");
    return EPS_OK;
}

extern "C" int eps_node_weights_f64(const double *colsum, int64_t n, int mode, double *w, void *stream)
{
    EPS_REQUIRE(n >= 0 && (mode == EPS_W_AA || mode == EPS_W_RA), "eps_node_weights_f64: bad size or mode");
    if (n == 0) return EPS_OK;
    EPS_REQUIRE(colsum && w, "eps_node_weights_f64: null pointer");
    hipLaunchKernelGGL((node_weights_kernel<double, double>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, colsum, n, mode, w);
    EPS_CHECK_LAUNCH("eps_node_weights_f64");
    return EPS_OK;
}


// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void pair_intersect_warm_kernel() {}
extern "C" void eps_warm_pair_intersect(void *stream) { hipLaunchKernelGGL(pair_intersect_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

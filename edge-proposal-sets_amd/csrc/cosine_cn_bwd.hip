// Cosine-weighted common neighbours ('simplecos' / 'mlpcos'), gfx950: the backward of the raw score, for TRAINING the
// embedding (train_and_eval.py:31-96 pushes its loss through models.py:528-575 into emb.weight).
//
//   raw_p = sum_{w in N(u_p) & N(v_p)} c[(u_p, w)] * c[(v_p, w)],   c[e] = xhat_row(e) . xhat_col(e),
//   xhat_r = x'_r / nrm_r,  nrm_r = max(||x'_r||, 1e-8),  x' = x + (A @ x) / (rowsum(A) + 1e-6)
//
// Given g_p = dL/draw_p:
//   eps_pair_cn_backward:       gc[(u, w)] += g_p * c[(v, w)],  gc[(v, w)] += g_p * c[(u, w)]  per (pair, common neighbour):
//                               the walk of row_intersect.h with two adds per hit instead of a per-pair sum.  The adds are 64-bit
//                               FIXED-POINT integer atomics -- integer addition commutes, so gc does not depend on the order the
//                               pairs arrive in (float atomics would) -- at a scale taken from max |g_p| (one reduction on the
//                               device); a convert pass writes float32.
//   eps_cos_features_backward:  a_r = sum_{e = (r, w)} (gc[e] + gc[rev(e)]) * xhat_w  (both stored copies of an undirected entry
//                               are the same dot product; a self loop gets its factor 2 here), then the normalisation's backward
//                               gx'_r = (a_r - xhat_r (xhat_r . a_r)) / nrm_r, or a_r / 1e-8 where the clamp was active.  A row
//                               gather of the shape of eps_edge_cosines (one wave per row, the slot / chunk layout of
//                               cosine_common.h).  Optionally also gx'_r / deg_r: the operand of the smoothing's backward
//                               gx = gx' + A (gx' / deg), which is one eps_spmm_csr on a symmetric adjacency.
#include "cosine_common.h"
#include "row_intersect.h"

#define PB_WAVES 4            // waves per workgroup
#define PB_SUM_BITS 60        // |every fixed-point sum| < 2^(PB_SUM_BITS + 1)

// ---- max |g_p| -> its float32 bit pattern (non-negative floats order like unsigned integers; a maximum commutes) ------------
__global__ __launch_bounds__(256) void pb_absmax_kernel(const float *__restrict__ g, int64_t n, unsigned int *__restrict__ gmax_bits)
{
    unsigned int m = 0u;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned int b = __builtin_bit_cast(unsigned int, g[i]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int other = (unsigned int)__shfl_xor((int)m, o);
        m = other > m ? other : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(gmax_bits, m);
}

// The power of two the products g_p * c are multiplied by before they are rounded to integers: with max |g| < 2^(E - 126) (E its
// biased exponent) and |c| <= 2, |g c| 2^k < 2^shift for k = shift - (E - 126) - 1; a destination receives at most 2 * n_pairs
// terms, and shift = PB_SUM_BITS - ceil(log2(2 n_pairs)) (host) keeps every sum inside the int64.
__device__ __forceinline__ int pb_scale_log2(unsigned int gmax_bits, int shift) { return shift - ((int)(gmax_bits >> 23) - 126) - 1; }

__device__ __forceinline__ void pb_add(long long *__restrict__ fx, int64_t e, float g, float c, double scale)
{
    const long long t = __double2ll_rn((double)g * (double)c * scale);         // (exact product, exact scaling, one rounding)
    atomicAdd(reinterpret_cast<unsigned long long *>(fx + e), (unsigned long long)t);
}

__global__ __launch_bounds__(PB_WAVES * 64) void pair_cn_backward_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ c, int64_t n_rows,
    const int32_t *__restrict__ pu, const int32_t *__restrict__ pv, const float *__restrict__ g, int64_t n_pairs,
    unsigned int *__restrict__ next_chunk, const unsigned int *__restrict__ gmax_bits, int shift, long long *__restrict__ fx)
{
    __shared__ __attribute__((aligned(16))) int32_t s_rows[PB_WAVES][ROW_CAP];
    const unsigned int gb = *gmax_bits;
    if (gb == 0u) return;                                    // every g_p is zero: nothing to add
    const double scale = ldexp(1.0, pb_scale_log2(gb, shift));
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int32_t *L = s_rows[wib];
    const int64_t n_chunks = (n_pairs + 63) >> 6;

    // 64-pair chunks handed out dynamically, the next ticket drawn while the current chunk is worked on (pair_intersect.hip)
    int64_t chunk = take_chunk(next_chunk, lane);
    while (chunk < n_chunks) {
        const int64_t next = take_chunk(next_chunk, lane);
        const int64_t p = chunk * 64 + lane;
        bool valid = p < n_pairs;
        int32_t nu = valid ? pu[p] : 0, nv = valid ? pv[p] : 0;
        valid = valid && (uint32_t)nu < (uint64_t)n_rows && (uint32_t)nv < (uint64_t)n_rows;   // (an id outside the graph adds nothing)
        if (!valid) nu = nv = 0;
        const float gp = valid ? g[p] : 0.0f;
        valid = valid && gp != 0.0f;
        const int64_t ub = rowptr[nu], vb = rowptr[nv];
        const int32_t du = valid ? (int32_t)(rowptr[nu + 1] - ub) : 0;
        const int32_t dv = valid ? (int32_t)(rowptr[nv + 1] - vb) : 0;

        for (int j = 0; j < 64; ++j) {
            const int32_t dju = __builtin_amdgcn_readlane(du, j);
            const int32_t djv = __builtin_amdgcn_readlane(dv, j);
            if (dju == 0 || djv == 0) continue;              // wave-uniform (also: lanes past the end of the list)
            const int64_t bju = eps_bcast64(ub, j), bjv = eps_bcast64(vb, j);
            const float gj = lane_get(gp, j);
            // (the two ends are interchangeable here: a hit at (short row, si) and (long row, li) adds g c[long] to the short
            //  row's entry and g c[short] to the long row's; u == v makes them one entry that receives both)
            const bool swapped = dju > djv;
            const int32_t slen = swapped ? djv : dju, llen = swapped ? dju : djv;
            const int64_t sbase = swapped ? bjv : bju, lbase = swapped ? bju : bjv;

            auto two_adds = [&](const bool found, int, const int si, const int li, bool) {
                if (!found) return;
                const int64_t es = sbase + si, el = lbase + li;
                const float cs = c[es], cl = c[el];
                pb_add(fx, es, gj, cl, scale);
                pb_add(fx, el, gj, cs, scale);
            };
            intersect_rows<ROW_CAP, ROW_INPLACE_RATIO>(col, sbase, slen, lbase, llen, L, lane, two_adds);
        }
        chunk = next;
    }
}

__global__ __launch_bounds__(256) void pb_convert_kernel(const long long *__restrict__ fx, int64_t nnz,
                                                         const unsigned int *__restrict__ gmax_bits, int shift,
                                                         float *__restrict__ gc)
{
    const unsigned int gb = *gmax_bits;
    const double inv = gb ? ldexp(1.0, -pb_scale_log2(gb, shift)) : 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * blockDim.x)
        gc[i] = (float)((double)fx[i] * inv);
}

extern "C" int64_t eps_pair_cn_backward_workspace_bytes(int64_t nnz) { return nnz < 0 ? -1 : nnz * 8 + 16; }

extern "C" int eps_pair_cn_backward(const int64_t *rowptr, const int32_t *col, const float *c, int64_t n_rows, int64_t nnz,
                                    const int32_t *u, const int32_t *v, const float *g, int64_t n_pairs, float *gc,
                                    void *workspace, int64_t workspace_bytes, void *stream)
{
    EPS_REQUIRE(n_rows >= 0 && nnz >= 0 && n_pairs >= 0, "eps_pair_cn_backward: negative size (n_rows=%lld nnz=%lld n_pairs=%lld)",
                (long long)n_rows, (long long)nnz, (long long)n_pairs);
    EPS_REQUIRE(n_rows < (1ll << 31), "eps_pair_cn_backward: node ids are int32");
    if (nnz == 0) return EPS_OK;
    EPS_REQUIRE(n_rows > 0, "eps_pair_cn_backward: %lld entries in a graph without rows", (long long)nnz);
    EPS_REQUIRE(rowptr && col && c && gc, "eps_pair_cn_backward: null graph, cosine or output pointer");
    EPS_REQUIRE(n_pairs == 0 || (u && v && g), "eps_pair_cn_backward: null pair or gradient pointer");
    EPS_REQUIRE(workspace && ((uintptr_t)workspace % 8) == 0 && workspace_bytes >= eps_pair_cn_backward_workspace_bytes(nnz),
                "eps_pair_cn_backward: workspace missing, misaligned or smaller than eps_pair_cn_backward_workspace_bytes(%lld)",
                (long long)nnz);
    hipStream_t s = (hipStream_t)stream;
    long long *fx = (long long *)workspace;
    unsigned int *gmax = (unsigned int *)(fx + nnz);
    if (hipMemsetAsync(workspace, 0, (size_t)eps_pair_cn_backward_workspace_bytes(nnz), s) != hipSuccess) {
        eps_set_error("eps_pair_cn_backward: memset failed");
        return EPS_ELAUNCH;
    }
    int shift = PB_SUM_BITS;
    for (int64_t terms = 1; terms < 2 * n_pairs; terms <<= 1) --shift;
    const int64_t cap = (int64_t)eps_num_cus() * 8;
    if (n_pairs > 0) {
        int64_t rb = (n_pairs + 255) / 256;
        if (rb > cap) rb = cap;
        hipLaunchKernelGGL(pb_absmax_kernel, dim3((unsigned)rb), dim3(256), 0, s, g, n_pairs, gmax);
        unsigned int *counter = nullptr;
        const int crc = eps_take_counter(&counter, s, "eps_pair_cn_backward");
        if (crc) return crc;
        const int64_t n_chunks = (n_pairs + 63) / 64;
        int64_t blocks = (n_chunks + PB_WAVES - 1) / PB_WAVES;
        if (blocks > cap) blocks = cap;                  // 32 waves per CU
        hipLaunchKernelGGL(pair_cn_backward_kernel, dim3((unsigned)blocks), dim3(PB_WAVES * 64), 0, s, rowptr, col, c, n_rows, u,
                           v, g, n_pairs, counter, gmax, shift, fx);
    }
    int64_t cb = (nnz + 255) / 256;
    if (cb > cap * 4) cb = cap * 4;
    hipLaunchKernelGGL(pb_convert_kernel, dim3((unsigned)cb), dim3(256), 0, s, fx, nnz, gmax, shift, gc);
    EPS_CHECK_LAUNCH("eps_pair_cn_backward");
    return EPS_OK;
}

// ---- gx'_r = d raw / d x'_r ----------------------------------------------------------------------------------------------------
// One wave per row r; slot s gathers entries s, s + S, ... of the row (FLIGHT neighbour rows in flight per slot) scaled by the
// entry's gc[e] + gc[rev(e)], the slots' partial sums are combined with cross-slot shuffles: a_r.  Rows wider than NCR chunks
// go in column panels: each panel writes a_r to gxp, xhat_r . a_r accumulates over the panels, and a last pass (every lane
// re-reading what it wrote itself) applies the normalisation's backward.
template <int NCR, bool HAS_VAL>
__global__ __launch_bounds__(CC_THREADS) void cos_features_backward_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int64_t n_rows,
    const float *__restrict__ xhat, int64_t ldh, int32_t f, int32_t lg, const float *__restrict__ nrm,
    const int32_t *__restrict__ revpos, const float *__restrict__ gc, float *__restrict__ gxp, float *__restrict__ gxs, int64_t ldg)
{
    constexpr int FLIGHT = (CC_FLIGHT_VEC4 / NCR) > 0 ? (CC_FLIGHT_VEC4 / NCR) : 1;
    const int lane = threadIdx.x & 63;
    const int G = 1 << lg, S = 64 >> lg;
    const int slot = lane >> lg, j = lane & (G - 1);
    const int span = G * 4, panel = NCR * span;
    const bool multi = f > panel;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;

    for (int64_t r = wave; r < n_rows; r += n_waves) {
        const int64_t b = rowptr[r], e = rowptr[r + 1];
        float inv_deg = 0.f;
        if (gxs) {                           // 1 / (rowsum(A) + 1e-6) as the forward forms it
            float rs;
            if (HAS_VAL) {
                float p = 0.f;
                for (int64_t k = b + lane; k < e; k += 64) p += val[k];
                rs = eps_wave_sum(p);
            } else {
                rs = (float)(e - b);
            }
            inv_deg = 1.0f / (rs + 1e-6f);
        }
        const float *__restrict__ hr = xhat + r * ldh;
        float *__restrict__ gr = gxp + r * ldg;
        float dotp = 0.f;                    // this lane's part of xhat_r . a_r (identical in every slot)
        float4 keep[NCR];
        for (int32_t c0 = 0; c0 < f; c0 += panel) {
            float4 acc[NCR];
#pragma unroll
            for (int t = 0; t < NCR; ++t) acc[t] = eps_zero(float4());
            for (int64_t k0 = b; k0 < e; k0 += 64) {
                const int nk = (e - k0) < 64 ? (int)(e - k0) : 64;
                const int my_col = lane < nk ? col[k0 + lane] : 0;
                const float my_s = lane < nk ? gc[k0 + lane] + gc[rowptr[my_col] + revpos[k0 + lane]] : 0.f;
                for (int q0 = 0; q0 < nk; q0 += S * FLIGHT) {
                    int cw[FLIGHT];
                    float sw[FLIGHT];
                    float4 xv[FLIGHT][NCR];
#pragma unroll
                    for (int q = 0; q < FLIGHT; ++q) {
                        const int idx = q0 + slot + S * q;
                        cw[q] = __shfl(my_col, idx & 63);
                        sw[q] = __shfl(my_s, idx & 63);
                        if (idx >= nk) cw[q] = -1;
                    }
#pragma unroll
                    for (int q = 0; q < FLIGHT; ++q)
#pragma unroll
                        for (int t = 0; t < NCR; ++t) {
                            const int c = c0 + t * span + j * 4;
                            xv[q][t] = eps_zero(float4());
                            if (cw[q] >= 0 && c < f) xv[q][t] = cc_load(xhat + (int64_t)cw[q] * ldh, c, f, float4());
                        }
#pragma unroll
                    for (int q = 0; q < FLIGHT; ++q)
                        if (cw[q] >= 0)
#pragma unroll
                            for (int t = 0; t < NCR; ++t) eps_fma(acc[t], sw[q], xv[q][t]);
                }
            }
#pragma unroll
            for (int t = 0; t < NCR; ++t) {
                acc[t] = cc_xor_sum(acc[t], G, 64);          // the slots' partial sums: a_r in every slot
                const int c = c0 + t * span + j * 4;
                if (c < f) dotp += eps_dot(cc_load(hr, c, f, float4()), acc[t]);
                keep[t] = acc[t];
                if (multi && slot == 0 && c < f) cc_store(gr, c, f, acc[t]);
            }
        }
        dotp = cc_xor_sum(dotp, 1, G);
        const float nr = nrm[r];
        const bool clamped = nr <= 1e-8f;        // xhat_r = x'_r / 1e-8 there: the norm took no part
        const float proj = clamped ? 0.f : dotp;
        if (slot == 0) {
            float *__restrict__ sr = gxs ? gxs + r * ldg : nullptr;
            auto finish = [&](int c, const float4 &a) {
                const float4 xr = cc_load(hr, c, f, float4());
                const float4 o = make_float4((a.x - xr.x * proj) / nr, (a.y - xr.y * proj) / nr, (a.z - xr.z * proj) / nr,
                                             (a.w - xr.w * proj) / nr);
                cc_store(gr, c, f, o);
                if (sr) cc_store(sr, c, f, make_float4(o.x * inv_deg, o.y * inv_deg, o.z * inv_deg, o.w * inv_deg));
            };
            if (!multi) {
#pragma unroll
                for (int t = 0; t < NCR; ++t) {
                    const int c = t * span + j * 4;
                    if (c < f) finish(c, keep[t]);
                }
            } else {
                for (int32_t c = j * 4; c < f; c += span) finish(c, cc_load(gr, c, f, float4()));
            }
        }
        for (int64_t c = f + lane; c < ldg; c += 64) {               // pad columns: zero
            gr[c] = 0.f;
            if (gxs) gxs[r * ldg + c] = 0.f;
        }
    }
}

extern "C" int eps_cos_features_backward(const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                                         const float *xhat, int64_t ldh, int32_t f, const float *nrm, const int32_t *revpos,
                                         const float *gc, float *gxp, float *gxs, int64_t ldg, void *stream)
{
    EPS_REQUIRE(n_rows >= 0 && f >= 1 && ldh >= f && ldg >= f, "eps_cos_features_backward: bad shape (n_rows=%lld f=%d ldh=%lld ldg=%lld)",
                (long long)n_rows, f, (long long)ldh, (long long)ldg);
    if (n_rows == 0) return EPS_OK;
    EPS_REQUIRE(rowptr && col && xhat && nrm && revpos && gc && gxp, "eps_cos_features_backward: null pointer");
    EPS_REQUIRE(n_rows < (1ll << 31), "eps_cos_features_backward: node ids are int32");
    EPS_REQUIRE(ldh % 4 == 0 && ((uintptr_t)xhat % 16) == 0 && ldg % 4 == 0 && ((uintptr_t)gxp % 16) == 0 && ((uintptr_t)gxs % 16) == 0,
                "eps_cos_features_backward: xhat, gxp and gxs need 16-byte aligned rows (ldh %% 4 == 0, ldg %% 4 == 0)");
    const int lg = cc_lanes_log2(f, 4);
    const int64_t chunks = (f + (4ll << lg) - 1) / (4ll << lg);
    const int ncr = cc_reg_chunks(chunks);
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = cc_blocks(n_rows);
#define CB_LAUNCH(NCR, HV)                                                                                                      \
    hipLaunchKernelGGL((cos_features_backward_kernel<NCR, HV>), dim3(blocks), dim3(CC_THREADS), 0, s, rowptr, col, val, n_rows,  \
                       xhat, ldh, f, lg, nrm, revpos, gc, gxp, gxs, ldg)
#define CB_LAUNCH_V(HV)                                                                                                         \
    do {                                                                                                                        \
        if (ncr == 1) CB_LAUNCH(1, HV);                                                                                         \
        else if (ncr == 2) CB_LAUNCH(2, HV);                                                                                    \
        else if (ncr == 4) CB_LAUNCH(4, HV);                                                                                    \
        else CB_LAUNCH(8, HV);                                                                                                  \
    } while (0)
    if (val) CB_LAUNCH_V(true);
    else CB_LAUNCH_V(false);
#undef CB_LAUNCH_V
#undef CB_LAUNCH
    EPS_CHECK_LAUNCH("eps_cos_features_backward");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void cosine_cn_bwd_warm_kernel() {}
extern "C" void eps_warm_cosine_cn_bwd(void *stream) { hipLaunchKernelGGL(cosine_cn_bwd_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

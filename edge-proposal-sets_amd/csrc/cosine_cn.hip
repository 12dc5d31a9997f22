// Cosine-weighted common neighbours ('simplecos' / 'mlpcos' of CommonNeighborsPredictor), gfx950: the prologue.
//
// The reference (models.py:556-575) computes, per (pair, common neighbour w), two F.cosine_similarity calls on rows of
//   x' = x + (A @ x) / (rowsum(A) + 1e-6)
// and sums their product per pair.  Both factors depend on ONE stored entry only -- cos(x'_u, x'_w) is a property of
// (u, w) -- so the score is the ordinary edge-valued common-neighbour sum over a graph whose values are cosines.  This
// unit builds that graph's values; the pair kernels / the fused expansion then score it like any valued graph.
//
//   eps_cos_node_features: xhat_i = x'_i / max(||x'_i||_2, 1e-8)   (F.cosine_similarity's per-vector clamp)
//   eps_edge_cosines:      c[e] = xhat_row(e) . xhat_col(e)        (one dot per stored entry)
//
// Both are row gathers like the SpMM: one wave per row, the row's part in registers, neighbour rows streamed.  A wave's
// 64 lanes form S = 64 / G slots of G lanes; a slot covers a feature row with G lanes x VEC floats per chunk (G the
// smallest power of two that spans the row, at most 64), so narrow rows (ppa: 58 features, padded to 64 = 16 lanes of
// float4) keep four neighbour rows per wave load instead of leaving 48 lanes idle.  Up to CC_REG_CHUNKS chunks live in
// registers; wider rows (F in the thousands) stream the rest (node features: column panels, normalised at the end;
// edge cosines: the row's chunks beyond the registers are re-read, from the cache).
#include "cosine_common.h"

// ---- xhat = normalise(x + (A @ x) / (rowsum(A) + 1e-6)) ---------------------------------------------------------------
// One wave per row r.  Slot s gathers entries s, s + S, ... of row r (FLIGHT rows in flight per slot), the slots' partial
// sums are combined with cross-slot shuffles, then x'_r, its squared norm (over the G lanes of a slot) and the clamped
// division.  Rows wider than NCR chunks are done in column panels of NCR chunks: each panel writes x' unnormalised, the
// row's norm accumulates over the panels, and a last pass (every lane re-reading what it wrote itself) divides.
template <int VEC, int NCR, bool HAS_VAL>
__global__ __launch_bounds__(CC_THREADS) void cos_node_features_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int64_t n_rows,
    const float *__restrict__ x, int64_t ldx, int32_t f, int32_t lg, float *__restrict__ xhat, int64_t ldh,
    float *__restrict__ nrm_out)
{
    using V = typename eps_vec<VEC>::type;
    constexpr int FLIGHT = (CC_FLIGHT_VEC4 * 4 / VEC / NCR) > 0 ? (CC_FLIGHT_VEC4 * 4 / VEC / NCR) : 1;
    const int lane = threadIdx.x & 63;
    const int G = 1 << lg, S = 64 >> lg;
    const int slot = lane >> lg, j = lane & (G - 1);
    const int span = G * VEC, panel = NCR * span;
    const bool multi = f > panel;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;

    for (int64_t r = wave; r < n_rows; r += n_waves) {
        const int64_t b = rowptr[r], e = rowptr[r + 1];
        float rs;
        if (HAS_VAL) {                       // rowsum(A) with A's values (models.py:546, collab is weighted)
            float p = 0.f;
            for (int64_t k = b + lane; k < e; k += 64) p += val[k];
            rs = eps_wave_sum(p);
        } else {
            rs = (float)(e - b);
        }
        const float deg = rs + 1e-6f;
        const float *__restrict__ xr = x + r * ldx;
        float *__restrict__ hr = xhat + r * ldh;
        float ss = 0.f;                      // this lane's part of ||x'_r||^2 (identical in every slot)
        V keep[NCR];
        for (int32_t c0 = 0; c0 < f; c0 += panel) {
            V acc[NCR];
#pragma unroll
            for (int t = 0; t < NCR; ++t) acc[t] = eps_zero(V());
            for (int64_t k0 = b; k0 < e; k0 += 64) {
                const int nk = (e - k0) < 64 ? (int)(e - k0) : 64;
                const int my_col = lane < nk ? col[k0 + lane] : 0;
                const float my_val = HAS_VAL ? (lane < nk ? val[k0 + lane] : 0.f) : 1.f;
                for (int q0 = 0; q0 < nk; q0 += S * FLIGHT) {
                    int cw[FLIGHT];
                    float vw[FLIGHT];
                    V xv[FLIGHT][NCR];
#pragma unroll
                    for (int q = 0; q < FLIGHT; ++q) {
                        const int idx = q0 + slot + S * q;
                        cw[q] = __shfl(my_col, idx & 63);
                        vw[q] = HAS_VAL ? __shfl(my_val, idx & 63) : 1.f;
                        if (idx >= nk) cw[q] = -1;
                    }
#pragma unroll
                    for (int q = 0; q < FLIGHT; ++q)
#pragma unroll
                        for (int t = 0; t < NCR; ++t) {
                            const int c = c0 + t * span + j * VEC;
                            xv[q][t] = eps_zero(V());
                            if (cw[q] >= 0 && c < f) xv[q][t] = cc_load(x + (int64_t)cw[q] * ldx, c, f, V());
                        }
#pragma unroll
                    for (int q = 0; q < FLIGHT; ++q)
                        if (cw[q] >= 0)
#pragma unroll
                            for (int t = 0; t < NCR; ++t) eps_fma(acc[t], vw[q], xv[q][t]);
                }
            }
#pragma unroll
            for (int t = 0; t < NCR; ++t) {
                acc[t] = cc_xor_sum(acc[t], G, 64);          // the slots' partial sums: (A @ x)_r in every slot
                const int c = c0 + t * span + j * VEC;
                V xp = eps_zero(V());
                if (c < f) xp = cc_axpy_div(cc_load(xr, c, f, V()), acc[t], deg);
                ss += eps_dot(xp, xp);
                keep[t] = xp;
                if (multi && slot == 0 && c < f) cc_store(hr, c, f, xp);
            }
        }
        ss = cc_xor_sum(ss, 1, G);
        const float nrm = fmaxf(sqrtf(ss), 1e-8f);
        if (nrm_out && lane == 0) nrm_out[r] = nrm;             // (kept for the backward: eps_cos_node_features_nrm)
        if (slot == 0) {
            if (!multi) {
#pragma unroll
                for (int t = 0; t < NCR; ++t) {
                    const int c = t * span + j * VEC;
                    if (c < f) cc_store(hr, c, f, cc_div(keep[t], nrm));
                }
            } else {
                for (int32_t c = j * VEC; c < f; c += span) cc_store(hr, c, f, cc_div(cc_load(hr, c, f, V()), nrm));
            }
        }
        for (int64_t c = f + lane; c < ldh; c += 64) hr[c] = 0.f;    // pad columns: zero
    }
}

// ---- c[e] = xhat_row(e) . xhat_col(e) ------------------------------------------------------------------------------------
// One wave per row r, xhat_r (its first NCR chunks) in registers, slot s takes entries s, s + S, ...: FLIGHT neighbour rows
// in flight per slot, one dot per entry (reduced over the slot's G lanes).  With revpos (symmetric pattern) row r takes only
// its entries w >= r -- a suffix of the ascending row -- and writes the value to (r, w) and to (w, r) = rowptr[w] +
// revpos[e]: each undirected entry is computed once, and no two waves write one position.
template <int NCR>
__global__ __launch_bounds__(CC_THREADS) void edge_cosines_kernel(const int64_t *__restrict__ rowptr,
                                                                   const int32_t *__restrict__ col, int64_t n_rows,
                                                                   const float *__restrict__ xhat, int64_t ldh, int32_t f,
                                                                   int32_t lg, const int32_t *__restrict__ revpos,
                                                                   float *__restrict__ c_out)
{
    constexpr int FLIGHT = (CC_FLIGHT_VEC4 / NCR) > 0 ? (CC_FLIGHT_VEC4 / NCR) : 1;
    const int lane = threadIdx.x & 63;
    const int G = 1 << lg, S = 64 >> lg;
    const int slot = lane >> lg, j = lane & (G - 1);
    const int span = G * 4;
    const int nc = (f + span - 1) / span;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;

    for (int64_t r = wave; r < n_rows; r += n_waves) {
        int64_t b = rowptr[r];
        const int64_t e = rowptr[r + 1];
        if (revpos) b = eps_lower_bound(col, b, e, r);      // first entry with col >= r (wave-uniform)
        if (b >= e) continue;
        const float *__restrict__ hr = xhat + r * ldh;
        float4 xr[NCR];
#pragma unroll
        for (int t = 0; t < NCR; ++t) {
            const int c = t * span + j * 4;
            xr[t] = c < f ? cc_load(hr, c, f, float4()) : eps_zero(float4());
        }
        for (int64_t k0 = b; k0 < e; k0 += 64) {
            const int nk = (e - k0) < 64 ? (int)(e - k0) : 64;
            const int my_col = lane < nk ? col[k0 + lane] : 0;
            for (int q0 = 0; q0 < nk; q0 += S * FLIGHT) {
                int cw[FLIGHT];
                float d[FLIGHT];
                float4 xw[FLIGHT][NCR];
#pragma unroll
                for (int q = 0; q < FLIGHT; ++q) {
                    const int idx = q0 + slot + S * q;
                    cw[q] = __shfl(my_col, idx & 63);
                    if (idx >= nk) cw[q] = -1;
                    d[q] = 0.f;
                }
#pragma unroll
                for (int q = 0; q < FLIGHT; ++q)
#pragma unroll
                    for (int t = 0; t < NCR; ++t) {
                        const int c = t * span + j * 4;
                        xw[q][t] = eps_zero(float4());
                        if (cw[q] >= 0 && c < f) xw[q][t] = cc_load(xhat + (int64_t)cw[q] * ldh, c, f, float4());
                    }
#pragma unroll
                for (int q = 0; q < FLIGHT; ++q)
#pragma unroll
                    for (int t = 0; t < NCR; ++t) d[q] += eps_dot(xr[t], xw[q][t]);
                for (int t = NCR; t < nc; ++t) {     // chunks beyond the registers (F > NCR x 4G): the row re-read from cache
                    const int c = t * span + j * 4;
                    if (c >= f) break;
                    const float4 xrt = cc_load(hr, c, f, float4());
#pragma unroll
                    for (int q = 0; q < FLIGHT; ++q)
                        if (cw[q] >= 0) d[q] += eps_dot(xrt, cc_load(xhat + (int64_t)cw[q] * ldh, c, f, float4()));
                }
#pragma unroll
                for (int q = 0; q < FLIGHT; ++q) {
                    const float dot = cc_xor_sum(d[q], 1, G);
                    if (j == 0 && cw[q] >= 0) {
                        const int64_t pos = k0 + q0 + slot + S * q;
                        c_out[pos] = dot;
                        if (revpos && cw[q] != r) c_out[rowptr[cw[q]] + revpos[pos]] = dot;
                    }
                }
            }
        }
    }
}

static int cos_node_features(const char *who, const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                             const float *x, int64_t ldx, int32_t f, float *xhat, int64_t ldh, float *nrm, bool want_nrm,
                             void *stream)
{
    EPS_REQUIRE(n_rows >= 0 && f >= 1 && ldx >= f && ldh >= f, "%s: bad shape (n_rows=%lld f=%d ldx=%lld ldh=%lld)", who,
                (long long)n_rows, f, (long long)ldx, (long long)ldh);
    if (n_rows == 0) return EPS_OK;
    EPS_REQUIRE(rowptr && col && x && xhat && (nrm || !want_nrm), "%s: null pointer", who);
    EPS_REQUIRE(n_rows < (1ll << 31), "%s: node ids are int32", who);
    const bool vec4 = ldx % 4 == 0 && ((uintptr_t)x % 16) == 0 && ldh % 4 == 0 && ((uintptr_t)xhat % 16) == 0;
    const int vec = vec4 ? 4 : 1;
    const int lg = cc_lanes_log2(f, vec);
    const int64_t chunks = (f + ((int64_t)vec << lg) - 1) / ((int64_t)vec << lg);
    const int ncr = cc_reg_chunks(chunks);
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = cc_blocks(n_rows);
#define CC_NODE(VEC, NCR, HV)                                                                                          \
    hipLaunchKernelGGL((cos_node_features_kernel<VEC, NCR, HV>), dim3(blocks), dim3(CC_THREADS), 0, s, rowptr, col, val, \
                       n_rows, x, ldx, f, lg, xhat, ldh, nrm)
#define CC_NODE_V(VEC, HV)                                                                                             \
    do {                                                                                                               \
        if (ncr == 1) CC_NODE(VEC, 1, HV);                                                                             \
        else if (ncr == 2) CC_NODE(VEC, 2, HV);                                                                        \
        else if (ncr == 4) CC_NODE(VEC, 4, HV);                                                                        \
        else CC_NODE(VEC, 8, HV);                                                                                      \
    } while (0)
    if (vec4) {
        if (val) CC_NODE_V(4, true);
        else CC_NODE_V(4, false);
    } else {
        if (val) CC_NODE_V(1, true);
        else CC_NODE_V(1, false);
    }
#undef CC_NODE_V
#undef CC_NODE
    EPS_CHECK_LAUNCH(who);
    return EPS_OK;
}

extern "C" int eps_cos_node_features(const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                                     const float *x, int64_t ldx, int32_t f, float *xhat, int64_t ldh, void *stream)
{
    return cos_node_features("eps_cos_node_features", rowptr, col, val, n_rows, x, ldx, f, xhat, ldh, nullptr, false, stream);
}

extern "C" int eps_cos_node_features_nrm(const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                                         const float *x, int64_t ldx, int32_t f, float *xhat, int64_t ldh, float *nrm,
                                         void *stream)
{
    return cos_node_features("eps_cos_node_features_nrm", rowptr, col, val, n_rows, x, ldx, f, xhat, ldh, nrm, true, stream);
}

extern "C" int eps_edge_cosines(const int64_t *rowptr, const int32_t *col, int64_t n_rows, const float *xhat, int64_t ldh,
                                int32_t f, const int32_t *revpos, float *c, void *stream)
{
    EPS_REQUIRE(n_rows >= 0 && f >= 1 && ldh >= f, "eps_edge_cosines: bad shape (n_rows=%lld f=%d ldh=%lld)",
                (long long)n_rows, f, (long long)ldh);
    if (n_rows == 0) return EPS_OK;
    EPS_REQUIRE(rowptr && col && xhat && c, "eps_edge_cosines: null pointer");
    EPS_REQUIRE(n_rows < (1ll << 31), "eps_edge_cosines: node ids are int32");
    EPS_REQUIRE(ldh % 4 == 0 && ((uintptr_t)xhat % 16) == 0,
                "eps_edge_cosines: xhat needs 16-byte aligned rows (ldh %% 4 == 0; eps_cos_node_features output)");
    const int lg = cc_lanes_log2(f, 4);
    const int64_t chunks = (f + (4ll << lg) - 1) / (4ll << lg);
    const int ncr = cc_reg_chunks(chunks);
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = cc_blocks(n_rows);
#define CC_EDGE(NCR)                                                                                                   \
    hipLaunchKernelGGL((edge_cosines_kernel<NCR>), dim3(blocks), dim3(CC_THREADS), 0, s, rowptr, col, n_rows, xhat, ldh, \
                       f, lg, revpos, c)
    if (ncr == 1) CC_EDGE(1);
    else if (ncr == 2) CC_EDGE(2);
    else if (ncr == 4) CC_EDGE(4);
    else CC_EDGE(8);
#undef CC_EDGE
    EPS_CHECK_LAUNCH("eps_edge_cosines");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void cosine_cn_warm_kernel() {}
extern "C" void eps_warm_cosine_cn(void *stream) { hipLaunchKernelGGL(cosine_cn_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

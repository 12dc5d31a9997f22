// Graph attention aggregate (GATConv) with the softmax fused into the gather, gfx950, float32.
//
//   out[i,h,:] = sum_{j in N(i) + {i}} alpha_ijh z[j,h,:] + bias,   alpha_i.h = softmax_j LeakyReLU(s_src[j,h] + s_dst[i,h])
//
// N(i): the stored entries of row i with col != i, plus i itself exactly once (a stored self loop is not counted twice; stored
// values are not read).  The structure is spmm_csr_kernel's: one wave per row, the 64 lanes cover 256 feature columns as float4
// (a lane's head is column / C, C = f / heads, C % 4 == 0: a float4 never straddles two heads), column ids are fetched 64 at a
// time, GA_FLIGHT neighbour rows are in flight per wave.  Per row:
//   pass 1   m_h = max_j e_ijh per head, over the entries and the self loop: reads only the small score table;
//   pass 2   per chunk of 64 entries, lane k computes p = expf(e - m_h) of ITS entry for every head into a wave-private LDS
//            tile [head][entry]; the gather loop reads the weight of entry q for the lane's own head from the tile (one
//            ds_read_b32, <= 8 distinct addresses per wave) and accumulates l_h += p, acc += p z[j];
//   finish   acc / l (one true division), + bias, ReLU.  alpha is never written.  lse = m + logf(l) is kept for the backward.
// ORDER (declared): the self loop comes FIRST, then the stored entries in stored order (ascending column for a sorted CSR); a
// stored entry with col == i contributes weight 0 at its place.  The sums are sequential in that order in every lane, so a row's
// output is a pure function of the row: the same bits on a second call and from any row block (``row0``).
//
// Backward (symmetric pattern; two gather launches, no floating-point atomics, no per-entry cross-lane reduction).  With
// alpha_ij = exp(e_ij - lse_i), w_ij = alpha_ij * (raw_ij > 0 ? 1 : slope), D_ih = <gout[i,h,:], out_nobias[i,h,:]> and
// ds_ij = w_ij (<gout[i,h,:], z[j,h,:]> - D_ih), both sums of ds are taken by linearity of the dot product:
//   launch 1, row i over z rows:     g_s_dst[i,h] = <gout[i,h,:], sum_j w_ij z[j,h,:]> - D_ih sum_j w_ij;   D is written out too;
//   launch 2, row j over gout rows:  gz[j] = sum_i alpha_ij gout[i];   g_s_src[j,h] = <z[j,h,:], sum_i w_ij gout[i,h,:]> - sum_i w_ij D_ih.
// Each is one weighted gather (two accumulators in launch 2) and ONE per-head dot product per row, reduced across the lanes of a
// head through a wave-private LDS strip in a fixed order.  The same self-first order as the forward.
#include "eps_common.h"

#include <type_traits>

#define GA_FLIGHT 16        // neighbour rows in flight per wave
#define GA_MAX_HEADS 8
#define GA_TILE_LD 65       // tile[head][entry] row length: 64 entries + 1 (a wave's reads for one entry then fall on distinct banks)
#define GA_WAVES 4          // waves per workgroup

__device__ __forceinline__ float ga_leaky(float raw, float slope) { return raw > 0.f ? raw : raw * slope; }

// Per-head sums of one value per lane (lane L holds columns c0 + 4L ..): lane h < heads adds, in ascending lane order, the lanes
// whose columns belong to head h, and returns the sum (other lanes: 0).  ``strip``: 64 wave-private floats.
__device__ __forceinline__ float ga_head_sum(float part, float *strip, int lane, int c0, int f, int heads, int C)
{
    lds_wave_sync();
    strip[lane] = part;
    lds_wave_sync();
    float s = 0.f;
    if (lane < heads) {
        int lo = lane * C, hi = lo + C;
        if (lo < c0) lo = c0;
        if (hi > c0 + 256) hi = c0 + 256;
        if (hi > f) hi = f;
        for (int c = lo; c < hi; c += 4) s += strip[(c - c0) >> 2];
    }
    return s;
}

// The gather of one row: acc (+ acc2) += weight x[col]; ``w1`` / ``w2`` / ``w3``: tile rows of this lane's head (w3: a scalar
// side sum).  NACC = 1: acc += w1 x, l += w1.  NACC = 2: acc += w1 x, acc2 += w2 x, l += w3.
template <int NACC>
__device__ __forceinline__ void ga_gather(const float *__restrict__ x, int64_t ldx, int c, bool act, int my_col, int nk,
                                          const float *w1, const float *w2, const float *w3, float4 &acc, float4 &acc2, float &l)
{
    auto group = [&](int j, auto guarded) {
        constexpr bool G = decltype(guarded)::value;
        int cj[GA_FLIGHT];
        float4 xv[GA_FLIGHT];
#pragma unroll
        for (int q = 0; q < GA_FLIGHT; ++q) cj[q] = __builtin_amdgcn_readlane(my_col, (j + q) & 63);
#pragma unroll
        for (int q = 0; q < GA_FLIGHT; ++q) {
            xv[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((!G || j + q < nk) && act) xv[q] = *reinterpret_cast<const float4 *>(x + (int64_t)cj[q] * ldx + c);
        }
#pragma unroll
        for (int q = 0; q < GA_FLIGHT; ++q) {
            if (!G || j + q < nk) {
                eps_fma(acc, w1[j + q], xv[q]);
                if (NACC == 2) {
                    eps_fma(acc2, w2[j + q], xv[q]);
                    l += w3[j + q];
                } else {
                    l += w1[j + q];
                }
            }
        }
    };
    int j = 0;
    for (; j + GA_FLIGHT <= nk; j += GA_FLIGHT) group(j, std::false_type{});
    if (j < nk) group(j, std::true_type{});
}

// ------------------------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(64 * GA_WAVES) void gat_aggregate_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t row0, int64_t n_rows, const float *__restrict__ z,
    int64_t ldz, int heads, int f, const float *__restrict__ s_src, const float *__restrict__ s_dst, int64_t lds, float slope,
    const float *__restrict__ bias, int relu, float *__restrict__ out, int64_t ldo, float *__restrict__ lse)
{
    __shared__ float tile_all[GA_WAVES][GA_MAX_HEADS * GA_TILE_LD];
    __shared__ float mx_all[GA_WAVES][GA_MAX_HEADS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float *tile = tile_all[wv], *mx = mx_all[wv];
    const int C = f / heads;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;

    for (int64_t r = wave; r < n_rows; r += n_waves) {
        const int64_t b = rowptr[r], e = rowptr[r + 1];
        const int64_t self = row0 + r;
        const float *sd = s_dst + self * lds, *ss_self = s_src + self * lds;
        // pass 1: the row's maximum per head (a stored self loop has the self loop's own score: it may take part)
        lds_wave_sync();
        for (int h = 0; h < heads; ++h) {
            const float d = sd[h];
            float m = ga_leaky(ss_self[h] + d, slope);
            for (int64_t k = b + lane; k < e; k += 64) m = fmaxf(m, ga_leaky(s_src[(int64_t)col[k] * lds + h] + d, slope));
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
            if (lane == 0) mx[h] = m;
        }
        lds_wave_sync();
        for (int c0 = 0; c0 < f; c0 += 256) {
            const int c = c0 + lane * 4;
            const bool act = c < f;
            const int hl = act ? c / C : 0;
            const float *w = tile + hl * GA_TILE_LD;
            // the self loop first
            float l = expf(ga_leaky(ss_self[hl] + sd[hl], slope) - mx[hl]);
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), none = acc;
            if (act) eps_fma(acc, l, *reinterpret_cast<const float4 *>(z + self * ldz + c));
            for (int64_t k0 = b; k0 < e; k0 += 64) {
                const int nk = (e - k0) < 64 ? (int)(e - k0) : 64;
                const int my_col = lane < nk ? col[k0 + lane] : 0;
                const bool live = lane < nk && my_col != self;
                lds_wave_sync();                      // (the previous chunk's reads of the tile are done)
                for (int h = 0; h < heads; ++h) {
                    float p = 0.f;
                    if (live) p = expf(ga_leaky(s_src[(int64_t)my_col * lds + h] + sd[h], slope) - mx[h]);
                    tile[h * GA_TILE_LD + lane] = p;
                }
                lds_wave_sync();
                ga_gather<1>(z, ldz, c, act, my_col, nk, w, w, w, acc, none, l);
            }
            if (act) {
                float a[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float t = a[i] / l;
                    if (bias) t += bias[c + i];
                    if (relu) t = t > 0.f ? t : 0.f;
                    a[i] = t;
                }
                *reinterpret_cast<float4 *>(out + r * ldo + c) = make_float4(a[0], a[1], a[2], a[3]);
                if (lse && c % C == 0) lse[r * heads + hl] = mx[hl] + logf(l);
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- backward
// Launch 1 (row i, gathers z): D[i,h] and g_s_dst[i,h].
__global__ __launch_bounds__(64 * GA_WAVES) void gat_backward_dst_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t n, const float *__restrict__ z, int64_t ldz, int heads,
    int f, const float *__restrict__ s_src, const float *__restrict__ s_dst, int64_t lds, float slope, const float *__restrict__ lse,
    const float *__restrict__ outnb, int64_t ldo, const float *__restrict__ gout, int64_t ldg, float *__restrict__ dwork,
    float *__restrict__ g_s_dst)
{
    __shared__ float tile_all[GA_WAVES][GA_MAX_HEADS * GA_TILE_LD];
    __shared__ float strip_all[GA_WAVES][64];
    __shared__ float ws_all[GA_WAVES][GA_MAX_HEADS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float *tile = tile_all[wv], *strip = strip_all[wv], *wsum = ws_all[wv];
    const int C = f / heads;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;

    for (int64_t r = wave; r < n; r += n_waves) {
        const int64_t b = rowptr[r], e = rowptr[r + 1];
        const float *sd = s_dst + r * lds, *ss_self = s_src + r * lds, *ls = lse + r * heads;
        float dsum = 0.f, tsum = 0.f;                 // lane h < heads: D[r,h] and <gout, sum_j w z[j]>
        for (int c0 = 0; c0 < f; c0 += 256) {
            const int c = c0 + lane * 4;
            const bool act = c < f;
            const int hl = act ? c / C : 0;
            const float *w = tile + hl * GA_TILE_LD;
            const float raw0 = ss_self[hl] + sd[hl];
            const float a0 = expf(ga_leaky(raw0, slope) - ls[hl]);
            float l = raw0 > 0.f ? a0 : a0 * slope;   // sum_j w_ij of this lane's head, the self loop first
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), none = acc, go = acc, ob = acc;
            if (act) {
                eps_fma(acc, l, *reinterpret_cast<const float4 *>(z + r * ldz + c));
                go = *reinterpret_cast<const float4 *>(gout + r * ldg + c);
                ob = *reinterpret_cast<const float4 *>(outnb + r * ldo + c);
            }
            for (int64_t k0 = b; k0 < e; k0 += 64) {
                const int nk = (e - k0) < 64 ? (int)(e - k0) : 64;
                const int my_col = lane < nk ? col[k0 + lane] : 0;
                const bool live = lane < nk && my_col != r;
                lds_wave_sync();
                for (int h = 0; h < heads; ++h) {
                    float p = 0.f;
                    if (live) {
                        const float raw = s_src[(int64_t)my_col * lds + h] + sd[h];
                        p = expf(ga_leaky(raw, slope) - ls[h]);
                        if (!(raw > 0.f)) p *= slope;
                    }
                    tile[h * GA_TILE_LD + lane] = p;
                }
                lds_wave_sync();
                ga_gather<1>(z, ldz, c, act, my_col, nk, w, w, w, acc, none, l);
            }
            dsum += ga_head_sum(eps_dot(go, ob), strip, lane, c0, f, heads, C);
            tsum += ga_head_sum(eps_dot(go, acc), strip, lane, c0, f, heads, C);
            lds_wave_sync();
            if (act && c % C == 0) wsum[hl] = l;      // (every lane of a head holds the same l)
            lds_wave_sync();
        }
        if (lane < heads) {
            dwork[r * heads + lane] = dsum;
            g_s_dst[r * heads + lane] = tsum - dsum * wsum[lane];
        }
    }
}

// Launch 2 (row j, gathers gout over the transposed = same pattern): gz[j] and g_s_src[j,h].
__global__ __launch_bounds__(64 * GA_WAVES) void gat_backward_src_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t n, const float *__restrict__ z, int64_t ldz, int heads,
    int f, const float *__restrict__ s_src, const float *__restrict__ s_dst, int64_t lds, float slope, const float *__restrict__ lse,
    const float *__restrict__ gout, int64_t ldg, const float *__restrict__ dwork, float *__restrict__ gz, int64_t ldgz,
    float *__restrict__ g_s_src)
{
    __shared__ float tile_all[GA_WAVES][3 * GA_MAX_HEADS * GA_TILE_LD];
    __shared__ float strip_all[GA_WAVES][64];
    __shared__ float ws_all[GA_WAVES][GA_MAX_HEADS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float *tile = tile_all[wv], *strip = strip_all[wv], *wsum = ws_all[wv];
    float *tile_w = tile + GA_MAX_HEADS * GA_TILE_LD, *tile_wd = tile + 2 * GA_MAX_HEADS * GA_TILE_LD;
    const int C = f / heads;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;

    for (int64_t r = wave; r < n; r += n_waves) {
        const int64_t b = rowptr[r], e = rowptr[r + 1];
        const float *ss = s_src + r * lds;
        float tsum = 0.f;                             // lane h < heads: <z[r,h,:], sum_i w gout[i,h,:]>
        for (int c0 = 0; c0 < f; c0 += 256) {
            const int c = c0 + lane * 4;
            const bool act = c < f;
            const int hl = act ? c / C : 0;
            const float raw0 = ss[hl] + s_dst[r * lds + hl];
            const float a0 = expf(ga_leaky(raw0, slope) - lse[r * heads + hl]);
            const float w0 = raw0 > 0.f ? a0 : a0 * slope;
            float l = w0 * dwork[r * heads + hl];     // sum_i w_ij D_ih of this lane's head, the self loop first
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), acc2 = acc, zr = acc;
            if (act) {
                const float4 g0 = *reinterpret_cast<const float4 *>(gout + r * ldg + c);
                eps_fma(acc, a0, g0);
                eps_fma(acc2, w0, g0);
                zr = *reinterpret_cast<const float4 *>(z + r * ldz + c);
            }
            for (int64_t k0 = b; k0 < e; k0 += 64) {
                const int nk = (e - k0) < 64 ? (int)(e - k0) : 64;
                const int my_col = lane < nk ? col[k0 + lane] : 0;
                const bool live = lane < nk && my_col != r;
                lds_wave_sync();
                for (int h = 0; h < heads; ++h) {
                    float p = 0.f, pw = 0.f, pd = 0.f;
                    if (live) {
                        const float raw = ss[h] + s_dst[(int64_t)my_col * lds + h];
                        p = expf(ga_leaky(raw, slope) - lse[(int64_t)my_col * heads + h]);
                        pw = raw > 0.f ? p : p * slope;
                        pd = pw * dwork[(int64_t)my_col * heads + h];
                    }
                    tile[h * GA_TILE_LD + lane] = p;
                    tile_w[h * GA_TILE_LD + lane] = pw;
                    tile_wd[h * GA_TILE_LD + lane] = pd;
                }
                lds_wave_sync();
                ga_gather<2>(gout, ldg, c, act, my_col, nk, tile + hl * GA_TILE_LD, tile_w + hl * GA_TILE_LD,
                             tile_wd + hl * GA_TILE_LD, acc, acc2, l);
            }
            if (act) *reinterpret_cast<float4 *>(gz + r * ldgz + c) = acc;
            tsum += ga_head_sum(eps_dot(zr, acc2), strip, lane, c0, f, heads, C);
            lds_wave_sync();
            if (act && c % C == 0) wsum[hl] = l;
            lds_wave_sync();
        }
        if (lane < heads) g_s_src[r * heads + lane] = tsum - wsum[lane];
    }
}

// ------------------------------------------------------------------------------------------------------------------- host
static bool ga_aligned(const void *p, int64_t ld) { return ((uintptr_t)p % 16 == 0) && (ld % 4 == 0); }

static unsigned ga_blocks(int64_t n_rows)
{
    int64_t blocks = (n_rows + GA_WAVES - 1) / GA_WAVES;
    const int64_t cap = (int64_t)eps_num_cus() * 8 * 4;   // grid-stride beyond 8 resident blocks/CU x4 for balance (as eps_spmm_csr)
    if (blocks > cap) blocks = cap;
    return (unsigned)blocks;
}

#define GA_REQUIRE_SHAPE(who)                                                                                                     \
    EPS_REQUIRE(heads >= 1 && heads <= GA_MAX_HEADS, who ": heads = %d is outside 1..%d", heads, GA_MAX_HEADS);                  \
    EPS_REQUIRE(f >= 4 && f % 4 == 0, who ": f = %d must be a positive multiple of 4", f);                                       \
    EPS_REQUIRE(f % heads == 0 && (f / heads) % 4 == 0, who ": f = %d must be heads = %d times a multiple of 4 (f %% heads, C %% 4)", f, heads)

extern "C" int eps_gat_aggregate(const int64_t *rowptr, const int32_t *col, int64_t row0, int64_t n_rows, int64_t n_nodes,
                                 const float *z, int64_t ldz, int32_t heads, int32_t f, const float *s_src, const float *s_dst,
                                 int64_t lds, float slope, const float *bias, int relu, float *out, int64_t ldo, float *lse,
                                 void *stream)
{
    GA_REQUIRE_SHAPE("eps_gat_aggregate");
    EPS_REQUIRE(n_rows >= 0 && row0 >= 0 && n_nodes >= 0 && row0 + n_rows <= n_nodes && ldz >= f && ldo >= f && lds >= heads,
                "eps_gat_aggregate: bad shape (row0=%lld n_rows=%lld n_nodes=%lld f=%d ldz=%lld ldo=%lld lds=%lld)", (long long)row0,
                (long long)n_rows, (long long)n_nodes, f, (long long)ldz, (long long)ldo, (long long)lds);
    if (n_rows == 0) return EPS_OK;
    EPS_REQUIRE(rowptr && col && z && s_src && s_dst && out, "eps_gat_aggregate: null pointer");
    EPS_REQUIRE(ga_aligned(z, ldz) && ga_aligned(out, ldo) && (!bias || (uintptr_t)bias % 16 == 0),
                "eps_gat_aggregate: z, out and bias need 16-byte aligned rows (ldz=%lld ldo=%lld)", (long long)ldz, (long long)ldo);
    hipLaunchKernelGGL(gat_aggregate_kernel, dim3(ga_blocks(n_rows)), dim3(64 * GA_WAVES), 0, (hipStream_t)stream, rowptr, col, row0,
                       n_rows, z, ldz, heads, f, s_src, s_dst, lds, slope, bias, relu, out, ldo, lse);
    EPS_CHECK_LAUNCH("eps_gat_aggregate");
    return EPS_OK;
}

extern "C" int eps_gat_aggregate_backward(const int64_t *rowptr, const int32_t *col, int64_t n_nodes, const float *z, int64_t ldz,
                                          int32_t heads, int32_t f, const float *s_src, const float *s_dst, int64_t lds, float slope,
                                          const float *lse, const float *out_nobias, int64_t ldo, const float *gout, int64_t ldg,
                                          float *gz, int64_t ldgz, float *g_s_src, float *g_s_dst, float *dwork, void *stream)
{
    GA_REQUIRE_SHAPE("eps_gat_aggregate_backward");
    EPS_REQUIRE(n_nodes >= 0 && ldz >= f && ldo >= f && ldg >= f && ldgz >= f && lds >= heads,
                "eps_gat_aggregate_backward: bad shape (n_nodes=%lld f=%d ldz=%lld ldo=%lld ldg=%lld ldgz=%lld lds=%lld)",
                (long long)n_nodes, f, (long long)ldz, (long long)ldo, (long long)ldg, (long long)ldgz, (long long)lds);
    if (n_nodes == 0) return EPS_OK;
    EPS_REQUIRE(rowptr && col && z && s_src && s_dst && lse && out_nobias && gout && gz && g_s_src && g_s_dst && dwork,
                "eps_gat_aggregate_backward: null pointer");
    EPS_REQUIRE(ga_aligned(z, ldz) && ga_aligned(out_nobias, ldo) && ga_aligned(gout, ldg) && ga_aligned(gz, ldgz),
                "eps_gat_aggregate_backward: z, out_nobias, gout and gz need 16-byte aligned rows");
    const dim3 grid(ga_blocks(n_nodes)), block(64 * GA_WAVES);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gat_backward_dst_kernel, grid, block, 0, s, rowptr, col, n_nodes, z, ldz, heads, f, s_src, s_dst, lds, slope, lse,
                       out_nobias, ldo, gout, ldg, dwork, g_s_dst);
    hipLaunchKernelGGL(gat_backward_src_kernel, grid, block, 0, s, rowptr, col, n_nodes, z, ldz, heads, f, s_src, s_dst, lds, slope, lse,
                       gout, ldg, dwork, gz, ldgz, g_s_src);
    EPS_CHECK_LAUNCH("eps_gat_aggregate_backward");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void gat_attend_warm_kernel() {}
extern "C" void eps_warm_gat_attend(void *stream) { hipLaunchKernelGGL(gat_attend_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

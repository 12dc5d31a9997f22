// Fused LinkPredictor decode for TRAINING on the f32-input MFMA, gfx950: forward with dropout masks, and the backward into
// h, the weights and the biases.
//
// Replaces, in training mode, the h[edges[0]] / h[edges[1]] gathers (models.py:506) + LinkPredictor.forward
// (models.py:478-485: Hadamard -> (L-1) x [Linear, ReLU, dropout] -> Linear(H,1) -> sigmoid) and what autograd records
// for them.  Same tile structure as csrc/mlp_decode.hip (64-edge tiles, X[64,H] in LDS, W fragments L2 -> registers, wave
// w owns column tile w) and the same arithmetic in the same order: without masks the scores are that kernel's bits.
//
//   mlp_decode_train_kernel   forward: relu -> `taken` bit (ReLU output > 0, before dropout) -> keep bit * keep_scale.
//                             The 32 lanes of a half wave hold the 32 columns of one mask word of one row, so a mask word
//                             is one ballot.
//   mlp_decode_bwd_kernel     per tile: gather, forward again in LDS (each layer's input tile goes out to the workspace
//                             on the way, its `taken` words stay in LDS), dz_L = g s (1 - s), then the chain backwards
//                             on the same MFMA loop with W^T (passed by the host) in W's place: dA_l = dZ_l W_l, masked
//                             by layer l-1's bits.  Every dZ_l tile goes out to the workspace, dA_0 = dx0 too.  The bias
//                             gradients and the H -> 1 layer's weight gradient are column sums over the tile: each
//                             workgroup keeps them in LDS over all its tiles and writes ONE row of partials at the end.
//   mlp_decode_dw_kernel      dW_l = dZ_l^T A_l: split over the edges (S chunks) x 128 x 128 output tiles, operands read
//                             straight from the [B, H] spills (a 32-column slice of a row is one 128-byte line), each
//                             wave 64 x 64 outputs in 64 accumulator registers; partials [S, H, H].
//   mlp_decode_sum_kernel     sums partial rows in row order (the dW chunks, the workgroups' column sums).
//   mlp_decode_gradh_kernel   grad_h[n] = sum over the incidences of n, in the order of the host's STABLE sort of
//                             cat(u, v), of dx0[e] (.) h[other endpoint of e]; one wave per node, float4 per lane.
// No atomics anywhere and every summation order is a function of the shapes alone: two calls on the same inputs give
// the same bits.  (An H x H accumulator per hidden layer would be 128 registers per lane at H = 256, hence the spills.)
#include "eps_common.h"

#define T_BM 64        // edges per tile
#define T_HMAX 256
#define T_HMIN 32      // at least one whole 32-column MFMA tile (narrower widths stay on the torch route)
#define T_XLD (T_HMAX + 4)
#define T_BK 32
#define T_MAXL 8
#define T_NW (T_HMAX / 32)   // mask words per row
#define T_THREADS 512
#define T_MAX_WG 512         // workgroups of the backward launch (rows of its column-sum partials)
#define T_GROW (T_MAXL * T_HMAX + 64)   // floats per partial row: [l][c] for l < L-1 grad_b[l], [L-1][c] grad_w[L-1], then grad_b[L-1]
#define T_DW_MAXS 256        // edge chunks of the dW product

struct TrainParams {
    const float *w[T_MAXL];    // forward: W_l [out, in]; backward kernel: also wt
    const float *wt[T_MAXL];   // W_l^T [in, out] of the hidden layers (backward only)
    const float *b[T_MAXL];
};

__device__ __forceinline__ const float *tpick(const float *const (&a)[T_MAXL], int l)
{
    const float *p = a[0];
#pragma unroll
    for (int i = 1; i < T_MAXL; ++i) p = (i == l) ? a[i] : p;
    return p;
}

// (mlp_decode.hip: b_gload)
__device__ __forceinline__ void t_gload(v4f (&bf)[4], __amdgpu_buffer_rsrc_t wr, int H, int t0, int r, int hh, int kc)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int kcol = kc * T_BK + 8 * j + 4 * hh;
        const int o0 = ((t0 * 32 + r) * H + kcol) * 4;
        bf[j] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(wr, kcol < H ? o0 : 0x7ffffff0, 0, 0));
    }
}

// gather + Hadamard of one tile into LDS: wave w builds rows 8w..8w+7.  Rows past n_pairs are zero.
__device__ __forceinline__ void t_gather(float (*Xs)[T_XLD], const float *__restrict__ hmat, int H, const int32_t *__restrict__ pu,
                                         const int32_t *__restrict__ pv, int64_t n_pairs, int64_t e0, int w, int lane)
{
    const int h4 = H >> 2, hp4 = ((H + 31) & ~31) >> 2;
    const int cl = lane < h4 ? lane : 0;
    const int64_t p = e0 + lane;
    const bool ok = p < n_pairs;
    const int32_t mu = ok ? pu[ok ? p : 0] : 0, mv = ok ? pv[ok ? p : 0] : 0;
    v4f a[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t un = __builtin_amdgcn_readlane(mu, w * 8 + i), vn = __builtin_amdgcn_readlane(mv, w * 8 + i);
        a[i] = *reinterpret_cast<const v4f *>(hmat + un * H + 4 * cl);
        b[i] = *reinterpret_cast<const v4f *>(hmat + vn * H + 4 * cl);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v4f pr = a[i] * b[i];
        if (lane >= h4 || e0 + w * 8 + i >= n_pairs) pr = (v4f){0.f, 0.f, 0.f, 0.f};
        if (lane < hp4) *reinterpret_cast<v4f *>(&Xs[w * 8 + i][4 * lane]) = pr;
    }
}

// acc = X[64, Hp] (LDS) x M^T for the 32 output columns of tile t0, M row-major [H, H]: mlp_decode_kernel's K loop.
__device__ __forceinline__ void t_matmul(f32x16 (&acc)[2], const float (*Xs)[T_XLD], const float *M, int H, int t0, bool has0,
                                         int r, int hh)
{
    const int nk = ((H + 31) & ~31) / T_BK;
    const __amdgpu_buffer_rsrc_t wr = eps_raw_rsrc(M, H * H * 4);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    v4f bnxt[4];
    t_gload(bnxt, wr, H, t0, r, hh, 0);
    for (int kc = 0; kc < nk; ++kc) {
        v4f bcur[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bcur[j] = bnxt[j];
        t_gload(bnxt, wr, H, t0, r, hh, kc + 1 < nk ? kc + 1 : kc);
        float4 af[2][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            af[0][j] = *reinterpret_cast<const float4 *>(&Xs[r][kc * T_BK + 8 * j + 4 * hh]);
            af[1][j] = *reinterpret_cast<const float4 *>(&Xs[32 + r][kc * T_BK + 8 * j + 4 * hh]);
        }
        if (has0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a0[4] = {af[0][j].x, af[0][j].y, af[0][j].z, af[0][j].w};
                const float a1[4] = {af[1][j].x, af[1][j].y, af[1][j].z, af[1][j].w};
#pragma unroll
                for (int ss = 0; ss < 4; ++ss) {
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[ss], bcur[j][ss], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[ss], bcur[j][ss], acc[1], 0, 0, 0);
                }
            }
        }
    }
}

// The keep words of one layer's tile -> LDS (thread = (row, word)); all ones without dropout, zeros past n_pairs.
__device__ __forceinline__ void t_stage_keep(uint32_t (*Ks)[T_NW], const uint32_t *__restrict__ keep_l, int nw, int64_t e0,
                                             int64_t n_pairs, int tid)
{
    const int row = tid >> 3, word = tid & 7;
    const int64_t p = e0 + row;
    uint32_t kw = ~0u;
    if (keep_l) kw = (p < n_pairs && word < nw) ? keep_l[p * nw + word] : 0u;
    Ks[row][word] = kw;
}

// One hidden layer's epilogue: X <- dropout(relu(acc + b)).  Lane (r, hh) holds column cc = t0 * 32 + r of the rows
// rr = mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh, so the `taken` word (rr, t0) is one half of a ballot; it goes to Tk[rr][t0].
// keep_scale is 1 without dropout (x * 1 is x).  Call with every wave past the barrier that ends the K loop.
__device__ __forceinline__ void t_epilogue(const f32x16 (&acc)[2], float (*Xs)[T_XLD], const float *__restrict__ Bv, int H, int t0,
                                           int r, int hh, const uint32_t (*Ks)[T_NW], float keep_scale, uint32_t (*Tk)[T_NW])
{
    const int cc = t0 * 32 + r;
    const float bv = cc < H ? Bv[cc] : 0.f;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int rr = mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
            const float t = acc[mi][e] + bv;
            const float x = t > 0.f ? t : 0.f;
            const unsigned long long bal = __ballot(x > 0.f);
            if (r == 0) Tk[rr][t0] = hh ? (uint32_t)(bal >> 32) : (uint32_t)bal;
            Xs[rr][cc] = (Ks[rr][t0] >> r) & 1u ? x * keep_scale : 0.f;
        }
}

// last layer: z[row] = X[row] . wl + b (8 lanes per row, mlp_decode_kernel's order); valid on the lanes with part == 0
__device__ __forceinline__ float t_last(const float (*Xs)[T_XLD], const float *__restrict__ wl, float bl, int H, int tid)
{
    const int h4 = H >> 2;
    const int row = tid >> 3, part = tid & 7;
    float s = 0.f;
    for (int c = part; c < h4; c += 8) {
        const float4 x = *reinterpret_cast<const float4 *>(&Xs[row][4 * c]);
        const float4 q = *reinterpret_cast<const float4 *>(wl + 4 * c);
        s = fmaf(x.x, q.x, s);
        s = fmaf(x.y, q.y, s);
        s = fmaf(x.z, q.z, s);
        s = fmaf(x.w, q.w, s);
    }
    s += eps_dpp_f<0xB1>(s);   // quad_perm [1,0,3,2]
    s += eps_dpp_f<0x4E>(s);   // quad_perm [2,3,0,1]
    s += eps_dpp_f<0x141>(s);  // row_half_mirror
    return s + bl;
}

__global__ __launch_bounds__(T_THREADS, 4) void mlp_decode_train_kernel(const float *__restrict__ hmat, int32_t H,
                                                                        const int32_t *__restrict__ pu,
                                                                        const int32_t *__restrict__ pv, int64_t n_pairs,
                                                                        TrainParams prm, int32_t n_layers,
                                                                        const uint32_t *__restrict__ keep, float keep_scale,
                                                                        int apply_sigmoid, float *__restrict__ out,
                                                                        uint32_t *__restrict__ taken)
{
    __shared__ __attribute__((aligned(16))) float Xs[T_BM][T_XLD];
    __shared__ uint32_t Ks[T_BM][T_NW], Tk[T_BM][T_NW];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int nw = (H + 31) >> 5;
    const bool has0 = w < nw;
    const int64_t n_tiles = (n_pairs + T_BM - 1) / T_BM;
    const int64_t lstride = n_pairs * nw;      // mask words per layer

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t e0 = tile * T_BM;
        t_gather(Xs, hmat, H, pu, pv, n_pairs, e0, w, lane);
        __syncthreads();
        for (int l = 0; l + 1 < n_layers; ++l) {
            t_stage_keep(Ks, keep ? keep + l * lstride : nullptr, nw, e0, n_pairs, tid);
            f32x16 acc[2];
            t_matmul(acc, Xs, tpick(prm.w, l), H, w, has0, r, hh);
            __syncthreads();  // every wave has finished reading X
            if (has0) t_epilogue(acc, Xs, tpick(prm.b, l), H, w, r, hh, Ks, keep_scale, Tk);
            __syncthreads();
            if (taken) {      // (Tk is rewritten only after the next layer's K loop and its barrier)
                const int row = tid >> 3, word = tid & 7;
                const int64_t p = e0 + row;
                if (word < nw && p < n_pairs) taken[l * lstride + p * nw + word] = Tk[row][word];
            }
        }
        {
            float z = t_last(Xs, tpick(prm.w, n_layers - 1), tpick(prm.b, n_layers - 1)[0], H, tid);
            const int64_t p = e0 + (tid >> 3);
            if ((tid & 7) == 0 && p < n_pairs) {
                if (apply_sigmoid) z = 1.0f / (1.0f + expf(-z));
                out[p] = z;
            }
        }
        __syncthreads();
    }
}

// X tile (rows e0.., H columns) -> dst [Bp, H] row-major; wave w writes rows 8w..8w+7, one float4 per lane
__device__ __forceinline__ void t_spill(const float (*Xs)[T_XLD], float *__restrict__ dst, int H, int64_t e0, int w, int lane)
{
    if (lane < (H >> 2)) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            *reinterpret_cast<v4f *>(dst + (e0 + w * 8 + i) * H + 4 * lane) = *reinterpret_cast<const v4f *>(&Xs[w * 8 + i][4 * lane]);
    }
}

// Gs[c] += sum over the tile's rows of X[row][c] (thread c < H); sequential in row order
__device__ __forceinline__ void t_colsum(const float (*Xs)[T_XLD], float *Gs, int H, int tid)
{
    if (tid < H) {
        float s = 0.f;
#pragma unroll 8
        for (int row = 0; row < T_BM; ++row) s += Xs[row][tid];
        Gs[tid] += s;
    }
}

// Workspace of the backward (floats, Bp = n_pairs rounded up to the tile):
//   A  [(L-1)][Bp][H]  the input tile of every hidden layer          dZ [(L-1)][Bp][H]  dL/d(pre-activation)
//   dx0 [Bp][H]        part [T_MAX_WG][T_GROW]                       dwp [T_DW_MAXS][H][H]
// DX0 = false (the BatchNorm route below): the chain stops at dZ_0 -- no dA_0 product, dx0 stays unwritten.
template <bool DX0>
__global__ __launch_bounds__(T_THREADS, 2) void mlp_decode_bwd_kernel(const float *__restrict__ hmat, int32_t H,
                                                                      const int32_t *__restrict__ pu,
                                                                      const int32_t *__restrict__ pv, int64_t n_pairs,
                                                                      TrainParams prm, int32_t n_layers,
                                                                      const uint32_t *__restrict__ keep, float keep_scale,
                                                                      int apply_sigmoid, const float *__restrict__ grad_out,
                                                                      float *__restrict__ As, float *__restrict__ dZs,
                                                                      float *__restrict__ dx0, float *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float Xs[T_BM][T_XLD];
    __shared__ uint32_t Ts[T_MAXL - 1][T_BM][T_NW], Ks[T_BM][T_NW];
    __shared__ float Gs[T_MAXL][T_HMAX];
    __shared__ float Dz[T_BM];
    __shared__ float Gb;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int nw = (H + 31) >> 5;
    const int Hp = nw * 32, hp4 = Hp >> 2;
    const bool has0 = w < nw;
    const int64_t n_tiles = (n_pairs + T_BM - 1) / T_BM;
    const int64_t Bp = n_tiles * T_BM;
    const int64_t lstride = n_pairs * nw;
    const int L = n_layers;

    for (int i = tid; i < T_MAXL * T_HMAX; i += T_THREADS) (&Gs[0][0])[i] = 0.f;
    if (tid == 0) Gb = 0.f;
    __syncthreads();

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t e0 = tile * T_BM;
        t_gather(Xs, hmat, H, pu, pv, n_pairs, e0, w, lane);
        __syncthreads();
        // ---- forward again: the input of every hidden layer goes out, the taken words stay -------------------------
        for (int l = 0; l + 1 < L; ++l) {
            t_spill(Xs, As + l * Bp * H, H, e0, w, lane);
            t_stage_keep(Ks, keep ? keep + l * lstride : nullptr, nw, e0, n_pairs, tid);
            f32x16 acc[2];
            t_matmul(acc, Xs, tpick(prm.w, l), H, w, has0, r, hh);
            __syncthreads();
            if (has0) t_epilogue(acc, Xs, tpick(prm.b, l), H, w, r, hh, Ks, keep_scale, Ts[l]);
            __syncthreads();
        }
        // ---- dz_L, the last layer's gradients --------------------------------------------------------------------
        const float *__restrict__ wl = tpick(prm.w, L - 1);
        {
            const float z = t_last(Xs, wl, tpick(prm.b, L - 1)[0], H, tid);
            const int row = tid >> 3;
            const int64_t p = e0 + row;
            if ((tid & 7) == 0) {
                float g = 0.f;
                if (p < n_pairs) {
                    g = grad_out[p];
                    if (apply_sigmoid) {
                        const float s = 1.0f / (1.0f + expf(-z));
                        g = g * (s * (1.0f - s));
                    }
                }
                Dz[row] = g;
            }
        }
        __syncthreads();
        if (tid < H) {                       // grad_w[L-1][c] += sum_row dz[row] X[row][c]
            float s = 0.f;
#pragma unroll 8
            for (int row = 0; row < T_BM; ++row) s += Dz[row] * Xs[row][tid];
            Gs[L - 1][tid] += s;
        }
        if (tid == T_THREADS - 1) {          // grad_b[L-1]
            float s = 0.f;
            for (int row = 0; row < T_BM; ++row) s += Dz[row];
            Gb += s;
        }
        __syncthreads();
        // ---- dZ_{L-2} = (dz_L wl) masked by layer L-2's bits (Ks still holds that layer's keep words), in place ------
        for (int idx = tid; idx < T_BM * hp4; idx += T_THREADS) {
            const int row = idx / hp4, c4 = idx - row * hp4;
            const int word = c4 >> 3, bit0 = (4 * c4) & 31;
            const uint32_t m = Ts[L - 2][row][word] & Ks[row][word];
            const float dz = Dz[row];
            v4f q = (v4f){0.f, 0.f, 0.f, 0.f};
            if (4 * c4 < H) q = *reinterpret_cast<const v4f *>(wl + 4 * c4);
            v4f o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (m >> (bit0 + k)) & 1u ? (dz * q[k]) * keep_scale : 0.f;
            *reinterpret_cast<v4f *>(&Xs[row][4 * c4]) = o;
        }
        __syncthreads();
        // ---- the chain backwards: X holds dZ_l ---------------------------------------------------------------------------
        for (int l = L - 2; l >= 0; --l) {
            t_spill(Xs, dZs + l * Bp * H, H, e0, w, lane);
            t_colsum(Xs, Gs[l], H, tid);         // grad_b[l]
            if (!DX0 && l == 0) {
                __syncthreads();                 // (the next tile's gather rewrites X)
                break;
            }
            if (l > 0) t_stage_keep(Ks, keep ? keep + (int64_t)(l - 1) * lstride : nullptr, nw, e0, n_pairs, tid);
            f32x16 acc[2];
            t_matmul(acc, Xs, tpick(prm.wt, l), H, w, has0, r, hh);   // dA_l[row][i] = sum_o dZ_l[row][o] W_l[o][i]
            __syncthreads();
            if (has0) {
                const int cc = w * 32 + r;
                float *__restrict__ drow = dx0 + e0 * H + cc;
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int rr = mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                        if (l == 0) {
                            if (cc < H) drow[rr * H] = acc[mi][e];      // (every row of the tile exists in the spills)
                        } else {
                            const uint32_t m = Ts[l - 1][rr][w] & Ks[rr][w];
                            Xs[rr][cc] = (m >> r) & 1u ? acc[mi][e] * keep_scale : 0.f;
                        }
                    }
            }
            __syncthreads();
        }
    }
    // ---- this workgroup's column sums: one row of partials ----------------------------------------------------------------
    float *row = part + (int64_t)blockIdx.x * T_GROW;
    for (int i = tid; i < T_MAXL * T_HMAX; i += T_THREADS) row[i] = (&Gs[0][0])[i];
    if (tid == 0) row[T_MAXL * T_HMAX] = Gb;
}

// dW[o][i] partial of chunk s = sum over the chunk's edges of dZ[e][o] A[e][i].  256 threads: wave (wo, wi) of a 2 x 2 grid takes
// 64 x 64 outputs of the workgroup's 128 x 128.  MFMA operands: a = dZ[e + hh][o0 + r], b = A[e + hh][i0 + r] -- one dword per
// lane, 128 contiguous bytes per half wave; 16 edges per trip so that 32 loads are in flight before the first MFMA.
__global__ __launch_bounds__(256) void mlp_decode_dw_kernel(const float *__restrict__ dZ, const float *__restrict__ A, int32_t H,
                                                            int64_t Bp, int64_t chunk, float *__restrict__ dwp)
{
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int nt = (H + 127) >> 7;
    const int to = blockIdx.x / nt, ti = blockIdx.x - to * nt;
    const int o0 = to * 128 + (wv >> 1) * 64, i0 = ti * 128 + (wv & 1) * 64;
    if (o0 >= H || i0 >= H) return;          // wave-uniform
    const int64_t k0 = (int64_t)blockIdx.y * chunk;
    const int64_t k1 = k0 + chunk < Bp ? k0 + chunk : Bp;   // multiples of the tile (64)

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
    const bool oa[2] = {o0 + r < H, o0 + 32 + r < H}, ib[2] = {i0 + r < H, i0 + 32 + r < H};
    for (int64_t k = k0; k < k1; k += 16) {
        float av[8][2], bv[8][2];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int64_t e = k + 2 * s + hh;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                av[s][t] = oa[t] ? dZ[e * H + o0 + 32 * t + r] : 0.f;
                bv[s][t] = ib[t] ? A[e * H + i0 + 32 * t + r] : 0.f;
            }
        }
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s][a], bv[s][b], acc[a][b], 0, 0, 0);
    }
    float *dst = dwp + (int64_t)blockIdx.y * H * H;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int o = o0 + 32 * a + (e & 3) + 8 * (e >> 2) + 4 * hh, i = i0 + 32 * b + r;
                if (o < H && i < H) dst[(int64_t)o * H + i] = acc[a][b][e];
            }
}

// dst[j] = sum over rows s = 0 .. S-1, in that order, of src[s * stride + j]
__global__ __launch_bounds__(256) void mlp_decode_sum_kernel(const float *__restrict__ src, int64_t stride, int32_t S, int64_t n,
                                                             float *__restrict__ dst)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    float s = 0.f;
    for (int i = 0; i < S; ++i) s += src[i * stride + j];
    dst[j] = s;
}

// grad_h[n] = sum over positions q of [ptr[n], ptr[n + 1]) of the sorted incidence list, in list order, of
// dx0[e] (.) h[other], with p = order[q], e = p mod n_pairs, other = p < n_pairs ? v[e] : u[e].  One wave per node.
__global__ __launch_bounds__(256) void mlp_decode_gradh_kernel(const float *__restrict__ hmat, int32_t H, int64_t n_nodes,
                                                               const int32_t *__restrict__ pu, const int32_t *__restrict__ pv,
                                                               int64_t n_pairs, const int32_t *__restrict__ order,
                                                               const int64_t *__restrict__ ptr, const float *__restrict__ dx0,
                                                               float *__restrict__ grad_h)
{
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= n_nodes || lane >= (H >> 2)) return;
    const int64_t q0 = ptr[n], q1 = ptr[n + 1];
    v4f s = (v4f){0.f, 0.f, 0.f, 0.f};
    int64_t q = q0;
    for (; q + 4 <= q1; q += 4) {           // four incidences' rows in flight; added in list order
        v4f d[4], o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t p = order[q + k];
            const bool first = p < n_pairs;
            const int64_t e = first ? p : p - n_pairs;
            const int64_t other = first ? pv[e] : pu[e];
            d[k] = *reinterpret_cast<const v4f *>(dx0 + e * H + 4 * lane);
            o[k] = *reinterpret_cast<const v4f *>(hmat + other * H + 4 * lane);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s += d[k] * o[k];
    }
    for (; q < q1; ++q) {
        const int64_t p = order[q];
        const bool first = p < n_pairs;
        const int64_t e = first ? p : p - n_pairs;
        const int64_t other = first ? pv[e] : pu[e];
        s += *reinterpret_cast<const v4f *>(dx0 + e * H + 4 * lane) * *reinterpret_cast<const v4f *>(hmat + other * H + 4 * lane);
    }
    *reinterpret_cast<v4f *>(grad_h + n * H + 4 * lane) = s;
}

// ---- host ---------------------------------------------------------------------------------------------------------------
static int64_t t_tiles(int64_t n_pairs) { return (n_pairs + T_BM - 1) / T_BM; }

static int t_dw_chunks(int64_t n_tiles, int64_t *chunk_rows)
{
    int64_t s = n_tiles / 8;
    if (s < 1) s = 1;
    if (s > T_DW_MAXS) s = T_DW_MAXS;
    const int64_t tiles_per = (n_tiles + s - 1) / s;
    *chunk_rows = tiles_per * T_BM;
    return (int)((n_tiles + tiles_per - 1) / tiles_per);
}

#define T_DOMAIN(name)                                                                                                           \
    EPS_REQUIRE(n_pairs >= 0 && n_nodes >= 0, name ": negative size");                                                            \
    EPS_REQUIRE(hdim >= T_HMIN && hdim % 4 == 0 && hdim <= T_HMAX, name ": hdim=%d unsupported (need %%4==0, %d..%d)", hdim,      \
                T_HMIN, T_HMAX);                                                                                                  \
    EPS_REQUIRE(n_layers >= 2 && n_layers <= T_MAXL, name ": n_layers=%d unsupported (2..%d)", n_layers, T_MAXL)

extern "C" int64_t eps_mlp_decode_backward_workspace_bytes(int64_t n_pairs, int32_t hdim, int32_t n_layers)
{
    if (n_pairs < 0 || hdim < T_HMIN || hdim > T_HMAX || n_layers < 2 || n_layers > T_MAXL) return 0;
    const int64_t bp = t_tiles(n_pairs) * T_BM;
    const int64_t floats = (2 * (int64_t)(n_layers - 1) + 1) * bp * hdim + (int64_t)T_MAX_WG * T_GROW +
                           (int64_t)T_DW_MAXS * hdim * hdim;
    return floats * 4;
}

static int t_params(TrainParams &prm, const float *const *w, const float *const *wt, const float *const *b, int32_t n_layers,
                    const char *who)
{
    for (int l = 0; l < T_MAXL; ++l) {
        prm.w[l] = l < n_layers ? w[l] : nullptr;
        prm.b[l] = l < n_layers ? b[l] : nullptr;
        prm.wt[l] = (wt && l + 1 < n_layers) ? wt[l] : nullptr;
        if (l < n_layers) {
            EPS_REQUIRE(w[l] && b[l], "%s: null weight/bias pointer at layer %d", who, l);
            EPS_REQUIRE((uintptr_t)w[l] % 16 == 0, "%s: weight %d must be 16-byte aligned", who, l);
        }
        if (wt && l + 1 < n_layers)
            EPS_REQUIRE(wt[l] && (uintptr_t)wt[l] % 16 == 0, "%s: transposed weight %d must be non-null and 16-byte aligned", who, l);
    }
    return EPS_OK;
}

extern "C" int eps_mlp_decode_train(const float *h, int64_t n_nodes, int32_t hdim, const int32_t *u, const int32_t *v,
                                    int64_t n_pairs, const float *const *w, const float *const *b, int32_t n_layers,
                                    const uint32_t *keep, float keep_scale, int apply_sigmoid, float *out, uint32_t *taken,
                                    void *stream)
{
    T_DOMAIN("eps_mlp_decode_train");
    if (n_pairs == 0) return EPS_OK;
    EPS_REQUIRE(h && u && v && w && b && out, "eps_mlp_decode_train: null pointer");
    EPS_REQUIRE(n_nodes > 0, "eps_mlp_decode_train: pairs over an empty node set");
    EPS_REQUIRE((uintptr_t)h % 16 == 0, "eps_mlp_decode_train: h must be 16-byte aligned");
    if (!keep && !taken)   // nothing the inference kernel does not do
        return eps_mlp_decode(h, n_nodes, hdim, u, v, n_pairs, w, b, n_layers, apply_sigmoid, out, stream);
    TrainParams prm;
    if (int rc = t_params(prm, w, nullptr, b, n_layers, "eps_mlp_decode_train")) return rc;
    if (!keep) keep_scale = 1.0f;
    int64_t blocks = (int64_t)eps_num_cus() * 2;
    const int64_t n_tiles = t_tiles(n_pairs);
    if (blocks > n_tiles) blocks = n_tiles;
    hipLaunchKernelGGL(mlp_decode_train_kernel, dim3((unsigned)blocks), dim3(T_THREADS), 0, (hipStream_t)stream, h, hdim, u, v,
                       n_pairs, prm, n_layers, keep, keep_scale, apply_sigmoid, out, taken);
    EPS_CHECK_LAUNCH("eps_mlp_decode_train");
    return EPS_OK;
}

extern "C" int eps_mlp_decode_backward(const float *h, int64_t n_nodes, int32_t hdim, const int32_t *u, const int32_t *v,
                                       int64_t n_pairs, const float *const *w, const float *const *wt, const float *const *b,
                                       int32_t n_layers, const uint32_t *keep, float keep_scale, int apply_sigmoid,
                                       const float *grad_out, const int32_t *inc_order, const int64_t *inc_ptr,
                                       float *const *grad_w, float *const *grad_b, float *grad_h, void *workspace,
                                       int64_t workspace_bytes, void *stream)
{
    T_DOMAIN("eps_mlp_decode_backward");
    const hipStream_t st = (hipStream_t)stream;
    const int H = hdim, L = n_layers;
    if (n_pairs == 0) {          // no launch for the pairs; the gradients of an empty batch are zeros
        hipError_t e = hipSuccess;
        for (int l = 0; l < L && e == hipSuccess; ++l) {
            const size_t rows = l + 1 < L ? H : 1;
            if (grad_w && grad_w[l]) e = hipMemsetAsync(grad_w[l], 0, rows * H * 4, st);
            if (grad_b && grad_b[l] && e == hipSuccess) e = hipMemsetAsync(grad_b[l], 0, rows * 4, st);
        }
        if (grad_h && n_nodes > 0 && e == hipSuccess) e = hipMemsetAsync(grad_h, 0, (size_t)n_nodes * H * 4, st);
        EPS_REQUIRE(e == hipSuccess, "eps_mlp_decode_backward: %s", hipGetErrorString(e));
        return EPS_OK;
    }
    EPS_REQUIRE(h && u && v && w && wt && b && grad_out && workspace, "eps_mlp_decode_backward: null pointer");
    EPS_REQUIRE(n_nodes > 0, "eps_mlp_decode_backward: pairs over an empty node set");
    EPS_REQUIRE(n_pairs < ((int64_t)1 << 30), "eps_mlp_decode_backward: n_pairs=%lld: the incidence list holds 32-bit positions",
                (long long)n_pairs);
    EPS_REQUIRE((uintptr_t)h % 16 == 0 && (uintptr_t)workspace % 16 == 0, "eps_mlp_decode_backward: h and workspace must be 16-byte aligned");
    EPS_REQUIRE(workspace_bytes >= eps_mlp_decode_backward_workspace_bytes(n_pairs, hdim, n_layers),
                "eps_mlp_decode_backward: workspace of %lld bytes, need %lld", (long long)workspace_bytes,
                (long long)eps_mlp_decode_backward_workspace_bytes(n_pairs, hdim, n_layers));
    EPS_REQUIRE(!grad_h || (inc_order && inc_ptr && (uintptr_t)grad_h % 16 == 0),
                "eps_mlp_decode_backward: grad_h needs the sorted incidence list (inc_order, inc_ptr) and 16-byte alignment");
    TrainParams prm;
    if (int rc = t_params(prm, w, wt, b, n_layers, "eps_mlp_decode_backward")) return rc;
    if (!keep) keep_scale = 1.0f;

    const int64_t n_tiles = t_tiles(n_pairs), bp = n_tiles * T_BM;
    float *As = (float *)workspace;
    float *dZs = As + (int64_t)(L - 1) * bp * H;
    float *dx0 = dZs + (int64_t)(L - 1) * bp * H;
    float *part = dx0 + bp * H;
    float *dwp = part + (int64_t)T_MAX_WG * T_GROW;

    int64_t blocks = eps_num_cus();          // 89 KiB of LDS: one workgroup per CU
    if (blocks > T_MAX_WG) blocks = T_MAX_WG;
    if (blocks > n_tiles) blocks = n_tiles;
    hipLaunchKernelGGL((mlp_decode_bwd_kernel<true>), dim3((unsigned)blocks), dim3(T_THREADS), 0, st, h, hdim, u, v, n_pairs, prm, n_layers,
                       keep, keep_scale, apply_sigmoid, grad_out, As, dZs, dx0, part);
    EPS_CHECK_LAUNCH("eps_mlp_decode_backward");

    auto sum_rows = [&](const float *src, int64_t stride, int S, int64_t n, float *dst) {
        hipLaunchKernelGGL(mlp_decode_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, stride, (int32_t)S, n, dst);
    };
    for (int l = 0; l < L; ++l) {
        if (grad_b && grad_b[l]) {
            if (l + 1 < L) sum_rows(part + l * T_HMAX, T_GROW, (int)blocks, H, grad_b[l]);
            else sum_rows(part + T_MAXL * T_HMAX, T_GROW, (int)blocks, 1, grad_b[l]);
        }
        if (!(grad_w && grad_w[l])) continue;
        if (l + 1 == L) {
            sum_rows(part + (L - 1) * T_HMAX, T_GROW, (int)blocks, H, grad_w[l]);
            continue;
        }
        int64_t chunk = 0;
        const int S = t_dw_chunks(n_tiles, &chunk);
        const int nt = (H + 127) / 128;
        hipLaunchKernelGGL(mlp_decode_dw_kernel, dim3((unsigned)(nt * nt), (unsigned)S), dim3(256), 0, st, dZs + (int64_t)l * bp * H,
                           As + (int64_t)l * bp * H, hdim, bp, chunk, dwp);
        sum_rows(dwp, (int64_t)H * H, S, (int64_t)H * H, grad_w[l]);
    }
    if (grad_h) {
        hipLaunchKernelGGL(mlp_decode_gradh_kernel, dim3((unsigned)((n_nodes + 3) / 4)), dim3(256), 0, st, h, hdim, n_nodes, u, v,
                           n_pairs, inc_order, inc_ptr, dx0, grad_h);
    }
    EPS_CHECK_LAUNCH("eps_mlp_decode_backward");
    return EPS_OK;
}

// ---- a two-layer decoder with BatchNorm1d on BATCH statistics between Linear(H, H) and the ReLU (DEA_GNN_JK) -------------------
//   z = x0 W0^T + b0,  mu / var over the batch,  sigma = sqrt(var + eps),  y = gamma (z - mu) / sigma + beta,  a = relu(y) keep scale
// With (mu, var) known the BatchNorm is a per-channel affine map: the forward is eps_mlp_decode_train on W' = diag(s) W0,
// b' = s b0 + beta - s mu (s = gamma / sigma), folded by the caller.
//   mlp_decode_bn_stats_kernel   per tile: gather, z = X W0^T + b0 on the decode's MFMA loop, then per column the tile's
//                                (count, mean, M2) in float64, merged (Chan) into the workgroup's running triple; one row of
//                                partials per workgroup.  mlp_decode_bn_merge_kernel merges the rows in workgroup order.
//   the backward                 mlp_decode_bwd_kernel<false> on (W', b') spills x0 and dy = dL/dy and sums g' = sum dy (= grad
//                                beta), grad w1, grad b1.
//   mlp_decode_bn_dgamma_kernel  per tile: x0 from its spill, zhat = (x0 W0^T + b0 - mu) / sigma, grad gamma = sum_e dy zhat:
//                                per-workgroup partials in float64, summed in workgroup order.
//   mlp_decode_bn_dz_kernel      per tile: zhat again, then
//                                dz = s (dy - g' / B - zhat grad_gamma / B) over the dy spill, and dx0 = dz W0.
//                                grad W0 = dz^T x0 is mlp_decode_dw_kernel once more; grad b0 is exactly 0.
// No atomics; every order is a function of the shapes and the CU count.
#define T_SROW (2 * T_HMAX + 8)   // doubles per row of the statistics partials: mean[c], M2[T_HMAX + c], the row count at 2 * T_HMAX

__device__ __forceinline__ void t_chan(double &cnt, double &mean, double &m2, double nt, double mt, double qt)
{
    const double tot = cnt + nt, delta = mt - mean;
    mean += delta * (nt / tot);
    m2 += qt + delta * delta * (cnt * nt / tot);
    cnt = tot;
}

__global__ __launch_bounds__(T_THREADS, 4) void mlp_decode_bn_stats_kernel(const float *__restrict__ hmat, int32_t H,
                                                                           const int32_t *__restrict__ pu,
                                                                           const int32_t *__restrict__ pv, int64_t n_pairs,
                                                                           const float *__restrict__ W0, const float *__restrict__ b0,
                                                                           double *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float Xs[T_BM][T_XLD];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int nw = (H + 31) >> 5;
    const bool has0 = w < nw;
    const int64_t n_tiles = (n_pairs + T_BM - 1) / T_BM;
    const int cc = w * 32 + r;
    const float bv = (has0 && cc < H) ? b0[cc] : 0.f;
    double cnt = 0.0, mean = 0.0, m2 = 0.0;      // of column tid over this workgroup's tiles so far

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t e0 = tile * T_BM;
        t_gather(Xs, hmat, H, pu, pv, n_pairs, e0, w, lane);
        __syncthreads();
        f32x16 acc[2];
        t_matmul(acc, Xs, W0, H, w, has0, r, hh);
        __syncthreads();  // every wave has finished reading X
        if (has0) {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int e = 0; e < 16; ++e) Xs[mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh][cc] = acc[mi][e] + bv;
        }
        __syncthreads();
        if (tid < H) {
            const int nt = n_pairs - e0 < T_BM ? (int)(n_pairs - e0) : T_BM;
            double s = 0.0;
            for (int row = 0; row < nt; ++row) s += (double)Xs[row][tid];
            const double mt = s / nt;
            double q = 0.0;
            for (int row = 0; row < nt; ++row) {
                const double d = (double)Xs[row][tid] - mt;
                q += d * d;
            }
            t_chan(cnt, mean, m2, (double)nt, mt, q);
        }
        __syncthreads();
    }
    double *row = part + (int64_t)blockIdx.x * T_SROW;
    if (tid < H) {
        row[tid] = mean;
        row[T_HMAX + tid] = m2;
    }
    if (tid == 0) row[2 * T_HMAX] = cnt;
}

// the workgroups' triples, merged in workgroup order: mean[c], var[c] = M2 / B (the biased variance)
__global__ __launch_bounds__(T_HMAX) void mlp_decode_bn_merge_kernel(const double *__restrict__ part, int32_t S, int32_t H,
                                                                     float *__restrict__ mean_out, float *__restrict__ var_out)
{
    const int c = threadIdx.x;
    if (c >= H) return;
    double cnt = 0.0, mean = 0.0, m2 = 0.0;
    for (int s = 0; s < S; ++s) {
        const double *row = part + (int64_t)s * T_SROW;
        t_chan(cnt, mean, m2, row[2 * T_HMAX], row[c], row[T_HMAX + c]);
    }
    mean_out[c] = (float)mean;
    var_out[c] = (float)(m2 / cnt);
}

// X tile <- rows e0.. of a [Bp, H] spill (the inverse of t_spill; the tile's 64 rows exist there); pad columns are zero
__device__ __forceinline__ void t_unspill(float (*Xs)[T_XLD], const float *__restrict__ src, int H, int64_t e0, int w, int lane)
{
    const int h4 = H >> 2, hp4 = ((H + 31) & ~31) >> 2;
    const float *__restrict__ base = src + e0 * H;       // (32-bit offsets inside the tile)
    if (lane < hp4) {
        v4f x[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = *reinterpret_cast<const v4f *>(base + (w * 8 + i) * H + 4 * (lane < h4 ? lane : 0));
#pragma unroll
        for (int i = 0; i < 8; ++i)
            *reinterpret_cast<v4f *>(&Xs[w * 8 + i][4 * lane]) = lane < h4 ? x[i] : (v4f){0.f, 0.f, 0.f, 0.f};
    }
}

// grad_gamma partials: per tile x0 from its spill, zhat = (x0 W0^T + b0 - mu) / sigma on the MFMA loop, then per column
// sum_rows dy zhat in float64 (lane (r, hh) holds column cc of 32 rows; the two halves meet in one exchange).  One row of
// partials per workgroup.
__global__ __launch_bounds__(T_THREADS, 4) void mlp_decode_bn_dgamma_kernel(int32_t H, int64_t n_pairs, const float *__restrict__ W0,
                                                                            const float *__restrict__ b0,
                                                                            const float *__restrict__ mean,
                                                                            const float *__restrict__ var, float eps,
                                                                            const float *__restrict__ A, const float *__restrict__ dZ,
                                                                            double *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float Xs[T_BM][T_XLD];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int nw = (H + 31) >> 5;
    const bool has0 = w < nw;
    const int64_t n_tiles = (n_pairs + T_BM - 1) / T_BM;
    const int cc = w * 32 + r;
    const bool okc = has0 && cc < H;
    const int loff = (4 * hh * H + cc) * 4;  // byte offset of (row 4 hh, column cc) in a tile; the rest of a row offset is wave-uniform
    double sum = 0.0;

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t e0 = tile * T_BM;
        t_unspill(Xs, A, H, e0, w, lane);
        __syncthreads();
        f32x16 acc[2];
        t_matmul(acc, Xs, W0, H, w, has0, r, hh);
        const int nv = n_pairs - e0 < T_BM ? (int)(n_pairs - e0) : T_BM;      // rows of the tile that are edges
        const double bm = okc ? (double)b0[cc] - (double)mean[cc] : 0.0;
        const double isig = okc ? 1.0 / sqrt((double)var[cc] + (double)eps) : 0.0;
        const __amdgpu_buffer_rsrc_t dyr = eps_raw_rsrc(dZ + e0 * H, T_BM * H * 4);
        if (has0) {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int rr = mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                    const float dy = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dyr, loff, (mi * 32 + (e & 3) + 8 * (e >> 2)) * H * 4, 0));
                    const float z = acc[mi][e];
                    // (rows past the batch: dy is 0 in the spill; other columns: isig is 0.  The factor keeps the chain free of
                    // branches -- as a select it compiles to 32 of them, each with its load inside)
                    sum += (double)dy * (((double)z + bm) * isig) * (rr < nv ? 1.0 : 0.0);
                }
        }
        __syncthreads();  // every wave has finished reading X
    }
    sum += __shfl_xor(sum, 32);              // (a + b on one half, b + a on the other: the same bits)
    if (okc && hh == 0) part[(int64_t)blockIdx.x * T_HMAX + cc] = sum;
}

// grad_gamma[c] = the workgroups' partials in workgroup order; `out` also gets it (float32) when non-null
__global__ __launch_bounds__(T_HMAX) void mlp_decode_bn_dgamma_sum_kernel(const double *__restrict__ part, int32_t S, int32_t H,
                                                                          double *__restrict__ dgamma, float *__restrict__ out)
{
    const int c = threadIdx.x;
    if (c >= H) return;
    double s = 0.0;
    for (int i = 0; i < S; ++i) s += part[(int64_t)i * T_HMAX + c];
    dgamma[c] = s;                           // (the dz pass subtracts in float64: at small B its terms cancel almost wholly)
    if (out) out[c] = (float)s;
}

__global__ __launch_bounds__(T_THREADS, 2) void mlp_decode_bn_dz_kernel(int32_t H, int64_t n_pairs, const float *__restrict__ W0,
                                                                        const float *__restrict__ W0t, const float *__restrict__ b0,
                                                                        const float *__restrict__ gamma,
                                                                        const float *__restrict__ mean, const float *__restrict__ var,
                                                                        float eps, const float *__restrict__ gsum,
                                                                        const double *__restrict__ dgamma, const float *__restrict__ A,
                                                                        float *__restrict__ dZ, float *__restrict__ dx0)
{
    __shared__ __attribute__((aligned(16))) float Xs[T_BM][T_XLD];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int nw = (H + 31) >> 5;
    const bool has0 = w < nw;
    const int64_t n_tiles = (n_pairs + T_BM - 1) / T_BM;
    const int cc = w * 32 + r;
    const bool okc = has0 && cc < H;
    const int loff = (4 * hh * H + cc) * 4;  // byte offset of (row 4 hh, column cc) in a tile; the rest of a row offset is wave-uniform

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t e0 = tile * T_BM;
        t_unspill(Xs, A, H, e0, w, lane);
        __syncthreads();
        f32x16 acc[2];
        t_matmul(acc, Xs, W0, H, w, has0, r, hh);
        const int nv = n_pairs - e0 < T_BM ? (int)(n_pairs - e0) : T_BM;      // rows of the tile that are edges
        // this lane's column, in float64 and formed as the grad_gamma pass forms them: at small B dz is what a near-total
        // cancellation leaves, and zhat has to be the zhat that grad_gamma summed
        double sc = 0.0, isig = 0.0, bm = 0.0, gB = 0.0, dgB = 0.0;
        if (okc) {
            isig = 1.0 / sqrt((double)var[cc] + (double)eps);
            sc = (double)gamma[cc] * isig;
            bm = (double)b0[cc] - (double)mean[cc];
            gB = (double)gsum[cc] / (double)n_pairs;
            dgB = dgamma[cc] / (double)n_pairs;
        }
        // (the tile's rows of dy / dx0 through buffer descriptors: one 32-bit offset per element, not a 64-bit address)
        const __amdgpu_buffer_rsrc_t dyr = eps_raw_rsrc(dZ + e0 * H, T_BM * H * 4);
        const __amdgpu_buffer_rsrc_t dxr = eps_raw_rsrc(dx0 + e0 * H, T_BM * H * 4);
        if (has0) {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int rr = mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                    // (no branch: a pad column's offset stays inside the tile or past its end, where the load gives 0)
                    const float dy = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dyr, loff, (mi * 32 + (e & 3) + 8 * (e >> 2)) * H * 4, 0));
                    const float z = acc[mi][e];
                    // (other columns: sc is 0.  A factor, not a select: see the grad_gamma pass)
                    acc[mi][e] = (float)(sc * ((double)dy - gB - (((double)z + bm) * isig) * dgB)) * (rr < nv ? 1.0f : 0.0f);
                }
        }
        __syncthreads();  // every wave has finished reading X
        if (has0) {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int e = 0; e < 16; ++e) Xs[mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh][cc] = acc[mi][e];
        }
        __syncthreads();
        t_spill(Xs, dZ, H, e0, w, lane);     // dz over dy: this workgroup alone reads and writes the tile's rows
        t_matmul(acc, Xs, W0t, H, w, has0, r, hh);   // dx0[row][i] = sum_o dz[row][o] W0[o][i]
        if (okc) {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float o = acc[mi][e];          // (a copy: the bit cast wants an object, not a vector element)
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o), dxr, loff, (mi * 32 + (e & 3) + 8 * (e >> 2)) * H * 4, 0);
                }
        }
        __syncthreads();
    }
}

#define T_BN_DOMAIN(name)                                                                                                        \
    EPS_REQUIRE(n_nodes >= 0, name ": negative size");                                                                            \
    EPS_REQUIRE(hdim >= T_HMIN && hdim % 4 == 0 && hdim <= T_HMAX, name ": hdim=%d unsupported (need %%4==0, %d..%d)", hdim,      \
                T_HMIN, T_HMAX);                                                                                                  \
    EPS_REQUIRE(n_layers == 2, name ": n_layers=%d unsupported (Linear, BatchNorm, ReLU, Linear: exactly 2)", n_layers);          \
    EPS_REQUIRE(n_pairs >= 2 && n_pairs < ((int64_t)1 << 30), name ": n_pairs=%lld unsupported (batch statistics need 2 .. 2^30 - 1 pairs)", \
                (long long)n_pairs)

static int64_t t_bn_backward_floats(int64_t n_pairs, int32_t hdim)
{
    return eps_mlp_decode_backward_workspace_bytes(n_pairs, hdim, 2) / 4 + 3 * T_HMAX;
}

extern "C" int64_t eps_mlp_decode_bn_workspace_bytes(int64_t n_pairs, int32_t hdim, int32_t n_layers)
{
    if (n_pairs < 2 || hdim < T_HMIN || hdim > T_HMAX || n_layers != 2) return 0;
    const int64_t stats = (int64_t)T_MAX_WG * T_SROW * 8, bwd = t_bn_backward_floats(n_pairs, hdim) * 4;
    return stats > bwd ? stats : bwd;
}

extern "C" int eps_mlp_decode_bn_stats(const float *h, int64_t n_nodes, int32_t hdim, const int32_t *u, const int32_t *v,
                                       int64_t n_pairs, const float *const *w, const float *const *b, int32_t n_layers, float *mean,
                                       float *var, void *workspace, int64_t workspace_bytes, void *stream)
{
    T_BN_DOMAIN("eps_mlp_decode_bn_stats");
    EPS_REQUIRE(h && u && v && w && b && mean && var && workspace, "eps_mlp_decode_bn_stats: null pointer");
    EPS_REQUIRE(w[0] && b[0], "eps_mlp_decode_bn_stats: null weight/bias pointer at layer 0");
    EPS_REQUIRE(n_nodes > 0, "eps_mlp_decode_bn_stats: pairs over an empty node set");
    EPS_REQUIRE((uintptr_t)h % 16 == 0 && (uintptr_t)w[0] % 16 == 0 && (uintptr_t)workspace % 16 == 0,
                "eps_mlp_decode_bn_stats: h, the weight and the workspace must be 16-byte aligned");
    EPS_REQUIRE(workspace_bytes >= (int64_t)T_MAX_WG * T_SROW * 8, "eps_mlp_decode_bn_stats: workspace of %lld bytes, need %lld",
                (long long)workspace_bytes, (long long)T_MAX_WG * T_SROW * 8);
    const hipStream_t st = (hipStream_t)stream;
    const int64_t n_tiles = t_tiles(n_pairs);
    int64_t blocks = (int64_t)eps_num_cus() * 2;
    if (blocks > T_MAX_WG) blocks = T_MAX_WG;
    if (blocks > n_tiles) blocks = n_tiles;
    double *part = (double *)workspace;
    hipLaunchKernelGGL(mlp_decode_bn_stats_kernel, dim3((unsigned)blocks), dim3(T_THREADS), 0, st, h, hdim, u, v, n_pairs, w[0], b[0],
                       part);
    hipLaunchKernelGGL(mlp_decode_bn_merge_kernel, dim3(1), dim3(T_HMAX), 0, st, part, (int32_t)blocks, hdim, mean, var);
    EPS_CHECK_LAUNCH("eps_mlp_decode_bn_stats");
    return EPS_OK;
}

extern "C" int eps_mlp_decode_bn_backward(const float *h, int64_t n_nodes, int32_t hdim, const int32_t *u, const int32_t *v,
                                          int64_t n_pairs, const float *const *w, const float *const *wt, const float *const *b,
                                          int32_t n_layers, const float *const *wf, const float *const *bf, const float *gamma,
                                          const float *mean, const float *var, float bn_eps, const uint32_t *keep, float keep_scale,
                                          const float *grad_out, const int32_t *inc_order, const int64_t *inc_ptr,
                                          float *const *grad_w, float *const *grad_b, float *grad_gamma, float *grad_beta,
                                          float *grad_h, void *workspace, int64_t workspace_bytes, void *stream)
{
    T_BN_DOMAIN("eps_mlp_decode_bn_backward");
    const hipStream_t st = (hipStream_t)stream;
    const int H = hdim, L = 2;
    EPS_REQUIRE(h && u && v && w && wt && b && wf && bf && gamma && mean && var && grad_out && workspace,
                "eps_mlp_decode_bn_backward: null pointer");
    EPS_REQUIRE(n_nodes > 0, "eps_mlp_decode_bn_backward: pairs over an empty node set");
    EPS_REQUIRE((uintptr_t)h % 16 == 0 && (uintptr_t)workspace % 16 == 0, "eps_mlp_decode_bn_backward: h and workspace must be 16-byte aligned");
    EPS_REQUIRE(workspace_bytes >= t_bn_backward_floats(n_pairs, hdim) * 4, "eps_mlp_decode_bn_backward: workspace of %lld bytes, need %lld",
                (long long)workspace_bytes, (long long)t_bn_backward_floats(n_pairs, hdim) * 4);
    EPS_REQUIRE(!grad_h || (inc_order && inc_ptr && (uintptr_t)grad_h % 16 == 0),
                "eps_mlp_decode_bn_backward: grad_h needs the sorted incidence list (inc_order, inc_ptr) and 16-byte alignment");
    EPS_REQUIRE(bn_eps > 0.f, "eps_mlp_decode_bn_backward: eps=%g must be positive", (double)bn_eps);
    TrainParams raw, prm;      // the layers as they are (W0 and its transpose for the dz pass); folded, for the pass that yields dy
    if (int rc = t_params(raw, w, wt, b, n_layers, "eps_mlp_decode_bn_backward")) return rc;
    const float *const wfold[2] = {wf[0], w[1]}, *const bfold[2] = {bf[0], b[1]};
    if (int rc = t_params(prm, wfold, nullptr, bfold, n_layers, "eps_mlp_decode_bn_backward")) return rc;
    if (!keep) keep_scale = 1.0f;

    const int64_t n_tiles = t_tiles(n_pairs), bp = n_tiles * T_BM;
    float *As = (float *)workspace;
    float *dZs = As + bp * H;
    float *dx0 = dZs + bp * H;
    float *part = dx0 + bp * H;
    float *dwp = part + (int64_t)T_MAX_WG * T_GROW;
    float *gsum = dwp + (int64_t)T_DW_MAXS * H * H;
    double *dgam = (double *)(gsum + T_HMAX);

    int64_t blocks = eps_num_cus();
    if (blocks > T_MAX_WG) blocks = T_MAX_WG;
    if (blocks > n_tiles) blocks = n_tiles;
    hipLaunchKernelGGL((mlp_decode_bwd_kernel<false>), dim3((unsigned)blocks), dim3(T_THREADS), 0, st, h, hdim, u, v, n_pairs, prm,
                       n_layers, keep, keep_scale, 0, grad_out, As, dZs, dx0, part);
    EPS_CHECK_LAUNCH("eps_mlp_decode_bn_backward");

    auto sum_rows = [&](const float *src, int64_t stride, int S, int64_t n, float *dst) {
        hipLaunchKernelGGL(mlp_decode_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, stride, (int32_t)S, n, dst);
    };
    int64_t chunk = 0;
    const int S = t_dw_chunks(n_tiles, &chunk);
    const int nt = (H + 127) / 128;
    auto dw = [&](float *dst) {           // dst = dZs^T As
        hipLaunchKernelGGL(mlp_decode_dw_kernel, dim3((unsigned)(nt * nt), (unsigned)S), dim3(256), 0, st, dZs, As, hdim, bp, chunk, dwp);
        sum_rows(dwp, (int64_t)H * H, S, (int64_t)H * H, dst);
    };
    sum_rows(part, T_GROW, (int)blocks, H, gsum);                                  // g' = sum dy
    if (grad_beta) sum_rows(part, T_GROW, (int)blocks, H, grad_beta);
    if (grad_w && grad_w[1]) sum_rows(part + (L - 1) * T_HMAX, T_GROW, (int)blocks, H, grad_w[1]);
    if (grad_b && grad_b[1]) sum_rows(part + T_MAXL * T_HMAX, T_GROW, (int)blocks, 1, grad_b[1]);
    int64_t blocks2 = (int64_t)eps_num_cus() * 2;
    if (blocks2 > T_MAX_WG) blocks2 = T_MAX_WG;
    if (blocks2 > n_tiles) blocks2 = n_tiles;
    double *dgp = (double *)dwp;             // [blocks2][T_HMAX] partials of grad gamma (the dW partials' room: 256 H^2 floats, free here)
    hipLaunchKernelGGL(mlp_decode_bn_dgamma_kernel, dim3((unsigned)blocks2), dim3(T_THREADS), 0, st, hdim, n_pairs, raw.w[0], raw.b[0],
                       mean, var, bn_eps, As, dZs, dgp);
    hipLaunchKernelGGL(mlp_decode_bn_dgamma_sum_kernel, dim3(1), dim3(T_HMAX), 0, st, dgp, (int32_t)blocks2, hdim, dgam, grad_gamma);
    // (193 registers per lane: one workgroup per CU, like the dy pass)
    hipLaunchKernelGGL(mlp_decode_bn_dz_kernel, dim3((unsigned)blocks), dim3(T_THREADS), 0, st, hdim, n_pairs, raw.w[0], raw.wt[0],
                       raw.b[0], gamma, mean, var, bn_eps, gsum, dgam, As, dZs, dx0);
    EPS_CHECK_LAUNCH("eps_mlp_decode_bn_backward");
    if (grad_w && grad_w[0]) dw(grad_w[0]);                                        // grad W0 = dz^T x0
    if (grad_b && grad_b[0]) {                                                     // a bias in front of batch statistics: exactly 0
        const hipError_t e = hipMemsetAsync(grad_b[0], 0, (size_t)H * 4, st);
        EPS_REQUIRE(e == hipSuccess, "eps_mlp_decode_bn_backward: %s", hipGetErrorString(e));
    }
    if (grad_h) {
        hipLaunchKernelGGL(mlp_decode_gradh_kernel, dim3((unsigned)((n_nodes + 3) / 4)), dim3(256), 0, st, h, hdim, n_nodes, u, v,
                           n_pairs, inc_order, inc_ptr, dx0, grad_h);
    }
    EPS_CHECK_LAUNCH("eps_mlp_decode_bn_backward");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void mlp_decode_train_warm_kernel() {}
extern "C" void eps_warm_mlp_decode_train(void *stream) { hipLaunchKernelGGL(mlp_decode_train_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

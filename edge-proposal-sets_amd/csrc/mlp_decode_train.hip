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

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));

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
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void *)M, 0, H * H * 4, 0x00020000);
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
    hipLaunchKernelGGL(mlp_decode_bwd_kernel, dim3((unsigned)blocks), dim3(T_THREADS), 0, st, h, hdim, u, v, n_pairs, prm, n_layers,
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

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void mlp_decode_train_warm_kernel() {}
extern "C" void eps_warm_mlp_decode_train(void *stream) { hipLaunchKernelGGL(mlp_decode_train_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

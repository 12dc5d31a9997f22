// Fused LinkPredictor decode on the f32-input MFMA, gfx950.
//
// Replaces h[edges[0]] / h[edges[1]] gathers (models.py:506) + LinkPredictor.forward
// (models.py:478-485): Hadamard -> (L-1) x [Linear, ReLU] -> Linear(H,1) -> sigmoid, one float
// per candidate edge out.  Dropout is the identity in eval mode (models.py:483 with
// training=False), which is the only mode the scoring path runs in.  The DEA_GNN_JK decoder
// (Hadamard -> Linear + BatchNorm + ReLU -> Linear, logits) runs here too, with each BatchNorm
// folded into the Linear before it on the host.
//
// Two 512-thread workgroups per CU walk 64-edge tiles (persistent, grid-stride):
//   1. gather: each wave builds 8 rows of X = h[u] (.) h[v] straight into LDS (one coalesced
//      1-KiB row read per endpoint, float4 per lane, all 16 reads of a wave in flight at once);
//   2. hidden layers: X[64,H] stays in LDS (66.5 KiB); the W fragments of each 32-wide K-chunk go
//      L2 -> registers directly (16 B per lane, one chunk ahead), so the K loop has no LDS staging
//      and no barrier; each wave owns one 32-wide column tile for all 64 rows (32 accumulator
//      registers), so no two waves read the same W bytes; bias + ReLU are applied in the accumulators and written back over X --
//      activations never leave the CU;
//   3. last layer (H -> 1) is an 8-lanes-per-row dot product over the LDS tile + sigmoid.
// That is mlp_decode_kernel, for H <= 256: 100 VGPRs, 2 workgroups = 4 waves per SIMD.
// 256 < H <= 512 runs mlp_decode_wide_kernel, chosen by H inside eps_mlp_decode: the same phases on 32-edge tiles.
// X is [32, 516] floats (64.5 KiB), so two workgroups per CU (4 waves per SIMD) still fit the 160 KiB of LDS and one
// gathers while the other multiplies; each wave owns two column tiles (w, w + 8) of 32 rows (2 x 16 accumulator
// registers, as many as the narrow kernel); 101 VGPRs, no spills.  The price: a [512, 512] layer (1 MiB, L2-resident
// like the 256 KiB ones) is read once per 32 edges -- 16 MFMA FLOP per L2 byte against the narrow kernel's 32.  A 64-edge
// tile (132 KiB of LDS) would halve that but leave one workgroup per CU and no gather/multiply overlap.
// f32 in, f32 accumulate (v_mfma_f32_32x32x2_f32 == fmaf chain): the 1e-5 parity gate rules out
// bf16/"xf32" shortcuts (and gfx950 has no xf32).
#include "eps_common.h"

#define D_BM 64        // edges per tile
#define D_HMAX 256     // widest hidden size of mlp_decode_kernel (wider: mlp_decode_wide_kernel)
#define D_XLD (D_HMAX + 4)
#define D_BK 32
#define D_MAXL 8

struct DecodeParams {
    const float *w[D_MAXL];
    const float *b[D_MAXL];
};

// Static-index select: a runtime index into the by-value kernel argument would force the
// struct into scratch memory.
__device__ __forceinline__ const float *pick(const float *const (&a)[D_MAXL], int l)
{
    const float *p = a[0];
#pragma unroll
    for (int i = 1; i < D_MAXL; ++i) p = (i == l) ? a[i] : p;
    return p;
}

#define D_THREADS 512  // 8 waves per workgroup; two workgroups per CU (66.5 KiB of LDS each) = 4 waves per SIMD

// Weight fragments go global/L2 -> registers directly: lane (c = lane&31, h = lane>>5) of the wave that owns column
// tile t needs W[t*32 + c][k .. k+3] for k = 32*kc + 8*j + 4*h -- 16 contiguous bytes of a row-major [out,in] matrix,
// and the four j of a K-chunk are the same 128-byte line (L1 hits after the first).  W (256 KiB per layer) lives in
// L2, shared by every workgroup.  Skipping the LDS for W removes the per-chunk staging, its double buffer AND every
// barrier inside the K loop (X is read-only during a layer), and halves the LDS footprint so that a second workgroup
// per CU gathers its rows while the first one is in its MFMA phase.
// Raw buffer loads: rows >= H fall outside the H*H descriptor (zeros, no branch); columns >= H (H % 32 != 0) are
// pushed out of range by a select on the offset.
__device__ __forceinline__ void b_gload(v4f (&bf)[4], __amdgpu_buffer_rsrc_t wr, int H, int t0, int r, int hh, int kc)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int kcol = kc * D_BK + 8 * j + 4 * hh;
        const int o0 = ((t0 * 32 + r) * H + kcol) * 4;
        bf[j] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(wr, kcol < H ? o0 : 0x7ffffff0, 0, 0));
    }
}

__global__ __launch_bounds__(D_THREADS, 4) void mlp_decode_kernel(const float *__restrict__ hmat, int32_t H,
                                                                  const int32_t *__restrict__ pu,
                                                                  const int32_t *__restrict__ pv, int64_t n_pairs,
                                                                  DecodeParams prm, int32_t n_layers, int apply_sigmoid,
                                                                  float *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float Xs[D_BM][D_XLD];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform -> scalar branches, no exec masking
    const int r = lane & 31, hh = lane >> 5;
    // wave w owns column tile w for all 64 rows (two 32x32 MFMA tiles stacked): no two waves read the same W bytes,
    // which halves the L2 -> CU weight traffic of a layer (256 KiB per tile instead of 512)
    const int Hp = (H + 31) & ~31;          // H padded to the MFMA tile width; pad columns are kept at zero
    const int n_ntiles = Hp >> 5;           // 32-column output tiles (<= 8)
    const int t0 = w;
    const bool has0 = t0 < n_ntiles;
    const int nk = Hp / D_BK;
    const int64_t n_tiles = (n_pairs + D_BM - 1) / D_BM;
    const int h4 = H >> 2;                  // float4 per row
    const int hp4 = Hp >> 2;
    const int cl = lane < h4 ? lane : 0;    // this lane's float4 column of a row (clamped for H < 256)

    // the endpoint ids of a tile are fetched one tile ahead: the gather then starts with its row addresses in hand
    int32_t mu_next = 0, mv_next = 0;
    {
        const int64_t p = (int64_t)blockIdx.x * D_BM + lane;
        if (p < n_pairs) {
            mu_next = pu[p];
            mv_next = pv[p];
        }
    }
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t e0 = tile * D_BM;
        // ---- 1. gather + Hadamard into LDS: wave w builds rows 8w..8w+7, all 16 row reads in flight at once ----
        {
            const int32_t mu = mu_next, mv = mv_next;
            {
                const int64_t pn = (tile + gridDim.x) * D_BM + lane;
                const bool okn = pn < n_pairs;
                mu_next = okn ? pu[okn ? pn : 0] : 0;
                mv_next = okn ? pv[okn ? pn : 0] : 0;
            }
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
                if (lane >= h4) pr = (v4f){0.f, 0.f, 0.f, 0.f};  // pad columns (and idle lanes when H < 256)
                if (lane < hp4) *reinterpret_cast<v4f *>(&Xs[w * 8 + i][4 * lane]) = pr;
            }
        }
        __syncthreads();

        // ---- 2. hidden layers: X from LDS, W fragments straight from L2, no barrier inside the K loop ----------
        for (int l = 0; l + 1 < n_layers; ++l) {
            const float *__restrict__ W = pick(prm.w, l);
            const float *__restrict__ Bv = pick(prm.b, l);
            const __amdgpu_buffer_rsrc_t wr = eps_raw_rsrc(W, H * H * 4);
            f32x16 acc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

            v4f bnxt[4];
            b_gload(bnxt, wr, H, t0, r, hh, 0);
            for (int kc = 0; kc < nk; ++kc) {
                // the weight fragments of the NEXT chunk (L2 -> registers) are requested before this chunk's MFMAs;
                // the last trip re-requests its own chunk (an L1 hit) so that the load stays unconditional
                v4f bcur[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) bcur[j] = bnxt[j];
                b_gload(bnxt, wr, H, t0, r, hh, kc + 1 < nk ? kc + 1 : kc);
                float4 af[2][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    af[0][j] = *reinterpret_cast<const float4 *>(&Xs[r][kc * D_BK + 8 * j + 4 * hh]);
                    af[1][j] = *reinterpret_cast<const float4 *>(&Xs[32 + r][kc * D_BK + 8 * j + 4 * hh]);
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
            __syncthreads();  // every wave has finished reading X: overwrite it with relu(acc + b)
            if (has0) {
                const int cc = t0 * 32 + r;
                const float bv = cc < H ? Bv[cc] : 0.f;
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int rr = mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                        const float t = acc[mi][e] + bv;
                        Xs[rr][cc] = t > 0.f ? t : 0.f;
                    }
            }
            __syncthreads();
        }

        // ---- 3. last layer: H -> 1, sigmoid (8 lanes per row) ---------------------------------------
        {
            const float *__restrict__ wl = pick(prm.w, n_layers - 1);
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
            s += eps_dpp_f<0x141>(s);  // row_half_mirror: the other quad of the 8-lane group
            const int64_t p = e0 + row;
            if (part == 0 && p < n_pairs) {
                float z = s + pick(prm.b, n_layers - 1)[0];
                if (apply_sigmoid) z = 1.0f / (1.0f + expf(-z));
                out[p] = z;
            }
        }
        __syncthreads();  // X is rebuilt by the next tile's gather
    }
}

// ---- 256 < H <= 512: 32-edge tiles, two column tiles per wave ------------------------------------------------------
// The same three phases as mlp_decode_kernel.  What changes with the width: a row is 128 float4, so each lane gathers two
// (columns lane and lane + 64) of each of its wave's 4 rows -- again 8 row reads per endpoint; wave w owns the column tiles
// w and w + 8 for all 32 rows (one 32 x 32 MFMA tile each); the last layer gives each row 16 lanes.  Each K-chunk reads
// one A fragment (float4) per j straight before its MFMAs and the weights go through one buffer per tile (below), which
// keeps the wave within the 128 registers that 4 waves per SIMD allow.
#define D_WBM 32
#define D_WHMAX 512
#define D_WXLD (D_WHMAX + 4)

// fragment j of b_gload alone
__device__ __forceinline__ v4f b_frag(__amdgpu_buffer_rsrc_t wr, int H, int t0, int r, int hh, int kc, int j)
{
    const int kcol = kc * D_BK + 8 * j + 4 * hh;
    const int o0 = ((t0 * 32 + r) * H + kcol) * 4;
    return __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(wr, kcol < H ? o0 : 0x7ffffff0, 0, 0));
}

__global__ __launch_bounds__(D_THREADS, 4) void mlp_decode_wide_kernel(const float *__restrict__ hmat, int32_t H,
                                                                       const int32_t *__restrict__ pu,
                                                                       const int32_t *__restrict__ pv, int64_t n_pairs,
                                                                       DecodeParams prm, int32_t n_layers,
                                                                       int apply_sigmoid, float *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float Xs[D_WBM][D_WXLD];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int Hp = (H + 31) & ~31;
    const int n_ntiles = Hp >> 5;           // 9 .. 16
    const bool has1 = w + 8 < n_ntiles;     // tile w always exists (H > 256)
    const int nk = Hp / D_BK;
    const int64_t n_tiles = (n_pairs + D_WBM - 1) / D_WBM;
    const int h4 = H >> 2;
    const int hp4 = Hp >> 2;
    const int cl0 = lane;                          // H > 256: the first float4 column always lies inside the row
    const int cl1 = lane + 64 < h4 ? lane + 64 : 0;

    int32_t mu_next = 0, mv_next = 0;
    {
        const int64_t p = (int64_t)blockIdx.x * D_WBM + lane;
        if (lane < D_WBM && p < n_pairs) {
            mu_next = pu[p];
            mv_next = pv[p];
        }
    }
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t e0 = tile * D_WBM;
        // ---- 1. gather + Hadamard: wave w builds rows 4w..4w+3 ----
        {
            const int32_t mu = mu_next, mv = mv_next;
            {
                const int64_t pn = (tile + gridDim.x) * D_WBM + lane;
                const bool okn = lane < D_WBM && pn < n_pairs;
                mu_next = okn ? pu[okn ? pn : 0] : 0;
                mv_next = okn ? pv[okn ? pn : 0] : 0;
            }
            v4f a[8], b[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t un = __builtin_amdgcn_readlane(mu, w * 4 + i), vn = __builtin_amdgcn_readlane(mv, w * 4 + i);
                a[2 * i] = *reinterpret_cast<const v4f *>(hmat + un * H + 4 * cl0);
                b[2 * i] = *reinterpret_cast<const v4f *>(hmat + vn * H + 4 * cl0);
                a[2 * i + 1] = *reinterpret_cast<const v4f *>(hmat + un * H + 4 * cl1);
                b[2 * i + 1] = *reinterpret_cast<const v4f *>(hmat + vn * H + 4 * cl1);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<v4f *>(&Xs[w * 4 + i][4 * lane]) = a[2 * i] * b[2 * i];
                v4f pr = a[2 * i + 1] * b[2 * i + 1];
                if (lane + 64 >= h4) pr = (v4f){0.f, 0.f, 0.f, 0.f};
                if (lane + 64 < hp4) *reinterpret_cast<v4f *>(&Xs[w * 4 + i][4 * (lane + 64)]) = pr;
            }
        }
        __syncthreads();

        // ---- 2. hidden layers ----
        for (int l = 0; l + 1 < n_layers; ++l) {
            const float *__restrict__ W = pick(prm.w, l);
            const float *__restrict__ Bv = pick(prm.b, l);
            const __amdgpu_buffer_rsrc_t wr = eps_raw_rsrc(W, H * H * 4);
            f32x16 acc[2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

            // one weight buffer per tile, refilled fragment by fragment: the load of (kc + 1, j) is issued as soon as the MFMAs
            // of (kc, j) have read its registers, and has the other three fragments' MFMAs to arrive (a second buffer, as
            // in mlp_decode_kernel, would not fit the register budget next to two tiles)
            v4f bw[2][4];
            b_gload(bw[0], wr, H, w, r, hh, 0);
            b_gload(bw[1], wr, H, w + 8, r, hh, 0);   // (rows >= H of a missing tile 1 read as zeros, no memory access)
            for (int kc = 0; kc < nk; ++kc) {
                const int kn = kc + 1 < nk ? kc + 1 : kc;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 af = *reinterpret_cast<const float4 *>(&Xs[r][kc * D_BK + 8 * j + 4 * hh]);
                    const float a0[4] = {af.x, af.y, af.z, af.w};
#pragma unroll
                    for (int ss = 0; ss < 4; ++ss) {
                        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[ss], bw[0][j][ss], acc[0], 0, 0, 0);
                        if (has1) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[ss], bw[1][j][ss], acc[1], 0, 0, 0);
                    }
                    bw[0][j] = b_frag(wr, H, w, r, hh, kn, j);
                    bw[1][j] = b_frag(wr, H, w + 8, r, hh, kn, j);
                }
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (t == 1 && !has1) break;
                const int cc = (w + 8 * t) * 32 + r;
                const float bv = cc < H ? Bv[cc] : 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int rr = (e & 3) + 8 * (e >> 2) + 4 * hh;
                    const float x = acc[t][e] + bv;
                    Xs[rr][cc] = x > 0.f ? x : 0.f;
                }
            }
            __syncthreads();
        }

        // ---- 3. last layer: H -> 1, sigmoid (16 lanes per row) ----
        {
            const float *__restrict__ wl = pick(prm.w, n_layers - 1);
            const int row = tid >> 4, part = tid & 15;
            float s = 0.f;
            for (int c = part; c < h4; c += 16) {
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
            s += eps_dpp_f<0x140>(s);  // row_mirror: the other 8 lanes of the 16-lane row
            const int64_t p = e0 + row;
            if (part == 0 && p < n_pairs) {
                float z = s + pick(prm.b, n_layers - 1)[0];
                if (apply_sigmoid) z = 1.0f / (1.0f + expf(-z));
                out[p] = z;
            }
        }
        __syncthreads();
    }
}

extern "C" int eps_mlp_decode(const float *h, int64_t n_nodes, int32_t hdim, const int32_t *u, const int32_t *v,
                              int64_t n_pairs, const float *const *w, const float *const *b, int32_t n_layers,
                              int apply_sigmoid, float *out, void *stream)
{
    EPS_REQUIRE(n_pairs >= 0 && n_nodes >= 0, "eps_mlp_decode: negative size");
    EPS_REQUIRE(hdim > 0 && hdim % 4 == 0 && hdim <= D_WHMAX, "eps_mlp_decode: hdim=%d unsupported (need %%4==0, <=%d)",
                hdim, D_WHMAX);
    EPS_REQUIRE(n_layers >= 1 && n_layers <= D_MAXL, "eps_mlp_decode: n_layers=%d unsupported (1..%d)", n_layers, D_MAXL);
    if (n_pairs == 0) return EPS_OK;
    EPS_REQUIRE(h && u && v && w && b && out, "eps_mlp_decode: null pointer");
    EPS_REQUIRE((uintptr_t)h % 16 == 0, "eps_mlp_decode: h must be 16-byte aligned");
    DecodeParams prm;
    for (int l = 0; l < D_MAXL; ++l) {
        prm.w[l] = l < n_layers ? w[l] : nullptr;
        prm.b[l] = l < n_layers ? b[l] : nullptr;
        if (l < n_layers) {
            EPS_REQUIRE(w[l] && b[l], "eps_mlp_decode: null weight/bias pointer at layer %d", l);
            EPS_REQUIRE((uintptr_t)w[l] % 16 == 0, "eps_mlp_decode: weight %d must be 16-byte aligned", l);
        }
    }
    const bool wide = hdim > D_HMAX;
    const int bm = wide ? D_WBM : D_BM;
    const int64_t n_tiles = (n_pairs + bm - 1) / bm;
    int64_t blocks = (int64_t)eps_num_cus() * 2;  // two resident workgroups per CU: one gathers while the other multiplies
    if (blocks > n_tiles) blocks = n_tiles;
    hipLaunchKernelGGL(wide ? mlp_decode_wide_kernel : mlp_decode_kernel, dim3((unsigned)blocks), dim3(D_THREADS), 0,
                       (hipStream_t)stream, h, hdim, u, v, n_pairs, prm, n_layers, apply_sigmoid, out);
    EPS_CHECK_LAUNCH("eps_mlp_decode");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void mlp_decode_warm_kernel() {}
extern "C" void eps_warm_mlp_decode(void *stream) { hipLaunchKernelGGL(mlp_decode_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

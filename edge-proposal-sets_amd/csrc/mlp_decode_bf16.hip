// Fused LinkPredictor decode on the bf16 MFMA (v_mfma_f32_32x32x16_bf16, fp32 accumulate), gfx950 -- the SCREENING pass of
// the GNN filters (filter.py --decode_precision bf16), and the float32 -> bfloat16 conversion it needs.
//
// Same job as eps_mlp_decode (mlp_decode.hip; models.py:478-485 through filter.py:116-121): gather h[u] (.) h[v], L - 1
// hidden layers with ReLU, the final dot, the optional sigmoid, float32 out.  The embedding table and the hidden weights
// are bf16; biases, the last layer and everything after the last hidden layer are fp32.  The rounding points are fixed
// (RNE = round to nearest, ties to even), so that a CPU emulation can follow them:
//   x0 = RNE_bf16(float(h_u) * float(h_v))          (the product of two bf16 values is exact in fp32)
//   a_l = sum_k x W accumulated in fp32, + b in fp32, ReLU; rounded RNE to bf16 for every hidden layer except the last
//   the last hidden layer's output stays fp32; final dot with the fp32 weight, + bias, sigmoid: fp32.
//
// Three 512-thread workgroups per CU walk 64-edge tiles (persistent, grid-stride), the phases of mlp_decode_kernel:
//   1. gather: a bf16 row is at most 512 bytes = 32 lanes x 16 B, so a wave reads TWO rows per load instruction (one per
//      32-lane half); wave w builds rows 8w .. 8w+7 of X = h[u] (.) h[v] in LDS as bf16 (33 KiB for the tile, against the
//      fp32 kernel's 66.5: three workgroups per CU instead of two, so a tile's gather hides under two other tiles' MFMAs);
//   2. hidden layers, TRANSPOSED: wave w computes out^T[32 channels of tile w][64 edges] = W . X^T.  The A operand is the
//      weight fragment (lane (r, h): W[32w + r][16kc + 8h .. +7], 16 contiguous bytes of the row-major [out, in] matrix,
//      L2 -> registers, two K-steps ahead, no LDS staging and no barrier inside the K loop), the B operand is the X
//      fragment (lane (r, h): X[edge r (+32)][16kc + 8h .. +7], one ds_read_b128).  In the result a lane holds ONE edge
//      (its column) and 16 channels (its registers: channel (e & 3) + 8 (e >> 2) + 4 h of the tile), so
//        - the write-back of a hidden layer packs 4 consecutive channels into one 8-byte LDS store, and
//        - the last layer's dot runs over the lane's own registers in fp32: the fp32 activations never go to LDS at all;
//   3. the 16 partial dots of an edge (8 waves x 2 halves) meet in a 4 KiB LDS table; 64 threads add them in a fixed
//      order, + bias, sigmoid.
// H % 16 == 0 keeps a K-step whole and every row 16-byte aligned; output tiles are 32 channels wide, and the half tile of
// H % 32 == 16 reads zeros past the end of W through the buffer descriptor and writes nothing.
#include "eps_common.h"

typedef int v2i __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define B_BM 64                 // edges per tile
#define B_HMAX 256              // widest hidden size
#define B_XLD (B_HMAX + 8)      // bf16 per LDS row: 528 bytes, 16-byte aligned, rows 4 banks apart
#define B_MAXL 8                // layers, as eps_mlp_decode
#define B_THREADS 512           // 8 waves per workgroup
#define B_WG_PER_CU 3           // 37 KiB of LDS and <= 80 VGPRs each: 6 waves per SIMD (4 would cap a wave at 64 registers: spills)

struct DecodeBf16Params {
    const void *w[B_MAXL];      // hidden layers: bf16 [H, H]; the last layer: float [1, H]
    const float *b[B_MAXL];
};

// Static-index select (a runtime index into the by-value kernel argument would force the struct into scratch memory).
template <typename T> __device__ __forceinline__ T pick(T const (&a)[B_MAXL], int l)
{
    T p = a[0];
#pragma unroll
    for (int i = 1; i < B_MAXL; ++i) p = (i == l) ? a[i] : p;
    return p;
}

// RNE float32 -> bfloat16 bits, as torch's c10::BFloat16 rounds: every NaN becomes the quiet 0x7FC0.
__device__ __forceinline__ uint32_t bf16_bits_rne(float x)
{
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ uint32_t pack2(float lo, float hi) { return bf16_bits_rne(lo) | (bf16_bits_rne(hi) << 16); }

__device__ __forceinline__ float bf_lo(int x) { return __builtin_bit_cast(float, (uint32_t)x << 16); }
__device__ __forceinline__ float bf_hi(int x) { return __builtin_bit_cast(float, (uint32_t)x & 0xffff0000u); }

// the weight fragment of K-step kc for output tile t: rows >= H fall outside the H*H descriptor and read as zeros
__device__ __forceinline__ v4i w_frag(__amdgpu_buffer_rsrc_t wr, int H, int t, int r, int hh, int kc)
{
    return __builtin_amdgcn_raw_buffer_load_b128(wr, ((t * 32 + r) * H + kc * 16 + 8 * hh) * 2, 0, 0);
}

__global__ __launch_bounds__(B_THREADS, 2 * B_WG_PER_CU) void mlp_decode_bf16_kernel(
    const uint16_t *__restrict__ hmat, int32_t H, const int32_t *__restrict__ pu, const int32_t *__restrict__ pv,
    int64_t n_pairs, DecodeBf16Params prm, int32_t n_layers, int apply_sigmoid, float *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint16_t Xs[B_BM][B_XLD];
    __shared__ float red[16][B_BM];      // [2 * wave + half][edge]: partial dots of the last layer

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int n_ntiles = (H + 31) >> 5;     // 32-channel output tiles (<= 8); wave w owns tile w
    const bool has = w < n_ntiles;
    const int nk = H >> 4;                  // K-steps of 16
    const int h8 = H >> 3;                  // 16-byte chunks per row (even)
    const int64_t n_tiles = (n_pairs + B_BM - 1) / B_BM;

    // the endpoint ids of a tile are fetched one tile ahead; rows past n_pairs gather node 0 (a valid row: the whole
    // X tile is always written, their results are not)
    int32_t mu_next = 0, mv_next = 0;
    {
        const int64_t p = (int64_t)blockIdx.x * B_BM + lane;
        if (p < n_pairs) {
            mu_next = pu[p];
            mv_next = pv[p];
        }
    }
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t e0 = tile * B_BM;
        // ---- 1. gather + Hadamard into LDS: wave w builds rows 8w .. 8w+7, two rows per load (one per half) ----
        {
            const int32_t mu = mu_next, mv = mv_next;
            {
                const int64_t pn = (tile + gridDim.x) * B_BM + lane;
                const bool okn = pn < n_pairs;
                mu_next = okn ? pu[okn ? pn : 0] : 0;
                mv_next = okn ? pv[okn ? pn : 0] : 0;
            }
            const int cl = r < h8 ? r : 0;
            v4i a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = w * 8 + 2 * i + hh;
                const int64_t un = __shfl(mu, row), vn = __shfl(mv, row);
                a[i] = *reinterpret_cast<const v4i *>(hmat + un * H + 8 * cl);
                b[i] = *reinterpret_cast<const v4i *>(hmat + vn * H + 8 * cl);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v4i pr;
#pragma unroll
                for (int q = 0; q < 4; ++q) pr[q] = (int)pack2(bf_lo(a[i][q]) * bf_lo(b[i][q]), bf_hi(a[i][q]) * bf_hi(b[i][q]));
                if (r < h8) *reinterpret_cast<v4i *>(&Xs[w * 8 + 2 * i + hh][8 * r]) = pr;
            }
        }
        __syncthreads();

        // ---- 2. hidden layers: X fragments from LDS, W fragments straight from L2 ------------------------------
        for (int l = 0; l + 1 < n_layers; ++l) {
            const bool last_hidden = l + 2 == n_layers;
            const float *__restrict__ Bv = pick(prm.b, l);
            const __amdgpu_buffer_rsrc_t wr = eps_raw_rsrc(pick(prm.w, l), H * H * 2);
            f32x16 acc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
            if (has) {
                // the fragments of K-steps kc + 1 and kc + 2 are in flight under step kc's MFMAs; the last trips re-request
                // the last step (an L1 hit) so that the load stays unconditional
                v4i b0 = w_frag(wr, H, w, r, hh, 0);
                v4i b1 = w_frag(wr, H, w, r, hh, nk > 1 ? 1 : 0);
                for (int kc = 0; kc < nk; ++kc) {
                    const v4i bc = b0;
                    b0 = b1;
                    b1 = w_frag(wr, H, w, r, hh, kc + 2 < nk ? kc + 2 : nk - 1);
                    const v4i x0 = *reinterpret_cast<const v4i *>(&Xs[r][kc * 16 + 8 * hh]);
                    const v4i x1 = *reinterpret_cast<const v4i *>(&Xs[32 + r][kc * 16 + 8 * hh]);
                    const bf16x8 wa = __builtin_bit_cast(bf16x8, bc);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, __builtin_bit_cast(bf16x8, x0), acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, __builtin_bit_cast(bf16x8, x1), acc[1], 0, 0, 0);
                }
            }
            __syncthreads();  // every wave has finished reading X
            // this lane's 16 channels: four groups of four consecutive ones, c0(g) = 32w + 8g + 4h (whole groups lie
            // inside or outside H, which is a multiple of 16)
            if (!last_hidden) {
                if (has) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int c0 = w * 32 + 8 * g + 4 * hh;
                        if (c0 < H) {
                            const v4f bv = *reinterpret_cast<const v4f *>(Bv + c0);
#pragma unroll
                            for (int mi = 0; mi < 2; ++mi) {
                                float t[4];
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    const float s = acc[mi][4 * g + q] + bv[q];
                                    t[q] = s > 0.f ? s : 0.f;
                                }
                                v2i pk;
                                pk[0] = (int)pack2(t[0], t[1]);
                                pk[1] = (int)pack2(t[2], t[3]);
                                *reinterpret_cast<v2i *>(&Xs[mi * 32 + r][c0]) = pk;
                            }
                        }
                    }
                }
                __syncthreads();
                continue;
            }
            // ---- 3. the last hidden layer stays fp32 in the accumulators: bias, ReLU and the H -> 1 dot in place ----
            {
                const float *__restrict__ wl = reinterpret_cast<const float *>(pick(prm.w, n_layers - 1));
                float s0 = 0.f, s1 = 0.f;
                if (has) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int c0 = w * 32 + 8 * g + 4 * hh;
                        if (c0 < H) {
                            const v4f bv = *reinterpret_cast<const v4f *>(Bv + c0);
                            const v4f q4 = *reinterpret_cast<const v4f *>(wl + c0);
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const float t0 = acc[0][4 * g + q] + bv[q], t1 = acc[1][4 * g + q] + bv[q];
                                s0 = fmaf(t0 > 0.f ? t0 : 0.f, q4[q], s0);
                                s1 = fmaf(t1 > 0.f ? t1 : 0.f, q4[q], s1);
                            }
                        }
                    }
                }
                red[2 * w + hh][r] = s0;          // (waves without a tile write their zeros: the table is whole)
                red[2 * w + hh][32 + r] = s1;
            }
            __syncthreads();
            if (tid < B_BM) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < 16; ++j) s += red[j][tid];
                const int64_t p = e0 + tid;
                if (p < n_pairs) {
                    float z = s + pick(prm.b, n_layers - 1)[0];
                    if (apply_sigmoid) z = 1.0f / (1.0f + expf(-z));
                    out[p] = z;
                }
            }
            // (the next tile's gather writes X, which nobody reads any more; red is rewritten only after that
            //  gather's barrier)
        }
    }
}

extern "C" int eps_mlp_decode_bf16(const uint16_t *h, int64_t n_nodes, int32_t hdim, const int32_t *u, const int32_t *v,
                                   int64_t n_pairs, const void *const *w, const float *const *b, int32_t n_layers,
                                   int apply_sigmoid, float *out, void *stream)
{
    EPS_REQUIRE(n_pairs >= 0 && n_nodes >= 0, "eps_mlp_decode_bf16: negative size");
    EPS_REQUIRE(hdim > 0 && hdim % 16 == 0 && hdim <= B_HMAX,
                "eps_mlp_decode_bf16: hdim=%d unsupported (need %%16==0, <=%d; wider or odd widths decode in fp32)", hdim, B_HMAX);
    EPS_REQUIRE(n_layers >= 2 && n_layers <= B_MAXL,
                "eps_mlp_decode_bf16: n_layers=%d unsupported (2..%d; one layer has no matrix work)", n_layers, B_MAXL);
    if (n_pairs == 0) return EPS_OK;
    EPS_REQUIRE(h && u && v && w && b && out, "eps_mlp_decode_bf16: null pointer");
    EPS_REQUIRE((uintptr_t)h % 16 == 0, "eps_mlp_decode_bf16: h must be 16-byte aligned");
    DecodeBf16Params prm;
    for (int l = 0; l < B_MAXL; ++l) {
        prm.w[l] = l < n_layers ? w[l] : nullptr;
        prm.b[l] = l < n_layers ? b[l] : nullptr;
        if (l < n_layers) {
            EPS_REQUIRE(w[l] && b[l], "eps_mlp_decode_bf16: null weight/bias pointer at layer %d", l);
            EPS_REQUIRE((uintptr_t)w[l] % 16 == 0, "eps_mlp_decode_bf16: weight %d must be 16-byte aligned", l);
            EPS_REQUIRE((uintptr_t)b[l] % 16 == 0 || l == n_layers - 1, "eps_mlp_decode_bf16: bias %d must be 16-byte aligned", l);
        }
    }
    const int64_t n_tiles = (n_pairs + B_BM - 1) / B_BM;
    int64_t blocks = (int64_t)eps_num_cus() * B_WG_PER_CU;
    if (blocks > n_tiles) blocks = n_tiles;
    hipLaunchKernelGGL(mlp_decode_bf16_kernel, dim3((unsigned)blocks), dim3(B_THREADS), 0, (hipStream_t)stream, h, hdim, u, v,
                       n_pairs, prm, n_layers, apply_sigmoid, out);
    EPS_CHECK_LAUNCH("eps_mlp_decode_bf16");
    return EPS_OK;
}

// ---- float32 -> bfloat16, RNE, the bits of torch's float32 -> bfloat16 (the table and the hidden weights) -----------
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float *__restrict__ x, int64_t n, uint16_t *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (uint16_t)bf16_bits_rne(x[i]);
}

extern "C" int eps_f32_to_bf16(const float *x, int64_t n, uint16_t *out, void *stream)
{
    EPS_REQUIRE(n >= 0, "eps_f32_to_bf16: negative size");
    if (n == 0) return EPS_OK;
    EPS_REQUIRE(x && out, "eps_f32_to_bf16: null pointer");
    int64_t blocks = (n + 255) / 256;
    const int64_t cap = (int64_t)eps_num_cus() * 16;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, n, out);
    EPS_CHECK_LAUNCH("eps_f32_to_bf16");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void mlp_decode_bf16_warm_kernel() {}
extern "C" void eps_warm_mlp_decode_bf16(void *stream) { hipLaunchKernelGGL(mlp_decode_bf16_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }

// Helpers shared by the cosine common-neighbour units (cosine_cn.hip: the forward prologue; cosine_cn_bwd.hip: its
// backward), gfx950: the slot / chunk layout of a wave over a feature row, float4 / scalar row access, slot reductions.
#pragma once
#include "eps_common.h"

#define CC_THREADS 256
#define CC_REG_CHUNKS 8          // chunks of G x VEC floats a lane keeps in registers (float4: 2048 features per wave)
#define CC_FLIGHT_VEC4 8         // float4 loads in flight per lane per batch (divided over the chunks of a row)

// elements [c, c + VEC) of row p, zero past column f (c < f)
__device__ __forceinline__ float4 cc_load(const float *__restrict__ p, int c, int f, float4)
{
    if (c + 4 <= f) return *reinterpret_cast<const float4 *>(p + c);
    float4 r = make_float4(p[c], 0.f, 0.f, 0.f);
    if (c + 1 < f) r.y = p[c + 1];
    if (c + 2 < f) r.z = p[c + 2];
    return r;
}
__device__ __forceinline__ float cc_load(const float *__restrict__ p, int c, int, float) { return p[c]; }

__device__ __forceinline__ void cc_store(float *__restrict__ p, int c, int f, const float4 &v)
{
    if (c + 4 <= f) {
        *reinterpret_cast<float4 *>(p + c) = v;
        return;
    }
    p[c] = v.x;
    if (c + 1 < f) p[c + 1] = v.y;
    if (c + 2 < f) p[c + 2] = v.z;
}
__device__ __forceinline__ void cc_store(float *__restrict__ p, int c, int, float v) { p[c] = v; }

// sum over the lanes whose ids differ only in the bits [lo, hi) of the lane id (lo, hi powers of two)
__device__ __forceinline__ float cc_xor_sum(float x, int lo, int hi)
{
    for (int o = lo; o < hi; o <<= 1) x += __shfl_xor(x, o);
    return x;
}
__device__ __forceinline__ float4 cc_xor_sum(float4 x, int lo, int hi)
{
    for (int o = lo; o < hi; o <<= 1) {
        x.x += __shfl_xor(x.x, o);
        x.y += __shfl_xor(x.y, o);
        x.z += __shfl_xor(x.z, o);
        x.w += __shfl_xor(x.w, o);
    }
    return x;
}
__device__ __forceinline__ float4 cc_axpy_div(const float4 &x, const float4 &a, float d)
{
    return make_float4(x.x + a.x / d, x.y + a.y / d, x.z + a.z / d, x.w + a.w / d);
}
__device__ __forceinline__ float cc_axpy_div(float x, float a, float d) { return x + a / d; }
__device__ __forceinline__ float4 cc_div(const float4 &x, float d) { return make_float4(x.x / d, x.y / d, x.z / d, x.w / d); }
__device__ __forceinline__ float cc_div(float x, float d) { return x / d; }

// log2 of the lanes per slot: the smallest power of two whose lanes x vec floats span f (at most 64 lanes)
static int cc_lanes_log2(int64_t f, int vec)
{
    const int64_t units = (f + vec - 1) / vec;
    int lg = 0;
    while (lg < 6 && (1ll << lg) < units) ++lg;
    return lg;
}

static int cc_reg_chunks(int64_t chunks)     // register chunk template: 1, 2, 4 or 8
{
    return chunks <= 1 ? 1 : chunks <= 2 ? 2 : chunks <= 4 ? 4 : 8;
}

static unsigned cc_blocks(int64_t n_rows)
{
    const int64_t waves_per_block = CC_THREADS / 64;
    int64_t b = (n_rows + waves_per_block - 1) / waves_per_block;
    const int64_t cap = (int64_t)eps_num_cus() * 16;
    return (unsigned)(b < cap ? b : cap);
}

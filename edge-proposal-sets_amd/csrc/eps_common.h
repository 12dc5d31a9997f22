// Shared host/device helpers for libeps_hip.so (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/eps_abi.h"

#define EPS_WAVE 64

void eps_set_error(const char *fmt, ...);

#define EPS_REQUIRE(cond, ...)            \
    do {                                  \
        if (!(cond)) {                    \
            eps_set_error(__VA_ARGS__);   \
            return EPS_EINVAL;            \
        }                                 \
    } while (0)

#define EPS_CHECK_LAUNCH(name)                                                   \
    do {                                                                         \
        hipError_t e__ = hipGetLastError();                                      \
        if (e__ != hipSuccess) {                                                 \
            eps_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
            return EPS_ELAUNCH;                                                  \
        }                                                                        \
    } while (0)

// Number of CUs of the current device (cached per process; 256 on MI355X).
int eps_num_cus();

// A zeroed device word for a kernel's dynamic work hand-out (see eps_common.hip).
int eps_take_counter(unsigned int **counter, hipStream_t stream, const char *who);
// ... eight consecutive zeroed words (a hand-out with one counter per XCD)
int eps_take_counters8(unsigned int **counters, hipStream_t stream, const char *who);

#if defined(__HIPCC__)
// ---- wave-level reductions (all 64 lanes receive the total) --------------------------
// quad_perm / row_mirror DPP for the first four butterfly steps (VALU rate, no LDS traffic),
// ds_bpermute-backed shuffles for the two cross-row steps.
template <int CTRL>
__device__ __forceinline__ float eps_dpp_f(float x)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int eps_dpp_i(int x)
{
    return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true);
}

__device__ __forceinline__ float eps_wave_sum(float x)
{
    x += eps_dpp_f<0xB1>(x);   // quad_perm [1,0,3,2]
    x += eps_dpp_f<0x4E>(x);   // quad_perm [2,3,0,1]
    x += eps_dpp_f<0x141>(x);  // row_half_mirror
    x += eps_dpp_f<0x140>(x);  // row_mirror
    x += __shfl_xor(x, 16);
    x += __shfl_xor(x, 32);
    return x;
}

__device__ __forceinline__ double eps_wave_sum(double x)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) x += __shfl_xor(x, o);
    return x;
}

__device__ __forceinline__ int eps_lane() { return threadIdx.x & 63; }

// Inclusive prefix of x over the wave's lanes (lane = 0..63 of the caller) ...
template <typename T>
__device__ __forceinline__ T eps_wave_incl_scan(T x, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T up = __shfl_up(x, o);
        if (lane >= o) x += up;
    }
    return x;
}
// ... and the exclusive one; total = the wave's sum, in every lane.
template <typename T>
__device__ __forceinline__ T eps_wave_excl_scan(T x, int lane, T &total)
{
    const T incl = eps_wave_incl_scan(x, lane);
    total = __shfl(incl, 63);
    return incl - x;
}

// The same inclusive prefix sum on the DPP path (row shifts inside the 16-lane rows, then the two row broadcasts): six
// VALU instructions, no LDS traffic.  Lanes a shift does not reach add 0; lane 63 holds the total.
__device__ __forceinline__ int eps_wave_incl_scan_dpp(int x)
{
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, false);   // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, false);   // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, false);   // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, false);   // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);   // row_bcast:15 -> rows 1, 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);   // row_bcast:31 -> rows 2, 3
    return x;
}

// Lane j's 64-bit value in every lane (j wave-uniform): two v_readlane.
__device__ __forceinline__ int64_t eps_bcast64(int64_t x, int j)
{
    const int lo = __builtin_amdgcn_readlane((int)(x & 0xffffffffll), j);
    const int hi = __builtin_amdgcn_readlane((int)(x >> 32), j);
    return ((int64_t)hi << 32) | (uint32_t)lo;
}

// LDS written by some lanes of the wave is read by others after this.
__device__ __forceinline__ void lds_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the vector-memory counter, which would
// end every global load a wave keeps in flight across the barrier (record and row prefetches).  A hand-off between waves
// that goes through global memory keeps __syncthreads().
__device__ __forceinline__ void eps_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Grid-wide hand-over on an arrival counter: returns once `target` workgroups have arrived (the caller counts epochs:
// target = epoch * gridDim.x), with every global write made before it visible after it.  The grid must be co-resident.
// SLEEP: the s_sleep argument of the waiting thread's poll.
template <int SLEEP>
__device__ __forceinline__ void eps_grid_sync(uint32_t *arrive, uint32_t target)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        atomicAdd(arrive, 1u);
        while (__atomic_load_n(arrive, __ATOMIC_RELAXED) < target) __builtin_amdgcn_s_sleep(SLEEP);
        __threadfence();
    }
    __syncthreads();
}

// ---- ordered float keys ---------------------------------------------------------------
// float -> uint32_t whose unsigned order is the floats' order, and back.  The one definition of the tie rule of the two
// zeros (NaN sorts where its bit pattern puts it).
__device__ __forceinline__ uint32_t eps_ordered_bits(float f)
{
    f = f + 0.0f;  // -0.0 -> +0.0 so that the two zeros tie, as they do in torch.sort
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float eps_unordered_bits(uint32_t o)
{
    const uint32_t b = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    return __builtin_bit_cast(float, b);
}

// ---- native vectors and raw buffer resources ------------------------------------------
// Native vectors stay in VGPRs (HIP's float4 struct copies lower to memcpy -> scratch); v4i is what a 16-byte raw buffer
// load returns, f32x16 a 32x32 MFMA accumulator.
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Raw (stride 0) buffer descriptor over `bytes` bytes at base: num_records = bytes, so a dwordx4 load needs no exec
// masking and no bounds branch -- out-of-range dwords come back as 0 (probed on gfx950: per-dword range check,
// 4-byte-aligned bases are fine; tools/probe_bufload.hip).  The flag word is the descriptor's last dword: DATA_FORMAT = 32
// (bits 15..18 = 4), every other field 0 -- no swizzle, no thread-id addressing.
#define EPS_RAW_RSRC_FLAGS 0x00020000
__device__ __forceinline__ __amdgpu_buffer_rsrc_t eps_raw_rsrc(const void *base, int bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, bytes, EPS_RAW_RSRC_FLAGS);
}

// ---- float / float4 feature-row helpers -----------------------------------------------
template <int VEC>
struct eps_vec;
template <>
struct eps_vec<4> {
    using type = float4;
};
template <>
struct eps_vec<1> {
    using type = float;
};
__device__ __forceinline__ float4 eps_zero(float4) { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float eps_zero(float) { return 0.f; }
__device__ __forceinline__ void eps_fma(float4 &a, float s, const float4 &x)
{
    a.x = fmaf(s, x.x, a.x);
    a.y = fmaf(s, x.y, a.y);
    a.z = fmaf(s, x.z, a.z);
    a.w = fmaf(s, x.w, a.w);
}
__device__ __forceinline__ void eps_fma(float &a, float s, float x) { a = fmaf(s, x, a); }
__device__ __forceinline__ float eps_dot(const float4 &a, const float4 &b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float eps_dot(float a, float b) { return a * b; }

// ---- per-lane lower bound -------------------------------------------------------------
// First index in [lo, hi) of the ascending array a whose element is not below key (hi if none).  Elements are compared
// as K, indices are I: a caller picks the width and signedness of both.
template <typename T, typename I, typename K>
__device__ __forceinline__ I eps_lower_bound(const T *__restrict__ a, I lo, I hi, K key)
{
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;
        if ((K)a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
#endif

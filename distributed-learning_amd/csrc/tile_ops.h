// Leaf device helpers of the tile kernels (mix_tile.hip, mix_sgd.hip, mix_cheb.hip, mix_multi.hip
// and mix_trace.hip, all through tile_core.h, which builds the shared per-tile pieces on them):
// 16-byte loads and stores with their cache policies, guarded row accesses, and the fp32 fold and
// wave-sum primitives.  Every function is force-inlined, in an unnamed namespace: each kernel
// file gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dl {
namespace {

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

typedef float f32x4 __attribute__((ext_vector_type(4)));

// 16-byte non-temporal load (global_load_dwordx4 ... nt): streamed once, keep it out of L2/MALL
__device__ __forceinline__ float4 nt_load4(const float4 *p) {
    const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p));
    return make_float4(x.x, x.y, x.z, x.w);
}

// 16-byte non-temporal store (global_store_dwordx4 ... nt)
__device__ __forceinline__ void nt_store4(float4 v, float4 *p) {
    f32x4 x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, reinterpret_cast<f32x4 *>(p));
}

// FAST-path streams of a tile through buffer instructions whose cache policy is an immediate.
// The non-temporal hint is a runtime choice (dl::TileArgs nt_load / nt_store), and two global
// accesses that differ only in it are one instruction to the optimizer, which merged the two
// arms of that choice and dropped the hint (round 5: every load and store of the c2 round plain,
// 446 -> 427 rounds/s on one box).  Buffer loads and stores carry the policy as an operand that
// must stay a constant, so the arms stay two instructions; tests/test_kernel_isa.py checks the
// built code object for them.  Base = a uniform tile pointer, 32-bit offsets as for the global
// forms (the host admits this path only when every operand spans < 4 GiB); the resource's
// record count is the whole 32-bit range, so no access is clipped.
constexpr int kBufNT = 2;   // cache-policy operand: nt (gfx950)
typedef unsigned int u32x4v __attribute__((vector_size(16)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void *base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, -1, 0x00020000);
}

template <int AUX>
__device__ __forceinline__ float4 buf_ld4(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, AUX));
    return make_float4(v.x, v.y, v.z, v.w);
}

template <int AUX>
__device__ __forceinline__ void buf_st4(float4 v, __amdgpu_buffer_rsrc_t r, uint32_t off) {
    const f32x4 x = {v.x, v.y, v.z, v.w};
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, x), r, off, 0, AUX);
}

// Load 4 consecutive floats starting at column c0 of `row`; columns >= P read as 0.
__device__ __forceinline__ float4 ld4(const float *__restrict__ row, int64_t c0, int64_t P,
                                      bool vec) {
    if (vec && c0 + 3 < P) return *reinterpret_cast<const float4 *>(row + c0);
    float4 v = zero4();
    if (c0 < P) v.x = row[c0];
    if (c0 + 1 < P) v.y = row[c0 + 1];
    if (c0 + 2 < P) v.z = row[c0 + 2];
    if (c0 + 3 < P) v.w = row[c0 + 3];
    return v;
}

__device__ __forceinline__ void st4(float *__restrict__ row, int64_t c0, int64_t P, bool vec,
                                    float4 v) {
    if (vec && c0 + 3 < P) {
        *reinterpret_cast<float4 *>(row + c0) = v;
        return;
    }
    if (c0 < P) row[c0] = v.x;
    if (c0 + 1 < P) row[c0 + 1] = v.y;
    if (c0 + 2 < P) row[c0 + 2] = v.z;
    if (c0 + 3 < P) row[c0 + 3] = v.w;
}

__device__ __forceinline__ void axpy4(float4 &acc, float w, float4 v) {
    acc.x = acc.x + w * v.x;
    acc.y = acc.y + w * v.y;
    acc.z = acc.z + w * v.z;
    acc.w = acc.w + w * v.w;
}

__device__ __forceinline__ void add4(float4 &a, float4 b) {
    a.x = a.x + b.x;
    a.y = a.y + b.y;
    a.z = a.z + b.z;
    a.w = a.w + b.w;
}

// v + v[lane ^ m] across the wave (m a power of two, a compile-time constant after unrolling),
// without the LDS unit where gfx950 has a register path: xor 1 / 2 are DPP quad permutes, xor
// 16 / 32 the v_permlane16/32_swap pair (their two results are {v, partner} per lane, in some
// order: the sum is the same IEEE add); xor 4 / 8 stay ds_bpermute.  Bit-identical to
// v + __shfl_xor(v, m) (a + b == b + a).
__device__ __forceinline__ float xor_add(float v, int m) {
    if (m == 1)
        return v + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));
    if (m == 2)
        return v + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));
    if (m == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v),
                                                        false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    if (m == 32) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v),
                                                        false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    return v + __shfl_xor(v, m);
}

__device__ __forceinline__ float4 shfl_xor4(float4 v, int m) {
    v.x = xor_add(v.x, m);
    v.y = xor_add(v.y, m);
    v.z = xor_add(v.z, m);
    v.w = xor_add(v.w, m);
    return v;
}

}  // namespace
}  // namespace dl

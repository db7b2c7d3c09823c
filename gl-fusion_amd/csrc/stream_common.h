// What the HBM-bound ("streaming") translation units share: the grid of a grid-stride pass, the wavefront sum, the dropout hash, the
// bf16 pack / unpack, and the storage trait Stream<T, W> through which ONE kernel body serves fp32 and bf16 storage (pointwise.hip).
#pragma once
#include "glf_common.h"

namespace glf {

typedef unsigned short u16;                // one bf16 element in memory

// grid of a grid-stride pass over `total` accesses: at most eight workgroups per CU
inline int stream_grid(long long total, int block) {
    long long g = (total + block - 1) / block;
    const long long cap = (long long)num_cus() * 8;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
// counter-based dropout hash: 24 bits of splitmix64
__device__ __forceinline__ unsigned mix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (unsigned)(z >> 40);
}

// W floats in registers
template <int W> struct FV { float v[W]; };
typedef FV<8> F8;

__device__ __forceinline__ F8 unpack8(const uint4 q) {
    F8 o;
    o.v[0] = __uint_as_float(q.x << 16); o.v[1] = __uint_as_float(q.x & 0xffff0000u);
    o.v[2] = __uint_as_float(q.y << 16); o.v[3] = __uint_as_float(q.y & 0xffff0000u);
    o.v[4] = __uint_as_float(q.z << 16); o.v[5] = __uint_as_float(q.z & 0xffff0000u);
    o.v[6] = __uint_as_float(q.w << 16); o.v[7] = __uint_as_float(q.w & 0xffff0000u);
    return o;
}
__device__ __forceinline__ F8 ld8(const u16* p) { return unpack8(*reinterpret_cast<const uint4*>(p)); }
// two floats -> two bf16 in one word, round-to-nearest-even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pack2(float a, float b) {
    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2_ __attribute__((ext_vector_type(2)));
    const f32x2_ v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_));
}
__device__ __forceinline__ void st8(u16* p, const F8& o) {
    *reinterpret_cast<uint4*>(p) = make_uint4(pack2(o.v[0], o.v[1]), pack2(o.v[2], o.v[3]), pack2(o.v[4], o.v[5]), pack2(o.v[6], o.v[7]));
}
__device__ __forceinline__ F8 ldf8(const float* p) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    F8 o;
    o.v[0] = a.x; o.v[1] = a.y; o.v[2] = a.z; o.v[3] = a.w; o.v[4] = b.x; o.v[5] = b.y; o.v[6] = b.z; o.v[7] = b.w;
    return o;
}
__device__ __forceinline__ float bf2f(u16 h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ u16 f2bf(float f) { return (u16)(pack2(f, 0.f) & 0xffffu); }

// Stream<T, W>: W consecutive elements of storage type T <-> floats in registers, in ONE memory access of W * sizeof(T) bytes
// (p aligned to that).  Arithmetic is fp32 either way; bf16 is rounded once, to nearest even, at the store.
template <class T, int W> struct Stream;
template <> struct Stream<float, 1> {
    static __device__ __forceinline__ FV<1> ld(const float* p) { return {{*p}}; }
    static __device__ __forceinline__ void st(float* p, const FV<1>& o) { *p = o.v[0]; }
};
// (The 16-byte forms also split a load into Raw ldraw(p) and unpack(Raw): a kernel that wants several rows' loads in flight issues
// the raw loads back to back and unpacks behind them.)
template <> struct Stream<float, 4> {
    typedef float4 Raw;
    static __device__ __forceinline__ Raw ldraw(const float* p) { return *reinterpret_cast<const float4*>(p); }
    static __device__ __forceinline__ FV<4> unpack(const Raw q) { return {{q.x, q.y, q.z, q.w}}; }
    static __device__ __forceinline__ FV<4> ld(const float* p) { return unpack(ldraw(p)); }
    static __device__ __forceinline__ void st(float* p, const FV<4>& o) { *reinterpret_cast<float4*>(p) = make_float4(o.v[0], o.v[1], o.v[2], o.v[3]); }
};
template <> struct Stream<float, 8> {
    static __device__ __forceinline__ F8 ld(const float* p) { return ldf8(p); }
};
template <> struct Stream<u16, 1> {
    static __device__ __forceinline__ FV<1> ld(const u16* p) { return {{bf2f(*p)}}; }
    static __device__ __forceinline__ void st(u16* p, const FV<1>& o) { *p = f2bf(o.v[0]); }
};
template <> struct Stream<u16, 8> {
    typedef uint4 Raw;
    static __device__ __forceinline__ Raw ldraw(const u16* p) { return *reinterpret_cast<const uint4*>(p); }
    static __device__ __forceinline__ F8 unpack(const Raw q) { return unpack8(q); }
    static __device__ __forceinline__ F8 ld(const u16* p) { return ld8(p); }
    static __device__ __forceinline__ void st(u16* p, const F8& o) { st8(p, o); }
};

}  // namespace glf

// argument checks of the 16-bit entry points (16-byte accesses of eight bf16)
#define REQ_C8(c) GLF_REQUIRE((c) > 0 && ((c) % 8) == 0, GLF_ERR_BAD_SHAPE, "channel count must be a positive multiple of 8 (got %d)", (c))
#define REQ_AL(p, name) GLF_REQUIRE(::glf::al16(p), GLF_ERR_BAD_SHAPE, name " must be 16-byte aligned")
#define REQ_LD8(ld, name) GLF_REQUIRE(((ld) % 8) == 0, GLF_ERR_BAD_SHAPE, name " must be a multiple of 8")

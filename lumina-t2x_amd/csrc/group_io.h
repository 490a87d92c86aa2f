// Groups of G = 1 / 2 / 4 consecutive state elements (bf16 or fp32) as ONE 2- .. 16-byte access each way, held as fp32 in registers: what the
// elementwise kernels around a model evaluation (tiled.hip, compose.hip) load and store.  The caller picks G so that the element index is a
// multiple of G and the buffer is aligned to G elements.
#pragma once
#include "common.h"

template <int BYTES> struct Unit;
template <> struct Unit<2> { using type = u16; };
template <> struct Unit<4> { using type = unsigned; };
template <> struct Unit<8> { using type = uint2; };
template <> struct Unit<16> { using type = uint4; };

template <bool BF, int G>
__device__ __forceinline__ void ldg(const void* p, long long i, float v[G]) {  // i % G == 0
    if constexpr (BF) {
        const typename Unit<2 * G>::type r = *(const typename Unit<2 * G>::type*)((const u16*)p + i);
        if constexpr (G == 1) v[0] = bf2f(r);
        else if constexpr (G == 2) { v[0] = __uint_as_float(r << 16); v[1] = __uint_as_float(r & 0xffff0000u); }
        else {
            v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xffff0000u);
            v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xffff0000u);
        }
    } else {
        const float* q = (const float*)p + i;
        if constexpr (G == 1) v[0] = q[0];
        else if constexpr (G == 2) { const float2 r = *(const float2*)q; v[0] = r.x; v[1] = r.y; }
        else { const float4 r = *(const float4*)q; v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w; }
    }
}
template <bool BF, int G>
__device__ __forceinline__ void stg(void* p, long long i, const float v[G]) {  // i % G == 0
    if constexpr (BF) {
        u16* q = (u16*)p + i;
        if constexpr (G == 1) q[0] = f2bf(v[0]);
        else if constexpr (G == 2) *(unsigned*)q = pack2bf(v[0], v[1]);
        else { uint2 r; r.x = pack2bf(v[0], v[1]); r.y = pack2bf(v[2], v[3]); *(uint2*)q = r; }
    } else {
        float* q = (float*)p + i;
        if constexpr (G == 1) q[0] = v[0];
        else if constexpr (G == 2) *(float2*)q = make_float2(v[0], v[1]);
        else *(float4*)q = make_float4(v[0], v[1], v[2], v[3]);
    }
}

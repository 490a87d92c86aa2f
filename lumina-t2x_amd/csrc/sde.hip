// SDE sampling (transport/integrators.py: class sde, transport.py: _sde_terms / _last_step) around the model evaluations of lt_sample_sde:
// fused elementwise kernels, ONE model output v per stage.  The reference forms sde_drift = drift + D * score with two model calls on the same
// (x, t); the engine is deterministic, so both calls return the same v and the chain below reads it twice instead.
//
// Every row of the batch carries the same t, so every time-dependent coefficient is a per-stage scalar.  A stage's record is 8 floats
// (LT_SDE_REC in lumina_dit.h): t, r, var, D, q, dt, sqrt_dt, hdt for a loop stage; t, r, var, D, h, a, c, 0 for the last step.  The caller
// computes them with the path plan's own torch expressions (transport/integrators.py: sde_table), so their rounding is torch's.
//
// Rounding points at a bf16 state (R = round to bf16, identity at fp32), read off the tensor expressions of integrators.py and path.py run on
// tensors of the state dtype; r, var, D, q are [B,1,1,1] tensors of the state dtype there, dt / sqrt_dt / hdt = 0.5 dt are 0-dim CPU fp32 tensors,
// which PyTorch multiplies with a bf16 device tensor in fp32 (the scalar is NOT cast to bf16 first):
//   drift(x, v; r, var, D) = R(v + R(D * s)),  s = R(R(R(r * v) - x) / var)                    (get_score_from_velocity, sde_drift)
//   Euler-Maruyama:  x' = R(R(x + R(drift * dt)) + R(q * R(w * sqrt_dt)))                     (q = sqrt(2 D) as a state-dtype tensor)
//   Heun:            xhat = R(x + R(q * R(w * sqrt_dt)))
//                    K1 = drift(xhat, v1),  xp = R(xhat + R(dt * K1))
//                    x' = R(xhat + R(hdt * R(K1 + K2))),  K2 = drift(xp, v2) with the coefficients of the stage at t + dt
// The last step (transport.py: _last_step) runs at an fp32 [B] time vector, so its coefficient tensors are fp32 and type promotion makes Mean and
// Tweedie fp32 expressions with an fp32 result whatever the state dtype:
//   Mean:     out = x + (v + D * ((r * v - x) / var)) * h                                      (fp32 throughout, fp32 out)
//   Tweedie:  out = R(x / a) + c * ((r * v - x) / var),  a = alpha rounded to the state dtype, c = sigma^2 / alpha in fp32   (fp32 out)
//   Euler:    out = R(x + R(v * h))                                                            (state dtype out)
// Every product, sum and quotient rounds on its own: no contraction, IEEE division.
#include <algorithm>
#include <cstring>

#include "../../include/lumina_dit.h"
#include "common.h"
#include "kernels.h"

namespace {

struct SdeRec { float t, r, var, D, q, dt, sqrt_dt, hdt; };

// W consecutive elements per thread: 8 (bf16) or 4 (fp32) = one 16-byte access; W == 1 serves unaligned buffers and the tail
template <bool BF, int W>
__device__ __forceinline__ void ldv(const void* p, long long i, float* v) {
    if constexpr (W == 1) {
        v[0] = BF ? bf2f(((const u16*)p)[i]) : ((const float*)p)[i];
    } else if constexpr (BF) {
        const u32x4 r = *(const u32x4*)((const u16*)p + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[2 * j] = __uint_as_float(r[j] << 16); v[2 * j + 1] = __uint_as_float(r[j] & 0xffff0000u); }
    } else {
        const f32x4 r = *(const f32x4*)((const float*)p + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = r[j];
    }
}
template <bool BF, int W>
__device__ __forceinline__ void stv(void* p, long long i, const float* v) {
    if constexpr (W == 1) {
        if (BF) ((u16*)p)[i] = f2bf(v[0]); else ((float*)p)[i] = v[0];
    } else if constexpr (BF) {
        u32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = pack2bf(v[2 * j], v[2 * j + 1]);
        *(u32x4*)((u16*)p + i) = r;
    } else {
        *(f32x4*)((float*)p + i) = f32x4{v[0], v[1], v[2], v[3]};
    }
}
// fp32 result of a kernel whose state is bf16 (W == 8: two 16-byte stores) or fp32
template <int W>
__device__ __forceinline__ void stf(float* p, long long i, const float* v) {
    if constexpr (W == 1) {
        p[i] = v[0];
    } else {
#pragma unroll
        for (int j = 0; j < W; j += 4) *(f32x4*)(p + i + j) = f32x4{v[j], v[j + 1], v[j + 2], v[j + 3]};
    }
}

template <bool BF>
__device__ __forceinline__ float R(float f) { return BF ? bfr(f) : f; }

template <bool BF>
__device__ __forceinline__ float sde_drift(float x, float v, const SdeRec& c) {
#pragma clang fp contract(off)
    const float rv = R<BF>(c.r * v);
    const float num = R<BF>(rv - x);
    const float s = R<BF>(num / c.var);
    const float ds = R<BF>(c.D * s);
    return R<BF>(v + ds);
}
template <bool BF>
__device__ __forceinline__ float sde_kick(float w, const SdeRec& c) {  // R(q * R(w * sqrt_dt))
#pragma clang fp contract(off)
    const float dw = R<BF>(w * c.sqrt_dt);
    return R<BF>(c.q * dw);
}

// one element of op `OP` (LT_SDE_OP_*); o2 is the second output of HEUN_K1 (K1 itself)
template <bool BF, int OP>
__device__ __forceinline__ float sde_elem(float x, float v, float w, float k1, float xp, const SdeRec& c, float& o2) {
#pragma clang fp contract(off)
    if constexpr (OP == LT_SDE_OP_EULER) {
        const float d = sde_drift<BF>(x, v, c);
        const float step = R<BF>(d * c.dt);
        const float mean = R<BF>(x + step);
        return R<BF>(mean + sde_kick<BF>(w, c));
    } else if constexpr (OP == LT_SDE_OP_HEUN_XHAT) {
        return R<BF>(x + sde_kick<BF>(w, c));
    } else if constexpr (OP == LT_SDE_OP_HEUN_K1) {
        o2 = sde_drift<BF>(x, v, c);
        const float step = R<BF>(c.dt * o2);
        return R<BF>(x + step);
    } else if constexpr (OP == LT_SDE_OP_HEUN_OUT) {
        const float k2 = sde_drift<BF>(xp, v, c);
        const float ks = R<BF>(k1 + k2);
        const float step = R<BF>(c.hdt * ks);
        return R<BF>(x + step);
    } else if constexpr (OP == LT_SDE_OP_LAST_MEAN) {  // record: t, r, var, D, h
        const float s = (c.r * v - x) / c.var;
        const float d = v + c.D * s;
        return x + d * c.q;
    } else if constexpr (OP == LT_SDE_OP_LAST_TWEEDIE) {  // record: t, r, var, D, h, a, c
        const float s = (c.r * v - x) / c.var;
        const float xa = R<BF>(x / c.dt);
        return xa + c.sqrt_dt * s;
    } else {  // LT_SDE_OP_LAST_EULER
        const float step = R<BF>(v * c.q);
        return R<BF>(x + step);
    }
}

template <int OP> struct OpTraits {
    static constexpr bool uses_v = OP != LT_SDE_OP_HEUN_XHAT;
    static constexpr bool uses_w = OP == LT_SDE_OP_EULER || OP == LT_SDE_OP_HEUN_XHAT;
    static constexpr bool uses_k = OP == LT_SDE_OP_HEUN_OUT;                                   // K1 and xp
    static constexpr bool two_out = OP == LT_SDE_OP_HEUN_K1;
    static constexpr bool f32_out = OP == LT_SDE_OP_LAST_MEAN || OP == LT_SDE_OP_LAST_TWEEDIE;
};

template <bool BF, int OP, int W>
__device__ __forceinline__ void sde_group(const void* x, const void* v, const void* w, const void* k1, const void* xp, void* out, void* out2,
                                          const SdeRec& c, long long i) {
    using T = OpTraits<OP>;
    float xv[W], vv[W], wv[W], kv[W], pv[W], ov[W], o2v[W];
    ldv<BF, W>(x, i, xv);
    if constexpr (T::uses_v) ldv<BF, W>(v, i, vv);
    if constexpr (T::uses_w) ldv<BF, W>(w, i, wv);
    if constexpr (T::uses_k) { ldv<BF, W>(k1, i, kv); ldv<BF, W>(xp, i, pv); }
#pragma unroll
    for (int j = 0; j < W; ++j) {
        o2v[j] = 0.f;
        ov[j] = sde_elem<BF, OP>(xv[j], T::uses_v ? vv[j] : 0.f, T::uses_w ? wv[j] : 0.f, T::uses_k ? kv[j] : 0.f, T::uses_k ? pv[j] : 0.f, c,
                                 o2v[j]);
    }
    if constexpr (T::f32_out) stf<W>((float*)out, i, ov);
    else stv<BF, W>(out, i, ov);
    if constexpr (T::two_out) stv<BF, W>(out2, i, o2v);
}

// grid-stride over groups of W elements; the n % W elements behind the last whole group are taken one by one by the first threads
template <bool BF, int OP, int W>
__global__ void __launch_bounds__(256) sde_kernel(const void* __restrict__ x, const void* __restrict__ v, const void* __restrict__ w,
                                                  const void* __restrict__ k1, const void* __restrict__ xp, void* __restrict__ out,
                                                  void* __restrict__ out2, SdeRec c, long long n) {
    const long long groups = n / W;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long long g = tid; g < groups; g += stride) sde_group<BF, OP, W>(x, v, w, k1, xp, out, out2, c, g * W);
    if constexpr (W > 1) {
        const long long i = groups * W + tid;
        if (i < n) sde_group<BF, OP, 1>(x, v, w, k1, xp, out, out2, c, i);
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <bool BF, int OP>
int launch_op(const void* x, const void* v, const void* w, const void* k1, const void* xp, void* out, void* out2, const SdeRec& c, long long n,
              hipStream_t s) {
    constexpr int W = BF ? 8 : 4;
    const bool vec = aligned16(x) && aligned16(v) && aligned16(w) && aligned16(k1) && aligned16(xp) && aligned16(out) && aligned16(out2);
    const long long groups = vec ? (n + W - 1) / W : n;  // (>= n % W threads exist: one block at least)
    const long long cap = (long long)num_cus() * 8;
    const int blocks = (int)std::max<long long>(1, std::min<long long>((groups + 255) / 256, cap));
    if (vec) hipLaunchKernelGGL((sde_kernel<BF, OP, W>), dim3(blocks), dim3(256), 0, s, x, v, w, k1, xp, out, out2, c, n);
    else hipLaunchKernelGGL((sde_kernel<BF, OP, 1>), dim3(blocks), dim3(256), 0, s, x, v, w, k1, xp, out, out2, c, n);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

template <bool BF>
int launch_dtype(int op, const void* x, const void* v, const void* w, const void* k1, const void* xp, void* out, void* out2, const SdeRec& c,
                 long long n, hipStream_t s) {
    switch (op) {
        case LT_SDE_OP_EULER: return launch_op<BF, LT_SDE_OP_EULER>(x, v, w, k1, xp, out, out2, c, n, s);
        case LT_SDE_OP_HEUN_XHAT: return launch_op<BF, LT_SDE_OP_HEUN_XHAT>(x, v, w, k1, xp, out, out2, c, n, s);
        case LT_SDE_OP_HEUN_K1: return launch_op<BF, LT_SDE_OP_HEUN_K1>(x, v, w, k1, xp, out, out2, c, n, s);
        case LT_SDE_OP_HEUN_OUT: return launch_op<BF, LT_SDE_OP_HEUN_OUT>(x, v, w, k1, xp, out, out2, c, n, s);
        case LT_SDE_OP_LAST_MEAN: return launch_op<BF, LT_SDE_OP_LAST_MEAN>(x, v, w, k1, xp, out, out2, c, n, s);
        case LT_SDE_OP_LAST_TWEEDIE: return launch_op<BF, LT_SDE_OP_LAST_TWEEDIE>(x, v, w, k1, xp, out, out2, c, n, s);
        default: return launch_op<BF, LT_SDE_OP_LAST_EULER>(x, v, w, k1, xp, out, out2, c, n, s);
    }
}

}  // namespace

int launch_sde_step(int op, const void* x, const void* v, const void* w, const void* k1, const void* xp, void* out, void* out2, const float* rec,
                    long long n, int dtype, hipStream_t stream) {
    LT_REQUIRE(op >= LT_SDE_OP_EULER && op <= LT_SDE_OP_LAST_EULER, "sde_step: unknown op %d", op);
    LT_REQUIRE(dtype == 0 || dtype == 1, "sde_step: state dtype must be f32 or bf16");
    LT_REQUIRE(rec && x && out && n >= 1, "sde_step: null argument");
    const bool uses_v = op != LT_SDE_OP_HEUN_XHAT, uses_w = op == LT_SDE_OP_EULER || op == LT_SDE_OP_HEUN_XHAT;
    LT_REQUIRE((!uses_v || v) && (!uses_w || w) && (op != LT_SDE_OP_HEUN_OUT || (k1 && xp)) && (op != LT_SDE_OP_HEUN_K1 || out2),
               "sde_step: null argument (an operand of op %d is missing)", op);
    SdeRec c;
    memcpy(&c, rec, sizeof(c));
    // pointers an op does not read are not passed on (they would only take part in the alignment test)
    if (!uses_v) v = nullptr;
    if (!uses_w) w = nullptr;
    if (op != LT_SDE_OP_HEUN_OUT) { k1 = nullptr; xp = nullptr; }
    if (op != LT_SDE_OP_HEUN_K1) out2 = nullptr;
    return dtype == 1 ? launch_dtype<true>(op, x, v, w, k1, xp, out, out2, c, n, stream)
                      : launch_dtype<false>(op, x, v, w, k1, xp, out, out2, c, n, stream);
}

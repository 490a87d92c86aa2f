// Linear multistep ODE stepping (transport/multistep.py): the Adams-Bashforth predictor and the Adams-Moulton corrector that costs no
// model evaluation, around the evaluations of lt_sample_ode_multistep.  One launch per grid interval forms, in the same thread,
//   y = R(y_prev + S(a, k))        the corrected state (has_corr), the sum over the newest slopes k_0 (newest) .. k_3
//   p = R(y + S(b, k))             the next predictor, from the STORED y (has_corr = 0: y = y_prev, and p is the one output)
//   S(c, k): acc = R(c_0 k_0); acc = R(acc + R(c_j k_j)) for 1 <= j < used(c)
// R = round to the state dtype (identity at fp32): the tensor expression `inc = k[0] * c0; inc = inc + k[j] * cj; y = y + inc` with Python-float
// weights, which enter torch's op-math as fp32.  used(c) = the entries of c up to the last one that is not 0 - the rule the weight table is
// read by on both sides; the weights themselves come from the caller (transport/multistep.py: multistep_table), nothing is computed here.
// Every product and sum rounds on its own: no contraction.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "kernels.h"

namespace {

struct MsCoef { float a[4], b[4]; int na, nb; };
struct MsSlopes { const void* k[4]; };

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

template <bool BF>
__device__ __forceinline__ float R(float f) { return BF ? bfr(f) : f; }

// y + S(c, k) over the first nc slopes (nc >= 1)
template <bool BF>
__device__ __forceinline__ float weight_sum(float y, const float* k, const float* c, int nc) {
#pragma clang fp contract(off)
    float acc = R<BF>(c[0] * k[0]);
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (j < nc) {
            const float term = R<BF>(c[j] * k[j]);
            acc = R<BF>(acc + term);
        }
    return R<BF>(y + acc);
}

template <bool BF, int W>
__device__ __forceinline__ void ms_group(const void* y_prev, const MsSlopes& ks, int nslopes, const MsCoef& c, void* y_out, void* p_out, long long i) {
    float yv[W], kv[4][W], yo[W], po[W];
    ldv<BF, W>(y_prev, i, yv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < nslopes) {
            ldv<BF, W>(ks.k[j], i, kv[j]);
        } else {
#pragma unroll
            for (int l = 0; l < W; ++l) kv[j][l] = 0.f;
        }
    }
#pragma unroll
    for (int l = 0; l < W; ++l) {
        const float k[4] = {kv[0][l], kv[1][l], kv[2][l], kv[3][l]};
        const float y = c.na > 0 ? weight_sum<BF>(yv[l], k, c.a, c.na) : yv[l];
        yo[l] = y;
        po[l] = c.nb > 0 ? weight_sum<BF>(y, k, c.b, c.nb) : y;
    }
    if (y_out) stv<BF, W>(y_out, i, yo);
    stv<BF, W>(p_out, i, po);
}

// grid-stride over groups of W elements; the n % W elements behind the last whole group are taken one by one by the first threads
template <bool BF, int W>
__global__ void __launch_bounds__(256) ode_multistep_kernel(const void* __restrict__ y_prev, MsSlopes ks, int nslopes, MsCoef c,
                                                            void* __restrict__ y_out, void* __restrict__ p_out, long long n) {
    const long long groups = n / W;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long long g = tid; g < groups; g += stride) ms_group<BF, W>(y_prev, ks, nslopes, c, y_out, p_out, g * W);
    if constexpr (W > 1) {
        const long long i = groups * W + tid;
        if (i < n) ms_group<BF, 1>(y_prev, ks, nslopes, c, y_out, p_out, i);
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <bool BF>
int launch_dtype(const void* y_prev, const MsSlopes& ks, int nslopes, const MsCoef& c, void* y_out, void* p_out, long long n, hipStream_t s) {
    constexpr int W = BF ? 8 : 4;
    bool vec = aligned16(y_prev) && aligned16(y_out) && aligned16(p_out);
    for (int j = 0; j < nslopes; ++j) vec = vec && aligned16(ks.k[j]);
    const long long groups = vec ? (n + W - 1) / W : n;  // (>= n % W threads exist: one block at least)
    const long long cap = (long long)num_cus() * 8;
    const int blocks = (int)std::max<long long>(1, std::min<long long>((groups + 255) / 256, cap));
    if (vec) hipLaunchKernelGGL((ode_multistep_kernel<BF, W>), dim3(blocks), dim3(256), 0, s, y_prev, ks, nslopes, c, y_out, p_out, n);
    else hipLaunchKernelGGL((ode_multistep_kernel<BF, 1>), dim3(blocks), dim3(256), 0, s, y_prev, ks, nslopes, c, y_out, p_out, n);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace

int multistep_used(const float* c) {
    int n = 0;
    for (int j = 0; j < 4; ++j)
        if (c[j] != 0.f) n = j + 1;
    return n;
}

int launch_ode_multistep(const void* y_prev, const void* const* k, int nslopes, const float* a, const float* b, int has_corr, void* y_out,
                         void* p_out, long long n, int dtype, hipStream_t stream) {
    LT_REQUIRE(dtype == 0 || dtype == 1, "ode_multistep: state dtype must be f32 or bf16");
    LT_REQUIRE(has_corr == 0 || has_corr == 1, "ode_multistep: has_corr %d is not 0 or 1", has_corr);
    LT_REQUIRE(y_prev && k && b && p_out && n >= 1, "ode_multistep: null argument");
    LT_REQUIRE(!has_corr || (a && y_out), "ode_multistep: null argument (the corrector needs its weights and y_out)");
    LT_REQUIRE(nslopes >= 1 && nslopes <= 4, "ode_multistep: nslopes %d outside 1..4", nslopes);
    MsCoef c{};
    MsSlopes ks{};
    for (int j = 0; j < 4; ++j) {
        c.a[j] = has_corr ? a[j] : 0.f;
        c.b[j] = b[j];
        LT_REQUIRE(std::isfinite(c.a[j]) && std::isfinite(c.b[j]), "ode_multistep: weight %d is not finite", j);
    }
    c.na = multistep_used(c.a);
    c.nb = multistep_used(c.b);
    LT_REQUIRE(c.na <= nslopes && c.nb <= nslopes, "ode_multistep: the weights name %d slopes, %d are given", std::max(c.na, c.nb), nslopes);
    for (int j = 0; j < nslopes; ++j) {
        LT_REQUIRE(k[j], "ode_multistep: slope %d of %d is null", j, nslopes);
        ks.k[j] = k[j];
    }
    if (!has_corr) y_out = nullptr;  // one output
    return dtype == 1 ? launch_dtype<true>(y_prev, ks, nslopes, c, y_out, p_out, n, stream)
                      : launch_dtype<false>(y_prev, ks, nslopes, c, y_out, p_out, n, stream);
}

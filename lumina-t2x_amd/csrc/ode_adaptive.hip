// Adaptive Runge-Kutta stepping (transport/integrators.py: adaptive_odeint - torchdiffeq's dopri5 / bosh3 / fehlberg2 / adaptive_heun) around
// the model evaluations of lt_sample_ode_adaptive: the stage arithmetic, the error estimate with its tolerance and norm, the dense-output
// coefficients and the interpolation as fused elementwise kernels.  The tableau is DATA (a coefficient row and the slope pointers it runs
// over): one code path serves every method.
//
// Rounding points (R = round to the state dtype, identity at fp32), read off the host loop's tensor expressions.  A Python float times a
// tensor is an fp32 product rounded once (the scalar becomes fp32, not bf16); dty = R(dt) is a 0-dim device tensor of the state dtype, so
// dty * tensor multiplies two state-dtype values; an integer factor is an fp32 scalar like a float:
//   chain(c)  = R(R(k0 c0) + R(kj cj)) ... in index order, terms with cj == 0 skipped for j >= 1 (k0 c0 is always formed)
//   stage     yi = R(y + R(dty chain(beta_i)))               also y1 of a non-FSAL tableau (c_sol), y_mid (c_mid) and, with the one
//                                                            coefficient 1.0, y0 + h0 f0 of the initial-step heuristic
//   error     err = R(dty chain(c_err)),  tol = R(atol + R(rtol max(|y|, |y1|))),  q = R(err / tol)
//   heuristic scale = R(atol + R(|y0| rtol)),  q = R(x / scale)  or  R(R(f1 - f0) / scale)
//   dense     c1 = R(dty fy)
//             a  = R(R(R(R(2 dty) R(f1 - fy)) - R(8 R(y1 + y))) + R(16 ymid))
//             b  = R(R(R(R(dty R(R(5 fy) - R(3 f1))) + R(18 y)) + R(14 y1)) - R(32 ymid))
//             c  = R(R(R(R(dty R(f1 - R(4 fy))) - R(11 y)) - R(5 y1)) + R(16 ymid))
//   interp    total = R(R(R(R(y + R(x c1)) + R(x2 c)) + R(x3 b)) + R(x4 a)),  x = R(x), x2 = R(x x), x3 = R(x2 x), x4 = R(x3 x) (0-dim tensors
//             of the state dtype: formed on the host)
//   norm      sqrt(mean(q^2)): q^2 exactly (float64 product of fp32 values), float64 sums in a fixed two-level tree - every thread over its
//             elements in index order, a workgroup over its 256 threads by halving, a second launch over the workgroups' partial sums the same
//             way - then ONE rounding to fp32.  No atomics: the same words on every run, and the launch geometry depends on n alone.
// Every product, sum and quotient rounds on its own: no contraction, IEEE division.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/lumina_dit.h"
#include "common.h"
#include "kernels.h"

namespace {

enum { RK_STAGE, RK_DENSE, RK_INTERP, RK_ERR, RK_SCALED, RK_DIFF, RK_PLAIN };
constexpr int RK_MAX_BLOCKS = LT_RK_WS_BYTES / 8;  // one float64 partial sum per workgroup

struct RkArgs {
    const void* k[LT_RK_MAX_SLOPES];  // the slopes a chain runs over (INTERP: the five coefficients; SCALED / DIFF / PLAIN: the operands)
    const void *y, *y1, *ymid;
    void* out[4];                     // STAGE / INTERP: out[0]; DENSE: c1, c, b, a; norms: q (may be null)
    float c[LT_RK_MAX_SLOPES];
    int nk;
    float dty, rtol, atol;
    float x[4];
    double* part;
    long long n;
};

// W consecutive elements: one 16-byte access (VEC: 8 bf16 or 4 fp32), or element by element (unaligned buffers; W == 1 is the tail)
template <bool BF, int W, bool VEC>
__device__ __forceinline__ void ld(const void* p, long long i, float* v) {
    if constexpr (VEC && W > 1 && BF) {
        const u32x4 r = *(const u32x4*)((const u16*)p + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[2 * j] = __uint_as_float(r[j] << 16); v[2 * j + 1] = __uint_as_float(r[j] & 0xffff0000u); }
    } else if constexpr (VEC && W > 1) {
        const f32x4 r = *(const f32x4*)((const float*)p + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = r[j];
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] = BF ? bf2f(((const u16*)p)[i + j]) : ((const float*)p)[i + j];
    }
}
template <bool BF, int W, bool VEC>
__device__ __forceinline__ void st(void* p, long long i, const float* v) {
    if constexpr (VEC && W > 1 && BF) {
        u32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = pack2bf(v[2 * j], v[2 * j + 1]);
        *(u32x4*)((u16*)p + i) = r;
    } else if constexpr (VEC && W > 1) {
        *(f32x4*)((float*)p + i) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            if (BF) ((u16*)p)[i + j] = f2bf(v[j]); else ((float*)p)[i + j] = v[j];
        }
    }
}

template <bool BF>
__device__ __forceinline__ float R(float f) { return BF ? bfr(f) : f; }

// chain(c) over the slopes: the loop is unrolled, so every pointer and coefficient is a kernel argument at a fixed place (no scratch)
template <bool BF, int W, bool VEC>
__device__ __forceinline__ void chain(const RkArgs& a, long long i, float* acc) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < LT_RK_MAX_SLOPES; ++j) {
        if (j < a.nk && (j == 0 || a.c[j] != 0.f)) {
            float kv[W];
            ld<BF, W, VEC>(a.k[j], i, kv);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const float term = R<BF>(kv[w] * a.c[j]);
                acc[w] = j == 0 ? term : R<BF>(acc[w] + term);
            }
        }
    }
}

template <bool BF>
__device__ __forceinline__ float rk_scale(float y0, float rtol, float atol) {
#pragma clang fp contract(off)
    const float yr = R<BF>(fabsf(y0) * rtol);
    return R<BF>(atol + yr);
}

// W elements at i of op `OP`; the norm ops add their q^2 to sum
template <bool BF, int OP, int W, bool VEC>
__device__ __forceinline__ void rk_group(const RkArgs& a, long long i, double& sum) {
#pragma clang fp contract(off)
    const float dty = R<BF>(a.dty);
    float o[W];
    if constexpr (OP == RK_STAGE) {
        float acc[W], yv[W];
        chain<BF, W, VEC>(a, i, acc);
        ld<BF, W, VEC>(a.y, i, yv);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const float inc = R<BF>(dty * acc[w]);
            o[w] = R<BF>(yv[w] + inc);
        }
        st<BF, W, VEC>(a.out[0], i, o);
    } else if constexpr (OP == RK_DENSE) {
        float y[W], y1[W], ym[W], fy[W], f1[W], c1[W], c[W], b[W];
        ld<BF, W, VEC>(a.y, i, y);
        ld<BF, W, VEC>(a.y1, i, y1);
        ld<BF, W, VEC>(a.ymid, i, ym);
        ld<BF, W, VEC>(a.k[0], i, fy);
        ld<BF, W, VEC>(a.k[1], i, f1);
        const float dty2 = R<BF>(2.f * dty);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            c1[w] = R<BF>(dty * fy[w]);
            const float df = R<BF>(f1[w] - fy[w]);
            const float a1 = R<BF>(dty2 * df);
            const float ys = R<BF>(y1[w] + y[w]);
            const float a2 = R<BF>(8.f * ys);
            const float a3 = R<BF>(a1 - a2);
            const float m16 = R<BF>(16.f * ym[w]);
            o[w] = R<BF>(a3 + m16);
            const float f5 = R<BF>(5.f * fy[w]);
            const float f3 = R<BF>(3.f * f1[w]);
            const float b0 = R<BF>(f5 - f3);
            const float b1 = R<BF>(dty * b0);
            const float y18 = R<BF>(18.f * y[w]);
            const float b2 = R<BF>(b1 + y18);
            const float y14 = R<BF>(14.f * y1[w]);
            const float b3 = R<BF>(b2 + y14);
            const float m32 = R<BF>(32.f * ym[w]);
            b[w] = R<BF>(b3 - m32);
            const float f4 = R<BF>(4.f * fy[w]);
            const float c0 = R<BF>(f1[w] - f4);
            const float cc1 = R<BF>(dty * c0);
            const float y11 = R<BF>(11.f * y[w]);
            const float c2 = R<BF>(cc1 - y11);
            const float y5 = R<BF>(5.f * y1[w]);
            const float c3 = R<BF>(c2 - y5);
            c[w] = R<BF>(c3 + m16);
        }
        st<BF, W, VEC>(a.out[0], i, c1);
        st<BF, W, VEC>(a.out[1], i, c);
        st<BF, W, VEC>(a.out[2], i, b);
        st<BF, W, VEC>(a.out[3], i, o);
    } else if constexpr (OP == RK_INTERP) {
        float cf[W];
        ld<BF, W, VEC>(a.k[0], i, o);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ld<BF, W, VEC>(a.k[j + 1], i, cf);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const float term = R<BF>(a.x[j] * cf[w]);
                o[w] = R<BF>(o[w] + term);
            }
        }
        st<BF, W, VEC>(a.out[0], i, o);
    } else {
        if constexpr (OP == RK_ERR) {
            float acc[W], y[W], y1[W];
            chain<BF, W, VEC>(a, i, acc);
            ld<BF, W, VEC>(a.y, i, y);
            ld<BF, W, VEC>(a.y1, i, y1);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const float err = R<BF>(dty * acc[w]);
                const float m = fmaxf(fabsf(y[w]), fabsf(y1[w]));
                const float rm = R<BF>(a.rtol * m);
                const float tol = R<BF>(a.atol + rm);
                o[w] = R<BF>(err / tol);
            }
        } else if constexpr (OP == RK_PLAIN) {
            ld<BF, W, VEC>(a.k[0], i, o);
        } else {
            float x[W], y0[W];
            ld<BF, W, VEC>(a.k[0], i, x);
            ld<BF, W, VEC>(a.y, i, y0);
            if constexpr (OP == RK_DIFF) {
                float f0[W];
                ld<BF, W, VEC>(a.k[1], i, f0);
#pragma unroll
                for (int w = 0; w < W; ++w) x[w] = R<BF>(x[w] - f0[w]);
            }
#pragma unroll
            for (int w = 0; w < W; ++w) o[w] = R<BF>(x[w] / rk_scale<BF>(y0[w], a.rtol, a.atol));
        }
        if (a.out[0]) st<BF, W, VEC>(a.out[0], i, o);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const double q = (double)o[w];
            sum += q * q;
        }
    }
}

// 256 float64 values -> their sum in sh[0], by halving: the same tree whatever the values
__device__ __forceinline__ void block_tree_sum(double* sh, double v) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
}

// grid-stride over groups of W elements; the n % W elements behind the last whole group are taken one by one by the first threads
template <bool BF, int OP, bool VEC>
__global__ void __launch_bounds__(256) rk_kernel(RkArgs a) {
    constexpr int W = BF ? 8 : 4;
    constexpr bool norm = OP >= RK_ERR;
    const long long groups = a.n / W;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    double sum = 0.0;
    for (long long g = tid; g < groups; g += stride) rk_group<BF, OP, W, VEC>(a, g * W, sum);
    const long long i = groups * W + tid;
    if (i < a.n) rk_group<BF, OP, 1, false>(a, i, sum);
    if constexpr (norm) {
        __shared__ double sh[256];
        block_tree_sum(sh, sum);
        if (threadIdx.x == 0) a.part[blockIdx.x] = sh[0];
    }
}

// the second level: one workgroup over the partial sums, then sqrt(sum / n) rounded once to fp32
__global__ void __launch_bounds__(256) rk_norm_finish(const double* __restrict__ part, int nparts, long long n, float* __restrict__ out) {
    __shared__ double sh[256];
    double v = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) v += part[i];
    block_tree_sum(sh, v);
    if (threadIdx.x == 0) *out = (float)sqrt(sh[0] / (double)n);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int rk_blocks(long long n, int W) {
    const long long groups = (n + W - 1) / W;  // (>= n % W threads exist: one block at least)
    return (int)std::max<long long>(1, std::min<long long>((groups + 255) / 256, RK_MAX_BLOCKS));
}

template <bool BF, int OP>
int launch_op(const RkArgs& a, float* norm_out, hipStream_t s) {
    bool vec = aligned16(a.y) && aligned16(a.y1) && aligned16(a.ymid);
    for (int j = 0; j < LT_RK_MAX_SLOPES; ++j) vec = vec && aligned16(a.k[j]);
    for (int j = 0; j < 4; ++j) vec = vec && aligned16(a.out[j]);
    const int blocks = rk_blocks(a.n, BF ? 8 : 4);
    if (vec) hipLaunchKernelGGL((rk_kernel<BF, OP, true>), dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((rk_kernel<BF, OP, false>), dim3(blocks), dim3(256), 0, s, a);
    LT_CHECK_HIP(hipGetLastError());
    if (OP >= RK_ERR) {
        hipLaunchKernelGGL(rk_norm_finish, dim3(1), dim3(256), 0, s, (const double*)a.part, blocks, a.n, norm_out);
        LT_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

template <int OP>
int launch(const RkArgs& a, int dtype, float* norm_out, hipStream_t s) {
    LT_REQUIRE(dtype == 0 || dtype == 1, "rk: state dtype must be f32 or bf16");
    LT_REQUIRE(a.n >= 1, "rk: n must be at least 1");
    return dtype == 1 ? launch_op<true, OP>(a, norm_out, s) : launch_op<false, OP>(a, norm_out, s);
}

int set_chain(RkArgs& a, const void* const* k, const float* coef, int nk) {
    LT_REQUIRE(k && coef && nk >= 1 && nk <= LT_RK_MAX_SLOPES, "rk: a chain runs over 1..%d slopes, got %d", LT_RK_MAX_SLOPES, nk);
    for (int j = 0; j < nk; ++j) {
        LT_REQUIRE(k[j], "rk: null slope %d", j);
        a.k[j] = k[j];
        a.c[j] = coef[j];
    }
    a.nk = nk;
    return 0;
}

float round_to(int dtype, float f) {
    if (dtype != 1) return f;
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return f;
    u += 0x7fffu + ((u >> 16) & 1u);
    u &= 0xffff0000u;
    memcpy(&f, &u, 4);
    return f;
}

}  // namespace

int launch_rk_stage(const void* y, const void* const* k, const float* coef, int nk, float dt, void* out, long long n, int dtype,
                    hipStream_t stream) {
    LT_REQUIRE(y && out, "rk_stage: null argument");
    RkArgs a = {};
    if (set_chain(a, k, coef, nk)) return 2;
    a.y = y; a.out[0] = out; a.dty = dt; a.n = n;
    return launch<RK_STAGE>(a, dtype, nullptr, stream);
}

int launch_rk_error_norm(const void* y, const void* y1, const void* const* k, const float* c_err, int nk, float dt, float rtol, float atol,
                         void* q_out, void* ws, float* norm_out, long long n, int dtype, hipStream_t stream) {
    LT_REQUIRE(y && y1 && ws && norm_out, "rk_error_norm: null argument");
    RkArgs a = {};
    if (set_chain(a, k, c_err, nk)) return 2;
    a.y = y; a.y1 = y1; a.out[0] = q_out; a.dty = dt; a.rtol = rtol; a.atol = atol; a.part = (double*)ws; a.n = n;
    return launch<RK_ERR>(a, dtype, norm_out, stream);
}

int launch_rms_norm(const void* x, const void* sub, const void* y0, float rtol, float atol, void* q_out, void* ws, float* norm_out, long long n,
                    int dtype, hipStream_t stream) {
    LT_REQUIRE(x && ws && norm_out, "rms_norm: null argument");
    LT_REQUIRE(!sub || y0, "rms_norm: a difference is formed in front of the scaled quotient only (y0 missing)");
    RkArgs a = {};
    a.k[0] = x; a.k[1] = sub; a.y = y0; a.out[0] = q_out; a.rtol = rtol; a.atol = atol; a.part = (double*)ws; a.n = n;
    if (sub) return launch<RK_DIFF>(a, dtype, norm_out, stream);
    if (y0) return launch<RK_SCALED>(a, dtype, norm_out, stream);
    return launch<RK_PLAIN>(a, dtype, norm_out, stream);
}

int launch_rk_dense(const void* y, const void* y1, const void* ymid, const void* fy, const void* f1, float dt, void* c1, void* c, void* b, void* a4,
                    long long n, int dtype, hipStream_t stream) {
    LT_REQUIRE(y && y1 && ymid && fy && f1 && c1 && c && b && a4, "rk_dense: null argument");
    RkArgs a = {};
    a.y = y; a.y1 = y1; a.ymid = ymid; a.k[0] = fy; a.k[1] = f1; a.dty = dt; a.n = n;
    a.out[0] = c1; a.out[1] = c; a.out[2] = b; a.out[3] = a4;
    return launch<RK_DENSE>(a, dtype, nullptr, stream);
}

int launch_rk_interp(const void* const* coeffs, float x, void* out, long long n, int dtype, hipStream_t stream) {
    LT_REQUIRE(coeffs && out, "rk_interp: null argument");
    RkArgs a = {};
    for (int j = 0; j < 5; ++j) {
        LT_REQUIRE(coeffs[j], "rk_interp: null coefficient %d", j);
        a.k[j] = coeffs[j];
    }
    // x and its powers are 0-dim tensors of the state dtype in the host loop: xp = xp * x rounds every time
    a.x[0] = round_to(dtype, x);
    for (int j = 1; j < 4; ++j) a.x[j] = round_to(dtype, a.x[j - 1] * a.x[0]);
    a.out[0] = out; a.n = n;
    return launch<RK_INTERP>(a, dtype, nullptr, stream);
}

// Multi-view (visual-anagram) sampling: the three kernels around the model evaluations of lt_sample_views (visual_anagrams/generate.py:389-414).
//
// A view is DATA: a pixel permutation of the [C, H, W] latent with a sign per channel,
//   view_v(x)[c, i]         = vsign[v][c] * x[c, perm[v][i]]
//   inverse_view_v(n)[c, i] = isign[v][c] * n[c, iperm[v][i]]
// (vsign / isign are separate: the reference's NegateView negates every channel going in and channels 0..2 coming back,
//  views/view_negate.py:12-22).  Tables: perm / iperm int32 [V][HW], vsign / isign float [V][C], HW = H * W (a multiple of 4: H and W are
//  multiples of the patch size 2).
//
// Access pattern: every thread owns FOUR consecutive output pixels of one (view, channel) row - the index table is read as one int4 and the
// result leaves as one 8-byte (bf16) / 16-byte (fp32) store, so table reads and stores are whole lines; the gathered side is the
// uncoalesced one (four scalar loads; a rotation or flip walks a column / a reversed row, a random permutation scatters).  At the sizes in
// scope (V x C x HW <= a few hundred KB) the latent stays in L2 and the launches are latency-bound, not bandwidth-bound.
//
// Rounding points at a bf16 state (R = round to bf16; none at fp32), all read off generate.py:212-219, :402-414 run on bf16 tensors, where
// dt / half_dt are Python floats and PyTorch multiplies a bf16 tensor by such a scalar in fp32 (tests/golden/views_tiny.npz: dt_rounding):
//   gather, mode 1:  x_mid = R(x + R(f0 * half_dt)),  x = view_v(y)                (generate.py:216-217)
//   reduce:          n_v = inverse_view_v(-R(f * dt))                              (generate.py:219, :402, :407)
//                    y'  = R(y - R((n_0 + n_1 + ... + n_{V-1}) / V))               (generate.py:410-414; fp32 sum in view order, ONE division)
// Negation, sign and permutation are exact.
//
// Phase Upscale (generate.py:465-494, midpoint_solver_extra :222-262): the model input of a stage is a time-dependent blend of the state, the
// guidance latent G and the initial noise Z, formed in the UN-VIEWED frame and viewed per view - views_guided_gather_kernel, with p = perm[v][i]:
//   stage 0:  s = y[c,p]                                                           (y0, :241)
//   stage 1:  s = R(y[c,p] + isign[v][c] * R(f0[v][c,i] * half_dt))                (:247-250: y_mid = y0 - inverse_view_v(-f0 * half_dt), read at p:
//                                                                                   iperm[v][p] = i, so f0 is read where it is written; the two negations are exact)
//   g = R(R(ft * G[c,p]) + R(f1t * Z[c,p]))                                        (:240 / :256; the anchor is all ones, the division exact)
//   m = R(R(k1c * s) + R(kc * g))                                                  (:241 / :257)
//   out[v][c,i] = vsign[v][c] * m                                                  (:242 / :258)
// ft = fp32(t), f1t = fp32(1 - t), kc = c, k1c = 1 - c are DATA (the host computes them with the reference's own expressions and decides whether
// c is rounded to the state dtype first: lumina_dit.h).  Every product and sum is one fp32 operation.  The interval's closing update is views_reduce.
#include "common.h"
#include "kernels.h"

namespace {

template <bool BF>
__device__ __forceinline__ float ld1(const void* p, long long i) {
    return BF ? bf2f(((const u16*)p)[i]) : ((const float*)p)[i];
}
template <bool BF>
__device__ __forceinline__ void ld4(const void* p, long long i, float v[4]) {  // i % 4 == 0
    if (BF) {
        const uint2 r = *(const uint2*)((const u16*)p + i);
        v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xffff0000u);
        v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xffff0000u);
    } else {
        const float4 r = *(const float4*)((const float*)p + i);
        v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
    }
}
template <bool BF>
__device__ __forceinline__ void st4(void* p, long long i, const float v[4]) {  // i % 4 == 0
    if (BF) {
        uint2 r;
        r.x = (unsigned)f2bf(v[0]) | ((unsigned)f2bf(v[1]) << 16);
        r.y = (unsigned)f2bf(v[2]) | ((unsigned)f2bf(v[3]) << 16);
        *(uint2*)((u16*)p + i) = r;
    } else {
        *(float4*)((float*)p + i) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// lt_set_views only accepts tables that passed the bijection check; the operator entry points take the caller's word for it, so an index is
// clamped before it is used as an address (a bad table then gives wrong values, never an access outside the buffer)
__device__ __forceinline__ int inb(int p, int HW) { return min(max(p, 0), HW - 1); }

// iperm[v][perm[v][i]] = i, and the bijection check: hits[v][p] counts how often target p is named; hits[V * HW] (the last word) counts
// entries that are out of range or name a target a second time.  HW entries, all in range, none twice <=> a bijection on [0, HW).
// Out-of-range entries are never used as an address.
__global__ void views_invert_kernel(const int* __restrict__ perm, int* __restrict__ iperm, int* __restrict__ hits, int V, int HW) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)V * HW) return;
    const int v = (int)(t / HW), i = (int)(t % HW);
    const int p = perm[t];
    if (p < 0 || p >= HW) {
        atomicAdd(&hits[(long long)V * HW], 1);
        return;
    }
    if (atomicAdd(&hits[(long long)v * HW + p], 1) != 0) atomicAdd(&hits[(long long)V * HW], 1);
    iperm[(long long)v * HW + p] = i;
}

// out[v][c][i] = view_v(y)[c][i]  (f0 == nullptr)   or   R(view_v(y)[c][i] + R(f0[v][c][i] * half_dt))
template <bool BF>
__global__ void views_gather_kernel(const void* __restrict__ y, const int* __restrict__ perm, const float* __restrict__ vsign,
                                    const void* __restrict__ f0, void* __restrict__ out, float half_dt, int V, int C, int HW) {
#pragma clang fp contract(off)  // torch rounds f0 * half_dt before the addition: no fma (matters at an fp32 state)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int q = HW / 4;
    if (t >= (long long)V * C * q) return;
    const int i = (int)(t % q) * 4;
    const int c = (int)((t / q) % C), v = (int)(t / ((long long)q * C));
    int4 p = *(const int4*)(perm + (long long)v * HW + i);
    p.x = inb(p.x, HW); p.y = inb(p.y, HW); p.z = inb(p.z, HW); p.w = inb(p.w, HW);
    const float sg = vsign[v * C + c];
    const long long row = (long long)c * HW;
    float x[4] = {sg * ld1<BF>(y, row + p.x), sg * ld1<BF>(y, row + p.y), sg * ld1<BF>(y, row + p.z), sg * ld1<BF>(y, row + p.w)};
    const long long o = ((long long)v * C + c) * HW + i;
    if (f0) {
        float k[4];
        ld4<BF>(f0, o, k);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] += BF ? bfr(k[j] * half_dt) : k[j] * half_dt;
    }
    st4<BF>(out, o, x);
}

// out[c][i] = R(y[c][i] - R((sum_v isign[v][c] * -R(f[v][c][iperm[v][i]] * dt)) / V)), views summed in fp32 in the order v = 0 .. V-1
template <bool BF>
__global__ void views_reduce_kernel(const void* __restrict__ y, const void* __restrict__ f, const int* __restrict__ iperm,
                                    const float* __restrict__ isign, void* __restrict__ out, float dt, int V, int C, int HW) {
#pragma clang fp contract(off)  // every product and sum rounds on its own, as the tensor expression does
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int q = HW / 4;
    if (t >= (long long)C * q) return;
    const int i = (int)(t % q) * 4, c = (int)(t / q);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < V; ++v) {
        const int4 p = *(const int4*)(iperm + (long long)v * HW + i);
        const int pj[4] = {inb(p.x, HW), inb(p.y, HW), inb(p.z, HW), inb(p.w, HW)};
        const float sg = isign[v * C + c];
        const long long row = ((long long)v * C + c) * HW;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float k = ld1<BF>(f, row + pj[j]) * dt;
            acc[j] += sg * -(BF ? bfr(k) : k);
        }
    }
    const long long o = (long long)c * HW + i;
    float yv[4];
    ld4<BF>(y, o, yv);
    const float nv = (float)V;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float m = acc[j] / nv;
        yv[j] -= BF ? bfr(m) : m;
    }
    st4<BF>(out, o, yv);
}

// out[v][c][i] = vsign[v][c] * R(R(k1c * s) + R(kc * R(R(ft * G[c][p]) + R(f1t * Z[c][p])))),  p = perm[v][i],
// s = y[c][p]  (f0 == nullptr)   or   R(y[c][p] + isign[v][c] * R(f0[v][c][i] * half_dt))
template <bool BF>
__global__ void views_guided_gather_kernel(const void* __restrict__ y, const void* __restrict__ G, const void* __restrict__ Z,
                                           const int* __restrict__ perm, const float* __restrict__ vsign, const float* __restrict__ isign,
                                           const void* __restrict__ f0, void* __restrict__ out, float half_dt, float ft, float f1t, float kc,
                                           float k1c, int V, int C, int HW) {
#pragma clang fp contract(off)  // every product rounds before its sum, as the tensor expressions do: no fma (matters at an fp32 state)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int q = HW / 4;
    if (t >= (long long)V * C * q) return;
    const int i = (int)(t % q) * 4;
    const int c = (int)((t / q) % C), v = (int)(t / ((long long)q * C));
    const int4 p = *(const int4*)(perm + (long long)v * HW + i);
    const int pj[4] = {inb(p.x, HW), inb(p.y, HW), inb(p.z, HW), inb(p.w, HW)};
    const float sg = vsign[v * C + c];
    const long long row = (long long)c * HW;
    const long long o = ((long long)v * C + c) * HW + i;
    float s[4], k[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = ld1<BF>(y, row + pj[j]);
    if (f0) {
        const float isg = isign[v * C + c];
        ld4<BF>(f0, o, k);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float h = k[j] * half_dt;
            const float ym = s[j] + isg * (BF ? bfr(h) : h);
            s[j] = BF ? bfr(ym) : ym;
        }
    }
    float m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a = ft * ld1<BF>(G, row + pj[j]), b = f1t * ld1<BF>(Z, row + pj[j]);
        const float gsum = BF ? bfr(a) + bfr(b) : a + b;
        const float g = BF ? bfr(gsum) : gsum;
        const float ms = k1c * s[j], mg = kc * g;
        const float msum = BF ? bfr(ms) + bfr(mg) : ms + mg;
        m[j] = sg * (BF ? bfr(msum) : msum);
    }
    st4<BF>(out, o, m);
}

inline int nblk(long long n, int bs) { return (int)((n + bs - 1) / bs); }

int check_shape(const char* who, int V, int C, int HW) {
    LT_REQUIRE(V >= 1 && C >= 1 && HW >= 4 && HW % 4 == 0, "%s: V %d, C %d, H*W %d (H*W must be a positive multiple of 4)", who, V, C, HW);
    return 0;
}

}  // namespace

int launch_views_invert(const int* perm, int* iperm, int* hits, int V, int HW, hipStream_t stream) {
    LT_REQUIRE(perm && iperm && hits, "views_invert: null argument");
    LT_REQUIRE(V >= 1 && HW >= 1, "views_invert: V %d, H*W %d", V, HW);
    const long long n = (long long)V * HW;
    LT_CHECK_HIP(hipMemsetAsync(hits, 0, (size_t)(n + 1) * sizeof(int), stream));
    hipLaunchKernelGGL(views_invert_kernel, dim3(nblk(n, 256)), dim3(256), 0, stream, perm, iperm, hits, V, HW);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_views_gather(const void* y, const int* perm, const float* vsign, const void* f0, void* out, float half_dt, int V, int C, int HW,
                        int dtype, hipStream_t stream) {
    LT_REQUIRE(y && perm && vsign && out, "views_gather: null argument");
    LT_REQUIRE(dtype == 0 || dtype == 1, "views_gather: state dtype must be f32 or bf16");
    if (check_shape("views_gather", V, C, HW)) return 1;
    const long long n = (long long)V * C * (HW / 4);
    if (dtype == 1) hipLaunchKernelGGL(views_gather_kernel<true>, dim3(nblk(n, 256)), dim3(256), 0, stream, y, perm, vsign, f0, out, half_dt, V, C, HW);
    else hipLaunchKernelGGL(views_gather_kernel<false>, dim3(nblk(n, 256)), dim3(256), 0, stream, y, perm, vsign, f0, out, half_dt, V, C, HW);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_views_reduce(const void* y, const void* f, const int* iperm, const float* isign, void* out, float dt, int V, int C, int HW, int dtype,
                        hipStream_t stream) {
    LT_REQUIRE(y && f && iperm && isign && out, "views_reduce: null argument");
    LT_REQUIRE(dtype == 0 || dtype == 1, "views_reduce: state dtype must be f32 or bf16");
    if (check_shape("views_reduce", V, C, HW)) return 1;
    const long long n = (long long)C * (HW / 4);
    if (dtype == 1) hipLaunchKernelGGL(views_reduce_kernel<true>, dim3(nblk(n, 256)), dim3(256), 0, stream, y, f, iperm, isign, out, dt, V, C, HW);
    else hipLaunchKernelGGL(views_reduce_kernel<false>, dim3(nblk(n, 256)), dim3(256), 0, stream, y, f, iperm, isign, out, dt, V, C, HW);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_views_guided_gather(const void* y, const void* guidance, const void* noise, const int* perm, const float* vsign, const float* isign,
                               const void* f0, void* out, float half_dt, const float* coef, int V, int C, int HW, int dtype, hipStream_t stream) {
    LT_REQUIRE(y && guidance && noise && perm && vsign && isign && out && coef, "views_guided_gather: null argument");
    LT_REQUIRE(dtype == 0 || dtype == 1, "views_guided_gather: state dtype must be f32 or bf16");
    if (check_shape("views_guided_gather", V, C, HW)) return 1;
    const long long n = (long long)V * C * (HW / 4);
    if (dtype == 1)
        hipLaunchKernelGGL(views_guided_gather_kernel<true>, dim3(nblk(n, 256)), dim3(256), 0, stream, y, guidance, noise, perm, vsign, isign, f0, out,
                           half_dt, coef[0], coef[1], coef[2], coef[3], V, C, HW);
    else
        hipLaunchKernelGGL(views_guided_gather_kernel<false>, dim3(nblk(n, 256)), dim3(256), 0, stream, y, guidance, noise, perm, vsign, isign, f0, out,
                           half_dt, coef[0], coef[1], coef[2], coef[3], V, C, HW);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

// Prompt-driven editing (FlowEdit, Kulikov et al. 2024): the two state kernels around the one model evaluation of an interval of
// lt_sample_flowedit.  The definition is transport/edit.py: sample_flowedit.  R = rounding to the state dtype (bf16; identity at fp32); t, 1 - t,
// dt and the two guidance scales are fp32 scalars that multiply in fp32; every product, sum and difference rounds on its own.
//   mix:      zs = R(R(x_src t) + R(noise (1 - t)))           the source on the straight path at t
//             zt = R(zs + R(z - x_src))                        the edit, shifted by the same amount (z == x_src gives zt == zs exactly)
//             out4 = [zs, zt, zs, zt], B' rows each: the model input under the source, target and the two negative prompts
//   combine:  channels <  ch:  v_s = R(u_s + R(w_s R(c_s - u_s))),  v_t = R(u_t + R(w_t R(c_t - u_t)))      (forward_with_cfg's expression per branch)
//             channels >= ch:  v_s = c_s,  v_t = c_t
//             z' = R(z + R(R(v_t - v_s) dt))                   out4 = the evaluation's rows [c_s, c_t, u_s, u_t]
#include "common.h"
#include "kernels.h"

namespace {

inline int nblk(long long n, int per) { return (int)((n + per - 1) / per); }

template <bool BF>
__device__ __forceinline__ float R(float f) { return BF ? bfr(f) : f; }
template <bool BF>
__device__ __forceinline__ float ld(const void* p, long long i) { return BF ? bf2f(((const u16*)p)[i]) : ((const float*)p)[i]; }
template <bool BF>
__device__ __forceinline__ void st(void* p, long long i, float v) {
    if (BF) ((u16*)p)[i] = f2bf(v);
    else ((float*)p)[i] = v;
}

// one thread per element of [B', C, H, W]; x_src may be z (neither is written)
template <bool BF>
__global__ __launch_bounds__(256) void flowedit_mix_kernel(const void* x_src, const void* z, const void* __restrict__ noise, void* __restrict__ out4,
                                                           float t, float omt, long long n_half) {
#pragma clang fp contract(off)  // every step of the chain rounds on its own, as the tensor expression does
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_half; i += (long long)gridDim.x * blockDim.x) {
        const float xs = ld<BF>(x_src, i), zz = ld<BF>(z, i), w = ld<BF>(noise, i);
        const float zs = R<BF>(R<BF>(xs * t) + R<BF>(w * omt));
        const float zt = R<BF>(zs + R<BF>(zz - xs));
        st<BF>(out4, i, zs);
        st<BF>(out4, i + n_half, zt);
        st<BF>(out4, i + 2 * n_half, zs);
        st<BF>(out4, i + 3 * n_half, zt);
    }
}

// one thread per element of [B', C, HW]; z_next may be z, not out4
template <bool BF>
__global__ __launch_bounds__(256) void flowedit_combine_kernel(const void* z, const void* __restrict__ out4, void* z_next, float w_s, float w_t, float dt,
                                                               long long n_half, int C, int HW, int ch) {
#pragma clang fp contract(off)
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_half; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)((i / HW) % C);
        float vs = ld<BF>(out4, i), vt = ld<BF>(out4, i + n_half);
        if (c < ch) {
            const float us = ld<BF>(out4, i + 2 * n_half), ut = ld<BF>(out4, i + 3 * n_half);
            vs = R<BF>(us + R<BF>(w_s * R<BF>(vs - us)));
            vt = R<BF>(ut + R<BF>(w_t * R<BF>(vt - ut)));
        }
        const float step = R<BF>(R<BF>(vt - vs) * dt);
        st<BF>(z_next, i, R<BF>(ld<BF>(z, i) + step));
    }
}

inline int grid_for(long long n) {
    const int g = nblk(n, 256);
    return g > 8192 ? 8192 : g;
}

}  // namespace

int launch_flowedit_mix(const void* x_src, const void* z, const void* noise, void* out4, float t, float omt, long long n_half, int dtype,
                        hipStream_t stream) {
    LT_REQUIRE(x_src && z && noise && out4, "flowedit_mix: null argument");
    LT_REQUIRE(dtype == 0 || dtype == 1, "flowedit_mix: state dtype %d is not 0 (f32) or 1 (bf16)", dtype);
    LT_REQUIRE(n_half >= 1, "flowedit_mix: %lld elements per row group (need at least 1)", n_half);
    if (dtype == 1) hipLaunchKernelGGL(flowedit_mix_kernel<true>, dim3(grid_for(n_half)), dim3(256), 0, stream, x_src, z, noise, out4, t, omt, n_half);
    else hipLaunchKernelGGL(flowedit_mix_kernel<false>, dim3(grid_for(n_half)), dim3(256), 0, stream, x_src, z, noise, out4, t, omt, n_half);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_flowedit_combine(const void* z, const void* out4, void* z_next, float w_s, float w_t, float dt, int Bp, int C, int HW, int ch, int dtype,
                            hipStream_t stream) {
    LT_REQUIRE(z && out4 && z_next, "flowedit_combine: null argument");
    LT_REQUIRE(dtype == 0 || dtype == 1, "flowedit_combine: state dtype %d is not 0 (f32) or 1 (bf16)", dtype);
    LT_REQUIRE(Bp >= 1 && C >= 1 && HW >= 1, "flowedit_combine: B' = %d, C = %d, H W = %d (each must be at least 1)", Bp, C, HW);
    LT_REQUIRE(ch >= 1 && ch <= C, "flowedit_combine: cfg_channels %d outside 1..%d", ch, C);
    const long long n_half = (long long)Bp * C * HW;
    const char *lo = (const char*)out4, *hi = lo + 4 * n_half * (dtype == 1 ? 2 : 4);
    LT_REQUIRE((const char*)z_next + n_half * (dtype == 1 ? 2 : 4) <= lo || (const char*)z_next >= hi,
               "flowedit_combine: z_next lies inside the evaluation's four row groups (it may alias z, not out4)");
    if (dtype == 1)
        hipLaunchKernelGGL(flowedit_combine_kernel<true>, dim3(grid_for(n_half)), dim3(256), 0, stream, z, out4, z_next, w_s, w_t, dt, n_half, C, HW, ch);
    else
        hipLaunchKernelGGL(flowedit_combine_kernel<false>, dim3(grid_for(n_half)), dim3(256), 0, stream, z, out4, z_next, w_s, w_t, dt, n_half, C, HW, ch);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

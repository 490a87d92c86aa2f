// Rescaled and norm-limited guidance: the per-sample factor of the guided output, formed between the final GEMM and the closing
// kernel.  guidance_stats_kernel reduces four float64 sums per sample over the final-layer rows; unpatchify_cfg_rule_kernel - the closing kernel
// of the guidance schedule (unpatchify_cfg_dev_kernel, misc.hip) with one opening phase - turns them into the factor and multiplies.  The
// definition is transport/guidance.py: guided_rule.
#include <cmath>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int GS_SLICES = LT_GUIDANCE_SLICES;
constexpr int GS_THREADS = 256;

inline int nblk(long long n, int per) { return (int)((n + per - 1) / per); }

// Grid (B / 2 samples) x (GS_SLICES slices).  Sample b's n = ch H W guided elements j = (c, hh, w) are cut into GS_SLICES runs of
// ceil(n / GS_SLICES); a block sums its run: c, c^2, g, g^2 with g = bfr(u + bfr(w bfr(c - u))), the closing kernel's chain, the products and
// the sums in float64.  Thread, wave and block order are fixed by the launch, so the result is a function of the inputs alone.
__global__ __launch_bounds__(GS_THREADS) void guidance_stats_kernel(const u16* __restrict__ rows, int ld, int half, int out_ch, int H, int W, int patch,
                                                                    const float* __restrict__ cfg_scale_dev, int ch, int wp_stride,
                                                                    double* __restrict__ partials) {
#pragma clang fp contract(off)  // the guidance chain rounds step by step; a float64 product rounds before the sum that takes it
    const int b = blockIdx.x, sl = blockIdx.y;
    const int Hp = H / patch;
    const long long n = (long long)ch * H * W;
    const long long per = (n + GS_SLICES - 1) / GS_SLICES;
    const long long j0 = (long long)sl * per;
    const long long j1 = j0 + per < n ? j0 + per : n;
    const float cfg_scale = cfg_scale_dev[0];
    double sc = 0.0, scc = 0.0, sg = 0.0, sgg = 0.0;
    for (long long j = j0 + threadIdx.x; j < j1; j += GS_THREADS) {
        const int w = (int)(j % W);
        const int hh = (int)((j / W) % H);
        const int c = (int)(j / ((long long)W * H));
        const int e = ((hh % patch) * patch + (w % patch)) * out_ch + c;
        const long long tok = (long long)(hh / patch) * wp_stride + (w / patch);  // eol column (if any) is skipped
        const float cond = bf2f(rows[((long long)b * Hp * wp_stride + tok) * ld + e]);
        const float unc = bf2f(rows[((long long)(b + half) * Hp * wp_stride + tok) * ld + e]);
        const float g = bfr(unc + bfr(cfg_scale * bfr(cond - unc)));
        const double dc = (double)cond, dg = (double)g;
        sc += dc; scc += dc * dc; sg += dg; sgg += dg * dg;
    }
    // lanes of a wave, then the waves in index order
    for (int off = 32; off > 0; off >>= 1) {
        sc += __shfl_down(sc, off); scc += __shfl_down(scc, off); sg += __shfl_down(sg, off); sgg += __shfl_down(sgg, off);
    }
    __shared__ double red[GS_THREADS / 64][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave][0] = sc; red[wave][1] = scc; red[wave][2] = sg; red[wave][3] = sgg; }
    __syncthreads();
    if (threadIdx.x < 4) {
        double v = red[0][threadIdx.x];
        for (int k = 1; k < GS_THREADS / 64; ++k) v += red[k][threadIdx.x];
        partials[((size_t)b * GS_SLICES + sl) * 4 + threadIdx.x] = v;  // (an empty run writes zeros)
    }
}

// guided_rule's step 3 in float64, no contraction: the one rounding is the cast of fr * fl
__device__ float guidance_factor(const double* __restrict__ p, double n, float rescale_f, float limit_f) {
#pragma clang fp contract(off)
    double Sc = 0.0, Scc = 0.0, Sg = 0.0, Sgg = 0.0;
    for (int s = 0; s < GS_SLICES; ++s) { Sc += p[s * 4 + 0]; Scc += p[s * 4 + 1]; Sg += p[s * 4 + 2]; Sgg += p[s * 4 + 3]; }
    const double rescale = (double)rescale_f, limit = (double)limit_f;
    const double mc = Sc / n, mg = Sg / n;
    const double vc = Scc / n - mc * mc;
    const double vg = Sgg / n - mg * mg;
    const double ratio = (vg > 0.0 && vc >= 0.0) ? sqrt(vc / vg) : 1.0;
    const double fr = rescale * ratio + (1.0 - rescale);
    double fl = 1.0;
    const double den = fr * sqrt(Sgg);
    if (limit_f < INFINITY && den > 0.0) {
        const double q = limit * sqrt(Scc) / den;
        fl = q < 1.0 ? q : 1.0;
    }
    return (float)(fr * fl);
}

// unpatchify_cfg_dev_kernel (misc.hip) with the rule: at block start the first B / 2 threads each add their sample's GS_SLICES partials in
// index order, form the factor and leave it in LDS; the element loop writes bfr(g f) where that kernel writes g.  dup, the channels at or
// past cfg_channels, both output dtypes and the index walk are that kernel's.  factor_out (may be null): the B / 2 factors, from block 0.
__global__ __launch_bounds__(256) void unpatchify_cfg_rule_kernel(const u16* __restrict__ rows, int ld, void* __restrict__ out, int out_dtype, int B,
                                                                  int C, int out_ch, int H, int W, int patch, int use_cfg,
                                                                  const float* __restrict__ cfg_scale_dev, int cfg_channels, int wp_stride, int dup,
                                                                  const double* __restrict__ partials, const float* __restrict__ rescale_dev,
                                                                  const float* __restrict__ limit_dev, float* __restrict__ factor_out) {
#pragma clang fp contract(off)  // every step of the guidance chain rounds on its own, as the tensor expression does
    __shared__ float fs[256];
    const long long total = (long long)B * C * H * W;
    const int Hp = H / patch;
    const int half = B / 2;
    const bool guided = use_cfg && !dup;
    if (guided) {
        if ((int)threadIdx.x < half) {
            const float f = guidance_factor(partials + (size_t)threadIdx.x * GS_SLICES * 4, (double)((long long)cfg_channels * H * W),
                                            rescale_dev[0], limit_dev[0]);
            fs[threadIdx.x] = f;
            if (factor_out && blockIdx.x == 0) factor_out[threadIdx.x] = f;
        }
        __syncthreads();
    }
    const float cfg_scale = guided ? cfg_scale_dev[0] : 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int w = (int)(i % W);
        const int hh = (int)((i / W) % H);
        const int c = (int)((i / ((long long)W * H)) % C);
        const int b = (int)(i / ((long long)W * H * C));
        const int e = ((hh % patch) * patch + (w % patch)) * out_ch + c;
        const long long tok = (long long)(hh / patch) * wp_stride + (w / patch);  // eol column (if any) is skipped
        auto rd = [&](int bb) { return bf2f(rows[((long long)bb * Hp * wp_stride + tok) * ld + e]); };
        float v;
        if (dup) {
            v = rd(b % half);
        } else if (use_cfg && c < cfg_channels) {
            const int bc = b % half;
            const float cond = rd(bc), unc = rd(bc + half);
            v = bfr(bfr(unc + bfr(cfg_scale * bfr(cond - unc))) * fs[bc]);
        } else {
            v = rd(b);
        }
        if (out_dtype == 0) ((float*)out)[i] = v;
        else ((u16*)out)[i] = f2bf(v);
    }
}

// scale, rescale and norm limit of one evaluation into the engine's fixed words (lt_forward_cfg_rule): a launch in stream order, no copy from
// pageable host memory
__global__ void guidance_params_store_kernel(float* __restrict__ dst, float scale, float rescale, float limit) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { dst[0] = scale; dst[1] = rescale; dst[2] = limit; }
}

int check_rule_shape(const char* who, int B, int C, int out_ch, int H, int W, int patch, int ld, int cfg_channels) {
    LT_REQUIRE(B >= 2 && B % 2 == 0, "%s: guidance needs an even count of rows (cond + uncond), got %d", who, B);
    LT_REQUIRE(C >= 1 && out_ch >= C && patch >= 1 && H >= patch && W >= patch && H % patch == 0 && W % patch == 0 && ld >= patch * patch * out_ch,
               "%s: bad shape", who);
    LT_REQUIRE(cfg_channels >= 1 && cfg_channels <= C, "%s: cfg_channels %d outside 1..%d", who, cfg_channels, C);
    LT_REQUIRE(B / 2 <= 256, "%s: %d samples exceed the 256 threads of a block that form their factors", who, B / 2);
    return 0;
}

}  // namespace

int launch_guidance_stats(const u16* rows, int ld, int B, int out_ch, int H, int W, int patch, const float* cfg_scale_dev, int cfg_channels,
                          int wp_stride, double* partials, hipStream_t stream) {
    LT_REQUIRE(rows && cfg_scale_dev && partials, "guidance_stats: null argument");
    if (check_rule_shape("guidance_stats", B, cfg_channels, out_ch, H, W, patch, ld, cfg_channels)) return 2;
    const int stride = wp_stride > 0 ? wp_stride : W / patch;
    LT_REQUIRE(stride >= W / patch, "guidance_stats: wp_stride %d below the %d tokens of a latent row", stride, W / patch);
    hipLaunchKernelGGL(guidance_stats_kernel, dim3(B / 2, GS_SLICES), dim3(GS_THREADS), 0, stream, rows, ld, B / 2, out_ch, H, W, patch,
                       cfg_scale_dev, cfg_channels, stride, partials);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_unpatchify_cfg_rule(const u16* rows, int ld, void* out, int out_dtype, int B, int C, int out_ch, int H, int W, int patch, int use_cfg,
                               const float* cfg_scale_dev, int cfg_channels, int wp_stride, int dup, const double* partials,
                               const float* rescale_dev, const float* limit_dev, float* factor_out, hipStream_t stream) {
    LT_REQUIRE(rows && out, "unpatchify_cfg_rule: null argument");
    if (check_rule_shape("unpatchify_cfg_rule", B, C, out_ch, H, W, patch, ld, use_cfg && !dup ? cfg_channels : 1)) return 2;
    LT_REQUIRE(dup || !use_cfg || (cfg_scale_dev && partials && rescale_dev && limit_dev), "unpatchify_cfg_rule: null scale, partials or rule parameter");
    const long long total = (long long)B * C * H * W;
    int g = nblk(total, 256);
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(unpatchify_cfg_rule_kernel, dim3(g), dim3(256), 0, stream, rows, ld, out, out_dtype, B, C, out_ch, H, W, patch, use_cfg,
                       cfg_scale_dev, cfg_channels, wp_stride > 0 ? wp_stride : W / patch, dup, partials, rescale_dev, limit_dev, factor_out);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_guidance_params_store(float* dst, float scale, float rescale, float limit, hipStream_t stream) {
    LT_REQUIRE(dst, "guidance_params_store: null argument");
    hipLaunchKernelGGL(guidance_params_store_kernel, dim3(1), dim3(64), 0, stream, dst, scale, rescale, limit);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

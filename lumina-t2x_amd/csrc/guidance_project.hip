// Projected guidance: APG (Sadat et al. 2024) and CFG-Zero* (Fan et al. 2025), the two forms of the guided output that need inner
// products between the conditional and the unconditional prediction.  guidance_project_stats_kernel reduces them per sample over the
// final-layer rows - and, under APG, advances the momentum buffer in the same pass; unpatchify_cfg_project_kernel - the closing kernel of the
// rule (unpatchify_cfg_rule_kernel, guidance.hip) with another opening phase and another chain - turns the sums into the coefficients and
// writes the output.  The definition is transport/guidance.py: guided_project.
#include <cmath>

#include "../../include/lumina_dit.h"
#include "common.h"
#include "kernels.h"

namespace {

constexpr int GP_SLICES = LT_GUIDANCE_SLICES;
constexpr int GP_THREADS = 256;
constexpr int GP_SUMS = LT_PROJECT_SUMS;  // per slice; the Zero* form leaves the third at 0

inline int nblk(long long n, int per) { return (int)((n + per - 1) / per); }

// Grid (B / 2 samples) x (GP_SLICES slices), guidance_stats_kernel's cut of the n = ch H W guided elements j = (c, hh, w) of a sample.
//   form 1 (APG): d = bfr(c - u); m = d + beta m_prev in fp32, written back over m_prev at (b, j) by the thread that read it; sums m^2, m c, c^2
//   form 2 (Zero*): sums c u, u^2, 0
// the products and the sums in float64.  par: { -, eta, beta, r } - beta alone is read here.  Thread, wave and block order are fixed by the
// launch, so the result is a function of the inputs alone.
__global__ __launch_bounds__(GP_THREADS) void guidance_project_stats_kernel(const u16* __restrict__ rows, int ld, int half, int out_ch, int H, int W,
                                                                            int patch, int ch, int wp_stride, int form,
                                                                            const float* __restrict__ par, float* __restrict__ mom,
                                                                            double* __restrict__ partials) {
#pragma clang fp contract(off)  // every step rounds on its own; a float64 product rounds before the sum that takes it
    const int b = blockIdx.x, sl = blockIdx.y;
    const int Hp = H / patch;
    const long long n = (long long)ch * H * W;
    const long long per = (n + GP_SLICES - 1) / GP_SLICES;
    const long long j0 = (long long)sl * per;
    const long long j1 = j0 + per < n ? j0 + per : n;
    const float beta = form == 1 ? par[2] : 0.f;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (long long j = j0 + threadIdx.x; j < j1; j += GP_THREADS) {
        const int w = (int)(j % W);
        const int hh = (int)((j / W) % H);
        const int c = (int)(j / ((long long)W * H));
        const int e = ((hh % patch) * patch + (w % patch)) * out_ch + c;
        const long long tok = (long long)(hh / patch) * wp_stride + (w / patch);  // eol column (if any) is skipped
        const float cond = bf2f(rows[((long long)b * Hp * wp_stride + tok) * ld + e]);
        const float unc = bf2f(rows[((long long)(b + half) * Hp * wp_stride + tok) * ld + e]);
        const double dc = (double)cond;
        if (form == 1) {
            const long long at = (long long)b * n + j;
            const float bm = beta * mom[at];
            const float m = bfr(cond - unc) + bm;
            mom[at] = m;
            const double dm = (double)m;
            s0 += dm * dm; s1 += dm * dc; s2 += dc * dc;
        } else {
            const double du = (double)unc;
            s0 += dc * du; s1 += du * du;
        }
    }
    // lanes of a wave, then the waves in index order
    for (int off = 32; off > 0; off >>= 1) { s0 += __shfl_down(s0, off); s1 += __shfl_down(s1, off); s2 += __shfl_down(s2, off); }
    __shared__ double red[GP_THREADS / 64][GP_SUMS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; }
    __syncthreads();
    if (threadIdx.x < GP_SUMS) {
        double v = red[0][threadIdx.x];
        for (int k = 1; k < GP_THREADS / 64; ++k) v += red[k][threadIdx.x];
        partials[((size_t)b * GP_SLICES + sl) * GP_SUMS + threadIdx.x] = v;  // (an empty run writes zeros)
    }
}

// guided_project's coefficients of one sample in float64, no contraction; each is rounded to fp32 once.
//   form 1: (a, b) = ((w - 1) tn, (w - 1)(eta - 1) p), tn the norm clip of m, p = tn <m, c> / <c, c>
//   form 2: (s, 0), s = <c, u> / <u, u>
__device__ float2 project_coefficients(const double* __restrict__ p, int form, float w_f, const float* __restrict__ par) {
#pragma clang fp contract(off)
    double S0 = 0.0, S1 = 0.0, S2 = 0.0;
    for (int s = 0; s < GP_SLICES; ++s) { S0 += p[s * GP_SUMS + 0]; S1 += p[s * GP_SUMS + 1]; S2 += p[s * GP_SUMS + 2]; }
    if (form == 2) return make_float2((float)(S1 > 0.0 ? S0 / S1 : 1.0), 0.f);
    const float r_f = par[3];
    const double w1 = (double)w_f - 1.0, eta1 = (double)par[1] - 1.0;
    double tn = 1.0;
    if (r_f < INFINITY && S0 > 0.0) {
        const double q = (double)r_f / sqrt(S0);
        tn = q < 1.0 ? q : 1.0;
    }
    const double pr = S2 > 0.0 ? tn * S1 / S2 : 0.0;
    return make_float2((float)(w1 * tn), (float)(w1 * eta1 * pr));
}

// unpatchify_cfg_rule_kernel (guidance.hip) with the projected chain: at block start the first B / 2 threads each add their sample's GP_SLICES
// partials in index order, form the coefficients and leave them in LDS; the element loop writes
//   form 1: bfr(c + (a m + b c)), m from the momentum buffer the stats kernel left       form 2: bfr(s u + w (c - s u))
// every operation in fp32, rounding on its own.  dup, the channels at or past cfg_channels, both output dtypes and the index walk are that
// kernel's.  coef_out (may be null): form 1 the B / 2 pairs (a, b), form 2 the B / 2 values s, from block 0.
__global__ __launch_bounds__(256) void unpatchify_cfg_project_kernel(const u16* __restrict__ rows, int ld, void* __restrict__ out, int out_dtype, int B,
                                                                     int C, int out_ch, int H, int W, int patch, int use_cfg,
                                                                     const float* __restrict__ cfg_scale_dev, int cfg_channels, int wp_stride, int dup,
                                                                     int form, const double* __restrict__ partials, const float* __restrict__ par,
                                                                     const float* __restrict__ mom, float* __restrict__ coef_out) {
#pragma clang fp contract(off)  // every step of the chain rounds on its own, as the tensor expression does
    __shared__ float2 cs[256];
    const long long total = (long long)B * C * H * W;
    const int Hp = H / patch;
    const int half = B / 2;
    const bool guided = use_cfg && !dup;
    const float cfg_scale = guided ? cfg_scale_dev[0] : 0.f;
    if (guided) {
        if ((int)threadIdx.x < half) {
            const float2 k = project_coefficients(partials + (size_t)threadIdx.x * GP_SLICES * GP_SUMS, form, cfg_scale, par);
            cs[threadIdx.x] = k;
            if (coef_out && blockIdx.x == 0) {
                if (form == 1) { coef_out[2 * threadIdx.x] = k.x; coef_out[2 * threadIdx.x + 1] = k.y; }
                else coef_out[threadIdx.x] = k.x;
            }
        }
        __syncthreads();
    }
    const long long chw = (long long)cfg_channels * H * W;
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
            const float cond = rd(bc);
            const float2 k = cs[bc];
            if (form == 1) {
                const float m = mom[(long long)bc * chw + ((long long)c * H + hh) * W + w];
                const float am = k.x * m, bcnd = k.y * cond;
                const float upd = am + bcnd;
                v = bfr(cond + upd);
            } else {
                const float su = k.x * rd(bc + half);
                const float diff = cond - su;
                const float wd = cfg_scale * diff;
                v = bfr(su + wd);
            }
        } else {
            v = rd(b);
        }
        if (out_dtype == 0) ((float*)out)[i] = v;
        else ((u16*)out)[i] = f2bf(v);
    }
}

// scale, eta, momentum and norm threshold of one evaluation into the engine's fixed words (lt_forward_cfg_project): a launch in stream order,
// no copy from pageable host memory
__global__ void guidance_project_params_store_kernel(float* __restrict__ dst, float scale, float eta, float beta, float r) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { dst[0] = scale; dst[1] = eta; dst[2] = beta; dst[3] = r; }
}

int check_project_shape(const char* who, int B, int C, int out_ch, int H, int W, int patch, int ld, int cfg_channels) {
    LT_REQUIRE(B >= 2 && B % 2 == 0, "%s: guidance needs an even count of rows (cond + uncond), got %d", who, B);
    LT_REQUIRE(C >= 1 && out_ch >= C && patch >= 1 && H >= patch && W >= patch && H % patch == 0 && W % patch == 0 && ld >= patch * patch * out_ch,
               "%s: bad shape", who);
    LT_REQUIRE(cfg_channels >= 1 && cfg_channels <= C, "%s: cfg_channels %d outside 1..%d", who, cfg_channels, C);
    LT_REQUIRE(B / 2 <= 256, "%s: %d samples exceed the 256 threads of a block that form their coefficients", who, B / 2);
    return 0;
}

}  // namespace

int launch_guidance_project_stats(const u16* rows, int ld, int B, int out_ch, int H, int W, int patch, int cfg_channels, int wp_stride, int form,
                                  const float* par_dev, float* mom, double* partials, hipStream_t stream) {
    LT_REQUIRE(rows && partials, "guidance_project_stats: null argument");
    LT_REQUIRE(form == LT_PROJECT_APG || form == LT_PROJECT_ZERO_STAR, "guidance_project_stats: form %d is not 1 (APG) or 2 (CFG-Zero*)", form);
    LT_REQUIRE(form != LT_PROJECT_APG || (par_dev && mom), "guidance_project_stats: null parameter words or momentum buffer (APG)");
    if (check_project_shape("guidance_project_stats", B, cfg_channels, out_ch, H, W, patch, ld, cfg_channels)) return 2;
    const int stride = wp_stride > 0 ? wp_stride : W / patch;
    LT_REQUIRE(stride >= W / patch, "guidance_project_stats: wp_stride %d below the %d tokens of a latent row", stride, W / patch);
    hipLaunchKernelGGL(guidance_project_stats_kernel, dim3(B / 2, GP_SLICES), dim3(GP_THREADS), 0, stream, rows, ld, B / 2, out_ch, H, W, patch,
                       cfg_channels, stride, form, par_dev, mom, partials);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_unpatchify_cfg_project(const u16* rows, int ld, void* out, int out_dtype, int B, int C, int out_ch, int H, int W, int patch, int use_cfg,
                                  const float* cfg_scale_dev, int cfg_channels, int wp_stride, int dup, int form, const double* partials,
                                  const float* par_dev, const float* mom, float* coef_out, hipStream_t stream) {
    LT_REQUIRE(rows && out, "unpatchify_cfg_project: null argument");
    LT_REQUIRE(form == LT_PROJECT_APG || form == LT_PROJECT_ZERO_STAR, "unpatchify_cfg_project: form %d is not 1 (APG) or 2 (CFG-Zero*)", form);
    const bool guided = use_cfg && !dup;
    if (check_project_shape("unpatchify_cfg_project", B, C, out_ch, H, W, patch, ld, guided ? cfg_channels : 1)) return 2;
    LT_REQUIRE(!guided || (cfg_scale_dev && partials), "unpatchify_cfg_project: null scale or partials");
    LT_REQUIRE(!guided || form != LT_PROJECT_APG || (par_dev && mom), "unpatchify_cfg_project: null parameter words or momentum buffer (APG)");
    const int stride = wp_stride > 0 ? wp_stride : W / patch;
    LT_REQUIRE(stride >= W / patch, "unpatchify_cfg_project: wp_stride %d below the %d tokens of a latent row", stride, W / patch);
    const long long total = (long long)B * C * H * W;
    int g = nblk(total, 256);
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(unpatchify_cfg_project_kernel, dim3(g), dim3(256), 0, stream, rows, ld, out, out_dtype, B, C, out_ch, H, W, patch, use_cfg,
                       cfg_scale_dev, cfg_channels, stride, dup, form, partials, par_dev, mom, coef_out);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_guidance_project_params_store(float* dst, float scale, float eta, float beta, float r, hipStream_t stream) {
    LT_REQUIRE(dst, "guidance_project_params_store: null argument");
    hipLaunchKernelGGL(guidance_project_params_store_kernel, dim3(1), dim3(64), 0, stream, dst, scale, eta, beta, r);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

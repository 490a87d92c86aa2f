// Skip-layer guidance: the closing kernel of the three evaluations of one guided stage.  The skip evaluation - the cond rows with a
// set of blocks left out (run_forward, e->skip) - keeps its guided channels k; the stage's own evaluation then forms
//   g = bfr(bfr(u + bfr(w bfr(c - u))) + bfr(s bfr(c - k)))        (w != 1: all 2 B' rows)
//   g = bfr(c + bfr(s bfr(c - k)))                                 (w == 1: the B' cond rows alone)
// The definition is transport/guidance.py: sample_cfg_slg.
#include "common.h"
#include "kernels.h"

namespace {

inline int nblk(long long n, int per) { return (int)((n + per - 1) / per); }

// B counts OUTPUT rows (2 B'), skip is bf16 [B', cfg_channels, H, W].  The index walk and the eol stride of unpatchify_cfg_reuse_kernel.
//   mode 0 (store):  `rows` holds B' rows; the thread of channel c < cfg_channels writes its (already bf16) word to skip; `out` is not touched.
//   mode 1 (guided): `rows` holds 2 B' rows; every thread of the 2 B' output rows forms its value - both halves get the same guided channels,
//                    the other channels pass row by row.
//   mode 2 (cond):   `rows` holds B' rows; thread i of the first half forms its value once and writes rows b and b + B' of the output.
__global__ __launch_bounds__(256) void unpatchify_cfg_slg_kernel(const u16* __restrict__ rows, int ld, void* __restrict__ out, int out_dtype, int B,
                                                                 int C, int out_ch, int H, int W, int patch,
                                                                 const float* __restrict__ cfg_scale_dev, const float* __restrict__ slg_scale_dev,
                                                                 int cfg_channels, int wp_stride, u16* __restrict__ skip, int mode) {
#pragma clang fp contract(off)  // every step of the guidance chain rounds on its own, as the tensor expression does
    const int Hp = H / patch;
    const int half = B / 2;
    const long long HW = (long long)W * H;
    const long long half_elems = (long long)half * C * HW;
    const long long total = mode == 1 ? 2 * half_elems : half_elems;
    const float cfg_scale = mode == 1 ? cfg_scale_dev[0] : 1.f;
    const float slg_scale = mode == 0 ? 0.f : slg_scale_dev[0];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int w = (int)(i % W);
        const int hh = (int)((i / W) % H);
        const int c = (int)((i / HW) % C);
        const int b = (int)(i / (HW * C));
        const int e = ((hh % patch) * patch + (w % patch)) * out_ch + c;
        const long long tok = (long long)(hh / patch) * wp_stride + (w / patch);  // eol column (if any) is skipped
        auto rd = [&](int bb) { return rows[((long long)bb * Hp * wp_stride + tok) * ld + e]; };
        const int bc = b % half;
        const long long ki = ((long long)bc * cfg_channels + c) * HW + (long long)hh * W + w;  // (used for c < cfg_channels only)
        if (mode == 0) {
            if (c < cfg_channels) skip[ki] = rd(b);
            continue;
        }
        float v;
        if (c < cfg_channels) {
            const float cond = bf2f(rd(bc));
            const float t = bfr(slg_scale * bfr(cond - bf2f(skip[ki])));
            if (mode == 1) {
                const float unc = bf2f(rd(bc + half));
                const float d = bfr(cond - unc);
                v = bfr(bfr(unc + bfr(cfg_scale * d)) + t);
            } else {
                v = bfr(cond + t);
            }
        } else {
            v = bf2f(rd(b));
        }
        if (out_dtype == 0) ((float*)out)[i] = v;
        else ((u16*)out)[i] = f2bf(v);
        if (mode == 2) {
            if (out_dtype == 0) ((float*)out)[i + half_elems] = v;
            else ((u16*)out)[i + half_elems] = f2bf(v);
        }
    }
}

// the two scales of a single guided call (lt_forward_cfg_slg) into the engine's fixed words: no host memory a later call could rewrite
__global__ void slg_params_store_kernel(float* __restrict__ g_cfg, float cfg_scale, float slg_scale) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { g_cfg[0] = cfg_scale; g_cfg[3] = slg_scale; }
}

}  // namespace

int launch_slg_params_store(float* g_cfg, float cfg_scale, float slg_scale, hipStream_t stream) {
    LT_REQUIRE(g_cfg, "slg_params_store: null argument");
    hipLaunchKernelGGL(slg_params_store_kernel, dim3(1), dim3(64), 0, stream, g_cfg, cfg_scale, slg_scale);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_unpatchify_cfg_slg(const u16* rows, int ld, void* out, int out_dtype, int B, int C, int out_ch, int H, int W, int patch,
                              const float* cfg_scale_dev, const float* slg_scale_dev, int cfg_channels, int wp_stride, u16* skip, int mode,
                              hipStream_t stream) {
    LT_REQUIRE(mode >= 0 && mode <= 2, "unpatchify_cfg_slg: mode %d is not 0 (store the skip rows), 1 (guided) or 2 (cond)", mode);
    LT_REQUIRE(rows && skip && (mode == 0 || (out && slg_scale_dev)) && (mode != 1 || cfg_scale_dev), "unpatchify_cfg_slg: null argument");
    LT_REQUIRE(out_dtype == 0 || out_dtype == 1, "unpatchify_cfg_slg: out_dtype %d is not 0 (f32) or 1 (bf16)", out_dtype);
    LT_REQUIRE(B >= 2 && B % 2 == 0, "unpatchify_cfg_slg: guidance needs an even count of output rows (cond + uncond), got %d", B);
    LT_REQUIRE(C >= 1 && out_ch >= C && patch >= 1 && H >= patch && W >= patch && H % patch == 0 && W % patch == 0 && ld >= patch * patch * out_ch,
               "unpatchify_cfg_slg: bad shape");
    LT_REQUIRE(cfg_channels >= 1 && cfg_channels <= C, "unpatchify_cfg_slg: cfg_channels %d outside 1..%d", cfg_channels, C);
    const int stride = wp_stride > 0 ? wp_stride : W / patch;
    LT_REQUIRE(stride >= W / patch, "unpatchify_cfg_slg: wp_stride %d below the %d tokens of a latent row", stride, W / patch);
    const long long total = (long long)(mode == 1 ? B : B / 2) * C * H * W;
    int g = nblk(total, 256);
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(unpatchify_cfg_slg_kernel, dim3(g), dim3(256), 0, stream, rows, ld, out, out_dtype, B, C, out_ch, H, W, patch, cfg_scale_dev,
                       slg_scale_dev, cfg_channels, stride, skip, mode);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

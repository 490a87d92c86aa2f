// Guidance reuse: the closing kernel of a guided evaluation that keeps, or reads, the difference d = bfr(cond - uncond) of its
// guided channels.  A refresh stage is the closing kernel of the guidance schedule (unpatchify_cfg_dev_kernel, misc.hip) that also stores d;
// a reuse stage evaluated the cond rows alone and forms bfr(bfr(c' - d) + bfr(w d)) from the stored d.  The definition is
// transport/guidance.py: sample_cfg_reuse.
#include "common.h"
#include "kernels.h"

namespace {

inline int nblk(long long n, int per) { return (int)((n + per - 1) / per); }

// B counts OUTPUT rows (2 B'), delta is bf16 [B', cfg_channels, H, W].
//   mode 0 (store): the index walk and the chain of unpatchify_cfg_dev_kernel at use_cfg = 1, dup = 0 over the 2 B' rows of `rows`; the thread
//   of sample b < B', channel c < cfg_channels also writes d.
//   mode 1 (reuse): `rows` holds B' rows; thread i of the first half forms its value once and writes rows b and b + B' of the output.
__global__ __launch_bounds__(256) void unpatchify_cfg_reuse_kernel(const u16* __restrict__ rows, int ld, void* __restrict__ out, int out_dtype, int B,
                                                                   int C, int out_ch, int H, int W, int patch,
                                                                   const float* __restrict__ cfg_scale_dev, int cfg_channels, int wp_stride,
                                                                   u16* __restrict__ delta, int mode) {
#pragma clang fp contract(off)  // every step of the guidance chain rounds on its own, as the tensor expression does
    const int Hp = H / patch;
    const int half = B / 2;
    const long long HW = (long long)W * H;
    const long long half_elems = (long long)half * C * HW;
    const long long total = mode ? half_elems : 2 * half_elems;
    const float cfg_scale = cfg_scale_dev[0];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int w = (int)(i % W);
        const int hh = (int)((i / W) % H);
        const int c = (int)((i / HW) % C);
        const int b = (int)(i / (HW * C));
        const int e = ((hh % patch) * patch + (w % patch)) * out_ch + c;
        const long long tok = (long long)(hh / patch) * wp_stride + (w / patch);  // eol column (if any) is skipped
        auto rd = [&](int bb) { return bf2f(rows[((long long)bb * Hp * wp_stride + tok) * ld + e]); };
        const int bc = b % half;
        const long long di = ((long long)bc * cfg_channels + c) * HW + (long long)hh * W + w;  // (read for c < cfg_channels only)
        float v;
        if (mode) {
            v = rd(b);  // b < half
            if (c < cfg_channels) {
                const float d = bf2f(delta[di]);
                v = bfr(bfr(v - d) + bfr(cfg_scale * d));
            }
            if (out_dtype == 0) { ((float*)out)[i] = v; ((float*)out)[i + half_elems] = v; }
            else { const u16 o = f2bf(v); ((u16*)out)[i] = o; ((u16*)out)[i + half_elems] = o; }
            continue;
        }
        if (c < cfg_channels) {
            const float cond = rd(bc), unc = rd(bc + half);
            const float d = bfr(cond - unc);
            v = bfr(unc + bfr(cfg_scale * d));
            if (b < half) delta[di] = f2bf(d);
        } else {
            v = rd(b);
        }
        if (out_dtype == 0) ((float*)out)[i] = v;
        else ((u16*)out)[i] = f2bf(v);
    }
}

}  // namespace

int launch_unpatchify_cfg_reuse(const u16* rows, int ld, void* out, int out_dtype, int B, int C, int out_ch, int H, int W, int patch,
                                const float* cfg_scale_dev, int cfg_channels, int wp_stride, u16* delta, int mode, hipStream_t stream) {
    LT_REQUIRE(rows && out && cfg_scale_dev && delta, "unpatchify_cfg_reuse: null argument");
    LT_REQUIRE(mode == 0 || mode == 1, "unpatchify_cfg_reuse: mode %d is not 0 (store the delta) or 1 (reuse it)", mode);
    LT_REQUIRE(out_dtype == 0 || out_dtype == 1, "unpatchify_cfg_reuse: out_dtype %d is not 0 (f32) or 1 (bf16)", out_dtype);
    LT_REQUIRE(B >= 2 && B % 2 == 0, "unpatchify_cfg_reuse: guidance needs an even count of output rows (cond + uncond), got %d", B);
    LT_REQUIRE(C >= 1 && out_ch >= C && patch >= 1 && H >= patch && W >= patch && H % patch == 0 && W % patch == 0 && ld >= patch * patch * out_ch,
               "unpatchify_cfg_reuse: bad shape");
    LT_REQUIRE(cfg_channels >= 1 && cfg_channels <= C, "unpatchify_cfg_reuse: cfg_channels %d outside 1..%d", cfg_channels, C);
    const int stride = wp_stride > 0 ? wp_stride : W / patch;
    LT_REQUIRE(stride >= W / patch, "unpatchify_cfg_reuse: wp_stride %d below the %d tokens of a latent row", stride, W / patch);
    const long long total = (long long)(mode ? B / 2 : B) * C * H * W;
    int g = nblk(total, 256);
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(unpatchify_cfg_reuse_kernel, dim3(g), dim3(256), 0, stream, rows, ld, out, out_dtype, B, C, out_ch, H, W, patch, cfg_scale_dev,
                       cfg_channels, stride, delta, mode);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

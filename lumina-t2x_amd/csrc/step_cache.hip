// Step caching (transport/cache.py: sample_teacache is the definition): the row passes around the block stack of an evaluation that
// may reuse the stack's residual.  cache_indicator_kernel compares the timestep-modulated input of the first block with the previous
// evaluation's (two float64 sums) and keeps it; cache_residual_store_kernel keeps r = bfr(x_L - x_0) of an evaluation that ran the stack; an
// evaluation that reuses it closes with launch_gated_residual_norm without a gate (x = bfr(x_0 + r), then the final layer's LayerNorm +
// modulate, next_mode 2).  All three are elementwise over whole 16-byte chunks: bandwidth-bound, no LDS beyond the reduction, and a launch
// geometry that does not depend on the device, so the summation order is a function of the element count alone.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int CI_BLOCKS = LT_CACHE_BLOCKS;
constexpr int CI_THREADS = 256;

// Chunk c (8 words) of the n / 8 chunks belongs to thread c % (CI_BLOCKS * CI_THREADS), which walks its chunks in ascending order and, inside
// a chunk, the words in ascending order: s1 += |h - h_prev|, s0 += |h_prev|, every difference and sum in float64 (the difference of two bf16
// values is exact there).  Then the lanes of a wave, then the waves in index order, as guidance_stats_kernel does; block b leaves
// partials[2 b] = s1, partials[2 b + 1] = s0 (a block without chunks: zeros).  h_prev <- h in the same pass.  The sums are elementwise, so h
// may be row-major or in the row-pair layout, as long as h_prev has the layout h has.
__global__ __launch_bounds__(CI_THREADS) void cache_indicator_kernel(const u16* __restrict__ h, u16* __restrict__ h_prev, long long nchunks,
                                                                     double* __restrict__ partials) {
#pragma clang fp contract(off)
    double s1 = 0.0, s0 = 0.0;
    for (long long c = (long long)blockIdx.x * CI_THREADS + threadIdx.x; c < nchunks; c += (long long)CI_BLOCKS * CI_THREADS) {
        const bf8_t a = *(const bf8_t*)(h + c * 8);
        const bf8_t b = *(const bf8_t*)(h_prev + c * 8);
        float fa[8], fb[8];
        unpack8(a, fa);
        unpack8(b, fb);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double da = (double)fa[i], db = (double)fb[i];
            s1 += fabs(da - db);
            s0 += fabs(db);
        }
        *(bf8_t*)(h_prev + c * 8) = a;
    }
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off); s0 += __shfl_down(s0, off); }
    __shared__ double red[CI_THREADS / 64][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave][0] = s1; red[wave][1] = s0; }
    __syncthreads();
    if (threadIdx.x < 2) {
        double v = red[0][threadIdx.x];
        for (int k = 1; k < CI_THREADS / 64; ++k) v += red[k][threadIdx.x];
        partials[2 * blockIdx.x + threadIdx.x] = v;
    }
}

// One wave: lane l adds the partials of blocks l * (CI_BLOCKS / 64) .. in index order, then the lanes as above.  sums[0] = S1, sums[1] = S0
__global__ __launch_bounds__(64) void cache_indicator_finish_kernel(const double* __restrict__ partials, double* __restrict__ sums) {
#pragma clang fp contract(off)
    constexpr int PER = CI_BLOCKS / 64;
    double s1 = 0.0, s0 = 0.0;
    for (int k = 0; k < PER; ++k) {
        s1 += partials[2 * ((int)threadIdx.x * PER + k)];
        s0 += partials[2 * ((int)threadIdx.x * PER + k) + 1];
    }
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off); s0 += __shfl_down(s0, off); }
    if (threadIdx.x == 0) { sums[0] = s1; sums[1] = s0; }
}

// r = bfr(x_L - x_0): fp32 from the bf16 words, one rounding
__global__ __launch_bounds__(CI_THREADS) void cache_residual_store_kernel(const u16* __restrict__ xl, const u16* __restrict__ x0, u16* __restrict__ r,
                                                                          long long nchunks) {
    for (long long c = (long long)blockIdx.x * CI_THREADS + threadIdx.x; c < nchunks; c += (long long)gridDim.x * CI_THREADS) {
        const bf8_t a = *(const bf8_t*)(xl + c * 8);
        const bf8_t b = *(const bf8_t*)(x0 + c * 8);
        float fa[8], fb[8];
        unpack8(a, fa);
        unpack8(b, fb);
#pragma unroll
        for (int i = 0; i < 8; ++i) fa[i] = fa[i] - fb[i];
        *(bf8_t*)(r + c * 8) = pack8(fa);
    }
}

}  // namespace

int launch_cache_indicator(const u16* h, u16* h_prev, long long n, double* partials, double* sums, hipStream_t stream) {
    LT_REQUIRE(h && h_prev && partials && sums, "cache_indicator: null argument");
    LT_REQUIRE(n > 0 && n % 8 == 0, "cache_indicator: %lld words are not a positive count of whole 16-byte chunks", n);
    hipLaunchKernelGGL(cache_indicator_kernel, dim3(CI_BLOCKS), dim3(CI_THREADS), 0, stream, h, h_prev, n / 8, partials);
    LT_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(cache_indicator_finish_kernel, dim3(1), dim3(64), 0, stream, partials, sums);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_cache_residual_store(const u16* xl, const u16* x0, u16* r, long long n, hipStream_t stream) {
    LT_REQUIRE(xl && x0 && r, "cache_residual_store: null argument");
    LT_REQUIRE(n > 0 && n % 8 == 0, "cache_residual_store: %lld words are not a positive count of whole 16-byte chunks", n);
    hipLaunchKernelGGL(cache_residual_store_kernel, dim3(CI_BLOCKS), dim3(CI_THREADS), 0, stream, xl, x0, r, n / 8);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_cache_residual_apply(u16* x, const u16* r, const u16* scale, const u16* shift, int ld_mod, u16* h, int rows, int rows_per_batch, int d,
                                hipStream_t stream) {
    LT_REQUIRE(x && r && scale && h, "cache_residual_apply: null argument");
    GatedResArgs g;
    g.x = x; g.y = r; g.post_w = nullptr; g.gate = nullptr; g.post_mode = 0; g.gate_mode = 2;  // no post-norm, no gate: x <- bfr(x + r)
    g.next_w = nullptr; g.next_scale = scale; g.next_shift = shift; g.next_mode = 2; g.h = h;
    g.rows = rows; g.rows_per_batch = rows_per_batch; g.d = d; g.ld_mod = ld_mod; g.eps = 1e-6f; g.eps_next = 1e-6f; g.scale_pre = 1;
    return launch_gated_residual_norm(g, stream);
}

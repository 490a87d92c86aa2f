// Smoothed-energy guidance: a separable 2-D blur of the post-RoPE query image q[B, H, N = Hp * grid_w, hd] over the token grid, into
// a second buffer of the same shape.  Per (b, h, channel), image columns 0 .. blur_w - 1 (the columns from blur_w on - Flag-DiT's end-of-line
// token - are copied word for word and are nobody's neighbour):
//   mode 0 (taps)  a[y][x]   = sum_{k = -r..r} w[k] * q[y][refl(x + k)]     fp32, one fused multiply-add per tap from k = -r upward, from 0.f
//                  out[y][x] = RN_bf16(sum_{k = -r..r} w[k] * a[refl(y + k)][x])  the same over y on the fp32 a; ONE rounding to bf16
//                  refl: reflection without repeating the edge (-i -> i, n - 1 + i -> n - 1 - i), which needs r <= n - 1
//   mode 1 (mean)  out[y][x] = RN_bf16(S / n), S = the sum of the n = Hp * blur_w words in float64, the quotient rounded ONCE to bf16
// The definition is transport/guidance.py: sample_cfg_seg (tests/exact_seg.py restates the arithmetic in float64).
#include <cmath>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int QB_TW = 16;       // columns of a tile
constexpr int QB_SR = 32;       // output rows of a strip; the strip's fp32 image has 2 r halo rows more
constexpr int QB_THREADS = 256;
constexpr int QB_GRID_CAP = 1024;  // (capped at four blocks per CU of 256 CUs: the loop strides)
constexpr int QB_TAPS = 2 * LT_SEG_MAX_RADIUS + 1;

__device__ __forceinline__ int refl(int i, int n) { return i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i; }

// A work item is (b * H + h, 8-channel chunk, strip of QB_SR rows, tile of QB_TW columns).  A head's image need not fit in LDS: the item holds
// the horizontal pass of its strip + halo, (rows + 2 r) x QB_TW x 8 fp32 (at most 94 x 16 x 32 B = 47 KB), behind the 64 tap words.
// Phase 1 reads the queries straight from global memory (16-byte accesses, the 2 r + 1 neighbours of a position are its row's next chunks);
// phase 2 reads the fp32 image and writes 16 bytes per position.  A thread owns all 8 channels of a position: no cross-lane traffic.
__global__ __launch_bounds__(QB_THREADS) void query_blur_taps_kernel(const u16* __restrict__ q, u16* __restrict__ out, const float* __restrict__ taps,
                                                                     int BH, int N, int hd, int grid_w, int blur_w, int Hp, int r, int tiles_x,
                                                                     int tiles_y, long long items) {
    extern __shared__ __attribute__((aligned(16))) char qb_smem[];
    float* w = (float*)qb_smem;               // 64 words (2 r + 1 used)
    float* a = (float*)(qb_smem + 64 * 4);    // [rows + 2 r][QB_TW][8]
    const int tid = threadIdx.x, cpr = hd >> 3, nt = 2 * r + 1;
    if (tid < 64) w[tid] = tid < nt ? taps[tid] : 0.f;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        long long rest = it;
        const int tx = (int)(rest % tiles_x); rest /= tiles_x;
        const int ty = (int)(rest % tiles_y); rest /= tiles_y;
        const int c8 = (int)(rest % cpr);
        const long long bh = rest / cpr;
        const int x0 = tx * QB_TW, y0 = ty * QB_SR;
        const int rows = min(QB_SR, Hp - y0), cols = min(QB_TW, grid_w - x0);
        const u16* src = q + ((size_t)bh * N) * hd + c8 * 8;
        u16* dst = out + ((size_t)bh * N) * hd + c8 * 8;
        __syncthreads();  // (the taps are in place; the previous item's phase 2 has read its image)
        for (int p = tid; p < (rows + 2 * r) * QB_TW; p += QB_THREADS) {
            const int yy = p / QB_TW, xx = p - yy * QB_TW, x = x0 + xx;
            if (x >= blur_w) continue;
            const int y = refl(y0 - r + yy, Hp);
            const u16* row = src + (size_t)y * grid_w * hd;
            float acc[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = 0.f;
            for (int k = 0; k < nt; ++k) {
                const bf8_t v = *(const bf8_t*)(row + (size_t)refl(x - r + k, blur_w) * hd);
                float f[8];
                unpack8(v, f);
                const float wk = w[k];
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[c] = __fmaf_rn(wk, f[c], acc[c]);
            }
            float* ap = a + (size_t)p * 8;
            *(f32x4*)ap = f32x4{acc[0], acc[1], acc[2], acc[3]};
            *(f32x4*)(ap + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
        }
        __syncthreads();
        for (int p = tid; p < rows * QB_TW; p += QB_THREADS) {
            const int yy = p / QB_TW, xx = p - yy * QB_TW, x = x0 + xx;
            if (xx >= cols) continue;
            const size_t o = ((size_t)(y0 + yy) * grid_w + x) * hd;
            if (x >= blur_w) { *(bf8_t*)(dst + o) = *(const bf8_t*)(src + o); continue; }  // end-of-line column: the words as they are
            float acc[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = 0.f;
            for (int k = 0; k < nt; ++k) {
                // (row yy + k of the strip's image is grid row refl(y0 + yy - r + k): phase 1 filled it by that rule)
                const float* ap = a + ((size_t)(yy + k) * QB_TW + xx) * 8;
                const f32x4 lo = *(const f32x4*)ap, hi = *(const f32x4*)(ap + 4);
                const float wk = w[k];
#pragma unroll
                for (int c = 0; c < 4; ++c) { acc[c] = __fmaf_rn(wk, lo[c], acc[c]); acc[4 + c] = __fmaf_rn(wk, hi[c], acc[4 + c]); }
            }
            *(bf8_t*)(dst + o) = pack8(acc);
        }
    }
}

// double -> bf16 with ONE rounding to nearest even: the float nearest to zero of the two that enclose d, its last bit set where d is not a
// float (round to odd; a float has 16 bits more than a bf16, so the sticky bit never meets the rounding position), then RN to bf16
__device__ __forceinline__ u16 d2bf(double d) {
    float f = (float)d;
    if ((double)f != d) {
        unsigned u = __float_as_uint(f);
        if (fabs((double)f) > fabs(d)) u -= 1;  // (same sign, not zero: one step towards zero)
        f = __uint_as_float(u | 1u);
    }
    return f2bf(f);
}

// mode 1: a work item is (b * H + h, 8-channel chunk).  Every thread sums its positions (p = tid, tid + 256, ...) in float64, the block adds the
// 256 partial sums in a fixed tree - a fixed order; and the sum is exact anyway - and every thread writes the mean to its positions.
__global__ __launch_bounds__(QB_THREADS) void query_blur_mean_kernel(const u16* __restrict__ q, u16* __restrict__ out, int N, int hd, int grid_w,
                                                                     int blur_w, int Hp, long long items) {
    __shared__ double part[QB_THREADS][8];
    const int tid = threadIdx.x, cpr = hd >> 3, n = Hp * blur_w;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int c8 = (int)(it % cpr);
        const long long bh = it / cpr;
        const u16* src = q + ((size_t)bh * N) * hd + c8 * 8;
        u16* dst = out + ((size_t)bh * N) * hd + c8 * 8;
        double acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = 0.0;
        for (int p = tid; p < n; p += QB_THREADS) {
            const int y = p / blur_w, x = p - y * blur_w;
            const bf8_t v = *(const bf8_t*)(src + ((size_t)y * grid_w + x) * hd);
            float f[8];
            unpack8(v, f);
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] += (double)f[c];
        }
        __syncthreads();  // (the previous item's mean has been read)
#pragma unroll
        for (int c = 0; c < 8; ++c) part[tid][c] = acc[c];
        __syncthreads();
        for (int half = QB_THREADS / 2; half >= 8; half >>= 1) {  // 256 x 8 -> 8 x 8: thread t adds (row t / 8 + half', channel t % 8)
            for (int i = tid; i < half * 8; i += QB_THREADS) part[i >> 3][i & 7] += part[(i >> 3) + half][i & 7];
            __syncthreads();
        }
        if (tid < 8) {
            double s = part[0][tid];
            for (int j = 1; j < 8; ++j) s += part[j][tid];
            part[0][tid] = s;
        }
        __syncthreads();
        bf8_t m;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            m.w[c] = (unsigned)d2bf(part[0][2 * c] / (double)n) | ((unsigned)d2bf(part[0][2 * c + 1] / (double)n) << 16);
        for (int p = tid; p < Hp * grid_w; p += QB_THREADS) {
            const int x = p % grid_w;
            const size_t o = (size_t)p * hd;
            *(bf8_t*)(dst + o) = x < blur_w ? m : *(const bf8_t*)(src + o);
        }
    }
}

}  // namespace

int seg_taps_host(float sigma, float* taps, int* radius, int* mode) {
#pragma clang fp contract(off)
    if (!(sigma > 0.f)) return 1;
    if (std::isinf(sigma)) { *radius = 0; *mode = 1; return 0; }
    const double sg = (double)sigma;
    const double r3 = std::ceil(3.0 * sg);
    const int r = r3 < (double)LT_SEG_MAX_RADIUS ? (int)r3 : LT_SEG_MAX_RADIUS;
    const double den = 2.0 * sg * sg;
    double g[QB_TAPS], sum = 0.0;
    for (int k = -r; k <= r; ++k) {
        g[k + r] = std::exp(-(double)(k * k) / den);
        sum += g[k + r];
    }
    for (int i = 0; i < 2 * r + 1; ++i) taps[i] = (float)(g[i] / sum);
    *radius = r; *mode = 0;
    return 0;
}

int launch_query_blur(const u16* q, u16* out, const float* taps, int B, int H, int N, int hd, int grid_w, int blur_w, int radius, int mode,
                      hipStream_t stream) {
    LT_REQUIRE(q && out && (mode == 1 || taps), "query_blur: null argument");
    LT_REQUIRE(mode == 0 || mode == 1, "query_blur: mode %d is neither 0 (taps) nor 1 (mean)", mode);
    LT_REQUIRE(B > 0 && H > 0 && N > 0 && grid_w > 0, "query_blur: bad shape B=%d H=%d N=%d grid_w=%d", B, H, N, grid_w);
    LT_REQUIRE(hd == 48 || hd == 72 || hd == 96 || hd == 128, "query_blur: head_dim %d not built (48, 72, 96, 128)", hd);
    LT_REQUIRE(N % grid_w == 0, "query_blur: N=%d is not a whole number of grid rows of grid_w=%d tokens", N, grid_w);
    LT_REQUIRE(blur_w >= 1 && blur_w <= grid_w, "query_blur: blur_w=%d outside 1..grid_w=%d", blur_w, grid_w);
    LT_REQUIRE(radius >= 0 && radius <= LT_SEG_MAX_RADIUS, "query_blur: radius %d outside 0..%d", radius, LT_SEG_MAX_RADIUS);
    const int Hp = N / grid_w;
    LT_REQUIRE(mode == 1 || radius < (Hp < blur_w ? Hp : blur_w), "query_blur: radius %d cannot be reflected on a grid of %d x %d image tokens "
               "(r <= min(Hp, blur_w) - 1)", radius, Hp, blur_w);
    LT_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)out & 15) == 0 && (mode == 1 || ((uintptr_t)taps & 3) == 0),
               "query_blur: pointer not aligned (q, out: 16 bytes; taps: 4)");
    LT_REQUIRE(q != out, "query_blur: q == out (the blur is not computed in place)");
    const long long bhc = (long long)B * H * (hd / 8);
    if (mode == 1) {
        const long long g = bhc < QB_GRID_CAP ? bhc : QB_GRID_CAP;
        hipLaunchKernelGGL(query_blur_mean_kernel, dim3((unsigned)g), dim3(QB_THREADS), 0, stream, q, out, N, hd, grid_w, blur_w, Hp, bhc);
    } else {
        const int tiles_x = (grid_w + QB_TW - 1) / QB_TW, tiles_y = (Hp + QB_SR - 1) / QB_SR;
        const long long items = bhc * tiles_x * tiles_y;
        const long long g = items < QB_GRID_CAP ? items : QB_GRID_CAP;
        const int rows = Hp < QB_SR ? Hp : QB_SR;
        const size_t lds = 64 * 4 + (size_t)(rows + 2 * radius) * QB_TW * 8 * 4;  // <= 48384 bytes
        hipLaunchKernelGGL(query_blur_taps_kernel, dim3((unsigned)g), dim3(QB_THREADS), lds, stream, q, out, taps, B * H, N, hd, grid_w, blur_w, Hp,
                           radius, tiles_x, tiles_y, items);
    }
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

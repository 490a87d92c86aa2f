// Tiled (MultiDiffusion, Bar-Tal et al. 2023) sampling: the three kernels around the model evaluations of lt_forward_tiled / lt_sample_ode_tiled
// (transport/tiled.py is the definition).
//
// A window is DATA: an offset (top, left) in latent pixels into the ONE canvas latent [C, Hc, Wc]; all n windows have one size h x w.  The table
// (WindowTable, kernels.h: at most LT_WINDOWS_MAX = 64 windows) travels as a kernel argument, so there is no device table to keep in step.
//   gather:  out[k][c][i][j] = y[c][top_k + i][left_k + j]                                      a pure copy, rows 0 .. n-1 of the model's 2 n
//   cover:   wsum[p]         = sum_{k = 0 .. n-1, window k holds p} weight[i][j]                  fp32, from +0, in window order
//   reduce:  v[c][p]         = R((sum_{k = 0 .. n-1, window k holds p} weight[i][j] * f[k][c][i][j]) / wsum[p])
//
// Rounding points (R = round to the state dtype, bf16 or none at fp32), all read off transport/tiled.py: fuse - every product weight * f is ONE
// fp32 multiplication, rounded before it is added (no fma: contraction is off), the sum is fp32 from +0 in the order k = 0 .. n-1 over the
// windows that hold the pixel (the windows that do not hold it add nothing in the definition either: their slice assignment does not touch
// it), the division by the stored wsum is ONE correctly rounded fp32 division, and R is applied once to its result.  The copy is exact.
//
// Access pattern: every thread owns ONE group of G consecutive pixels of one row - of one (window, channel) row in the gather, of one
// (channel, canvas row) in the reduce; of one pixel in the cover, which runs once per table.  G is the widest of 4 / 2 / 1 that divides the
// window width, the canvas width and every left offset, and for which the buffers are aligned (launchers below): a group then lies in a
// window whole or not at all, and leaves as one 4- / 8- / 16-byte access.  Offsets and sizes are multiples of the patch size (2 in every
// model of the reference), so G = 2 - one patch row - always holds under lt_set_windows, and G = 4 at the usual sizes.  The reduce
// walks the n <= 64 windows in a uniform loop whose trip count and bounds sit in scalar registers; it reads a pixel once per window that
// holds it.
//
// These launches are latency-bound at the sizes in scope (a canvas of C x Hc x Wc <= a few hundred KB stays in L2; n x C x h x w words move
// once per stage, next to a model evaluation of 2 n rows): nothing here was tuned against a measurement, and the mapping is the plain one.
//
// No table content can make a kernel address outside its buffers: every launcher checks the table on the host first (window_table_build:
// 1 <= n <= 64, every window inside the canvas), and the reduce / cover kernels address a window's row only behind the same bounds test
// that decides whether the window holds the pixel.
#include <cstdint>

#include "common.h"
#include "group_io.h"
#include "kernels.h"

namespace {

// out[k][c][i][j .. j+G) = y[c][top_k + i][left_k + j ..)
template <bool BF, int G>
__global__ void windows_gather_kernel(const void* __restrict__ y, void* __restrict__ out, WindowTable t, int C) {
    using U = typename Unit<(BF ? 2 : 4) * G>::type;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int qw = t.win_w / G;
    if (tid >= (long long)t.n * C * t.win_h * qw) return;
    const int j = (int)(tid % qw) * G, i = (int)((tid / qw) % t.win_h);
    const long long kc = tid / ((long long)qw * t.win_h);
    const int c = (int)(kc % C), k = (int)(kc / C);
    const long long src = ((long long)c * t.canvas_h + t.off[2 * k] + i) * t.canvas_w + t.off[2 * k + 1] + j;
    const long long dst = (kc * t.win_h + i) * t.win_w + j;
    ((U*)out)[dst / G] = ((const U*)y)[src / G];
}

// wsum[p] and the count of pixels whose sum is not finite and strictly positive
__global__ void windows_cover_kernel(const float* __restrict__ weight, float* __restrict__ wsum, int* __restrict__ bad, WindowTable t) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= t.canvas_h * t.canvas_w) return;
    const int x = p % t.canvas_w, yy = p / t.canvas_w;
    float s = 0.f;
    for (int k = 0; k < t.n; ++k) {
        const int i = yy - t.off[2 * k], j = x - t.off[2 * k + 1];
        if (i < 0 || i >= t.win_h || j < 0 || j >= t.win_w) continue;
        s = s + (weight ? weight[i * t.win_w + j] : 1.f);
    }
    wsum[p] = s;
    if (!(s > 0.f && s < INFINITY)) atomicAdd(bad, 1);
}

// v[c][y][x .. x+G) = R((sum_k weight[i][j] * f[k][c][i][j]) / wsum[y][x])
template <bool BF, int G>
__global__ void windows_reduce_kernel(const void* __restrict__ f, const float* __restrict__ weight, const float* __restrict__ wsum,
                                      void* __restrict__ out, WindowTable t, int C) {
#pragma clang fp contract(off)  // the product rounds before the sum, as the two tensor operations of fuse do: no fma
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int qw = t.canvas_w / G;
    if (tid >= (long long)C * t.canvas_h * qw) return;
    const int x = (int)(tid % qw) * G, yy = (int)((tid / qw) % t.canvas_h), c = (int)(tid / ((long long)qw * t.canvas_h));
    float acc[G];
#pragma unroll
    for (int u = 0; u < G; ++u) acc[u] = 0.f;
    for (int k = 0; k < t.n; ++k) {
        const int i = yy - t.off[2 * k], j = x - t.off[2 * k + 1];
        if (i < 0 || i >= t.win_h || j < 0 || j + G > t.win_w) continue;  // (x, the lefts and the width are multiples of G: whole or not at all)
        float fv[G];
        ldg<BF, G>(f, (((long long)k * C + c) * t.win_h + i) * t.win_w + j, fv);
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const float prod = (weight ? weight[i * t.win_w + j + u] : 1.f) * fv[u];
            acc[u] = acc[u] + prod;
        }
    }
    const long long o = ((long long)c * t.canvas_h + yy) * t.canvas_w + x;
    float v[G];
#pragma unroll
    for (int u = 0; u < G; ++u) v[u] = acc[u] / wsum[(long long)yy * t.canvas_w + x + u];
    stg<BF, G>(out, o, v);
}

inline int nblk(long long n, int bs) { return (int)((n + bs - 1) / bs); }

// the widest group the table and the two buffers allow
int group_of(const WindowTable& t, const void* a, const void* b, int elem_bytes) {
    int g = 4;
    auto fits = [&](int v) { while (g > 1 && v % g) g >>= 1; };
    fits(t.win_w); fits(t.canvas_w);
    for (int k = 0; k < t.n; ++k) fits(t.off[2 * k + 1]);
    while (g > 1 && (((uintptr_t)a | (uintptr_t)b) % (size_t)(g * elem_bytes))) g >>= 1;
    return g;
}

}  // namespace

int window_table_build(const char* who, const int32_t* offsets_host, int n, int win_h, int win_w, int canvas_h, int canvas_w, WindowTable* out) {
    LT_REQUIRE(offsets_host && out, "%s: null argument", who);
    LT_REQUIRE(n >= 1 && n <= LT_WINDOWS_MAX, "%s: %d windows (1 .. %d)", who, n, LT_WINDOWS_MAX);
    LT_REQUIRE(win_h >= 1 && win_w >= 1 && canvas_h >= win_h && canvas_w >= win_w && (long long)canvas_h * canvas_w <= 0x7fffffffLL / 64,
               "%s: a window of %dx%d on a canvas of %dx%d (need 1 <= window <= canvas)", who, win_h, win_w, canvas_h, canvas_w);
    for (int k = 0; k < n; ++k) {
        const int top = offsets_host[2 * k], left = offsets_host[2 * k + 1];
        LT_REQUIRE(top >= 0 && left >= 0 && top <= canvas_h - win_h && left <= canvas_w - win_w,
                   "%s: window %d at (%d, %d) of size %dx%d lies outside the canvas %dx%d", who, k, top, left, win_h, win_w, canvas_h, canvas_w);
    }
    out->n = n; out->win_h = win_h; out->win_w = win_w; out->canvas_h = canvas_h; out->canvas_w = canvas_w;
    for (int k = 0; k < 2 * LT_WINDOWS_MAX; ++k) out->off[k] = k < 2 * n ? offsets_host[k] : 0;
    return 0;
}

int launch_windows_gather(const void* y, const WindowTable& t, void* out, int C, int dtype, hipStream_t stream) {
    LT_REQUIRE(y && out, "windows_gather: null argument");
    LT_REQUIRE(dtype == 0 || dtype == 1, "windows_gather: state dtype must be f32 or bf16");
    LT_REQUIRE(C >= 1, "windows_gather: C %d", C);
    WindowTable chk;
    if (window_table_build("windows_gather", t.off, t.n, t.win_h, t.win_w, t.canvas_h, t.canvas_w, &chk)) return 2;
    const int g = group_of(t, y, out, dtype == 1 ? 2 : 4);
    const long long n = (long long)t.n * C * t.win_h * (t.win_w / g);
#define LT_GATHER(BF, G) hipLaunchKernelGGL((windows_gather_kernel<BF, G>), dim3(nblk(n, 256)), dim3(256), 0, stream, y, out, t, C)
    if (dtype == 1) { if (g == 4) LT_GATHER(true, 4); else if (g == 2) LT_GATHER(true, 2); else LT_GATHER(true, 1); }
    else { if (g == 4) LT_GATHER(false, 4); else if (g == 2) LT_GATHER(false, 2); else LT_GATHER(false, 1); }
#undef LT_GATHER
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_windows_cover(const WindowTable& t, const float* weight, float* wsum, int* bad, hipStream_t stream) {
    LT_REQUIRE(wsum && bad, "windows_cover: null argument");
    WindowTable chk;
    if (window_table_build("windows_cover", t.off, t.n, t.win_h, t.win_w, t.canvas_h, t.canvas_w, &chk)) return 2;
    LT_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(int), stream));
    hipLaunchKernelGGL(windows_cover_kernel, dim3(nblk((long long)t.canvas_h * t.canvas_w, 256)), dim3(256), 0, stream, weight, wsum, bad, t);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_windows_reduce(const void* f, const WindowTable& t, const float* weight, const float* wsum, void* out, int C, int dtype,
                          hipStream_t stream) {
    LT_REQUIRE(f && wsum && out, "windows_reduce: null argument");
    LT_REQUIRE(dtype == 0 || dtype == 1, "windows_reduce: state dtype must be f32 or bf16");
    LT_REQUIRE(C >= 1, "windows_reduce: C %d", C);
    WindowTable chk;
    if (window_table_build("windows_reduce", t.off, t.n, t.win_h, t.win_w, t.canvas_h, t.canvas_w, &chk)) return 2;
    const int g = group_of(t, f, out, dtype == 1 ? 2 : 4);
    const long long n = (long long)C * t.canvas_h * (t.canvas_w / g);
#define LT_REDUCE(BF, G) hipLaunchKernelGGL((windows_reduce_kernel<BF, G>), dim3(nblk(n, 256)), dim3(256), 0, stream, f, weight, wsum, out, t, C)
    if (dtype == 1) { if (g == 4) LT_REDUCE(true, 4); else if (g == 2) LT_REDUCE(true, 2); else LT_REDUCE(true, 1); }
    else { if (g == 4) LT_REDUCE(false, 4); else if (g == 2) LT_REDUCE(false, 2); else LT_REDUCE(false, 1); }
#undef LT_REDUCE
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

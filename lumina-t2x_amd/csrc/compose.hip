// Composed guidance (Composable Diffusion, Liu et al. 2022): the two kernels around the one model evaluation of lt_forward_compose and of every
// stage of lt_sample_ode_compose (transport/guidance.py: guided_compose / sample_cfg_compose are the definition).
//
// The state has B' rows.  An evaluation is a plain forward of (K + 1) B' rows: rows k B' + b carry prompt k of image b (k = 0 .. K-1), rows
// K B' + b the base (negative / empty) prompt.  With n = B' C H W elements per row group:
//   replicate:  out[r n + i] = y[i]                  r = 0 .. K             an exact copy of the state under every prompt
//   guidance:   channels <  ch:  acc = R(w_1 R(c_1 - u));  acc = R(acc + R(w_k R(c_k - u)))  k = 2 .. K, in this order;  g = R(u + acc)
//               channels >= ch:  g = c_1                                    (the reference's cfg_channels = 3 quirk: prompt 1's row, copied)
//
// Rounding points: R rounds to bf16 - the model's output dtype WHATEVER the state dtype (an fp32 state's words hold bf16 values, as
// unpatchify_cfg_kernel leaves them) - and every difference, product and sum is one fp32 operation that rounds on its own: contraction is
// off.  At K = 1 the chain is R(u + R(w R(c - u))), lt_forward_cfg's word for word.
//
// Access pattern: every thread owns ONE group of G consecutive elements of one (image, channel) row; G is the widest of 4 / 2 / 1 that divides
// H W and to which both buffers are aligned (launchers below), so a group is one 2- .. 16-byte access each way (group_io.h) and lies in one
// channel whole.  The K weights travel as a kernel argument; the loop over k has a uniform trip count K <= LT_COMPOSE_MAX = 7.
//
// Both launches are latency-bound at every size in scope: (K + 2) B' C H W words move once - a few hundred KB, resident in L2 - next to a
// model evaluation of (K + 1) B' rows.  Nothing here was tuned against a measurement; the mapping is the plain one.
//
// No argument can make a kernel address outside its buffers: the launchers check the counts on the host, the grid covers exactly the
// n / G groups of one row group, and a thread addresses the same in-group offset of row groups 0 .. K only.
#include <cmath>
#include <cstdint>

#include "common.h"
#include "group_io.h"
#include "kernels.h"

namespace {

// out[r n + i .. i+G) = y[i ..), r = 0 .. K
template <bool BF, int G>
__global__ void compose_replicate_kernel(const void* __restrict__ y, void* __restrict__ out, long long n, int K) {
    using U = typename Unit<(BF ? 2 : 4) * G>::type;
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n / G) return;
    const U v = ((const U*)y)[q];
    for (int r = 0; r <= K; ++r) ((U*)out)[r * (n / G) + q] = v;
}

// g[b][c][j .. j+G) of the chain above; f [(K+1) B', C, HW], out [B', C, HW]
template <bool BF, int G>
__global__ void compose_guidance_kernel(const void* __restrict__ f, void* __restrict__ out, ComposeWeights w, int K, long long n, int C, int HW,
                                        int ch) {
#pragma clang fp contract(off)  // every step of the chain rounds on its own, as the tensor expression does: no fma
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n / G) return;
    const int per_row = HW / G;
    const int c = (int)((q / per_row) % C);
    const long long o = q * G;  // (HW % G == 0: the group lies in one (image, channel) row)
    float g[G];
    ldg<BF, G>(f, o, g);  // prompt 1's row
    if (c < ch) {
        float u[G], acc[G];
        ldg<BF, G>(f, (long long)K * n + o, u);
#pragma unroll
        for (int i = 0; i < G; ++i) acc[i] = bfr(w.w[0] * bfr(g[i] - u[i]));
        for (int k = 1; k < K; ++k) {
            float cv[G];
            ldg<BF, G>(f, (long long)k * n + o, cv);
#pragma unroll
            for (int i = 0; i < G; ++i) acc[i] = bfr(acc[i] + bfr(w.w[k] * bfr(cv[i] - u[i])));
        }
#pragma unroll
        for (int i = 0; i < G; ++i) g[i] = bfr(u[i] + acc[i]);
    }
    stg<BF, G>(out, o, g);
}

inline int nblk(long long n, int bs) { return (int)((n + bs - 1) / bs); }

// the widest group H W and the two buffers allow
int group_of(int HW, const void* a, const void* b, int elem_bytes) {
    int g = 4;
    while (g > 1 && (HW % g || (((uintptr_t)a | (uintptr_t)b) % (size_t)(g * elem_bytes)))) g >>= 1;
    return g;
}

// what both launchers refuse of the shape; n = B' C H W
int check_compose_shape(const char* who, int K, int Bp, int C, int HW, int dtype, long long* n) {
    LT_REQUIRE(dtype == 0 || dtype == 1, "%s: state dtype %d is not 0 (f32) or 1 (bf16)", who, dtype);
    LT_REQUIRE(K >= 1 && K <= LT_COMPOSE_MAX, "%s: K = %d prompts (1 .. %d)", who, K, LT_COMPOSE_MAX);
    LT_REQUIRE(Bp >= 1 && C >= 1 && HW >= 1, "%s: B' = %d, C = %d, H W = %d (each must be at least 1)", who, Bp, C, HW);
    *n = (long long)Bp * C * HW;
    LT_REQUIRE(*n <= 0x7fffffffLL / (LT_COMPOSE_MAX + 1), "%s: %lld elements per row group exceed %lld", who, *n, 0x7fffffffLL / (LT_COMPOSE_MAX + 1));
    return 0;
}

}  // namespace

int launch_compose_replicate(const void* y, void* out, int K, int Bp, int C, int HW, int dtype, hipStream_t stream) {
    LT_REQUIRE(y && out, "compose_replicate: null argument");
    long long n;
    if (check_compose_shape("compose_replicate", K, Bp, C, HW, dtype, &n)) return 2;
    const int eb = dtype == 1 ? 2 : 4, g = group_of(HW, y, out, eb);
    const char *lo = (const char*)out, *hi = lo + (K + 1) * n * eb;
    LT_REQUIRE((const char*)y + n * eb <= lo || (const char*)y >= hi, "compose_replicate: y lies inside the %d row groups it is copied to", K + 1);
#define LT_REPLICATE(BF, G) hipLaunchKernelGGL((compose_replicate_kernel<BF, G>), dim3(nblk(n / G, 256)), dim3(256), 0, stream, y, out, n, K)
    if (dtype == 1) { if (g == 4) LT_REPLICATE(true, 4); else if (g == 2) LT_REPLICATE(true, 2); else LT_REPLICATE(true, 1); }
    else { if (g == 4) LT_REPLICATE(false, 4); else if (g == 2) LT_REPLICATE(false, 2); else LT_REPLICATE(false, 1); }
#undef LT_REPLICATE
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_compose_guidance(const void* f, void* out, const float* w_host, int K, int Bp, int C, int HW, int ch, int dtype, hipStream_t stream) {
    LT_REQUIRE(f && out && w_host, "compose_guidance: null argument");
    long long n;
    if (check_compose_shape("compose_guidance", K, Bp, C, HW, dtype, &n)) return 2;
    LT_REQUIRE(ch >= 1 && ch <= C, "compose_guidance: cfg_channels %d outside 1..%d", ch, C);
    ComposeWeights w = {};
    for (int k = 0; k < K; ++k) {
        LT_REQUIRE(std::isfinite(w_host[k]), "compose_guidance: the weight of prompt %d is not finite", k);
        w.w[k] = w_host[k];
    }
    const int eb = dtype == 1 ? 2 : 4, g = group_of(HW, f, out, eb);
    const char *lo = (const char*)f, *hi = lo + (K + 1) * n * eb;
    LT_REQUIRE((const char*)out + n * eb <= lo || (const char*)out >= hi, "compose_guidance: out lies inside the evaluation's %d row groups", K + 1);
#define LT_GUIDANCE(BF, G) \
    hipLaunchKernelGGL((compose_guidance_kernel<BF, G>), dim3(nblk(n / G, 256)), dim3(256), 0, stream, f, out, w, K, n, C, HW, ch)
    if (dtype == 1) { if (g == 4) LT_GUIDANCE(true, 4); else if (g == 2) LT_GUIDANCE(true, 2); else LT_GUIDANCE(true, 1); }
    else { if (g == 4) LT_GUIDANCE(false, 4); else if (g == 2) LT_GUIDANCE(false, 2); else LT_GUIDANCE(false, 1); }
#undef LT_GUIDANCE
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

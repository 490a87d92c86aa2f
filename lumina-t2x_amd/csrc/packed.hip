// Ragged boundary kernels of a packed (variable-resolution) batch: the list branch of NextDiT.patchify_and_embed / unpatchify
// (lumina_next_t2i/models/model.py:789-834, :757-768) on ONE flat state buffer, one launch each for all samples.
//
// State layout: the I/O dtype, sample b = [C, H_b, W_b] row-major at element offset sum_{j<b} C H_j W_j.
// Table (PackedTable, kernels.h): five rows of LT_PK_MAX ints - element offset, H_b, W_b, token count (H_b / p)(W_b / p), grid width
// W_b / p - built on the host by packed_table_build and written to device memory by ONE small launch per call (the table travels as a
// kernel argument: no host buffer to keep alive, nothing to synchronise on, safe under stream capture).  The token-count and grid-width
// rows are also what qk_norm_rope (QkPostArgs::n_tok_b / grid_w_b) and the attention key mask (AttnArgs::nk_batch) read.
//
// Token rows keep the padded layout of the rest of the evaluation: sample b owns rows b N .. b N + N - 1 with N the longest sequence.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "kernels.h"

namespace {

inline int nblk(long long n, int per) { return (int)((n + per - 1) / per); }

__global__ void packed_table_store_kernel(PackedTable t, int* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < LT_PK_ROWS * LT_PK_MAX) dst[i] = t.v[i];
}

// patchify_kernel (misc.hip) per sample: rows (i, j) of sample b at row b N + i Wp_b + j, columns (c, ph, pw), zero padded to kpad.
// dup_first_half: rows of sample b >= B / 2 read the pixels of sample b - B / 2 (combined = cat([half, half]), model.py:901-902).
__global__ void patchify_packed_kernel(const void* __restrict__ x, int x_dtype, u16* __restrict__ out, const int* __restrict__ tab, int B, int C,
                                       int patch, int kpad, int N, int dup_first_half) {
    const int b = blockIdx.y;
    const int bs = dup_first_half ? b % (B / 2) : b;
    const int off = tab[LT_PK_OFF * LT_PK_MAX + bs], H = tab[LT_PK_H * LT_PK_MAX + bs], W = tab[LT_PK_W * LT_PK_MAX + bs];
    const int ntok = tab[LT_PK_NTOK * LT_PK_MAX + b], Wp = tab[LT_PK_GW * LT_PK_MAX + b];
    const long long total = (long long)ntok * kpad;
    const int kreal = C * patch * patch;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i % kpad);
        const int row = (int)(i / kpad);
        u16 v = 0;
        if (k < kreal) {
            const int j = row % Wp, ii = row / Wp;
            const int c = k / (patch * patch), ph = (k / patch) % patch, pw = k % patch;
            const size_t idx = (size_t)off + ((size_t)c * H + (ii * patch + ph)) * W + (j * patch + pw);
            v = x_dtype == 0 ? f2bf(((const float*)x)[idx]) : ((const u16*)x)[idx];
        }
        out[((size_t)b * N + row) * kpad + k] = v;
    }
}

// rows ntok_b .. N - 1 of every sample = pad_token (model.py:811-817)
__global__ void fill_pad_packed_kernel(u16* __restrict__ x, const u16* __restrict__ pad, const int* __restrict__ tab, int N, int d) {
    const int b = blockIdx.y;
    const int ntok = tab[LT_PK_NTOK * LT_PK_MAX + b];
    const long long total = (long long)(N - ntok) * d;
    u16* dst = x + ((size_t)b * N + ntok) * d;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        dst[i] = pad[i % d];
}

// unpatchify_cfg_kernel (misc.hip) per sample, written to the flat layout: row layout (pH, pW, C_out), the first C channels kept (the
// sigma half dropped, model.py:859-864), guidance on the first cfg_channels channels with the bf16 rounding of each step (:908-913)
__global__ void unpatchify_packed_kernel(const u16* __restrict__ rows, int ld, void* __restrict__ out, int out_dtype, const int* __restrict__ tab,
                                         int B, int C, int out_ch, int patch, int N, int use_cfg, float cfg_scale, int cfg_channels) {
#pragma clang fp contract(off)  // every step of the guidance chain rounds on its own, as the tensor expression does
    const int b = blockIdx.y;
    const int off = tab[LT_PK_OFF * LT_PK_MAX + b], H = tab[LT_PK_H * LT_PK_MAX + b], W = tab[LT_PK_W * LT_PK_MAX + b];
    const int Wp = tab[LT_PK_GW * LT_PK_MAX + b];
    const int total = C * H * W;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int w = i % W;
        const int hh = (i / W) % H;
        const int c = i / (W * H);
        const int e = ((hh % patch) * patch + (w % patch)) * out_ch + c;
        const int tok = (hh / patch) * Wp + (w / patch);
        auto rd = [&](int bb) { return bf2f(rows[((size_t)bb * N + tok) * ld + e]); };
        float v;
        if (use_cfg && c < cfg_channels) {
            const int half = B / 2;
            const int bc = b % half;
            const float cond = rd(bc), unc = rd(bc + half);
            v = bfr(unc + bfr(cfg_scale * bfr(cond - unc)));
        } else {
            v = rd(b);
        }
        if (out_dtype == 0) ((float*)out)[(size_t)off + i] = v;
        else ((u16*)out)[(size_t)off + i] = f2bf(v);
    }
}

}  // namespace

int packed_table_build(const int32_t* hw, int B, int C, int patch, PackedTable* t, long long* elems, int* n_max, int* hp_max, int* wp_max) {
    LT_REQUIRE(hw && t, "packed table: null argument");
    LT_REQUIRE(B >= 1 && B <= LT_PK_MAX, "packed batch of %d samples outside 1..%d", B, LT_PK_MAX);
    LT_REQUIRE(C >= 1 && patch >= 1, "packed table: channels and patch size must be positive");
    memset(t, 0, sizeof(*t));
    long long off = 0;
    int nm = 0, hm = 0, wm = 0;
    for (int b = 0; b < B; ++b) {
        const int h = hw[2 * b], w = hw[2 * b + 1];
        LT_REQUIRE(h > 0 && w > 0 && h % patch == 0 && w % patch == 0, "packed sample %d: latent %dx%d is not a positive multiple of the patch size %d", b,
                   h, w, patch);
        LT_REQUIRE((long long)(h / patch) * (w / patch) < (1LL << 24), "packed sample %d: latent %dx%d is too large", b, h, w);
        t->v[LT_PK_OFF * LT_PK_MAX + b] = (int)off;
        t->v[LT_PK_H * LT_PK_MAX + b] = h;
        t->v[LT_PK_W * LT_PK_MAX + b] = w;
        t->v[LT_PK_NTOK * LT_PK_MAX + b] = (h / patch) * (w / patch);
        t->v[LT_PK_GW * LT_PK_MAX + b] = w / patch;
        nm = std::max(nm, (h / patch) * (w / patch)); hm = std::max(hm, h / patch); wm = std::max(wm, w / patch);
        off += (long long)C * h * w;
        LT_REQUIRE(off < (1LL << 31), "packed batch: the flat state exceeds 2^31 elements at sample %d", b);
    }
    if (elems) *elems = off;
    if (n_max) *n_max = nm;
    if (hp_max) *hp_max = hm;
    if (wp_max) *wp_max = wm;
    return 0;
}

int launch_packed_table_store(const PackedTable& t, int* tab_dev, hipStream_t stream) {
    LT_REQUIRE(tab_dev, "packed table: null device table");
    hipLaunchKernelGGL(packed_table_store_kernel, dim3(nblk(LT_PK_ROWS * LT_PK_MAX, 64)), dim3(64), 0, stream, t, tab_dev);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_patchify_packed(const void* x, int x_dtype, u16* out, const int* tab_dev, int B, int C, int patch, int kpad, int N, int dup_first_half,
                           hipStream_t stream) {
    LT_REQUIRE(x && out && tab_dev, "patchify_packed: null argument");
    LT_REQUIRE(B >= 1 && B <= LT_PK_MAX && N >= 1, "patchify_packed: batch %d outside 1..%d or no tokens", B, LT_PK_MAX);
    LT_REQUIRE(C * patch * patch <= kpad, "patchify_packed: kpad too small");
    LT_REQUIRE(!dup_first_half || B % 2 == 0, "patchify_packed: CFG needs an even batch");
    LT_REQUIRE(x_dtype == 0 || x_dtype == 1, "patchify_packed: state dtype must be f32 or bf16");
    const int g = std::min(nblk((long long)N * kpad, 256), 1024);
    hipLaunchKernelGGL(patchify_packed_kernel, dim3(g, B), dim3(256), 0, stream, x, x_dtype, out, tab_dev, B, C, patch, kpad, N, dup_first_half);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_fill_pad_packed(u16* x, const u16* pad_token, const int* tab_dev, int B, int N, int d, hipStream_t stream) {
    LT_REQUIRE(x && pad_token && tab_dev, "fill_pad_packed: null argument");
    LT_REQUIRE(B >= 1 && B <= LT_PK_MAX && N >= 1 && d >= 1, "fill_pad_packed: batch %d outside 1..%d or empty rows", B, LT_PK_MAX);
    const int g = std::min(nblk((long long)N * d, 256), 1024);
    hipLaunchKernelGGL(fill_pad_packed_kernel, dim3(g, B), dim3(256), 0, stream, x, pad_token, tab_dev, N, d);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_unpatchify_packed(const u16* rows, int ld, void* out, int out_dtype, const int* tab_dev, int B, int C, int out_ch, int patch, int N,
                             int use_cfg, float cfg_scale, int cfg_channels, hipStream_t stream) {
    LT_REQUIRE(rows && out && tab_dev, "unpatchify_packed: null argument");
    LT_REQUIRE(B >= 1 && B <= LT_PK_MAX && N >= 1, "unpatchify_packed: batch %d outside 1..%d or no tokens", B, LT_PK_MAX);
    LT_REQUIRE(!use_cfg || B % 2 == 0, "unpatchify_packed: CFG needs an even batch");
    LT_REQUIRE(C <= out_ch && patch * patch * out_ch <= ld, "unpatchify_packed: %d channels of %d do not fit rows of %d", C, out_ch, ld);
    LT_REQUIRE(out_dtype == 0 || out_dtype == 1, "unpatchify_packed: state dtype must be f32 or bf16");
    const int g = std::min(nblk((long long)C * N * patch * patch, 256), 1024);
    hipLaunchKernelGGL(unpatchify_packed_kernel, dim3(g, B), dim3(256), 0, stream, rows, ld, out, out_dtype, tab_dev, B, C, out_ch, patch, N, use_cfg,
                       cfg_scale, cfg_channels);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

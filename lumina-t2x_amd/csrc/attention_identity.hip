// Perturbed-attention guidance: self-attention with the attention map replaced by the identity.  Every query's output is its own
// value row, so the "attention" of a perturbed layer is a copy
//   out[b, n, h, :] = V[b, n, h / (H / Hkv), :]
// of the V columns of the row-major QKV projection into the [B * N][H * hd] buffer the O projection reads.  The words are copied: no rounding.
// The definition is transport/guidance.py: sample_cfg_pag.
#include "common.h"
#include "kernels.h"

namespace {

// One thread per 16-byte chunk (8 bf16 words) of the output, grid-stride.  A head's hd words are a whole number of chunks (hd % 8 == 0), so a
// chunk lies in one head; and a chunk starts at a column c % 8 == 0, so it lies in one 32-word (64-byte) piece of the pair layout
// (GemmArgs::pair_ab: element (r, c) of [rows][ld] at (r >> 1) * 2 * ld + (c >> 5) * 64 + (r & 1) * 32 + (c & 31)).
__global__ __launch_bounds__(256) void attention_identity_kernel(const u16* __restrict__ src, int ld_src, int col0, u16* __restrict__ out,
                                                                 long long rows, int H, int rep, int hd, int out_pair) {
    const int width = H * hd, cpr = width >> 3;
    const long long total = rows * cpr;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / cpr;
        const int c = (int)(i - r * cpr) << 3;
        const int h = c / hd;
        const uint4 v = *(const uint4*)(src + r * ld_src + col0 + (h / rep) * hd + (c - h * hd));
        const long long o = out_pair ? (r >> 1) * 2 * width + (c >> 5) * 64 + (r & 1) * 32 + (c & 31) : r * width + c;
        *(uint4*)(out + o) = v;
    }
}

}  // namespace

int launch_attention_identity(const u16* src, int ld_src, int col0, u16* out, int B, int N, int H, int Hkv, int hd, int out_pair, hipStream_t stream) {
    LT_REQUIRE(src && out, "attention_identity: null argument");
    LT_REQUIRE(B > 0 && N > 0 && H > 0 && Hkv > 0, "attention_identity: bad shape B=%d N=%d H=%d Hkv=%d", B, N, H, Hkv);
    LT_REQUIRE(H % Hkv == 0, "attention_identity: H=%d not a multiple of Hkv=%d", H, Hkv);
    LT_REQUIRE(hd == 48 || hd == 72 || hd == 96 || hd == 128, "attention_identity: head_dim %d not built (48, 72, 96, 128)", hd);
    LT_REQUIRE(col0 >= 0 && col0 % 8 == 0 && ld_src % 8 == 0 && col0 + Hkv * hd <= ld_src && ((uintptr_t)src & 15) == 0 && ((uintptr_t)out & 15) == 0,
               "attention_identity: 16-byte accesses need col0 %% 8 == 0, ld_src %% 8 == 0, aligned pointers and the V columns inside a row "
               "(col0 %d, %d columns, ld_src %d)", col0, Hkv * hd, ld_src);
    const long long rows = (long long)B * N;
    LT_REQUIRE(!out_pair || (rows % 2 == 0 && (H * hd) % 32 == 0), "attention_identity: out_pair needs an even row count and H * hd %% 32 == 0 "
               "(got %lld rows of %d)", rows, H * hd);
    const long long total = rows * (H * hd / 8);
    long long g = (total + 255) / 256;
    if (g > 2048) g = 2048;  // (capped at one resident wave of 256 CUs: the loop strides)
    hipLaunchKernelGGL(attention_identity_kernel, dim3((unsigned)g), dim3(256), 0, stream, src, ld_src, col0, out, rows, H, H / Hkv, hd, out_pair);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

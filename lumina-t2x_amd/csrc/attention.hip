// Non-causal flash attention for gfx950, head_dim 48 / 72 / 96 / 128 (Next-DiT 600M / 2B, Flag-DiT 5B, the 7B models).
//
// Replaces flash_attn_varlen_func on the all-ones mask (lumina_next_t2i/models/model.py:378-405; the
// unpad/pad gathers are identities in sampling, model.py:781) and, in accumulate mode, the zero-init
// tanh-gated text cross-attention (model.py:420-434):  out += tanh(gate_h) * softmax(q ky^T/sqrt(hd)+mask) vy.
//
// Structure (wave64 / MFMA-first):
//  * workgroup = 4 waves, each wave owns 32 query rows; K/V tiles of 64 keys are shared through LDS,
//    double buffered, filled with buffer_load...lds (K tile is one contiguous 64*hd*2-byte run thanks
//    to the head-major layout written by qk_norm_rope; V^T tile rows are 128 B, bank-swizzled on the
//    source address).
//  * "swapped" QK^T: S^T = K * Q^T via v_mfma_f32_32x32x16_bf16, so a lane holds 16 scores of ONE
//    query row per 32-key sub-tile -> running max / sum are lane-local (one shuffle with lane^32).
//  * O^T = V^T * P^T: the P fragment is exactly the lane's own registers (converted to bf16) because
//    v_transpose stores keys in the matching permuted order -> no cross-lane traffic for P.
//  * hd = 72 is padded to 80 in the QK^T reduction (5 k-steps, Q's tail zero) and to 96 rows of O^T.
//  * workgroup -> (head, q-block) map keeps all q-blocks of a head on one XCD (private L2) in order.
#include "common.h"
#include "kernels.h"
#include "options.h"
#include <type_traits>

namespace {

// ---- v1: straightforward online softmax (kept for A/B and as the fallback for head_dim % 32 == 0: hd 96 with a key bias, and the
//      general path of hd 128 - key bias, partial last tile, accumulate, per-sample key counts; whole tiles go to attention_hd128.hip) -------
template <int HD>
__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnArgs p) {
    constexpr int KS = (HD + 15) / 16;   // QK^T k-steps
    constexpr int DT = (HD + 31) / 32;   // O^T row tiles
    constexpr int CPR = HD / 8;          // 16-byte chunks per K row == 1-KiB pieces per tile
    constexpr int KTILE = 64 * HD * 2;   // bytes of a K tile
    constexpr int VTILE = HD * 128;      // bytes of a V^T tile
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, l31 = lane & 31;

    const int nqb = (p.N + 127) / 128;
    const int BH = p.B * p.H;
    int bh, qb;
    if ((BH & 7) == 0) {  // XCD-aware: head bh lives on XCD bh % 8, its q-blocks run back to back
        const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
        bh = xcd + 8 * (idx / nqb);
        qb = idx % nqb;
    } else {
        bh = blockIdx.x / nqb;
        qb = blockIdx.x % nqb;
    }
    const int b = bh / p.H, h = bh - b * p.H;
    const int bhk = b * p.Hkv + h / (p.H / p.Hkv);

    // ---- Q fragments (B operand of S^T = K Q^T): lane = (q row l31, d = 16 s + 8 hi .. +8) ----------
    int qrow = qb * 128 + wave * 32 + l31;
    const bool q_ok = qrow < p.N;
    if (!q_ok) qrow = p.N - 1;
    const u16* qptr = p.q + ((size_t)((p.q_batch_map ? p.q_batch_map[b] : b) * p.H + h) * p.N + qrow) * HD;
    bf16x8 qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int d0 = 16 * s + 8 * hi;
        if (d0 < HD) qf[s] = *(const bf16x8*)(qptr + d0);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[s][e] = (__bf16)0.0f;
        }
    }

    // ---- staging descriptors (bounded to this head: keys past the end read as zero) ---------------
    const size_t kbytes = (size_t)p.Nk * HD * 2;
    __amdgpu_buffer_rsrc_t rK = __builtin_amdgcn_make_buffer_rsrc((void*)(p.k + (size_t)bhk * p.Nk * HD), 0, (int)kbytes, 0x00020000);
    __amdgpu_buffer_rsrc_t rV = __builtin_amdgcn_make_buffer_rsrc((void*)(p.vt + (size_t)bhk * HD * p.Nkpad), 0, (int)((size_t)HD * p.Nkpad * 2), 0x00020000);
    auto stage = [&](int buf, int k0) {
        char* kb = smem + buf * KTILE;
        char* vb = smem + 2 * KTILE + buf * VTILE;
#pragma unroll
        for (int i = 0; i < (CPR + 3) / 4; ++i) {
            const int j = wave + 4 * i;
            if (j < CPR) {
                // hd 128: K rows are 256 bytes = all 64 banks, so chunk c of row r lives at position c ^ (r & 15); the LDS image of a DMA is
                // lane-linear, so the swizzle goes on the per-lane SOURCE address (position 64 j + lane = row 4 j + lane / 16, position lane % 16)
                const int ksrc = (HD == 128) ? (4 * j + (lane >> 4)) * 256 + (((lane & 15) ^ ((4 * j + (lane >> 4)) & 15)) << 4) : j * 1024 + lane * 16;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rK, LDS_PTR(kb + j * 1024), 16, ksrc, k0 * HD * 2, 0, 0);
                const int d = 8 * j + (lane >> 3);
                const int sc = (lane & 7) ^ ((d >> 1) & 7);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rV, LDS_PTR(vb + j * 1024), 16, d * p.Nkpad * 2 + sc * 16, k0 * 2, 0, 0);
            }
        }
    };

    // ---- per-lane LDS read offsets --------------------------------------------------------------------
    int koff[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        int ch = 2 * s + hi;
        if (ch > CPR - 1) ch = CPR - 1;  // hd=72: pad chunk re-reads valid data, multiplied by Q's zero tail
        koff[s] = l31 * HD * 2 + ((HD == 128 ? ch ^ (l31 & 15) : ch) << 4);  // (rows 32 apart share l31 & 15: one offset serves both sub-tiles)
    }
    int voff[DT][4];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        int d = dt * 32 + l31;
        if (d > HD - 1) d = HD - 1;  // rows past hd are never stored
#pragma unroll
        for (int g = 0; g < 4; ++g) voff[dt][g] = d * 128 + (((2 * g + hi) ^ ((d >> 1) & 7)) << 4);
    }

    const float sl2 = p.k_prescaled ? 1.0f : p.scale * 1.44269504088896340736f;  // work in the log2 domain
    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m_run = -1.0e30f, l_run = 0.f;

    const int Nk_eff = p.nk_batch ? p.nk_batch[b] : p.Nk;  // packed batches: this sample's valid keys (layout stride stays p.Nk)
    const int ntile = (Nk_eff + 63) / 64;
    const float* bias = p.bias ? p.bias + (size_t)b * p.Nkpad : nullptr;
    stage(0, 0);
    for (int t = 0; t < ntile; ++t) {
        const int cur = t & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 1 < ntile) stage(cur ^ 1, (t + 1) * 64);
        const char* kb = smem + cur * KTILE;
        const char* vb = smem + 2 * KTILE + cur * VTILE;
        const int k0 = t * 64;

        // S^T sub-tiles: lane holds keys 32 kt2 + (r&3) + 8 (r>>2) + 4 hi for its query row
        f32x16 sc[2];
#pragma unroll
        for (int kt2 = 0; kt2 < 2; ++kt2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[kt2][r] = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const bf16x8 kf = *(const bf16x8*)(kb + kt2 * 32 * HD * 2 + koff[s]);
                sc[kt2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], sc[kt2], 0, 0, 0);
            }
        }
        float mx = -INFINITY;
        const bool tail = (k0 + 64 > Nk_eff);
#pragma unroll
        for (int kt2 = 0; kt2 < 2; ++kt2) {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int kbase = k0 + 32 * kt2 + 8 * q4 + 4 * hi;
                float bv[4] = {0.f, 0.f, 0.f, 0.f};
                if (bias) {
                    const f32x4 t4 = *(const f32x4*)(bias + kbase);
                    bv[0] = t4[0]; bv[1] = t4[1]; bv[2] = t4[2]; bv[3] = t4[3];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float v = sc[kt2][4 * q4 + j] * sl2 + bv[j];
                    if (tail && kbase + j >= Nk_eff) v = -INFINITY;
                    sc[kt2][4 * q4 + j] = v;
                    mx = fmaxf(mx, v);
                }
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        float psum = 0.f;
#pragma unroll
        for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = __builtin_amdgcn_exp2f(sc[kt2][r] - m_new);
                sc[kt2][r] = e;
                psum += e;
            }
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;

        // O^T += V^T P^T : group g = keys 16g..16g+15, P fragment = this lane's own 8 values
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bf16x8 pf;
#pragma unroll
            for (int e = 0; e < 8; ++e) pf[e] = (__bf16)sc[g >> 1][8 * (g & 1) + e];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const bf16x8 vf = *(const bf16x8*)(vb + voff[dt][g]);
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[dt], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: lane holds out[q = l31][d = 32 dt + 8 q4 + 4 hi + j] ---------------------------------
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    float gate = 0.f;
    if (p.accumulate) gate = bfr(tanhf(bf2f(p.gate[h])));
    if (q_ok) {
        u16* orow = p.out + ((size_t)b * p.N + qrow) * ((size_t)p.H * HD) + (size_t)h * HD;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int d0 = 32 * dt + 8 * q4 + 4 * hi;
                if (d0 < HD) {
                    float v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = o[dt][4 * q4 + j] * inv;
                    u32x2* dst = (u32x2*)(orow + d0);
                    if (p.accumulate) {
                        // output + bf16(output_y * tanh(gate))  (model.py:433-434, bf16 rounding points)
                        const u32x2 prev = *dst;
                        const float pv[4] = {bf_lo(prev[0]), bf_hi(prev[0]), bf_lo(prev[1]), bf_hi(prev[1])};
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = pv[j] + bfr(bfr(v[j]) * gate);
                    }
                    u32x2 w = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
                    *dst = w;
                }
            }
    }
}

// ---- v2: VALU diet ------------------------------------------------------------------------------------
// The v1 loop is VALU-bound (MFMA pipe ~25 % busy): per 64-key tile a lane spends ~300 VALU ops on 22 MFMAs.
// v2 removes most of them:
//  * the softmax scale is folded into the exponent: p = exp2(fma(s, scale*log2e, -m));
//  * the running max is only raised when the tile max exceeds it by more than THR (log2 units), so the
//    O rescale is a rare wave-uniform branch (guide T13; P <= 2^THR stays exact enough in bf16);
//  * the row sum l comes out of the PV MFMA for free: V^T gets one extra LDS row of ones in the padding of
//    the last 32-row tile (hd 72 -> row 72, hd 48 -> row 48), so O^T[hd][q] = sum_k P[q][k];
//  * s_setprio(1) around the MFMA clusters.
// The key-bias path (text cross-attention, a few tiles only) keeps the explicit fma+bias form.
template <int HD>
__global__ __launch_bounds__(256) void attn_fwd_kernel_v2(AttnArgs p) {
    constexpr int KS = (HD + 15) / 16;
    constexpr int DT = (HD + 31) / 32;
    constexpr int CPR = HD / 8;
    constexpr int KTILE = 64 * HD * 2;
    constexpr int VTILE = HD * 128 + 128;  // + the row of ones
    constexpr float THR = 8.0f;
    static_assert(HD % 32 != 0, "v2 needs a spare row in the last O^T tile");
    constexpr int LI = HD % 32, L_DT = HD / 32, L_HI = (LI >> 2) & 1, L_REG = (LI & 3) + 4 * (LI >> 3);
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, l31 = lane & 31;

    const int nqb = (p.N + 127) / 128;
    const int BH = p.B * p.H;
    int bh, qb;
    if ((BH & 7) == 0) {
        const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
        bh = xcd + 8 * (idx / nqb);
        qb = idx % nqb;
    } else {
        bh = blockIdx.x / nqb;
        qb = blockIdx.x % nqb;
    }
    const int b = bh / p.H, h = bh - b * p.H;
    const int bhk = b * p.Hkv + h / (p.H / p.Hkv);

    // row of ones (bf16 1.0 = 0x3F80) behind each V^T buffer
    if (tid < 64) {
        const int buf = tid >> 5, w = tid & 31;
        *(unsigned*)(smem + 2 * KTILE + buf * VTILE + HD * 128 + w * 4) = 0x3F803F80u;
    }

    int qrow = qb * 128 + wave * 32 + l31;
    const bool q_ok = qrow < p.N;
    if (!q_ok) qrow = p.N - 1;
    const u16* qptr = p.q + ((size_t)((p.q_batch_map ? p.q_batch_map[b] : b) * p.H + h) * p.N + qrow) * HD;
    bf16x8 qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int d0 = 16 * s + 8 * hi;
        if (d0 < HD) qf[s] = *(const bf16x8*)(qptr + d0);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[s][e] = (__bf16)0.0f;
        }
    }

    const size_t kbytes = (size_t)p.Nk * HD * 2;
    __amdgpu_buffer_rsrc_t rK = __builtin_amdgcn_make_buffer_rsrc((void*)(p.k + (size_t)bhk * p.Nk * HD), 0, (int)kbytes, 0x00020000);
    __amdgpu_buffer_rsrc_t rV = __builtin_amdgcn_make_buffer_rsrc((void*)(p.vt + (size_t)bhk * HD * p.Nkpad), 0, (int)((size_t)HD * p.Nkpad * 2), 0x00020000);
    auto stage = [&](int buf, int k0) {
        char* kb = smem + buf * KTILE;
        char* vb = smem + 2 * KTILE + buf * VTILE;
#pragma unroll
        for (int i = 0; i < (CPR + 3) / 4; ++i) {
            const int j = wave + 4 * i;
            if (j < CPR) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rK, LDS_PTR(kb + j * 1024), 16, j * 1024 + lane * 16, k0 * HD * 2, 0, 0);
                const int d = 8 * j + (lane >> 3);
                const int sc = (lane & 7) ^ ((d >> 1) & 7);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rV, LDS_PTR(vb + j * 1024), 16, d * p.Nkpad * 2 + sc * 16, k0 * 2, 0, 0);
            }
        }
    };

    int koff[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        int ch = 2 * s + hi;
        if (ch > CPR - 1) ch = CPR - 1;
        koff[s] = l31 * HD * 2 + ch * 16;
    }
    int voff[DT][4];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        int d = dt * 32 + l31;
        if (d > HD) d = HD;  // row HD is the row of ones; rows past it are never stored
#pragma unroll
        for (int g = 0; g < 4; ++g) voff[dt][g] = d * 128 + (((2 * g + hi) ^ ((d >> 1) & 7)) << 4);
    }

    const float sl2 = p.k_prescaled ? 1.0f : p.scale * 1.44269504088896340736f;
    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m_run = -1.0e30f;

    const int Nk_eff = p.nk_batch ? p.nk_batch[b] : p.Nk;
    const int ntile = (Nk_eff + 63) / 64;
    const float* bias = p.bias ? p.bias + (size_t)b * p.Nkpad : nullptr;
    stage(0, 0);
    for (int t = 0; t < ntile; ++t) {
        const int cur = t & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 1 < ntile) stage(cur ^ 1, (t + 1) * 64);
        const char* kb = smem + cur * KTILE;
        const char* vb = smem + 2 * KTILE + cur * VTILE;
        const int k0 = t * 64;

        f32x16 sc[2];
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kt2 = 0; kt2 < 2; ++kt2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[kt2][r] = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const bf16x8 kf = *(const bf16x8*)(kb + kt2 * 32 * HD * 2 + koff[s]);
                sc[kt2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], sc[kt2], 0, 0, 0);
            }
        }
        __builtin_amdgcn_s_setprio(0);

        float mx = -INFINITY;
        if (bias) {  // key-bias path: v = s * sl2 + bias, then plain max / exp2(v - m)
#pragma unroll
            for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const f32x4 t4 = *(const f32x4*)(bias + k0 + 32 * kt2 + 8 * q4 + 4 * hi);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float v = __builtin_fmaf(sc[kt2][4 * q4 + j], sl2, t4[j]);
                        sc[kt2][4 * q4 + j] = v;
                        mx = fmaxf(mx, v);
                    }
                }
        } else {
            if (k0 + 64 > Nk_eff) {  // tail tile: keys past Nk
#pragma unroll
                for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = k0 + 32 * kt2 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                        if (key >= Nk_eff) sc[kt2][r] = -INFINITY;
                    }
            }
#pragma unroll
            for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[kt2][r]);
            mx *= sl2;  // scale > 0
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const bool raise = mx > m_run + THR;
        if (__any(raise)) {
            const float m_new = raise ? mx : m_run;
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            m_run = m_new;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
        }
        if (bias) {
#pragma unroll
            for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                for (int r = 0; r < 16; ++r) sc[kt2][r] = __builtin_amdgcn_exp2f(sc[kt2][r] - m_run);
        } else {
            const float nm = -m_run;
#pragma unroll
            for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                for (int r = 0; r < 16; ++r) sc[kt2][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[kt2][r], sl2, nm));
        }

#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bf16x8 pf;
#pragma unroll
            for (int e = 0; e < 8; ++e) pf[e] = (__bf16)sc[g >> 1][8 * (g & 1) + e];
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const bf16x8 vf = *(const bf16x8*)(vb + voff[dt][g]);
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[dt], 0, 0, 0);
            }
            __builtin_amdgcn_s_setprio(0);
        }
    }

    // l = O^T[HD][q] lives in register L_REG of tile L_DT on the hi == L_HI lane of this query row
    const float l_tot = __shfl(o[L_DT][L_REG], l31 + 32 * L_HI, 64);
    const float inv = 1.0f / l_tot;
    float gate = 0.f;
    if (p.accumulate) gate = bfr(tanhf(bf2f(p.gate[h])));
    if (q_ok) {
        u16* orow = p.out + ((size_t)b * p.N + qrow) * ((size_t)p.H * HD) + (size_t)h * HD;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int d0 = 32 * dt + 8 * q4 + 4 * hi;
                if (d0 < HD) {
                    float v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = o[dt][4 * q4 + j] * inv;
                    u32x2* dst = (u32x2*)(orow + d0);
                    if (p.accumulate) {
                        const u32x2 prev = *dst;
                        const float pv[4] = {bf_lo(prev[0]), bf_hi(prev[0]), bf_lo(prev[1]), bf_hi(prev[1])};
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = pv[j] + bfr(bfr(v[j]) * gate);
                    }
                    u32x2 w = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
                    *dst = w;
                }
            }
    }
}


}  // namespace

// (named namespace + explicit instantiation: hipcc 7.2 drops the host stub of an internal-linkage kernel template whose
//  body holds a local class, the same limitation gemm_bf16.hip works around)
namespace lt_attn {

// ---- v3: ping-pong wave groups for head_dim 72 (the Next-DiT 2B self-attention) ----------------------------------
// At hd = 72 the softmax VALU work per score is as expensive as the MFMA work (the v2 loop keeps the matrix pipe
// ~37 % busy), so v3 removes VALU work and makes the two waves of a SIMD alternate between a pure-MFMA phase and
// a pure-VALU phase:
//  * workgroup = 8 waves = 256 query rows (32 per wave), K / V^T tiles of 64 keys in 4-slot LDS rings shared by
//    all 8 waves (half the staging traffic and DMA issue per query row of v2).
//  * the waves form two groups (wave / 4); per tile a wave runs
//        X(t): PV MFMAs of tile t-1 + QK^T MFMAs of tile t (22 MFMAs, fragment ds_reads in between)  | s_barrier
//        Y(t): softmax of tile t (max3 tree, exp2, bf16 pack) + LDS-DMA issue for K(t+3), V(t+2)      | s_barrier
//    and group 1 runs one barrier interval late: on every SIMD one wave feeds the matrix pipe while the other
//    does exp2 - the two pipes overlap by construction instead of by luck.
//  * the running max is folded INTO the QK^T MFMA: hd 72 is padded to 80 in the reduction, so two of the pad
//    slots carry K-side 1.0 (a constant LDS chunk) x Q-side (-m_hi, -m_lo); Q is pre-scaled by scale*log2(e).
//    The MFMA therefore yields s*scale*log2e - m directly and P = exp2(.) needs no fma.  m only moves when a tile
//    max exceeds it by 2^THR (rare wave-uniform branch that rescales O, fixes this tile's scores and rewrites
//    the two pad values); a bf16-split m is exact enough because numerator and row sum use the same P.
//  * row sum l from the ones-row of V^T, as in v2.  DMA waits are counted (never vmcnt(0) in the loop).
// Hazards (barrier-interval units; X(t) of group g in interval 2t+g, Y(t) in 2t+g+1):
//   K(t+3) / V(t+2) are issued in Y(t), waited for at the end of X(t+2) (leaving Y(t+1)'s batch in flight) and
//   first read in X(t+3) - a barrier all waves pass lies between wait and read for either group; they overwrite
//   the slots of K(t-1) / V(t-2), last read in X(t-1) = interval 2t-2+g' < 2t+g+1.
// HD = 96 (Flag-DiT 5B, lumina_t2i/models/model.py:507-621) runs the same two-group ping-pong with three differences (FOLD = false):
//  * there are no spare slots: QK^T is 6 exact k-steps, O^T is 3 exact row tiles.  The running max is subtracted on the VALU
//    (p = exp2(s - m), one v_sub per score) and the row sum is accumulated on the VALU (one v_add per score); both sit in
//    the Y phase, which stays shorter than the partner group's X phase (24 MFMAs = 768 matrix-pipe cycles);
//  * a K row is 192 bytes = 12 sixteen-byte chunks: rows 4 apart would share an LDS slot in a fragment read (4-way conflict), so
//    chunk c of row r is stored at position c ^ ((r >> 2) & 3) - applied to the per-lane SOURCE address of the LDS-DMA (the
//    LDS image of a DMA is lane-linear) and again on the fragment reads (guide rule 21);
//  * 24 one-KiB pieces per (K, V^T) tile pair = exactly three per wave, no duplicates.
template <int HD, bool TRACE = false>
__global__ __launch_bounds__(512, 2) void attn_fwd_kernel_v3(AttnArgs p) {
    static_assert(HD == 72 || HD == 96, "v3 is built for hd 72 (max / row sum folded into the MFMAs through the pad slots) and hd 96");
    constexpr bool FOLD = (HD == 72);
    constexpr int KS = (HD + 15) / 16, DT = 3;
    constexpr int NKP = 64 * HD * 2 / 1024, NVP = HD / 8;   // 1-KiB pieces of a K tile / a V^T tile: 9 + 9 or 12 + 12
    constexpr int KTILE = 64 * HD * 2;                      // 9216 / 12288
    constexpr int VTILE = HD * 128 + (FOLD ? 128 : 0);      // incl. the row of ones (FOLD)
    constexpr int V_BASE = 0, K_BASE = 4 * VTILE, CONST_OFF = K_BASE + 4 * KTILE;
    constexpr float THR = 8.0f;
    constexpr int LI = HD % 32, L_DT = FOLD ? HD / 32 : 0, L_HI = (LI >> 2) & 1, L_REG = (LI & 3) + 4 * (LI >> 3);
    static_assert(NKP + NVP <= 24, "three staging pieces per wave");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;
    const int hi = lane >> 5, l31 = lane & 31;

    const int nqb = (p.N + 255) / 256;
    const int BH = p.B * p.H;
    int bh, qb;
    if ((BH & 7) == 0) {  // XCD-aware: head bh lives on XCD bh % 8, its q-blocks run back to back (K/V stay in that L2)
        const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
        bh = xcd + 8 * (idx / nqb);
        qb = idx % nqb;
    } else {
        bh = blockIdx.x / nqb;
        qb = blockIdx.x % nqb;
    }
    const int b = bh / p.H, h = bh - b * p.H;
    const int bhk = b * p.Hkv + h / (p.H / p.Hkv);

    // constants in LDS: ones rows behind each V^T slot, and the K-side pad chunk (1, 1, 0, ...)
    if constexpr (FOLD) {
        if (tid < 128) *(unsigned*)(smem + V_BASE + (tid >> 5) * VTILE + HD * 128 + (tid & 31) * 4) = 0x3F803F80u;
        if (tid >= 128 && tid < 132) *(unsigned*)(smem + CONST_OFF + (tid - 128) * 4) = (tid == 128) ? 0x3F803F80u : 0u;
    }

    // ---- Q fragments, pre-scaled to the log2 domain -------------------------------------------------
    int qrow = qb * 256 + wave * 32 + l31;
    const bool q_ok = qrow < p.N;
    if (!q_ok) qrow = p.N - 1;
    const u16* qptr = p.q + ((size_t)bh * p.N + qrow) * HD;
    // scores must come out of the MFMA in the log2 domain: either K already carries scale * log2(e) (engine path: folded
    // into K's single bf16 rounding by qk_norm_rope, no extra rounding anywhere) or Q is pre-scaled here (one extra
    // bf16 rounding of Q; operator-level calls with plain K)
    const float sl2 = p.k_prescaled ? 1.0f : p.scale * 1.44269504088896340736f;
    bf16x8 qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int d0 = 16 * s + 8 * hi;
        if (d0 < HD) {
            const bf8_t raw = *(const bf8_t*)(qptr + d0);
            float f[8];
            unpack8(raw, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[s][e] = (__bf16)(f[e] * sl2);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[s][e] = (__bf16)0.0f;  // pad: slots 0,1 become -m_hi, -m_lo
        }
    }

    // ---- staging ------------------------------------------------------------------------------------
    // NKP + NVP one-KiB pieces per (K, V^T) tile pair: K piece j = bytes [1024 j, +1024) of the K tile's LDS image (j < NKP),
    // V piece j = V^T rows 8j..8j+7 (j < NVP).  Every wave issues exactly three LDS-DMA loads per batch, branch-free, so one
    // vmcnt literal fits all waves.
    //   hd 72 (9 + 9):   A = K piece w;  B = K piece 8 (wave 0) or V piece w-1;  C = V piece 7 (wave 0), 8 (wave 1) or V piece
    //                    w-1 again (waves 2..7: same bytes to the same place, harmless)
    //   hd 96 (12 + 12): A = K piece w;  B = K piece 8 + w (waves 0..3) or V piece w - 4;  C = V piece 4 + w
    const bool b_is_k = FOLD ? (wave == 0) : (wave < 4);
    const int jb = FOLD ? (b_is_k ? 8 : wave - 1) : (b_is_k ? 8 + wave : wave - 4);
    const int jc = FOLD ? ((wave == 0) ? 7 : (wave == 1 ? 8 : wave - 1)) : 4 + wave;
    // per-lane source offset of K piece j: lane-linear at hd 72; at hd 96 chunk position 64 j + lane = (row, c') is filled from
    // source chunk c = c' ^ ((row >> 2) & 3) of that row
    auto k_voff = [&](int j) __attribute__((always_inline)) {
        if constexpr (FOLD) return j * 1024 + lane * 16;
        const int pos = 64 * j + lane, row = pos / 12, c = (pos - 12 * row) ^ ((row >> 2) & 3);
        return row * (HD * 2) + c * 16;
    };
    // two K / V^T sources to stage from: [0] the image keys, [1] the text keys of the fused cross-attention
    // (plain arrays with constant indices: a local class holding buffer descriptors breaks hipcc 7.2's host-side pass)
    __amdgpu_buffer_rsrc_t srcA[2], srcB[2], srcC[2];
    int svoffB[2], svoffC[2];
    auto make_src = [&](int which, const u16* k_head, int k_rows, const u16* v_head, int v_ld) __attribute__((always_inline)) {
        const int kbytes = (int)((size_t)k_rows * HD * 2), vbytes = (int)((size_t)HD * v_ld * 2);
        auto v_voff = [&](int j) __attribute__((always_inline)) {
            const int d = 8 * j + (lane >> 3);
            return d * v_ld * 2 + (((lane & 7) ^ ((d >> 1) & 7)) << 4);
        };
        srcA[which] = __builtin_amdgcn_make_buffer_rsrc((void*)k_head, 0, kbytes, 0x00020000);
        srcB[which] = __builtin_amdgcn_make_buffer_rsrc((void*)(b_is_k ? k_head : v_head), 0, b_is_k ? kbytes : vbytes, 0x00020000);
        srcC[which] = __builtin_amdgcn_make_buffer_rsrc((void*)v_head, 0, vbytes, 0x00020000);
        svoffB[which] = b_is_k ? k_voff(jb) : v_voff(jb);
        svoffC[which] = v_voff(jc);
    };
    make_src(0, p.k + (size_t)bhk * p.Nk * HD, p.Nk, p.vt + (size_t)bhk * HD * p.Nkpad, p.Nkpad);
    const int voffA = k_voff(wave);
    // batch = {K(tk), V(tv)}; slots are tile index & 3
    auto dma_a_from = [&](int sr, int tk) __attribute__((always_inline)) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(srcA[sr], LDS_PTR(smem + K_BASE + (tk & 3) * KTILE + wave * 1024), 16, voffA, tk * KTILE, 0, 0);
    };
    auto dma_b_from = [&](int sr, int tk, int tv) __attribute__((always_inline)) {
        const int lds = b_is_k ? K_BASE + (tk & 3) * KTILE + jb * 1024 : V_BASE + (tv & 3) * VTILE + jb * 1024;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(srcB[sr], LDS_PTR(smem + lds), 16, svoffB[sr], b_is_k ? tk * KTILE : tv * 128, 0, 0);
    };
    auto dma_c_from = [&](int sr, int tv) __attribute__((always_inline)) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(srcC[sr], LDS_PTR(smem + V_BASE + (tv & 3) * VTILE + jc * 1024), 16, svoffC[sr], tv * 128, 0, 0);
    };
    auto dma_a = [&](int tk) __attribute__((always_inline)) { dma_a_from(0, tk); };
    auto dma_b = [&](int tk, int tv) __attribute__((always_inline)) { dma_b_from(0, tk, tv); };
    auto dma_c = [&](int tv) __attribute__((always_inline)) { dma_c_from(0, tv); };
    const int Nk_eff = p.nk_batch ? p.nk_batch[b] : p.Nk;
    const int ntile = (Nk_eff + 63) / 64;
    // prologue: K(0); K(1), V(0); K(2), V(1)  (the batches X(-3), X(-2), X(-1) would have issued; tile indices past
    // the end read zeros through the descriptor bounds and are never consumed)
    dma_a(0);
    if (b_is_k) dma_b(0, 0);  // (the K-piece part of batch 0; its V half would be "V(-1)")
    dma_a(1); dma_b(1, 0); dma_c(0);
    dma_a(2); dma_b(2, 1); dma_c(1);

    // ---- per-lane LDS read offsets ------------------------------------------------------------------
    const int kb_lane = K_BASE + l31 * (HD * 2) + (FOLD ? hi * 16 : 0);  // + slot * KTILE + kt2 * 32 * HD * 2 + chunk offset
    int kco[KS];  // byte offset of k-step s inside the lane's K row: hd 72 plain (2 s chunks on top of the hi chunk), hd 96 swizzled
#pragma unroll
    for (int s_ = 0; s_ < KS; ++s_) kco[s_] = FOLD ? s_ * 32 : (((2 * s_ + hi) ^ ((l31 >> 2) & 3)) << 4);
    int voff[DT][4];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        int d = dt * 32 + l31;
        if (FOLD && d > HD) d = HD;  // row HD is the row of ones; rows past it are never stored
#pragma unroll
        for (int g = 0; g < 4; ++g) voff[dt][g] = V_BASE + d * 128 + (((2 * g + hi) ^ ((d >> 1) & 7)) << 4);
    }

    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    f32x16 sc[2];
    bf16x8 pa[4];
    float m_run = FOLD ? 0.f : -1.0e30f;  // FOLD: scores leave the MFMA relative to the running max already
    float l_run = 0.f;                    // !FOLD: this lane's half of the row sum (the other half lives on lane ^ 32)

    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // DMA landed, constant rows written
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (grp == 1) {
        asm volatile("s_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    }

    auto bar = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };

    // X phase: PV of the previous tile (P in pa, V^T slot (t+3)&3) and QK^T of tile t (K slot t&3); with DMA it also
    // issues the batch {K(t+3), V(t+2)} between the MFMAs.  All 22 fragment reads are written first and the order is
    // pinned with sched_group_barrier: six reads ahead of the first MFMA, then one read per MFMA, so the in-order
    // wave never sits on LDS latency (the compiler's own just-in-time placement kept the matrix pipe ~60 % busy).
    bf16x8 fpre[6];  // first six V^T fragments of the next X phase, read at the end of the Y phase before it
    auto pre_reads = [&](int t_next) __attribute__((always_inline)) {  // V(t_next - 1) lives in slot (t_next + 3) & 3
        const char* vb = smem + ((t_next + 3) & 3) * VTILE;
#pragma unroll
        for (int i = 0; i < 6; ++i) fpre[i] = *(const bf16x8*)(vb + voff[i % 3][i / 3]);
    };
    auto phase_x = [&](int t, auto pv_c, auto qk_c, auto dma_c_) __attribute__((always_inline)) {
        constexpr bool PV = decltype(pv_c)::value, QK = decltype(qk_c)::value, DMA = decltype(dma_c_)::value;
        __builtin_amdgcn_s_setprio(1);
        const char* kb = smem + (t & 3) * KTILE + kb_lane;
        const char* vb = smem + ((t + 3) & 3) * VTILE;
        const char* kpad = hi ? (const char*)(smem + CONST_OFF) : kb + (KS - 1) * 32;  // FOLD only
        bf16x8 fr[12 + 2 * KS];
        int n = 0;
        // LDS-DMA writes cannot be scheduled across LDS reads they might alias, so their place among the reads is
        // fixed here in source order (beside MFMAs 2 / 6 / 10 of the pinned pipeline)
        auto dma_at = [&](int k) __attribute__((always_inline)) {
            if constexpr (DMA) {
                constexpr int P0 = PV ? 9 : 3, P1 = PV ? 13 : 6, P2 = PV ? 17 : 9;
                if (k == P0) dma_a(t + 3);
                if (k == P1) dma_b(t + 3, t + 2);
                if (k == P2) dma_c(t + 2);
            }
        };
        if constexpr (PV) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    dma_at(n);
                    if (n < 6) fr[n] = fpre[n];
                    else fr[n] = *(const bf16x8*)(vb + voff[dt][g]);
                    ++n;
                }
        }
        if constexpr (QK) {
#pragma unroll
            for (int s = 0; s < KS; ++s)
#pragma unroll
                for (int kt2 = 0; kt2 < 2; ++kt2) {
                    dma_at(n);
                    if constexpr (FOLD)
                        fr[n++] = (s < KS - 1) ? *(const bf16x8*)(kb + kt2 * 32 * HD * 2 + s * 32)
                                               : *(const bf16x8*)(kpad + (hi ? 0 : kt2 * 32 * HD * 2));
                    else
                        fr[n++] = *(const bf16x8*)(kb + kt2 * 32 * HD * 2 + kco[s]);
                }
        }
        n = 0;
        if constexpr (PV) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[n++], pa[g], o[dt], 0, 0, 0);
        }
        if constexpr (QK) {
            const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s)
#pragma unroll
                for (int kt2 = 0; kt2 < 2; ++kt2)
                    sc[kt2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[n++], qf[s], s == 0 ? zero : sc[kt2], 0, 0, 0);
        }
        if constexpr (PV && QK) {  // the first six fragments are already in flight (pre_reads): one read per MFMA
#pragma unroll
            for (int i = 0; i < 6 + 2 * KS; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                if (DMA && (i == 2 || i == 6 || i == 10)) __builtin_amdgcn_sched_group_barrier(0x10, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x8, 6, 0);
        }
        __builtin_amdgcn_s_setprio(0);
    };
    using T_ = std::true_type;
    using F_ = std::false_type;

    // Y phase: softmax of the tile in sc -> pa
    auto phase_y_gen = [&](int t, bool tail, int nk, const float* bias) __attribute__((always_inline)) {
        if (bias) {  // text keys: additive 0 / -inf mask (already in the log2 domain: 0 and -inf are scale free)
#pragma unroll
            for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const f32x4 t4 = *(const f32x4*)(bias + t * 64 + 32 * kt2 + 8 * q4 + 4 * hi);
#pragma unroll
                    for (int j = 0; j < 4; ++j) sc[kt2][4 * q4 + j] += t4[j];
                }
        }
        if (tail) {  // partial last tile: keys past Nk get probability 0
#pragma unroll
            for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = t * 64 + 32 * kt2 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (key >= nk) sc[kt2][r] = -INFINITY;
                }
        }
        float mx = fmaxf(sc[0][0], sc[1][0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(fmaxf(mx, sc[0][r]), sc[1][r]);
        {
            auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
            mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
        }
        if constexpr (!FOLD) {
            // explicit running max / row sum (no spare MFMA slots at hd 96): m only moves when a tile max exceeds it by 2^THR
            // (then O and l are rescaled - rare wave-uniform branch, guide T13 order: the previous tile's PV is complete)
            const bool raise = mx > m_run + THR;
            if (__builtin_expect(__any(raise), 0)) {
                const float m_new = raise ? mx : m_run;
                const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
                m_run = m_new;
                l_run *= alpha;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
            }
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float pe = __builtin_amdgcn_exp2f(sc[g >> 1][8 * (g & 1) + e] - m_run);
                    if (e & 1) s1 += pe; else s0 += pe;
                    pa[g][e] = (__bf16)pe;
                }
            l_run += s0 + s1;
#pragma unroll
            for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(pa[g]));
            return;
        }
        const bool first = (t == 0);
        const bool raise = first || (mx > THR);
        if (__builtin_expect(__any(raise), 0)) {
            // new running max = m_run + mx (scores are relative to m_run already), rounded to the bf16 pair
            // (hi + lo) the MFMA will actually subtract from now on; delta is the step between the two
            // REPRESENTED values, so this tile's scores, O and all later tiles stay on one scale
            const float nm = -(m_run + (raise ? mx : 0.f));
            const float nm_hi = bfr(nm);
            const float nm_lo = bfr(nm - nm_hi);
            const float m_new = -(nm_hi + nm_lo);
            const float delta = m_new - m_run;
            const float alpha = first ? 1.f : __builtin_amdgcn_exp2f(-delta);
            m_run = m_new;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
#pragma unroll
            for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                for (int r = 0; r < 16; ++r) sc[kt2][r] -= delta;
            if (hi) {  // pad slots 0 and 1 of the last k-step live on the hi half
                qf[KS - 1][0] = (__bf16)nm_hi;
                qf[KS - 1][1] = (__bf16)nm_lo;
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 8; ++e) pa[g][e] = (__bf16)__builtin_amdgcn_exp2f(sc[g >> 1][8 * (g & 1) + e]);
        // keep the bf16 packing in THIS phase (hipcc otherwise sinks the cvt_pk next to the PV MFMAs of the X phase)
#ifndef LT_ATTN_UNPIN_CVT
#pragma unroll
        for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(pa[g]));
#endif
    };
    auto phase_y = [&](int t) __attribute__((always_inline)) { phase_y_gen(t, t == ntile - 1 && (Nk_eff & 63), Nk_eff, nullptr); };

    unsigned long long tr[5] = {0, 0, 0, 0, 0}, t0 = 0, t1 = 0;
    if constexpr (TRACE) t0 = __builtin_amdgcn_s_memtime();
    auto stamp = [&](int i) __attribute__((always_inline)) {
        if constexpr (TRACE) {
            __builtin_amdgcn_sched_barrier(0);
            t1 = __builtin_amdgcn_s_memtime();
            tr[i] += t1 - t0;
            t0 = t1;
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // after X(t): K(t+2), V(t+1) (the batch issued in X(t-1)) must have landed - V(t+1)'s first fragments are read by
    // the other group as early as the end of its Y(t+1), one interval before its X(t+2); only the batch issued in
    // X(t) itself (three loads) may stay in flight
    auto rest = [&](int t) __attribute__((always_inline)) {
        stamp(0);
        if (t + 2 < ntile) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stamp(1);
        bar();
        stamp(2);
        phase_y(t);
        pre_reads(t + 1);
        stamp(3);
        bar();
        stamp(4);
    };
    {
        if (2 < ntile) phase_x(0, F_{}, T_{}, T_{});
        else phase_x(0, F_{}, T_{}, F_{});
        rest(0);
    }
    int t = 1;
    for (; t + 2 < ntile; ++t) {
        phase_x(t, T_{}, T_{}, T_{});
        rest(t);
    }
    for (; t < ntile; ++t) {
        phase_x(t, T_{}, T_{}, F_{});
        rest(t);
    }
    if constexpr (TRACE) {
        if (p.trace && lane == 0 && (blockIdx.x & 63) == 5) {
            unsigned long long* o = p.trace + ((size_t)(blockIdx.x >> 6) * 8 + wave) * 8;
#pragma unroll
            for (int i = 0; i < 5; ++i) o[i] = tr[i];
            o[5] = (unsigned long long)ntile;
        }
    }
    phase_x(ntile, T_{}, F_{}, F_{});  // PV of the last tile (V slot (ntile + 3) & 3 = (ntile - 1) & 3)
    if (grp == 0) bar();                       // the barrier group 1 still needs after its last Y phase

    // FOLD: l = O^T[HD][q] lives in register L_REG of tile L_DT on the hi == L_HI lane of this query row; else the two halves'
    // partial sums are added
    auto row_inv = [&]() __attribute__((always_inline)) {
        if constexpr (FOLD) return 1.0f / __shfl(o[L_DT][L_REG], l31 + 32 * L_HI, 64);
        else return 1.0f / (l_run + __shfl_xor(l_run, 32, 64));
    };
    float inv = row_inv();
    u32x2 res[DT][4];  // self-attention result, bf16 (flash-attn output dtype, model.py:392-405)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            res[dt][q4][0] = pack2bf(o[dt][4 * q4] * inv, o[dt][4 * q4 + 1] * inv);
            res[dt][q4][1] = pack2bf(o[dt][4 * q4 + 2] * inv, o[dt][4 * q4 + 3] * inv);
        }

    if (p.tk) {
        // ---- fused zero-init gated text cross-attention (model.py:420-434): same Q rows (post-RoPE, :427), text K / V^T
        //      staged into the now idle ring slots, plain tile loop (2-4 tiles), same max-folding softmax ----------------
        const int bhk_t = bhk;  // text K / V share the kv-head layout
        make_src(1, p.tk + (size_t)bhk_t * p.Tk * HD, p.Tk, p.tvt + (size_t)bhk_t * HD * p.Tkpad, p.Tkpad);
        const float* tb = p.tbias + (size_t)b * p.Tkpad;
        const int ntt = (p.Tk + 63) / 64;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
        m_run = FOLD ? 0.f : -1.0e30f;
        l_run = 0.f;
        if (FOLD && hi) {
            qf[KS - 1][0] = (__bf16)0.0f;
            qf[KS - 1][1] = (__bf16)0.0f;
        }
        for (int g0 = 0; g0 < ntt; g0 += 4) {  // up to four tiles per pass through the ring
            const int g1 = min(ntt, g0 + 4);
            bar();  // every wave is done with the ring slots (self-attention, or the previous pass)
            for (int tt = g0; tt < g1; ++tt) {
                dma_a_from(1, tt);
                dma_b_from(1, tt, tt);
                dma_c_from(1, tt);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            bar();
            for (int tt = g0; tt < g1; ++tt) {
                phase_x(tt, F_{}, T_{}, F_{});                 // S = K_txt(tt) Q^T (log2 domain, minus the folded max)
                phase_y_gen(tt, false, p.Tk, tb);               // + mask, exp2, bf16 (first tile sets the max)
                pre_reads(tt + 1);
                phase_x(tt + 1, T_{}, F_{}, F_{});             // O_txt += V_txt(tt)^T P   (V slot (tt + 4) & 3 = tt & 3)
            }
        }
        inv = row_inv();
        const float gate = bfr(tanhf(bf2f(p.tgate[h])));
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                // output + bf16(output_y * tanh(gate))  (model.py:433-434, bf16 rounding points)
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = bfr(bfr(o[dt][4 * q4 + j] * inv) * gate);
                res[dt][q4][0] = pack2bf(bf_lo(res[dt][q4][0]) + v[0], bf_hi(res[dt][q4][0]) + v[1]);
                res[dt][q4][1] = pack2bf(bf_lo(res[dt][q4][1]) + v[2], bf_hi(res[dt][q4][1]) + v[3]);
            }
    }

    if (q_ok) {
        u16* orow = p.out + ((size_t)b * p.N + qrow) * ((size_t)p.H * HD) + (size_t)h * HD;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int d0 = 32 * dt + 8 * q4 + 4 * hi;
                if (d0 < HD) *(u32x2*)(orow + d0) = res[dt][q4];
            }
    }
}

template __global__ void attn_fwd_kernel_v3<72, false>(AttnArgs);
template __global__ void attn_fwd_kernel_v3<72, true>(AttnArgs);
template __global__ void attn_fwd_kernel_v3<96, false>(AttnArgs);

}  // namespace lt_attn

using lt_attn::attn_fwd_kernel_v3;

// option attention_variant (options.h): 4 (default) = one wave per SIMD x 64 query rows where it applies (hd 72 / 96 / 48, whole tiles), else 3 =
// ping-pong kernel (hd 72 / 96), v2 elsewhere; 6 = 4 with the hd-48 one-wave kernel forced at every size

// true when launch_attention() can take the text keys along with the image keys (one kernel instead of two)
bool attention_fuses_text(int hd) { return lt_opt(OPT_ATTENTION_VARIANT) >= 3 && (hd == 72 || hd == 96); }

// THE dispatch condition of attn_fwd_kernel_v4<72>, with or without per-sample key counts (launch_attention, attention_is_one_wave, attention_describe
// and launch_attention_v4 all ask this one function)
bool attention_one_wave_hd72(const AttnArgs& a) {
    return lt_opt(OPT_ATTENTION_VARIANT) >= 4 && a.hd == 72 && a.bias == nullptr && !a.accumulate && a.Nk % 64 == 0 && (!a.tk || a.Tkpad <= 256);
}

// ... and without per-sample key counts: the
// prologue takes ONE rope_grid_w, a packed batch has a grid width per sample (qk_norm_rope keeps doing Q there: QkPostArgs::grid_w_b)
bool attention_takes_raw_q(const AttnArgs& a) { return attention_one_wave_hd72(a) && !a.nk_batch; }

// launch_attention would run this call on one of the one-wave-per-SIMD kernels (hd 72 / 48 / 96: the ones that can write their output in the
// pair layout, AttnArgs::out_pair) - the same expressions as the dispatch below.  hd 128 is not among them: attention_hd128.hip's kernel
// (two waves per SIMD) writes row-major rows, so the 7B's dense block keeps row-major GEMM operands (run_forward's `pair` stays false)
bool attention_is_one_wave(const AttnArgs& a) {
    const int g_attn_variant = lt_opt(OPT_ATTENTION_VARIANT);
    if (attention_one_wave_hd72(a)) return true;
    if (g_attn_variant >= 4 && a.hd == 48 && a.bias == nullptr && !a.accumulate && !a.nk_batch && !a.trace && a.Nk % 64 == 0 && !a.tk &&
        (g_attn_variant == 6 || (long long)a.B * a.H * ((a.N + 255) / 256) >= 200)) return true;
    if (g_attn_variant >= 4 && a.hd == 96 && a.bias == nullptr && !a.accumulate && !a.nk_batch && !a.trace && a.Nk % 64 == 0 && a.Nk == a.Nkpad &&
        (!a.tk || (a.Tkpad <= 256 && a.Tkpad % 64 == 0))) return true;
    return false;
}

int launch_attention(const AttnArgs& a, hipStream_t stream) {
    const int g_attn_variant = lt_opt(OPT_ATTENTION_VARIANT);
    LT_REQUIRE(a.H % a.Hkv == 0, "attention: H=%d not a multiple of Hkv=%d", a.H, a.Hkv);
    LT_REQUIRE(a.q_raw == nullptr || a.nk_batch == nullptr,
               "attention: q_raw with nk_batch (per-sample key counts) is not built: the prologue takes one rope_grid_w, packed batches have one per sample");
    LT_REQUIRE(a.q_raw == nullptr || (attention_takes_raw_q(a) && a.q_stat && a.q_ln_w && a.q_ln_b && a.rope_cs && a.rope_cs_t && a.rope_grid_w > 0 && a.rope_cs_len > 0),
               "attention: q_raw (q_norm + RoPE in the prologue) needs the head_dim-72 one-wave kernel's conditions and the LayerNorm / RoPE inputs");
    LT_REQUIRE(a.q_raw == nullptr || ((a.N - 1) / a.rope_grid_w < a.rope_cs_len && a.rope_grid_w <= a.rope_cs_len),
               "attention: q_raw token grid exceeds the RoPE table (%d)", a.rope_cs_len);
    LT_REQUIRE(a.q != nullptr || a.q_raw != nullptr, "attention: no query tensor");
    LT_REQUIRE(a.Nkpad % 64 == 0 && a.Nkpad >= a.Nk && a.Nk > 0 && a.N > 0, "attention: bad key counts Nk=%d Nkpad=%d", a.Nk, a.Nkpad);
    LT_REQUIRE(!a.accumulate || a.gate != nullptr, "attention: accumulate mode needs a gate");
    LT_REQUIRE(a.scale > 0.f, "attention: softmax scale must be positive");
    LT_REQUIRE(a.q_batch_map == nullptr || a.bias != nullptr, "attention: q_batch_map is built for the masked (text) kernels only");
    LT_REQUIRE(!a.out_pair || attention_is_one_wave(a), "attention: out_pair (pair layout of the output) is written by the one-wave kernels only");
    const int nqb = (a.N + 127) / 128;
    dim3 grid(a.B * a.H * nqb), block(256);
#define LAUNCH_V1(HD_) hipLaunchKernelGGL(attn_fwd_kernel<HD_>, grid, block, 2 * (64 * HD_ * 2) + 2 * (HD_ * 128), stream, a)
#define LAUNCH_V2(HD_) hipLaunchKernelGGL(attn_fwd_kernel_v2<HD_>, grid, block, 2 * (64 * HD_ * 2) + 2 * (HD_ * 128 + 128), stream, a)
    if (a.tk) {
        LT_REQUIRE(a.k_prescaled && a.tvt && a.tbias && a.tgate && a.Tk > 0 && a.Tkpad % 64 == 0 && a.Tkpad >= a.Tk,
                   "attention: incomplete fused text arguments");
    }
    // variant 4: one wave per SIMD, 64 query rows per wave (attention_v4.hip); whole 64-key tiles and <= 256 text keys, else the ping-pong kernel
    // (nk_batch, per-sample key counts: its second instantiation; the hd 48 / 96 / 128 one-wave kernels below have none and keep refusing it)
    if (attention_one_wave_hd72(a))
        return launch_attention_v4(a, stream);
    // ... its head_dim 48 form (attention_v4_48.hip, round 4: the 600M ImageNet / MoE models)
    // (no text keys: no head_dim 48 model of the reference has a text branch, and the kernel's inherited text phase has no test)
    // From ~200 workgroups of 256 query rows on (2 x 32 heads x 1024 tokens): at the 600M models' 256 tokens the round-1 kernel's 128-row
    // workgroups fill the chip better (11.4 vs 12.2 us, profiles/r04/opbench_attn_hd48_v4_vs_v2.log); attention_variant 6 forces it.
    if (g_attn_variant >= 4 && a.hd == 48 && a.bias == nullptr && !a.accumulate && !a.nk_batch && !a.trace && a.Nk % 64 == 0 && !a.tk &&
        (g_attn_variant == 6 || (long long)a.B * a.H * ((a.N + 255) / 256) >= 200))
        return launch_attention_v4_hd48(a, stream);
    // ... and its head_dim 96 form (attention_v4_96.hip): whole tiles, the text phase's mask on the VALU
    if (g_attn_variant >= 4 && a.hd == 96 && a.bias == nullptr && !a.accumulate && !a.nk_batch && !a.trace && a.Nk % 64 == 0 && a.Nk == a.Nkpad &&
        (!a.tk || (a.Tkpad <= 256 && a.Tkpad % 64 == 0)))
        return launch_attention_v4_hd96(a, stream);
    // head_dim 128 (the 7B models), whole tiles: attention_hd128.hip; everything else at this head dim falls to attn_fwd_kernel<128> below
    if (attention_takes_hd128_fast(a)) return launch_attention_hd128(a, stream);
    if (g_attn_variant >= 3 && (a.hd == 72 || a.hd == 96) && a.bias == nullptr && !a.accumulate) {
        constexpr int SMEM72 = 4 * (72 * 128 + 128) + 4 * (64 * 72 * 2) + 16, SMEM96 = 4 * (96 * 128) + 4 * (64 * 96 * 2) + 16;
        if (ensure_dynamic_lds((const void*)attn_fwd_kernel_v3<72>, SMEM72) || ensure_dynamic_lds((const void*)attn_fwd_kernel_v3<96>, SMEM96)) return 1;
        const int nqb3 = (a.N + 255) / 256;
        if (a.trace) {
            LT_REQUIRE(a.hd == 72, "attention trace: the hd 72 kernel is the instrumented one");
            if (ensure_dynamic_lds((const void*)attn_fwd_kernel_v3<72, true>, SMEM72)) return 1;  // (per device, under its mutex)
            hipLaunchKernelGGL((attn_fwd_kernel_v3<72, true>), dim3(a.B * a.H * nqb3), dim3(512), SMEM72, stream, a);
        } else if (a.hd == 72) {
            hipLaunchKernelGGL(attn_fwd_kernel_v3<72>, dim3(a.B * a.H * nqb3), dim3(512), SMEM72, stream, a);
        } else {
            hipLaunchKernelGGL(attn_fwd_kernel_v3<96>, dim3(a.B * a.H * nqb3), dim3(512), SMEM96, stream, a);
        }
        LT_CHECK_HIP(hipGetLastError());
        return 0;
    }
    LT_REQUIRE(a.trace == nullptr, "attention trace: only the hd 72 self-attention kernel (variant 3) is instrumented");
    LT_REQUIRE(a.tk == nullptr, "attention: fused text cross-attention needs the ping-pong kernel (hd 72 / 96, use attention_fuses_text())");
    const bool v2 = g_attn_variant >= 2;  // (variant 3 falls back to v2 for text attention and other head dims)
    switch (a.hd) {
        case 48: if (v2) LAUNCH_V2(48); else LAUNCH_V1(48); break;
        case 72: if (v2) LAUNCH_V2(72); else LAUNCH_V1(72); break;
        case 96: LAUNCH_V1(96); break;
        case 128:  // exactly 64 KiB of dynamic LDS
            if (ensure_dynamic_lds((const void*)attn_fwd_kernel<128>, 2 * (64 * 128 * 2) + 2 * (128 * 128))) return 1;
            LAUNCH_V1(128);
            break;
        default: lt_set_error("attention: head_dim %d not built (48, 72, 96, 128)", a.hd); return 2;
    }
#undef LAUNCH_V1
#undef LAUNCH_V2
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

// name of the kernel launch_attention() would launch for `a` under the current options: the dispatch above, expression by expression
const char* attention_describe(const AttnArgs& a) {
    const int g_attn_variant = lt_opt(OPT_ATTENTION_VARIANT);
    if (a.hd != 48 && a.hd != 72 && a.hd != 96 && a.hd != 128) return "none";
    if (attention_one_wave_hd72(a)) return "attn_fwd_kernel_v4<72>";  // (both instantiations: with nk_batch its PerSampleKeys one)
    if (attention_is_one_wave(a)) return a.hd == 48 ? "attn_fwd_kernel_v4h48" : "attn_fwd_kernel_v4h96";
    if (attention_takes_hd128_fast(a)) return "attn_fwd_kernel_hd128";
    if (g_attn_variant >= 3 && (a.hd == 72 || a.hd == 96) && a.bias == nullptr && !a.accumulate) return a.hd == 72 ? "attn_fwd_kernel_v3<72>" : "attn_fwd_kernel_v3<96>";
    if (a.tk) return "none";
    if (a.hd == 96) return "attn_fwd_kernel<96>";
    if (a.hd == 128) return "attn_fwd_kernel<128>";
    if (g_attn_variant >= 2) return a.hd == 48 ? "attn_fwd_kernel_v2<48>" : "attn_fwd_kernel_v2<72>";
    return a.hd == 48 ? "attn_fwd_kernel<48>" : "attn_fwd_kernel<72>";
}

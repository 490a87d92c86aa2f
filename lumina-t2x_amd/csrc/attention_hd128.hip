// Self-attention for head_dim 128 (the 7B Next-DiT / Flag-DiT / Next-DiT-MoE factories: dim 4096, 32 heads), whole 64-key tiles, no key bias.
// Plain HIP with MFMA builtins; the structure is the two-group ping-pong of attn_fwd_kernel_v3 (attention.hip) carried to the head dim
// that pads nothing and fills a phase with matrix work:
//  * workgroup = 8 waves = 256 query rows (32 per wave), two waves per SIMD.  K / V^T tiles of 64 keys live in 4-slot LDS rings shared by
//    all 8 waves (2 x 64 KiB), filled by LDS-DMA (buffer_load ... lds, 1-KiB pieces, four per wave and tile pair) from the layouts the
//    engine already writes: K head-major [B, Hkv, N, 128], V^T [B, Hkv, 128, Npad] key-permuted by v_transpose.
//  * "swapped" QK^T (S^T = K Q^T, v_mfma_f32_32x32x16_bf16): a lane holds 32 scores of ONE query row, P's fragment for O^T = V^T P^T is the
//    lane's own registers.  8 exact k-steps, 4 exact 32-row blocks of O^T: 32 MFMAs per tile and wave, every flop a useful one.
//  * per tile a wave runs   X(t): P.V of tile t-1 + QK^T of tile t (32 MFMAs, one fragment ds_read per MFMA, pinned with
//    sched_group_barrier) + the LDS-DMA issue for {K(t+3), V(t+2)} | s_barrier |   Y(t): softmax of tile t on the VALU | s_barrier,
//    and waves 4..7 run one barrier interval late: on every SIMD one wave feeds the matrix pipe (1024 cycles) while the other does its
//    max / exp2 / pack / row sum (~130 VALU issues).
//  * arithmetic of the other kernels: exp2 domain (K pre-scaled by the engine, else Q pre-scaled here), online softmax with the deferred
//    rescale (threshold 2^8; the decision is taken with the previous tile's P.V complete and before this tile's P exists), P rounded to
//    bf16 before P.V, the row sum taken from the SAME rounded P (v_dot2_f32_bf16 with (1, 1)), fp32 O^T.
//  * K rows are 256 bytes = all 64 LDS banks: chunk c of row r is kept at position c ^ (r & 15), applied on the per-lane SOURCE address of
//    the DMA (its LDS image is lane-linear) and on the fragment reads; V^T rows (128 bytes) keep the chunk swizzle c ^ ((d >> 1) & 7).
//  * XCD-aware block order (a head's query blocks run back to back on one XCD); the output leaves through wave-private LDS strips as
//    whole 256-byte rows.
// Hazards (barrier-interval units; X(t) of group g runs in interval 2t + g, Y(t) in 2t + g + 1):
//   {K(t+3), V(t+2)} are issued in X(t) into the slots of K(t-1) / V(t-2), both last read in X(t-1) = interval 2t - 2 + g' < 2t + g with a
//   barrier in between; a wave waits for them at the end of X(t+1) (vmcnt(4): only X(t+1)'s own batch stays in flight), i.e. by interval
//   2t + 3 at the latest, and they are first read in X(t+2) (V) / X(t+3) (K) = interval 2t + 4 or later.
// No text phase (no head_dim-128 model of the reference has a text branch) and no pair-layout output: launch_attention keeps
// attention_is_one_wave() false at this head dim.
#include "common.h"
#include "kernels.h"
#include "options.h"
#include <type_traits>

namespace lt_attn128 {

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

__global__ __launch_bounds__(512, 1) void attn_fwd_kernel_hd128(AttnArgs p) {
    constexpr int HD = 128, KS = 8, DT = 4;
    constexpr int KTILE = 64 * HD * 2, VTILE = HD * 128;  // 16 KiB each
    constexpr int K_BASE = 0, V_BASE = 4 * KTILE;          // K ring | V^T ring; the K ring doubles as the output strips (8 x 8 KiB)
    constexpr float THR = 8.0f;
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
    const int ntile = p.Nk / 64;

    // ---- staging: 16 + 16 one-KiB pieces per (K, V^T) tile pair, wave w issues K pieces w, w + 8 and V^T pieces w, w + 8 -----------------
    // K piece j = chunk positions 64 j + lane of the tile's LDS image: row 4 j + lane / 16, position lane % 16, fetched from source chunk
    // position ^ (row & 15); V^T piece j = rows 8 j .. 8 j + 7 (128-byte rows, chunk-swizzled on the source)
    const __amdgpu_buffer_rsrc_t rK = __builtin_amdgcn_make_buffer_rsrc((void*)(p.k + (size_t)bhk * p.Nk * HD), 0, (int)((size_t)p.Nk * HD * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rV = __builtin_amdgcn_make_buffer_rsrc((void*)(p.vt + (size_t)bhk * HD * p.Nkpad), 0, (int)((size_t)HD * p.Nkpad * 2), 0x00020000);
    int kvo[2], vvo[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int j = wave + 8 * i;
        const int row = 4 * j + (lane >> 4);
        kvo[i] = row * (HD * 2) + (((lane & 15) ^ (row & 15)) << 4);
        const int d = 8 * j + (lane >> 3);
        vvo[i] = d * p.Nkpad * 2 + (((lane & 7) ^ ((d >> 1) & 7)) << 4);
    }
    auto dma_k = [&](int t) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rK, LDS_PTR(smem + K_BASE + (t & 3) * KTILE + (wave + 8 * i) * 1024), 16, kvo[i], t * KTILE, 0, 0);
    };
    auto dma_v = [&](int t) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rV, LDS_PTR(smem + V_BASE + (t & 3) * VTILE + (wave + 8 * i) * 1024), 16, vvo[i], t * 128, 0, 0);
    };
    // prologue: K(0), K(1), K(2), V(0), V(1) (tiles past the end read zeros through the descriptor bounds and are never consumed)
    dma_k(0); dma_v(0); dma_k(1); dma_v(1); dma_k(2);

    // ---- Q fragments (B operand of S^T = K Q^T): lane = (q row l31, d = 16 s + 8 hi .. +8), in the log2 domain ------------------------
    int qrow = qb * 256 + wave * 32 + l31;
    if (qrow > p.N - 1) qrow = p.N - 1;
    const u16* qptr = p.q + ((size_t)bh * p.N + qrow) * HD;
    const float sl2 = p.k_prescaled ? 1.0f : p.scale * 1.44269504088896340736f;
    bf16x8 qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const bf8_t raw = *(const bf8_t*)(qptr + 16 * s + 8 * hi);
        if (p.k_prescaled) qf[s] = __builtin_bit_cast(bf16x8, raw);
        else {
            float f[8];
            unpack8(raw, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[s][e] = (__bf16)(f[e] * sl2);
        }
    }

    // ---- per-lane LDS read offsets: K row l31 (+ 32 kt2), chunk 2 s + hi swizzled by the row; V^T row 32 dt + l31, chunk 2 g + hi ------
    int kco[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) kco[s] = K_BASE + l31 * (HD * 2) + (((2 * s + hi) ^ (l31 & 15)) << 4);
    int vco[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) vco[g] = V_BASE + l31 * 128 + (((2 * g + hi) ^ ((l31 >> 1) & 7)) << 4);  // (+ dt * 4096: bits 1..3 of the row are l31's)

    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    f32x16 sc[2];
    bf16x8 pa[4];
    float m_run = -1.0e30f;
    float l4[4] = {0.f, 0.f, 0.f, 0.f};  // this lane's half of the row sum, four chains (the other half lives on lane ^ 32)

    auto bar = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    bar();
    if (grp == 1) bar();

    // X phase: P.V of the previous tile (P in pa, V^T slot (t - 1) & 3) and QK^T of tile t (K slot t & 3).  All fragment reads are written
    // first and the order is pinned: six reads ahead of the first MFMA, then one read per MFMA.
    auto phase_x = [&](int t, auto pv_c, auto qk_c) __attribute__((always_inline)) {
        constexpr bool PV = decltype(pv_c)::value, QK = decltype(qk_c)::value;
        constexpr int NF = (PV ? 16 : 0) + (QK ? 16 : 0);
        __builtin_amdgcn_s_setprio(1);
        const char* kb = smem + (t & 3) * KTILE;
        const char* vb = smem + ((t + 3) & 3) * VTILE;
        bf16x8 fr[NF];
        int n = 0;
        if constexpr (PV) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) fr[n++] = *(const bf16x8*)(vb + dt * 4096 + vco[g]);
        }
        if constexpr (QK) {
#pragma unroll
            for (int s = 0; s < KS; ++s)
#pragma unroll
                for (int kt2 = 0; kt2 < 2; ++kt2) fr[n++] = *(const bf16x8*)(kb + kt2 * (32 * HD * 2) + kco[s]);
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
        __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
        for (int i = 0; i < NF - 6; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x8, 6, 0);
        __builtin_amdgcn_s_setprio(0);
    };
    using T_ = std::true_type;
    using F_ = std::false_type;

    // Y phase: softmax of the tile in sc -> pa.  The previous tile's P.V is complete (X phase), this tile's P does not exist yet: the
    // rescale multiplies O and l only.
    auto phase_y = [&]() __attribute__((always_inline)) {
        float mx = fmaxf(sc[0][0], sc[1][0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(fmaxf(mx, sc[0][r]), sc[1][r]);
        {
            auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
            mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
        }
        const bool raise = mx > m_run + THR;
        if (__builtin_expect(__any(raise), 0)) {
            const float m_new = raise ? mx : m_run;
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            m_run = m_new;
#pragma unroll
            for (int j = 0; j < 4; ++j) l4[j] *= alpha;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
        }
        const bf16x2_t ones = {(__bf16)1.0f, (__bf16)1.0f};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                const float p0 = __builtin_amdgcn_exp2f(sc[g >> 1][8 * (g & 1) + e] - m_run);
                const float p1 = __builtin_amdgcn_exp2f(sc[g >> 1][8 * (g & 1) + e + 1] - m_run);
                const bf16x2_t pk = __builtin_convertvector(f32x2{p0, p1}, bf16x2_t);
                pa[g][e] = pk[0];
                pa[g][e + 1] = pk[1];
                l4[(e >> 1) & 3] = __builtin_amdgcn_fdot2_f32_bf16(pk, ones, l4[(e >> 1) & 3], false);  // the row sum of the ROUNDED P
            }
        }
        // keep the bf16 packing in THIS phase (hipcc otherwise sinks the cvt_pk next to the P.V MFMAs of the X phase)
#pragma unroll
        for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(pa[g]));
    };

    for (int t = 0; t < ntile; ++t) {
        const bool more = t + 2 < ntile;
        if (more) { dma_k(t + 3); dma_v(t + 2); }
        __builtin_amdgcn_sched_barrier(0);
        if (t == 0) phase_x(0, F_{}, T_{});
        else phase_x(t, T_{}, T_{});
        __builtin_amdgcn_sched_barrier(0);
        // the batch issued in X(t-1) must have landed; only X(t)'s own four loads may stay in flight
        if (more) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bar();
        phase_y();
        bar();
    }
    phase_x(ntile, T_{}, F_{});  // P.V of the last tile
    if (grp == 0) bar();         // the barrier group 1 still needs after its last Y phase

    // ---- epilogue: lane holds out[q = l31][d = 32 dt + 8 q4 + 4 hi + j]; rows leave through the wave's own 8-KiB strip of the (now idle)
    //      K ring - its last reader was X(ntile - 1), two barriers ago for either group - as whole 256-byte rows.  16-byte chunk c of row r
    //      sits at position c ^ (r & 15) in the strip (the per-lane 8-byte writes of one row stride would otherwise share their banks). ------
    float l_run = (l4[0] + l4[1]) + (l4[2] + l4[3]);
    l_run += __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_run;
    char* strip = smem + K_BASE + wave * (32 * HD * 2);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int ch = 4 * dt + q4;  // 16-byte chunk of d0 = 32 dt + 8 q4 (+ 4 hi: its upper half)
            u32x2 w = {pack2bf(o[dt][4 * q4] * inv, o[dt][4 * q4 + 1] * inv), pack2bf(o[dt][4 * q4 + 2] * inv, o[dt][4 * q4 + 3] * inv)};
            *(u32x2*)(strip + l31 * (HD * 2) + ((ch ^ (l31 & 15)) << 4) + 8 * hi) = w;
        }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int row0 = qb * 256 + wave * 32;
    u16* obase = p.out + ((size_t)b * p.N + row0) * ((size_t)p.H * HD) + (size_t)h * HD;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = 4 * i + (lane >> 4), c = lane & 15;
        if (row0 + r < p.N)
            *(u32x4*)(obase + (size_t)r * ((size_t)p.H * HD) + c * 8) = *(const u32x4*)(strip + r * (HD * 2) + ((c ^ (r & 15)) << 4));
    }
}

}  // namespace lt_attn128

// the dispatch condition of the kernel above (launch_attention and the describe entry use this one expression)
bool attention_takes_hd128_fast(const AttnArgs& a) {
    return lt_opt(OPT_ATTENTION_VARIANT) >= 4 && a.hd == 128 && a.bias == nullptr && !a.accumulate && !a.nk_batch && !a.trace && !a.q_raw && !a.q_batch_map &&
           !a.out_pair && a.Nk % 64 == 0 && a.Nk == a.Nkpad && !a.tk;
}

int launch_attention_hd128(const AttnArgs& a, hipStream_t stream) {
    LT_REQUIRE(a.hd == 128 && !a.bias && !a.accumulate && !a.nk_batch && !a.tk && !a.out_pair && a.q && a.Nk % 64 == 0 && a.Nk == a.Nkpad && a.N > 0,
               "attention hd 128: the whole-tile kernel needs Nk %% 64 == 0 == Nkpad - Nk, no bias / accumulate / per-sample key counts / text keys");
    // 32-bit buffer offsets inside one head: K tile offsets run to (ntile + 2) tiles, V^T rows to 128 x Nkpad x 2 bytes
    LT_REQUIRE((long long)a.Nkpad * 128 * 2 + 3 * 16384 < (1ll << 31), "attention hd 128: %d keys exceed the 32-bit buffer offsets", a.Nk);
    constexpr int SMEM = 8 * 16384;
    if (ensure_dynamic_lds((const void*)lt_attn128::attn_fwd_kernel_hd128, SMEM)) return 1;  // per (device, kernel)
    const int nqb = (a.N + 255) / 256;
    hipLaunchKernelGGL(lt_attn128::attn_fwd_kernel_hd128, dim3(a.B * a.H * nqb), dim3(512), SMEM, stream, a);
    LT_CHECK_HIP(hipGetLastError());
    return 0;
}

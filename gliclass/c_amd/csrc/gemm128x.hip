// 128x128 tile of the MX cross-term GEMM (gemm256x.hip) for forwards too small to fill the chip with 256x256 tiles: C = A . W^T on the same
// GX operand rows (glc_common.h), the same weight copies and exponents, the same fp8 range counter.  Opt-in: the engine reaches it only
// through glc_engine_set_mx_small_forwards (engine.hip GemmGs); tests reach it through glc_debug_gemm_run (GLC_GEMM_RUN_MX128).
//
// Geometry: four waves (2 x 2), each a 64 x 64 sub-tile = acc[2][2] blocks of 32x32 fp32.  K goes in 32-element groups; the 128 A rows and
// the 128 W rows of a group are one 128-byte GX group per row and come into LDS by LDS-DMA (global_load_lds_dwordx4; every wave fetches 32
// rows of each operand as 4 + 4 one-KiB pieces), landing as [128 rows][128 B] with the source-side 16-byte chunk swizzle c ^ ((row >> 1) & 7)
// of the 256 tile, so the ds_read_b128 fragment reads stay conflict-free.  Ring: 4 stages of 16 KiB (A and W of two groups) = 64 KiB, so two
// workgroups share a CU and one's load phase hides behind the other's MFMAs (as attention_mx.hip with NW = 4).  One barrier per group:
//   request group s + 1 | read the f16 and fp8 fragments of group s | 8 x 32x32x16 f16, 4 x 32x32x64 scaled | wait for my pieces | barrier
// Hazards: group s + 1 lands in the stages group s - 1 was read from; every wave's reads of s - 1 are complete (their values fed MFMAs)
// before it reaches the barrier that closes step s - 1, and the requests are issued behind that barrier.  A wave waits for its own pieces
// (vmcnt(0)) ahead of the barrier, so behind it all of group s + 1 is in LDS.
//
// Arithmetic order per accumulator block and group — f16 k 0-15, f16 k 16-31, then the scaled MFMA of both cross terms, groups ascending —
// is that of both wave tiles of gemm256x.hip, and the epilogues below are that file's (its 8-wave tile: a wave's sub-tile there is
// 128 x 64, here 64 x 64, i.e. two 32-row chunks instead of four): on the same operand images the outputs, the ln_part partials and the range
// counter must be bit-identical to the 256 tile's (tests/test_gpu_gemm128x.py asserts it).  Fragment maps, row formats and the epilogue's staging: see
// gemm256x.hip.  Epilogues: EPI_BIAS, EPI_GELU, EPI_RESID (GX residual), EPI_QKV; the decoder / ModernBERT ones are not built here.
#include <stdlib.h>
#include "glc_common.h"
#include "glc_kernels.h"
#include "glc_layout.h"

namespace {

constexpr int TM = 128, TN = 128;
constexpr int LINE = 128;                  // bytes per row and group
constexpr int STAGE = TM * LINE;           // 16 KiB: one operand's rows of one group
constexpr int NSLOT = 4;                   // ring stages: stage 2 s = A rows of group s, 2 s + 1 = W rows; slot = stage & 3
constexpr int EPI_PATCH = 9216;            // bytes of wave-private fp32 epilogue staging (4 waves: 36 KiB of the ring)
static_assert(NSLOT * STAGE <= 80 * 1024 && 4 * EPI_PATCH <= NSLOT * STAGE, "two workgroups per CU; the epilogue stages inside the ring");
extern __shared__ __attribute__((aligned(16))) unsigned char smem128x[];
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;

// (the request through the compiler's builtin: it sets m0 itself — no hand-written m0 write to get the clobbers of wrong)
__device__ __forceinline__ void glds16(const void* g, unsigned char* l) {
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)g, (void __attribute__((address_space(3)))*)l, 16, 0, 0);
}

// XCD-aware tile order (gemm256s.hip): this workgroup's (M-tile, N-tile) of a launch over ntn N-tiles, row-major inside an XCD's share
__device__ __forceinline__ void s_tile_of_block(int ntn, int& mt, int& nt) {
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
    const int tile = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
    mt = tile / ntn; nt = tile % ntn;
}

template <int EPI, bool VMODE>
__device__ __forceinline__ void gemm128x_tile(const GemmArgs& p, int n_tile0, int ntn) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int c32 = lane & 31, h = lane >> 5;
    const int K = p.K, N = p.N;

    int mt, nt;
    s_tile_of_block(ntn, mt, nt);
    const int m0 = mt * TM, n0 = (n_tile0 + nt) * TN;
    if constexpr (EPI == EPI_QKV && !VMODE) {
        if (p.q_tile_flag && n0 < p.H) {                // Q third, pruned last layer: nobody reads query tiles without selected rows
            const unsigned f4 = *reinterpret_cast<const unsigned*>(p.q_tile_flag + (m0 >> 5));      // this tile's four 32-row flags
            if (f4 == 0u) return;
        }
    }

    const unsigned char* __restrict__ A = reinterpret_cast<const unsigned char*>(p.A);
    const unsigned char* __restrict__ W = reinterpret_cast<const unsigned char*>(p.W);
    const size_t rsb = (size_t)4 * K;          // row stride in bytes (GX rows)
    const int ng = K / 32;
    // DMA map (gemm256x.hip): lane L lands at (row L >> 3, physical chunk L & 7) of an 8-row piece and fetches logical chunk (L & 7) ^ ((row >> 1) & 7)
    const int lrow8 = lane >> 3, pch = lane & 7;
    const unsigned char* fa[2];
    const unsigned char* fw[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = wave * 32 + i * 8 + lrow8;
        const int lc = pch ^ ((row >> 1) & 7);
        fa[i] = A + (size_t)(m0 + row) * rsb + lc * 16;
        fw[i] = W + (size_t)(n0 + row) * rsb + lc * 16;
    }
    auto stage_fl = [&](int grp) {          // this wave's 32 A rows and 32 W rows of group grp: 4 + 4 one-KiB pieces
        unsigned char* sa = smem128x + ((2 * grp) & (NSLOT - 1)) * STAGE + (wave * 32) * LINE;
        unsigned char* sw = smem128x + ((2 * grp + 1) & (NSLOT - 1)) * STAGE + (wave * 32) * LINE;
        const size_t o = (size_t)grp * LINE;
#pragma unroll
        for (int i = 0; i < 4; ++i) glds16(fa[i & 1] + (size_t)(i >> 1) * 16 * rsb + o, sa + i * 8 * LINE);
#pragma unroll
        for (int i = 0; i < 4; ++i) glds16(fw[i & 1] + (size_t)(i >> 1) * 16 * rsb + o, sw + i * 8 * LINE);
    };

    f32x16 acc[2][2];          // [row block][column block]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment read offsets inside a slot
    const int hsw = (c32 >> 1) & 7;
    const int arow = (wm * 64 + c32) * LINE, wrow = (wn * 64 + c32) * LINE;
    const int ck0 = ((0 + h) ^ hsw) * 16, ck1 = ((2 + h) ^ hsw) * 16;               // f16 k-steps 0 / 1: logical chunks h / 2 + h
    const int cx0 = ((4 + 2 * h) ^ hsw) * 16, cx1 = ((5 + 2 * h) ^ hsw) * 16;       // the fp8 parts of elements 16 h .. 16 h + 7 / + 8 .. + 15
    const int sc_a = 127 - GLC_GX_SHIFT - p.act_sc;        // e8m0 scale of the A blocks: 2^-(SHIFT + sc) (glc_common.h)
    const int sc_w = 127 - p.mx_ws;

    auto ld32 = [&](const unsigned char* q0, int o0, int o1) __attribute__((always_inline)) {      // two 16-byte chunks -> one 32-byte MX operand
        const i32x4 t0 = *reinterpret_cast<const i32x4*>(q0 + o0);
        const i32x4 t1 = *reinterpret_cast<const i32x4*>(q0 + o1);
        i32x8 r;
        r[0] = t0[0]; r[1] = t0[1]; r[2] = t0[2]; r[3] = t0[3]; r[4] = t1[0]; r[5] = t1[1]; r[6] = t1[2]; r[7] = t1[3];
        return r;
    };
    stage_fl(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();              // group 0 is in LDS for everyone
    for (int s = 0; s < ng; ++s) {
        if (s + 1 < ng) stage_fl(s + 1);       // (wave-uniform; the last group requests nothing)
        f16x8 a16[2][2], w16[2][2];
        i32x8 xa[2], xw[2];
        const unsigned char* sa = smem128x + ((2 * s) & (NSLOT - 1)) * STAGE + arow;
        const unsigned char* sw = smem128x + ((2 * s + 1) & (NSLOT - 1)) * STAGE + wrow;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            w16[j][0] = *reinterpret_cast<const f16x8*>(sw + j * 32 * LINE + ck0);
            w16[j][1] = *reinterpret_cast<const f16x8*>(sw + j * 32 * LINE + ck1);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a16[i][0] = *reinterpret_cast<const f16x8*>(sa + i * 32 * LINE + ck0);
            a16[i][1] = *reinterpret_cast<const f16x8*>(sa + i * 32 * LINE + ck1);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) xw[j] = ld32(sw + j * 32 * LINE, cx0, cx1);      // [w_hi8 w_lo8 | w_hi8 w_lo8] of 2 x 8 elements
#pragma unroll
        for (int i = 0; i < 2; ++i) xa[i] = ld32(sa + i * 32 * LINE, cx0, cx1);      // [a_lo8 a_hi8 | a_lo8 a_hi8]
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (!VMODE) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w16[j][ks], a16[i][ks], acc[i][j], 0, 0, 0);      // D[n][m]
                    else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a16[i][ks], w16[j][ks], acc[i][j], 0, 0, 0);            // D[m][n]
                }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (!VMODE) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(xw[j], xa[i], acc[i][j], 0, 0, 0, sc_w, 0, sc_a);
                else acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(xa[i], xw[j], acc[i][j], 0, 0, 0, sc_a, 0, sc_w);
            }
        // my pieces of group s + 1 have landed and my reads of group s are done; behind the barrier that holds for every wave
        // (the scheduling fence keeps the MFMAs ahead of the wait: they are what the requests' latency hides behind)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    // (every wave is through its last fragment read: the ring becomes the epilogue's staging space)

    // ---------------- epilogue (gemm256x.hip's, over two 32-row chunks) ----------------
    typedef f16_t T;
    typedef __attribute__((ext_vector_type(8))) T vec8T;
    const float* __restrict__ bias = p.bias;
    float* stg = reinterpret_cast<float*>(smem128x + wave * EPI_PATCH);
    const int qkv_b0 = EPI == EPI_QKV ? m0 / p.Sp : 0;
    const float kHi = gx_act_khi(p.act_sc), kLo = gx_act_klo(p.act_sc), kInvLo = gx_pow2_inv(kLo);       // activation rows in and out: exponent act_sc
    constexpr float kInvLo0 = 1.0f / (float)(1 << GLC_GX_SHIFT);                                          // MX tiles (attention operands): exponent 0
    if constexpr (!VMODE) {
        // D[n = 32 J + 8 q + 4 h + e][m = 32 I + c32]; patch [32 rows m][64 cols n], row stride 68 floats
        const int which = (EPI == EPI_QKV) ? n0 / p.H : 0;
        const bool lnf = EPI != EPI_RESID && p.a_stats != nullptr;
        f32x4 bj[2][4], cj[2][4];
#pragma unroll
        for (int J = 0; J < 2; ++J)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int nn = n0 + wn * 64 + 32 * J + 8 * q + 4 * h;
                bj[J][q] = bias ? *reinterpret_cast<const f32x4*>(bias + nn) : (f32x4){0.f, 0.f, 0.f, 0.f};
                cj[J][q] = (lnf && p.ln_c) ? *reinterpret_cast<const f32x4*>(p.ln_c + nn) : (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        float rg[8], rb[8];
        const bool rln = EPI == EPI_RESID && p.r_stats != nullptr;
        const bool gxout = EPI == EPI_RESID && p.ln_part != nullptr;      // raw GX rows + statistics partials out
        if constexpr (EPI == EPI_RESID) {
            if (rln) {
                const int nb = n0 + wn * 64 + (lane & 7) * 8;
#pragma unroll
                for (int e = 0; e < 8; ++e) { rg[e] = p.r_gamma[nb + e]; rb[e] = p.r_beta[nb + e]; }
            }
        }
        // residual rows (GX) one 32-row chunk ahead of their use: lane = 8 consecutive columns
        gs_h8 rpre[4]; u32x2 rpre_lo[4]; float2 rst_pre[4];
        auto load_resid = [&](int c, gs_h8 (&r)[4], u32x2 (&rl)[4], float2 (&rst)[4]) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int idx = lane + 64 * k, row = idx >> 3, g8 = idx & 7;
                if (rln) rst[k] = p.r_stats[m0 + wm * 64 + c * 32 + row];
                const int n = n0 + wn * 64 + g8 * 8;
                const unsigned char* rp = reinterpret_cast<const unsigned char*>(p.resid) + (size_t)(m0 + wm * 64 + c * 32 + row) * 4 * N + (n >> 5) * 128;
                r[k] = *reinterpret_cast<const gs_h8*>(rp + (n & 31) * 2);
                rl[k] = *reinterpret_cast<const u32x2*>(rp + 64 + (n & 31) * 2);
            }
        };
        if constexpr (EPI == EPI_RESID) { load_resid(0, rpre, rpre_lo, rst_pre); }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            gs_h8 rcur[4]; u32x2 rcur_lo[4]; float2 rst_cur[4];
            if (EPI == EPI_RESID) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { rcur[k] = rpre[k]; rcur_lo[k] = rpre_lo[k]; rst_cur[k] = rst_pre[k]; }
                if (c + 1 < 2) load_resid(c + 1, rpre, rpre_lo, rst_pre);
            }
            const float2 sm = lnf ? p.a_stats[m0 + wm * 64 + c * 32 + c32] : make_float2(0.f, 1.f);
#pragma unroll
            for (int J = 0; J < 2; ++J)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f32x4 v = {acc[c][J][4 * q], acc[c][J][4 * q + 1], acc[c][J][4 * q + 2], acc[c][J][4 * q + 3]};
                    if constexpr (EPI != EPI_RESID) {
                        if (lnf) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) v[r] = sm.y * (v[r] - sm.x * cj[J][q][r]);
                        }
                    }
                    v += bj[J][q];
                    if (EPI == EPI_GELU) { const f32x2 g0 = glc_gelu2_f32((f32x2){v[0], v[1]}), g1 = glc_gelu2_f32((f32x2){v[2], v[3]}); v = (f32x4){g0[0], g0[1], g1[0], g1[1]}; }
                    *reinterpret_cast<f32x4*>(stg + c32 * 68 + 32 * J + 8 * q + 4 * h) = v;
                }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int idx = lane + 64 * k, row = idx >> 3, g8 = idx & 7;
                const f32x4 lo = *reinterpret_cast<const f32x4*>(stg + row * 68 + g8 * 8);
                const f32x4 hi = *reinterpret_cast<const f32x4*>(stg + row * 68 + g8 * 8 + 4);
                float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                const int m = m0 + wm * 64 + c * 32 + row;
                const int n = n0 + wn * 64 + g8 * 8;
                if constexpr (EPI == EPI_RESID) {
                    float r[8];
                    gx_decode8(rcur[k], rcur_lo[k], kInvLo, r);
                    if (rln) {           // raw residual row: LayerNorm on the fly
                        const float2 rs = rst_cur[k];
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] += (r[e] - rs.x) * rs.y * rg[e] + rb[e];
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] += r[e];
                    }
                    if (gxout) {
                        // raw GX row out + this 64-column block's (sum, squared deviations from the block mean) of the row (the 256 tile's reduction)
                        float s1 = 0.f, s2 = 0.f;
#pragma unroll
                        for (int e = 0; e < 8; ++e) s1 += v[e];
#pragma unroll
                        for (int o = 1; o < 8; o <<= 1) s1 += __shfl_xor(s1, o, 64);
                        const float bm = s1 * (1.0f / 64.0f);
#pragma unroll
                        for (int e = 0; e < 8; ++e) { const float dv = v[e] - bm; s2 += dv * dv; }
#pragma unroll
                        for (int o = 1; o < 8; o <<= 1) s2 += __shfl_xor(s2, o, 64);
                        if (g8 == 0) p.ln_part[(size_t)m * (N >> 6) + ((n0 + wn * 64) >> 6)] = make_float2(s1, s2);
                        gx_store8(reinterpret_cast<unsigned char*>(p.C) + (size_t)m * 4 * N, n, v, kHi, kLo, m < p.gx_rows ? p.gx_sat : nullptr);
                    } else {             // plain fp32 row (LayerNorm input)
                        float* cp = reinterpret_cast<float*>(p.C) + (size_t)m * N + n;
                        *reinterpret_cast<f32x4*>(cp) = (f32x4){v[0], v[1], v[2], v[3]};
                        *reinterpret_cast<f32x4*>(cp + 4) = (f32x4){v[4], v[5], v[6], v[7]};
                    }
                } else if constexpr (EPI == EPI_QKV) {
                    if (m < p.Mvalid) {
                        vec8T o, ol;
#pragma unroll
                        for (int e = 0; e < 8; ++e) { o[e] = (T)v[e]; ol[e] = (T)(v[e] - (float)o[e]); }
                        int b = qkv_b0, sq = m - qkv_b0 * p.Sp;
                        while (sq >= p.Sp) { sq -= p.Sp; ++b; }
                        const int nn = n - which * p.H, hh = nn >> 6, dd = nn & 63;
                        const int bh = b * p.nh + hh;
                        if (p.qkv_mxt) {        // MX tiles (glc_layout.h): f16 unit piece + the fp8 parts, Q as (hi8 | lo8), K as (lo8 | hi8)
                            gx_range_note(v, 1.0f, p.gx_sat && m < p.gx_rows ? p.gx_sat + 1 : nullptr);      // (tiles: the guard's second word)
                            u32x2 l8, h8;
                            gs_h8 oh;
                            gx_split8(v, 1.0f, kInvLo0, oh, l8, h8);
                            const int tile = bh * (p.Sp >> 5) + (sq >> 5), slot = which == 0 ? (sq & 31) : glc_pi32(sq & 31);
                            unsigned char* bq = reinterpret_cast<unsigned char*>(which == 0 ? p.Qh : p.Kh);
                            unsigned char* px = bq + glc_mxt_mx(tile, slot, dd);
                            *reinterpret_cast<vec8T*>(bq + glc_mxt_f16(tile, slot, dd)) = o;
                            *reinterpret_cast<u32x2*>(px) = which == 0 ? h8 : l8;
                            *reinterpret_cast<u32x2*>(px + 16) = which == 0 ? l8 : h8;
                            continue;
                        }
                        const size_t off = which == 0 ? glc_qoff(p.Sp, bh, sq, dd) : glc_koff(p.Sp, bh, sq, dd);
                        T* base = reinterpret_cast<T*>(which == 0 ? p.Qh : p.Kh);
                        *reinterpret_cast<vec8T*>(base + 2 * off) = o;          // split-f16 unit [8 hi | 8 lo]
                        *reinterpret_cast<vec8T*>(base + 2 * off + 8) = ol;
                    }
                } else {
                    if (p.gs_c_plain) {
                        float* cp = reinterpret_cast<float*>(p.C) + (size_t)m * N + n;
                        *reinterpret_cast<f32x4*>(cp) = (f32x4){v[0], v[1], v[2], v[3]};
                        *reinterpret_cast<f32x4*>(cp + 4) = (f32x4){v[4], v[5], v[6], v[7]};
                    } else
                    gx_store8<false, true>(reinterpret_cast<unsigned char*>(p.C) + (size_t)m * 4 * N, n, v, kHi, kLo, m < p.gx_rows ? p.gx_sat : nullptr);      // FFN1's intermediate: streams (non-temporal)
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
        }
    } else {
        // V third: D[m = 32 I + 8 q + 4 h + e][n = 32 J + c32]; patch [64 rows dd][32 cols key], row stride 36 floats
        float bn[2], cn[2] = {0.f, 0.f};
        const bool lnf = p.a_stats != nullptr;
#pragma unroll
        for (int J = 0; J < 2; ++J) {
            bn[J] = bias ? bias[n0 + wn * 64 + 32 * J + c32] : 0.f;
            if (lnf && p.ln_c) cn[J] = p.ln_c[n0 + wn * 64 + 32 * J + c32];
        }
        const int hh = (n0 + wn * 64 - 2 * p.H) >> 6;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int J = 0; J < 2; ++J)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f32x4 v = {acc[c][J][4 * q], acc[c][J][4 * q + 1], acc[c][J][4 * q + 2], acc[c][J][4 * q + 3]};
                    if (lnf) {      // accumulator rows m0 + 64 wm + 32 c + 8 q + 4 h + r
                        const float2* sp = p.a_stats + m0 + wm * 64 + c * 32 + 8 * q + 4 * h;
#pragma unroll
                        for (int r = 0; r < 4; ++r) { const float2 sm = sp[r]; v[r] = sm.y * (v[r] - sm.x * cn[J]); }
                    }
                    v[0] += bn[J]; v[1] += bn[J]; v[2] += bn[J]; v[3] += bn[J];
                    *reinterpret_cast<f32x4*>(stg + (32 * J + c32) * 36 + 8 * q + 4 * h) = v;
                }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int idx = lane + 64 * k, dd = idx >> 2, kg = idx & 3;
                const f32x4 lo = *reinterpret_cast<const f32x4*>(stg + dd * 36 + kg * 8);
                const f32x4 hi = *reinterpret_cast<const f32x4*>(stg + dd * 36 + kg * 8 + 4);
                vec8T o, ol;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] = (T)lo[e]; o[4 + e] = (T)hi[e];
                    ol[e] = (T)(lo[e] - (float)o[e]); ol[4 + e] = (T)(hi[e] - (float)o[4 + e]);
                }
                const int m = m0 + wm * 64 + c * 32 + kg * 8;           // first of 8 consecutive keys
                if (m < p.Mvalid) {
                    int b = qkv_b0, sq = m - qkv_b0 * p.Sp;
                    while (sq >= p.Sp) { sq -= p.Sp; ++b; }
                    if (p.qkv_mxt) {            // V^T MX tiles: (lo8 | hi8)
                        const float x8[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                        gx_range_note(x8, 1.0f, p.gx_sat && m < p.gx_rows ? p.gx_sat + 1 : nullptr);
                        u32x2 l8, h8;
                        gs_h8 oh;
                        gx_split8(x8, 1.0f, kInvLo0, oh, l8, h8);
                        const int tile = (b * p.nh + hh) * (p.Sp >> 5) + (sq >> 5);
                        unsigned char* bv = reinterpret_cast<unsigned char*>(p.Vt);
                        unsigned char* px = bv + glc_mxt_v_mx(tile, dd, sq);
                        *reinterpret_cast<vec8T*>(bv + glc_mxt_v_f16(tile, dd, sq)) = o;
                        *reinterpret_cast<u32x2*>(px) = l8;
                        *reinterpret_cast<u32x2*>(px + 16) = h8;
                        continue;
                    }
                    const size_t off = glc_voff(p.Sp, b * p.nh + hh, dd, sq);
                    *reinterpret_cast<vec8T*>(reinterpret_cast<T*>(p.Vt) + 2 * off) = o;
                    *reinterpret_cast<vec8T*>(reinterpret_cast<T*>(p.Vt) + 2 * off + 8) = ol;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// four waves, two workgroups per CU (64 KiB of LDS and at most 256 registers each)
template <int EPI, bool VMODE>
__global__ __launch_bounds__(256, 2) void gemm128x_kernel(GemmArgs p, int n_tile0, int ntn) { gemm128x_tile<EPI, VMODE>(p, n_tile0, ntn); }

template <int EPI, bool VMODE> const char* launch_x128(hipStream_t st, const GemmArgs& a, int n_tile0, int ntn) {
    static std::atomic<unsigned> lds_ok{0};
    constexpr int lds_bytes = NSLOT * STAGE;
    if (ntn <= 0) return nullptr;
    if (!glc_raise_lds_limit(gemm128x_kernel<EPI, VMODE>, lds_bytes, lds_ok)) return "gemm128x: cannot raise the dynamic LDS limit";
    hipLaunchKernelGGL((gemm128x_kernel<EPI, VMODE>), dim3((a.Mpad / TM) * ntn), dim3(256), lds_bytes, st, a, n_tile0, ntn);
    return nullptr;
}

}  // namespace

// Shapes the 128 tile takes.  EPI_QKV: the conditions of glc_gemm256x_supported with H % 128 (a tile must not straddle the Q / K / V thirds;
// the tile writers need no more: a wave's 64 columns are one head)
bool glc_gemm128x_supported(const GemmArgs& a, int epi) {
    if (!(a.Mpad > 0 && a.Mpad % TM == 0 && a.N > 0 && a.N % TN == 0 && a.K > 0 && a.K % 32 == 0)) return false;
    if (a.mx_ws < -40 || a.mx_ws > 60) return false;
    if (epi == EPI_QKV) return a.H > 0 && a.H % 128 == 0 && a.N == 3 * a.H && a.Sp % 64 == 0 && a.Sp >= 64 && a.nh * 64 == a.H;
    return epi == EPI_BIAS || epi == EPI_GELU || epi == EPI_RESID;
}

const char* glc_launch_gemm128x(hipStream_t st, int epi, const GemmArgs& a_in) {
    GemmArgs a = a_in;
    if (a.stamps || a.prio_mode >= 4) return "gemm128x: the MX GEMM has no stamped or timing-only build";
    if (!a.gx_sat) a.gx_sat = glc_gx_sat_ptr();              // fp8 range guard of the activation images this launch writes
    if (!a.act_sc) a.act_sc = glc_gx_act_sc();               // ... and the exponent of the activation rows (engine.hip act_sc)
    if (a.gx_rows <= 0) a.gx_rows = a.Mvalid > 0 ? a.Mvalid : a.Mpad;     // ... over the rows that exist (slack rows up to Mpad hold leftovers)
    if (epi != EPI_BIAS && epi != EPI_GELU && epi != EPI_RESID && epi != EPI_QKV) return "gemm128x: this epilogue is built for the 256 tile only";
    if (!glc_gemm128x_supported(a, epi)) return "gemm128x: unsupported shape";
    if (!a.A || !a.W) return "gemm128x: null operand";
    if (epi == EPI_QKV) { if (!a.Qh || !a.Kh || !a.Vt) return "gemm128x: null QKV output"; }
    else if (!a.C) return "gemm128x: null output";
    if (epi == EPI_RESID && !a.resid) return "gemm128x: null residual";
    if (epi == EPI_RESID && a.gs_resid_plain) return "gemm128x: a plain fp32 residual is built for the 256 tile only";
    if (epi == EPI_BIAS && a.perm_cols) return "gemm128x: permuted columns are built for the 256 tile only";
    const int ntn = a.N / TN;
    switch (epi) {
        case EPI_BIAS: return launch_x128<EPI_BIAS, false>(st, a, 0, ntn);
        case EPI_GELU: return launch_x128<EPI_GELU, false>(st, a, 0, ntn);
        case EPI_RESID: return launch_x128<EPI_RESID, false>(st, a, 0, ntn);
        case EPI_QKV: {
            const int nqk = 2 * a.H / TN, nq = a.qkv_skip_q ? a.H / TN : 0;
            const char* m = launch_x128<EPI_QKV, false>(st, a, nq, nqk - nq);
            return m ? m : launch_x128<EPI_QKV, true>(st, a, nqk, ntn - nqk);
        }
    }
    return "gemm128x: bad epilogue";
}

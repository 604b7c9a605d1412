// 256x256 GEMM of the default mode with MX cross terms (round 3): C = A . W^T on "GX" operand rows (glc_common.h):
//   a * w = a_hi * w_hi            two v_mfma_f32_32x32x16_f16 per 32 k and 32x32 block            (2 x 32 cycles)
//         + a_hi * w_lo + a_lo * w_hi   ONE v_mfma_scale_f32_32x32x64_f8f6f4 on the fp8 parts         (64 cycles)
// instead of the six f16 MFMAs (192 cycles) of the split-f16 kernel (gemm256s.hip, GS).  Measured on the instruction mix alone
// (scripts/probes/mx32_probe.hip): 128 vs 192 matrix-pipe cycles per product and a clock the chip holds 6 % higher (1.77 vs 1.67 GHz);
// the round-3 stamps of the GS main loop showed its matrix pipe ~85 % busy, i.e. the pipe, not the loads, is what this removes.
// Operand error: the cross terms are ~2^-11 of a product and come out to ~4 bits, so a product is good to ~2^-15 relative
// (single f16: 2^-11; full split: 2^-21) — DESIGN.md has the measured per-label probability error of the whole forward.
//
// Structure = the full-line ring of gemm256s.hip (FL): ring stage 2s = A rows of 32-group s, stage 2s + 1 = W rows (one 128-byte GX
// group per row: 8 whole lines per LDS-DMA wave-instruction), slot = stage & 3, LDS image [256 rows][128 B] with the 16-byte chunk
// swizzle c ^ ((row >> 1) & 7); the same two-phase step and wave-group stagger, with EQUAL halves:
//   E: phase A = request group s + 1 (8 pieces per wave), read the f16 fragments (8 + 4); phase B = 16 x 32x32x16 f16      (512 cycles)
//   O: phase A = read the fp8 fragments (4 + 2 operands of 32 B), wait for my pieces;     phase B =  8 x 32x32x64 scaled   (512 cycles)
// Hazards: as argued in gemm256s.hip (FL).  Fragment maps: f16 32x32x16 lane (c = l & 31, h = l >> 5) holds row c, k = 16 ks + 8 h + j
// = chunk 2 ks + h of the group; fp8 32x32x64 lane (c, h) holds bytes [0,16) = slots 16 h .. 16 h + 15 of MX block 0 and [16,32) = the
// same slots of block 1 (probe: byte y <-> k-slot 16 h + (y & 15) + 32 (y >> 4)); the scale of block b of row c is taken from lane
// c + 32 b.  The lane's 32 bytes are chunks 4 + 2 h and 5 + 2 h of the group — the fp8 parts of elements 16 h .. 16 h + 15, A rows as
// [lo8 x 8 | hi8 x 8] per 8 elements, W rows as [hi8 x 8 | lo8 x 8] — so slot by slot a_lo8 meets w_hi8 and a_hi8 meets w_lo8 over
// the same element, and every slot's product carries 2^-(SHIFT + ws): one scale per operand for all blocks (glc_common.h).
// Accumulators are 32x32 blocks, acc[I][J]: non-transposed launches D[n][m] (lane = m, registers = n: 4 consecutive n per register
// quad), the V third D[m][n].  The epilogue is gemm_mx_epilogue.h, shared with the 128 x 128 tile (gemm128x.hip).
#include <stdlib.h>
#include <type_traits>
#include "gemm_mx_tile.h"

namespace {

constexpr int TM = 256, TN = 256;
constexpr int STAGE = TM * LINE;           // 32 KiB: one operand's rows of one group
extern __shared__ __attribute__((aligned(16))) unsigned char smem256x[];

#ifndef GLC_GX_A_AUX
#define GLC_GX_A_AUX 0
#endif
#ifndef GLC_GX_W_AUX
#define GLC_GX_W_AUX 0
#endif

// W128 (round 6; the launcher takes it for the large bias / GELU / SwiGLU / residual shapes): the same tile by FOUR waves, one per SIMD with 512 registers (the
// 256 accumulator registers in AGPRs — hipcc's default; -amdgpu-mfma-vgpr-form would fill the loop with accumulator copies), each a 128 x 128 sub-tile = 16 blocks.  One in-order wave overlaps its MFMAs with its own loads when they alternate in program
// order (profiles/r06/overlap_bisect.txt): per 32-group the wave issues F = 32 x 32x32x16 f16 with the group's fp8 fragment reads between them, then X = 16 scaled
// 32x32x64 with the NEXT group's f16 fragment reads and its 16 DMA pieces of the group after that between them — every fragment register is loaded one phase
// (1024 matrix-pipe cycles) before its use and dies with its phase, so no fragment is double-buffered (a16 / w16 / xa / xw: 128 registers), ONE barrier per group.
// LDS reads per group and CU 128 KiB instead of 192; requests enter the vector-memory path one per MFMA gap instead of in bursts.
// EPI_RESIDP = EPI_RESID with the residual rows as plain fp32 (RPLAIN; its own build, so that the GX-residual build keeps its registers)
template <int EPI_IN, bool VMODE, bool W128 = false>
__device__ __forceinline__ void gemm256x_tile(const GemmArgs& p, int n_tile0, int ntn) {
    constexpr bool RPLAIN = EPI_IN == EPI_RESIDP;
    constexpr int EPI = RPLAIN ? (int)EPI_RESID : EPI_IN;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm_outer = W128 ? (wave >> 1) : (wave >> 2), wn_outer = W128 ? (wave & 1) : (wave & 3);
    const int c32 = lane & 31, h = lane >> 5;
    const int K = p.K, N = p.N;

    int mt, nt;
    x_tile_of_block(p.n_group, ntn, mt, nt);
    const int m0 = mt * TM, n0 = (n_tile0 + nt) * TN;
    if constexpr (EPI == EPI_QKV && !VMODE) {
        if (p.q_tile_flag && n0 < p.H) {                // Q third, pruned last layer: nobody reads query tiles without selected rows
            const unsigned long long f8 = *reinterpret_cast<const unsigned long long*>(p.q_tile_flag + (m0 >> 5));
            if (f8 == 0ull) return;
        }
    }

    const unsigned char* __restrict__ A = reinterpret_cast<const unsigned char*>(p.A);
    const unsigned char* __restrict__ W = reinterpret_cast<const unsigned char*>(p.W);
    const size_t rsb = (size_t)4 * K;          // row stride in bytes (GX rows)
    const int ng = K / 32;
    // DMA map (FL): lane L lands at (row L >> 3, physical chunk L & 7) of an 8-row piece and fetches logical chunk (L & 7) ^ ((row >> 1) & 7)
    const int lrow8 = lane >> 3, pch = lane & 7;
    const unsigned char* fa[2];
    const unsigned char* fw[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = wave * (W128 ? 64 : 32) + i * 8 + lrow8;
        const int lc = pch ^ ((row >> 1) & 7);
        fa[i] = A + (size_t)(m0 + row) * rsb + lc * 16;
        fw[i] = W + (size_t)(n0 + row) * rsb + lc * 16;
    }
    auto stage_a = [&](int grp) {           // this wave's 32 A rows of group grp: 4 one-KiB pieces
        unsigned char* sa = smem256x + ((2 * grp) & (NSLOT - 1)) * STAGE + (wave * 32) * LINE;
        const size_t o = (size_t)grp * LINE;
#pragma unroll
        for (int i = 0; i < 4; ++i) glds16<GLC_GX_A_AUX>(fa[i & 1] + (size_t)(i >> 1) * 16 * rsb + o, sa + i * 8 * LINE);
    };
    auto stage_w = [&](int grp) {           // ... and its 32 W rows
        unsigned char* sw = smem256x + ((2 * grp + 1) & (NSLOT - 1)) * STAGE + (wave * 32) * LINE;
        const size_t o = (size_t)grp * LINE;
#pragma unroll
        for (int i = 0; i < 4; ++i) glds16<GLC_GX_W_AUX>(fw[i & 1] + (size_t)(i >> 1) * 16 * rsb + o, sw + i * 8 * LINE);
    };
    auto stage_fl = [&](int grp) { stage_a(grp); stage_w(grp); };

    f32x16 accs[W128 ? 2 : 1][4][2];          // W128: [column half ch][row block][column block of the half] — the epilogue below runs once per half
#pragma unroll
    for (int ch = 0; ch < (W128 ? 2 : 1); ++ch)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) accs[ch][i][j][r] = 0.f;

    // fragment read offsets inside a slot
    const int hsw = (c32 >> 1) & 7;
    const int arow = (wm_outer * 128 + c32) * LINE, wrow = (wn_outer * (W128 ? 128 : 64) + c32) * LINE;
    const int ck0 = ((0 + h) ^ hsw) * 16, ck1 = ((2 + h) ^ hsw) * 16;               // f16 k-steps 0 / 1: logical chunks h / 2 + h
    const int cx0 = ((4 + 2 * h) ^ hsw) * 16, cx1 = ((5 + 2 * h) ^ hsw) * 16;       // the fp8 parts of elements 16 h .. 16 h + 7 / + 8 .. + 15
    // e8m0 scales, one per operand for every block: A rows (activations) carry 2^-(SHIFT + act_sc), W rows their 2^-ws (glc_common.h)
    const int sc_a = 127 - GLC_GX_SHIFT - p.act_sc;
    const int sc_w = 127 - p.mx_ws;

    if constexpr (W128) {
        f16x8 a16[4][2], w16[4][2];
        i32x8 xa[4], xw[4];
        auto slot_a = [&](int grp) -> unsigned char* { return smem256x + ((2 * grp) & (NSLOT - 1)) * STAGE; };
        auto slot_w = [&](int grp) -> unsigned char* { return smem256x + ((2 * grp + 1) & (NSLOT - 1)) * STAGE; };
        // piece q = 0 .. 15 of this wave's 64 A rows (q < 8) and 64 W rows of group grp
        // (the request in its scalar-base form: wave-uniform base + a 32-bit lane offset that never changes — no 64-bit address arithmetic per lane and piece)
        const unsigned voffs[2] = {(unsigned)((size_t)lrow8 * rsb + (pch ^ (((wave * 64 + lrow8) >> 1) & 7)) * 16), (unsigned)((size_t)(8 + lrow8) * rsb + (pch ^ (((wave * 64 + 8 + lrow8) >> 1) & 7)) * 16)};
        const unsigned char* const ubA = A + (size_t)(m0 + wave * 64) * rsb;
        const unsigned char* const ubW = W + (size_t)(n0 + wave * 64) * rsb;
        auto dma_piece = [&](int grp, int q) __attribute__((always_inline)) {
            const int i = q & 7;
            const unsigned char* ub = (q < 8 ? ubA : ubW) + (size_t)grp * LINE + (size_t)(i >> 1) * 16 * rsb;
            unsigned char* l = (q < 8 ? slot_a(grp) : slot_w(grp)) + (wave * 64 + i * 8) * LINE;
            const unsigned la = (unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)l;
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" :: "s"(la), "v"(voffs[i & 1]), "s"(ub) : "memory");
        };
        // fragment read r = 0 .. 15 of a group: the f16 k-steps (r < 8: W blocks, r >= 8: A blocks; two reads per block) ...
        auto rd_f16 = [&](int grp, int r) __attribute__((always_inline)) {
            const int b = (r & 7) >> 1, ks = r & 1;
            if (r < 8) w16[b][ks] = *reinterpret_cast<const f16x8*>(slot_w(grp) + wrow + b * 32 * LINE + (ks ? ck1 : ck0));
            else a16[b][ks] = *reinterpret_cast<const f16x8*>(slot_a(grp) + arow + b * 32 * LINE + (ks ? ck1 : ck0));
        };
        // ... and the fp8 operands (two 16-byte chunks each)
        auto rd_x = [&](int grp, int r) __attribute__((always_inline)) {
            const int b = (r & 7) >> 1, half = r & 1;
            const unsigned char* q0 = (r < 8 ? slot_w(grp) + wrow : slot_a(grp) + arow) + b * 32 * LINE + (half ? cx1 : cx0);
            const i32x4 t = *reinterpret_cast<const i32x4*>(q0);
            i32x8& d = r < 8 ? xw[b] : xa[b];
            d[4 * half] = t[0]; d[4 * half + 1] = t[1]; d[4 * half + 2] = t[2]; d[4 * half + 3] = t[3];
        };
#pragma unroll
        for (int q = 0; q < 16; ++q) dma_piece(0, q);
        if (ng > 1) {
#pragma unroll
            for (int q = 0; q < 16; ++q) dma_piece(1, q);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int r = 0; r < 16; ++r) rd_f16(0, r);
        // one group; M1 / M2 (compile time: the tail is peeled, a branch inside a phase would let hipcc sink the MFMAs behind the loads): groups s + 1 / s + 2 exist
        auto step = [&](const int s, auto m1, auto m2) __attribute__((always_inline)) {
            constexpr bool M1 = decltype(m1)::value, M2 = decltype(m2)::value;
            // ---- F(s): a_hi w_hi of group s; its fp8 fragments are read underneath ----
#pragma unroll
            for (int k = 0; k < 32; ++k) {
                const int ks = k >> 4, i = (k >> 2) & 3, j = k & 3;
                f32x16& a = accs[j >> 1][i][j & 1];
                if (!VMODE) a = __builtin_amdgcn_mfma_f32_32x32x16_f16(w16[j][ks], a16[i][ks], a, 0, 0, 0);      // D[n][m]
                else a = __builtin_amdgcn_mfma_f32_32x32x16_f16(a16[i][ks], w16[j][ks], a, 0, 0, 0);            // D[m][n]
                if ((k & 1) == 0) rd_x(s, k >> 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            // group s + 1 (requested during X(s - 1)) has landed; every wave has read the last of group s: its slots are free
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            // ---- X(s): both cross terms of group s; the f16 fragments of group s + 1 are read and group s + 2 is requested underneath ----
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int i = k >> 2, j = k & 3;
                f32x16& a = accs[j >> 1][i][j & 1];
                if (!VMODE) a = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(xw[j], xa[i], a, 0, 0, 0, sc_w, 0, sc_a);
                else a = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(xa[i], xw[j], a, 0, 0, 0, sc_a, 0, sc_w);
                if constexpr (M1) rd_f16(s + 1, k);
                if constexpr (M2) dma_piece(s + 2, k);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        for (int s = 0; s + 2 < ng; ++s) step(s, std::true_type{}, std::true_type{});
        if (ng > 1) step(ng - 2, std::true_type{}, std::false_type{});
        step(ng - 1, std::false_type{}, std::false_type{});
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();              // every wave is through its last fragment read: the ring becomes the epilogue's staging space
    } else {
        const int wm = wm_outer;
        f32x16 (&acc)[4][2] = accs[0];
        f16x8 a16[4][2], w16[2][2];
        i32x8 xa[4], xw[2];
        const int pm = p.prio_mode;     // 0: no priorities; 1: MFMA phase at priority 1; 2: load phase at priority 2; 3: the late wave group at priority 1 throughout
        if (pm == 3 && wm == 1) __builtin_amdgcn_s_setprio(1);
        stage_fl(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();              // group 0 is in LDS for everyone
        if (wm == 1) __builtin_amdgcn_s_barrier(); // the stagger
        auto ld32 = [&](const unsigned char* q0, int o0, int o1) __attribute__((always_inline)) {      // two 16-byte chunks -> one 32-byte MX operand
            const i32x4 t0 = *reinterpret_cast<const i32x4*>(q0 + o0);
            const i32x4 t1 = *reinterpret_cast<const i32x4*>(q0 + o1);
            i32x8 r;
            r[0] = t0[0]; r[1] = t0[1]; r[2] = t0[2]; r[3] = t0[3]; r[4] = t1[0]; r[5] = t1[1]; r[6] = t1[2]; r[7] = t1[3];
            return r;
        };
        auto sub = [&](const int s, const int odd) __attribute__((always_inline)) {
            // ---- phase A ----
            if (pm == 2) __builtin_amdgcn_s_setprio(2);
            if (!odd && s + 1 < ng) stage_fl(s + 1);
            {
                const unsigned char* sa = smem256x + ((2 * s) & (NSLOT - 1)) * STAGE + arow;
                const unsigned char* sw = smem256x + ((2 * s + 1) & (NSLOT - 1)) * STAGE + wrow;
                if (!odd) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        w16[j][0] = *reinterpret_cast<const f16x8*>(sw + j * 32 * LINE + ck0);
                        w16[j][1] = *reinterpret_cast<const f16x8*>(sw + j * 32 * LINE + ck1);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        a16[i][0] = *reinterpret_cast<const f16x8*>(sa + i * 32 * LINE + ck0);
                        a16[i][1] = *reinterpret_cast<const f16x8*>(sa + i * 32 * LINE + ck1);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 2; ++j) xw[j] = ld32(sw + j * 32 * LINE, cx0, cx1);      // [w_hi8 w_lo8 | w_hi8 w_lo8] of 2 x 8 elements
#pragma unroll
                    for (int i = 0; i < 4; ++i) xa[i] = ld32(sa + i * 32 * LINE, cx0, cx1);      // [a_lo8 a_hi8 | a_lo8 a_hi8]
                }
            }
            if (odd) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            if (pm == 2) __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_s_barrier();
            // ---- phase B ----
            if (pm == 1) __builtin_amdgcn_s_setprio(1);
            if (!odd) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            if (!VMODE) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w16[j][ks], a16[i][ks], acc[i][j], 0, 0, 0);      // D[n][m]
                            else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a16[i][ks], w16[j][ks], acc[i][j], 0, 0, 0);            // D[m][n]
                        }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        if (!VMODE) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(xw[j], xa[i], acc[i][j], 0, 0, 0, sc_w, 0, sc_a);
                        else acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(xa[i], xw[j], acc[i][j], 0, 0, 0, sc_a, 0, sc_w);
                    }
            }
            if (pm == 1) __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
        };
        for (int s = 0; s < ng; ++s) { sub(s, 0); sub(s, 1); }
        if (wm == 0) __builtin_amdgcn_s_barrier();   // pairs with the late group's last barrier
    }

    // ---------------- epilogue ----------------
    // (W128: the wave's 128 x 128 as two 128 x 64 halves through the code of the 8-wave tiles — wave (wm, wn) there = (wave >> 1, 2 (wave & 1) + ch) here)
#pragma unroll
    for (int ch = 0; ch < (W128 ? 2 : 1); ++ch) {
        const int wm = wm_outer, wn = W128 ? 2 * wn_outer + ch : wn_outer;
        f32x16 (&acc)[4][2] = accs[ch];
        constexpr int NCHUNK = 4, WROWS = 128;
        constexpr bool PERM = true;
        unsigned char* const smem = smem256x;
#include "gemm_mx_epilogue.h"
    }
}

template <int EPI, bool VMODE>
__global__ __launch_bounds__(512, 2) void gemm256x_kernel(GemmArgs p, int n_tile0, int ntn) { gemm256x_tile<EPI, VMODE>(p, n_tile0, ntn); }
// four waves, one per SIMD, 128 x 128 per wave (W128 above)
template <int EPI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gemm256w_kernel(GemmArgs p, int n_tile0, int ntn) { gemm256x_tile<EPI, false, true>(p, n_tile0, ntn); }
// Decoder QKV with the RoPE / MX-tile epilogue in ONE launch: the N-tiles of the V heads (nt >= nqk) run the transposed tile (c5: 7 + 1 N-tiles x
// 128 M-tiles = 4 full rounds of the chip; as two launches the V heads' 128 workgroups would be a fifth, half-empty round)
__global__ __launch_bounds__(512, 2) void gemm256x_qkvr_kernel(GemmArgs p, int nqk, int ntn) {
    int mt, nt;
    x_tile_of_block(p.n_group, ntn, mt, nt);
    if (nt < nqk) gemm256x_tile<EPI_QKVR, false>(p, 0, ntn);
    else gemm256x_tile<EPI_QKVR, true>(p, 0, ntn);
}

template <int EPI, bool VMODE> const char* launch_x(hipStream_t st, const GemmArgs& a, int n_tile0, int ntn) {
    static std::atomic<unsigned> lds_ok{0};
    constexpr int lds_bytes = NSLOT * STAGE;
    if (!glc_raise_lds_limit(gemm256x_kernel<EPI, VMODE>, lds_bytes, lds_ok)) return "gemm256x: cannot raise the dynamic LDS limit";
    const int grid = (a.Mpad / TM) * ntn;
    GemmArgs b = a;
    b.n_group = 0;
    static const int prio_env = glc_dev_env("GLC_GEMM_PRIO") ? atoi(glc_dev_env("GLC_GEMM_PRIO")) : 1;      // developer A/B switch
    b.prio_mode = a.prio_mode >= 0 ? a.prio_mode : prio_env;
    if (ntn >= 8 && (a.Mpad / TM) % 8 == 0) b.n_group = ntn % 4 == 0 ? 4 : (ntn % 3 == 0 ? 3 : 0);      // wide N: as gemm256s.hip
#ifdef GLC_GX_NB
    { constexpr int nbv = (GLC_GX_NB) > 0 ? (GLC_GX_NB) : 1;          // build-time A/B of the tile order (scripts/gemm_cache_policy_ab.sh; profiles/r05/gemm_cache_policy.txt)
      if ((a.Mpad / TM) % 8 == 0) b.n_group = (GLC_GX_NB) > 0 && ntn % nbv == 0 ? nbv : 0; }
#endif
    // Wave-tile choice (round 6, measured in the forwards of c3 / c4 / c5: profiles/r06/gemm_w128.txt): the one-wave-per-SIMD 128 x 128 tile reads a third less
    // LDS per MAC and pays its own request issue; it wins where the K loop and the tile count amortise its double epilogue — N K >= 768 x 3072 (FFN1 / FFN2
    // of every encoder shape: -2...-4 %; the decoder's gate|up, down and o_proj: -4...-12 %) — and loses below (attn-out of base / large: +1...+3 %) and on the
    // QKV epilogues (more registers than it has left: spills).  GLC_GEMM_W128 = 0 / 1 (developer builds) forces the 8-wave / the one-wave tile.
    if constexpr (!VMODE && (EPI == EPI_BIAS || EPI == EPI_GELU || EPI == EPI_RESID || EPI == EPI_SWIGLU)) {
        static const int w128_env = glc_dev_env("GLC_GEMM_W128") ? atoi(glc_dev_env("GLC_GEMM_W128")) : -1;
        const bool big = (long long)a.N * a.K >= 768LL * 3072LL;
        if (w128_env == 1 || (w128_env < 0 && big)) {
            static std::atomic<unsigned> lds_okw{0};
            if (!glc_raise_lds_limit(gemm256w_kernel<EPI>, lds_bytes, lds_okw)) return "gemm256x: cannot raise the dynamic LDS limit";
            hipLaunchKernelGGL((gemm256w_kernel<EPI>), dim3(grid), dim3(256), lds_bytes, st, b, n_tile0, ntn);
            return nullptr;
        }
    }
    hipLaunchKernelGGL((gemm256x_kernel<EPI, VMODE>), dim3(grid), dim3(512), lds_bytes, st, b, n_tile0, ntn);
    return nullptr;
}

// fp32 values -> GX rows in place (weights at load): exponent sc on the fp8 parts
__global__ __launch_bounds__(256) void to_gx_kernel(float* __restrict__ w, size_t ngroups, float k_hi, float k_lo, int worder) {
    const size_t gi = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= ngroups) return;
    float* base = w + gi * 32;
    f32x4 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const f32x4*>(base + 4 * i);      // the whole group is read before it is overwritten
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float x[8] = {v[2 * i][0], v[2 * i][1], v[2 * i][2], v[2 * i][3], v[2 * i + 1][0], v[2 * i + 1][1], v[2 * i + 1][2], v[2 * i + 1][3]};
        if (worder) gx_store8<true>(reinterpret_cast<unsigned char*>(base), 8 * i, x, k_hi, k_lo);
        else gx_store8<false>(reinterpret_cast<unsigned char*>(base), 8 * i, x, k_hi, k_lo);
    }
}

// group-split rows ([32 hi | 32 lo] f16 halves per 32 values) -> the largest |hi + lo| (as float bits: non-negative floats order like integers)
__global__ __launch_bounds__(256) void gs_absmax_kernel(const f16_t* __restrict__ gs, size_t ngroups, unsigned* __restrict__ out) {
    const size_t gi = (size_t)blockIdx.x * 256 + threadIdx.x;
    float m = 0.f;
    if (gi < ngroups) {
        const gs_h8* p = reinterpret_cast<const gs_h8*>(gs + gi * 64);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const gs_h8 hi = p[i], lo = p[4 + i];
#pragma unroll
            for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf((float)hi[e] + (float)lo[e]));
        }
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));
}
// group-split rows -> GX rows (weight order, fp8 exponent sc): the MX copies of the projection weights from their split-f16 copies on the device
__global__ __launch_bounds__(256) void gs_to_gx_kernel(const f16_t* __restrict__ gs, unsigned char* __restrict__ gx, size_t ngroups, float k_hi, float k_lo) {
    const size_t gi = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= ngroups) return;
    const gs_h8* p = reinterpret_cast<const gs_h8*>(gs + gi * 64);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const gs_h8 hi = p[i], lo = p[4 + i];
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = (float)hi[e] + (float)lo[e];
        gx_store8<true>(gx + gi * 128, 8 * i, x, k_hi, k_lo);
    }
}

}  // namespace

// n values (n % 32 == 0) as group-split rows: *d_bits (zeroed by the caller) = float bits of the largest magnitude
const char* glc_launch_gs_absmax(hipStream_t st, const void* gs, size_t n, unsigned* d_bits) {
    if (!gs || !d_bits || n % 32) return "gs_absmax: bad args";
    const size_t groups = n / 32;
    if (groups) hipLaunchKernelGGL(gs_absmax_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, (const f16_t*)gs, groups, d_bits);
    return nullptr;
}
// ... -> GX rows in weight order with fp8 exponent sc (what glc_launch_to_gx(.., sc, 1) makes of the fp32 values)
const char* glc_launch_gs_to_gx(hipStream_t st, const void* gs, void* gx, size_t n, int sc) {
    if (!gs || !gx || n % 32) return "gs_to_gx: bad args";
    if (sc < -40 || sc > 60) return "gs_to_gx: exponent out of range";
    const size_t groups = n / 32;
    if (groups) hipLaunchKernelGGL(gs_to_gx_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, (const f16_t*)gs, (unsigned char*)gx, groups, ldexpf(1.0f, sc), ldexpf(1.0f, sc + GLC_GX_SHIFT));
    return nullptr;
}

bool glc_gemm256x_supported(const GemmArgs& a, int epi) {
    if (!(a.Mpad > 0 && a.Mpad % TM == 0 && a.N > 0 && a.N % TN == 0 && a.K > 0 && a.K % 32 == 0)) return false;
    if (a.mx_ws < -40 || a.mx_ws > 60) return false;
    if (epi == EPI_QKV) return a.H % 256 == 0 && a.N == 3 * a.H && a.Sp % 64 == 0 && a.Sp >= 64 && a.nh * 64 == a.H;
    if (epi == EPI_QKVR) return a.nq > 0 && a.nkv > 0 && a.nq % 2 == 0 && a.nkv % 2 == 0 && a.N == (a.nq + 2 * a.nkv) * 128 && a.Sp % 32 == 0 && a.Sp >= 32 &&
                                a.Mvalid > 0 && a.Mvalid % a.Sp == 0 && a.Mvalid <= a.Mpad;
    if (epi == EPI_GEGLU) return a.glu_interleaved != 0;          // (the caller vouches for the row order of W: glc_kernels.h)
    return epi == EPI_BIAS || epi == EPI_GELU || epi == EPI_RESID || epi == EPI_SWIGLU;
}

const char* glc_launch_gemm256x(hipStream_t st, int epi, const GemmArgs& a_in) {
    GemmArgs a = a_in;
    if (const char* m = glc_mx_gemm_prepare(a, epi, false)) return m;
    const int ntn = a.N / TN;
    switch (epi) {
        case EPI_BIAS: return launch_x<EPI_BIAS, false>(st, a, 0, ntn);
        case EPI_GELU: return launch_x<EPI_GELU, false>(st, a, 0, ntn);
        case EPI_RESID:
            if (!a.gs_resid_plain) return launch_x<EPI_RESID, false>(st, a, 0, ntn);
            // plain fp32 residual rows (ModernBERT's MX pipeline: the residual stream itself): the 8-wave tile's own build, plain fp32 out
            return a.ln_part || a.r_stats ? "gemm256x: a plain fp32 residual takes no statistics and writes plain fp32 rows" : launch_x<EPI_RESIDP, false>(st, a, 0, ntn);
        case EPI_SWIGLU: return a.bias ? "gemm256x: the SwiGLU epilogue takes no bias" : launch_x<EPI_SWIGLU, false>(st, a, 0, ntn);
        // (the 8-wave tile only: the one-wave tile has no GeGLU build)
        case EPI_GEGLU: return a.bias || a.a_stats ? "gemm256x: the GeGLU epilogue takes no bias and no folded norm" : launch_x<EPI_GEGLU, false>(st, a, 0, ntn);
        case EPI_QKV: {
            const int nqk = 2 * a.H / TN, nq = a.qkv_skip_q ? a.H / TN : 0;
            const char* m = launch_x<EPI_QKV, false>(st, a, nq, nqk - nq);      // (one launch for both, as EPI_QKVR below: measured +-0 at c3 — 6 + 3 full rounds either way)
            return m ? m : launch_x<EPI_QKV, true>(st, a, nqk, ntn - nqk);
        }
        case EPI_QKVR: {
            const int nqk = (a.nq + a.nkv) / 2;              // 256-column tiles of the Q and K heads; the V heads run transposed
            static std::atomic<unsigned> lds_ok{0};
            if (!glc_raise_lds_limit(gemm256x_qkvr_kernel, NSLOT * STAGE, lds_ok)) return "gemm256x: cannot raise the dynamic LDS limit";
            GemmArgs b = a;
            b.n_group = 0;
            b.prio_mode = a.prio_mode >= 0 ? a.prio_mode : 1;
            if (ntn >= 8 && (a.Mpad / TM) % 8 == 0) b.n_group = ntn % 4 == 0 ? 4 : (ntn % 3 == 0 ? 3 : 0);
            hipLaunchKernelGGL(gemm256x_qkvr_kernel, dim3((a.Mpad / TM) * ntn), dim3(512), NSLOT * STAGE, st, b, nqk, ntn);
            return nullptr;
        }
    }
    return "gemm256x: bad epilogue";
}

// In place: n fp32 values (n % 32 == 0) -> GX rows with fp8 exponent sc (glc_common.h): weights at load (sc = glc_gx_weight_exponent,
// worder = 1: [hi8 | lo8] per 8 elements), activations in tests (sc = 0, worder = 0: [lo8 | hi8]).
const char* glc_launch_to_gx(hipStream_t st, void* w, size_t n, int sc, int worder) {
    if (!w || n % 32) return "to_gx: element count must be a multiple of 32";
    if (sc < -40 || sc > 60) return "to_gx: exponent out of range";
    const size_t groups = n / 32;
    if (groups) hipLaunchKernelGGL(to_gx_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, (float*)w, groups, ldexpf(1.0f, sc), ldexpf(1.0f, sc + GLC_GX_SHIFT), worder);
    return nullptr;
}


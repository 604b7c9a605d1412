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
// is that of both wave tiles of gemm256x.hip, and the epilogue is the one all three tiles share (gemm_mx_epilogue.h; a wave's sub-tile is 64 x 64 here,
// i.e. two 32-row chunks where the 8-wave tile has four): on the same operand images the outputs, the ln_part partials and the range
// counter must be bit-identical to the 256 tile's (tests/test_gpu_gemm128x.py asserts it).  Fragment maps and row formats: gemm256x.hip.
// Epilogues: EPI_BIAS, EPI_GELU, EPI_RESID (GX residual), EPI_QKV; the decoder / ModernBERT ones are not built here.
#include <stdlib.h>
#include "gemm_mx_tile.h"

namespace {

constexpr int TM = 128, TN = 128;
constexpr int STAGE = TM * LINE;           // 16 KiB: one operand's rows of one group
static_assert(NSLOT * STAGE <= 80 * 1024 && 4 * EPI_PATCH <= NSLOT * STAGE, "two workgroups per CU; the epilogue stages inside the ring");      // (4 waves: 36 KiB of it)
extern __shared__ __attribute__((aligned(16))) unsigned char smem128x[];

template <int EPI, bool VMODE>
__device__ __forceinline__ void gemm128x_tile(const GemmArgs& p, int n_tile0, int ntn) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int c32 = lane & 31, h = lane >> 5;
    const int K = p.K, N = p.N;

    int mt, nt;
    x_tile_of_block(0, ntn, mt, nt);
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
    // e8m0 scales, one per operand for every block: A rows (activations) carry 2^-(SHIFT + act_sc), W rows their 2^-ws (glc_common.h)
    const int sc_a = 127 - GLC_GX_SHIFT - p.act_sc;
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
    constexpr int NCHUNK = 2, WROWS = 64;
    constexpr bool RPLAIN = false, PERM = false;
    unsigned char* const smem = smem128x;
#include "gemm_mx_epilogue.h"
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

// Shapes and arguments the 128 tile takes.  EPI_QKV: the conditions of glc_gemm256x_supported with H % 128 (a tile must not straddle the Q / K / V
// thirds; the tile writers need no more: a wave's 64 columns are one head).  A plain fp32 residual and permuted columns are built for the 256 tile only.
bool glc_gemm128x_supported(const GemmArgs& a, int epi) {
    if (!(a.Mpad > 0 && a.Mpad % TM == 0 && a.N > 0 && a.N % TN == 0 && a.K > 0 && a.K % 32 == 0)) return false;
    if (a.mx_ws < -40 || a.mx_ws > 60) return false;
    if (epi == EPI_QKV) return a.H > 0 && a.H % 128 == 0 && a.N == 3 * a.H && a.Sp % 64 == 0 && a.Sp >= 64 && a.nh * 64 == a.H;
    if (epi == EPI_RESID) return !a.gs_resid_plain;
    if (epi == EPI_BIAS) return !a.perm_cols;
    return epi == EPI_GELU;
}

const char* glc_launch_gemm128x(hipStream_t st, int epi, const GemmArgs& a_in) {
    GemmArgs a = a_in;
    if (epi != EPI_BIAS && epi != EPI_GELU && epi != EPI_RESID && epi != EPI_QKV) return "gemm128x: this epilogue is built for the 256 tile only";
    if (epi == EPI_RESID && a.gs_resid_plain) return "gemm128x: a plain fp32 residual is built for the 256 tile only";
    if (epi == EPI_BIAS && a.perm_cols) return "gemm128x: permuted columns are built for the 256 tile only";
    if (const char* m = glc_mx_gemm_prepare(a, epi, true)) return m;
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

// The epilogue of the MX cross-term GEMM's wave tiles, as program text: gemm256x.hip (8-wave tile: once; one-wave-per-SIMD tile: once per
// column half) and gemm128x.hip include this file INSIDE their tile function, behind the main loop — one definition, compiled in place.
// (Not a function: hipcc simplifies a force-inlined function on its own before it inlines it, and the epilogue then comes out in another
//  instruction order with other register counts — as a function it cost gemm256x_kernel<EPI_RESID> 14 spilled registers (60 bytes of scratch)
//  at its limit of 256 and moved gemm256w_kernel<EPI_BIAS / EPI_GELU> from 452 / 456 to 464 / 468; profiles/mx_epilogue/kernel_resources.txt.
//  Included as text the kernels are instruction for instruction those of the two copies this file replaces.)
//
// In scope at the place of inclusion:
//   p (GemmArgs), N = p.N, lane, c32 = lane & 31, h = lane >> 5, wave; m0, n0: first row / column of the workgroup's tile;
//   wm, wn: the wave's sub-tile is NCHUNK x 32 = WROWS rows from m0 + wm * WROWS by 64 columns from n0 + wn * 64;
//   acc[NCHUNK][2] (f32x16): acc[c][J] = the 32 x 32 block of row chunk c and column block J (non-transposed launches D[n][m]: lane = m,
//   registers = n, 4 consecutive n per register quad; VMODE, the V third: D[m][n]);
//   smem: the ring, free once every wave is through its last fragment read — wave `wave` stages in its own EPI_PATCH bytes;
//   constants EPI, VMODE, RPLAIN (EPI_RESID with the residual rows as plain fp32: its own build, EPI_RESIDP, so that the GX-residual build
//   keeps its registers), NCHUNK, WROWS, PERM (built with the perm_cols remap of the plain fp32 store: the 256 tiles).
// As gemm256s.hip's epilogue (LDS-staged 16-byte stores, LayerNorm fold, residual prefetch), reading and writing GX rows where that kernel has GS rows.
{
    typedef f16_t T;
    typedef __attribute__((ext_vector_type(8))) T vec8T;
    const float* __restrict__ bias = p.bias;
    float* stg = reinterpret_cast<float*>(smem + wave * EPI_PATCH);
    const int qkv_b0 = (EPI == EPI_QKV || EPI == EPI_QKVR) ? m0 / p.Sp : 0;
    const float kHi = gx_act_khi(p.act_sc), kLo = gx_act_klo(p.act_sc), kInvLo = gx_pow2_inv(kLo);       // activation rows in and out: exponent act_sc
    constexpr float kInvLo0 = 1.0f / (float)(1 << GLC_GX_SHIFT);                                          // MX tiles (attention operands): exponent 0
    if constexpr (EPI == EPI_SWIGLU || EPI == EPI_GEGLU) {
        // W rows alternate 16 gate / 16 up features (engine.hip interleaves them at load): in D[n = 32 J + 8 q + 4 h + e][m] the register quads
        // q = 0, 1 hold gate features 8 q + 4 h + e of block J and q + 2 the matching up features — same lane, no exchange.  The wave's
        // 64 columns become 32 outputs silu(gate) * up (Q2:47); patch [32 rows][32 features], row stride 36 floats.
        // RMSNorm folded into this GEMM (a_stats: W holds W diag(gain), the rows are raw): gate and up scale by the row's rstd first.
        // EPI_GEGLU (ModernBERT, MB:89-91): the same quads hold [input | gate], the output is gelu(input) * gate with the erf GELU of EPI_GELU; no folded norm.
        const int Iw = N >> 1;
        const bool lnf = EPI == EPI_SWIGLU && p.a_stats != nullptr;
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            const float rs = lnf ? p.a_stats[m0 + wm * WROWS + c * 32 + c32].y : 1.0f;
#pragma unroll
            for (int J = 0; J < 2; ++J)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    f32x4 v;
                    if constexpr (EPI == EPI_GEGLU) {
                        const f32x2 g0 = glc_gelu2_f32((f32x2){acc[c][J][4 * q], acc[c][J][4 * q + 1]}), g1 = glc_gelu2_f32((f32x2){acc[c][J][4 * q + 2], acc[c][J][4 * q + 3]});
                        v = (f32x4){g0[0] * acc[c][J][4 * (q + 2)], g0[1] * acc[c][J][4 * (q + 2) + 1], g1[0] * acc[c][J][4 * (q + 2) + 2], g1[1] * acc[c][J][4 * (q + 2) + 3]};
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float gt = acc[c][J][4 * q + e] * rs, up = acc[c][J][4 * (q + 2) + e] * rs;
                            v[e] = gt * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * gt)) * up;
                        }
                    }
                    *reinterpret_cast<f32x4*>(stg + c32 * 36 + 16 * J + 8 * q + 4 * h) = v;
                }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int idx = lane + 64 * k, row = idx >> 2, g4 = idx & 3;
                const f32x4 lo = *reinterpret_cast<const f32x4*>(stg + row * 36 + g4 * 8);
                const f32x4 hi = *reinterpret_cast<const f32x4*>(stg + row * 36 + g4 * 8 + 4);
                const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                const int m = m0 + wm * WROWS + c * 32 + row;
                gx_store8(reinterpret_cast<unsigned char*>(p.C) + (size_t)m * 4 * Iw, (n0 >> 1) + wn * 32 + g4 * 8, v, kHi, kLo, m < p.gx_rows ? p.gx_sat : nullptr);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
        }
    } else if constexpr (!VMODE) {
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
        // (RPLAIN: the 8 fp32 values of a plain residual row instead, ONE buffer loaded at the top of its chunk — behind the patch writes —
        //  since a second one does not fit the registers)
        f32x4 pnone[RPLAIN ? 4 : 1][2];
        auto load_resid = [&](int c, gs_h8 (&r)[4], u32x2 (&rl)[4], float2 (&rst)[4], f32x4 (&pp)[RPLAIN ? 4 : 1][2]) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int idx = lane + 64 * k, row = idx >> 3, g8 = idx & 7;
                if (rln) rst[k] = p.r_stats[m0 + wm * WROWS + c * 32 + row];
                const int n = n0 + wn * 64 + g8 * 8;
                if constexpr (RPLAIN) {
                    const float* fp = reinterpret_cast<const float*>(p.resid) + (size_t)(m0 + wm * WROWS + c * 32 + row) * N + n;
                    pp[k][0] = *reinterpret_cast<const f32x4*>(fp);
                    pp[k][1] = *reinterpret_cast<const f32x4*>(fp + 4);
                    continue;
                }
                const unsigned char* rp = reinterpret_cast<const unsigned char*>(p.resid) + (size_t)(m0 + wm * WROWS + c * 32 + row) * 4 * N + (n >> 5) * 128;
                r[k] = *reinterpret_cast<const gs_h8*>(rp + (n & 31) * 2);
                rl[k] = *reinterpret_cast<const u32x2*>(rp + 64 + (n & 31) * 2);
            }
        };
        if constexpr (EPI == EPI_RESID && !RPLAIN) { load_resid(0, rpre, rpre_lo, rst_pre, pnone); }
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            gs_h8 rcur[4]; u32x2 rcur_lo[4]; float2 rst_cur[4];
            f32x4 pcur[RPLAIN ? 4 : 1][2];
            if (EPI == EPI_RESID) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { rcur[k] = rpre[k]; rcur_lo[k] = rpre_lo[k]; rst_cur[k] = rst_pre[k]; }
                if constexpr (RPLAIN) load_resid(c, rcur, rcur_lo, rst_cur, pcur);
                else if (c + 1 < NCHUNK) load_resid(c + 1, rpre, rpre_lo, rst_pre, pnone);
            }
            const float2 sm = lnf ? p.a_stats[m0 + wm * WROWS + c * 32 + c32] : make_float2(0.f, 1.f);
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
            if constexpr (EPI == EPI_QKVR) {
                // Decoder Q / K heads (head_dim 128): this wave's 64 columns are features [32 hf, 32 hf + 32) (patch columns 0 .. 31) and their
                // rotate-half partners 64 + the same (columns 32 .. 63) of one head (W rows in glc_rope_perm128 order).  A lane takes 8
                // consecutive pairs of one row: RoPE (Q2:211) and, on Q, the softmax scale in fp32, then the two 8-value pieces of the MX
                // tile (decoder_mx.hip layout; Q as (hi8 | lo8) at slot r, K as (lo8 | hi8) at slot pi(r)).
                const int col0 = n0 + wn * 64, head = col0 >> 7, hf = (col0 >> 6) & 1;
                const bool isq = head < p.nq;
                const int ntl = p.Sp >> 5;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int idx = lane + 64 * k, row = idx >> 2, g4 = idx & 3;
                    const f32x4 a0 = *reinterpret_cast<const f32x4*>(stg + row * 68 + g4 * 8), a1 = *reinterpret_cast<const f32x4*>(stg + row * 68 + g4 * 8 + 4);
                    const f32x4 b0 = *reinterpret_cast<const f32x4*>(stg + row * 68 + 32 + g4 * 8), b1 = *reinterpret_cast<const f32x4*>(stg + row * 68 + 32 + g4 * 8 + 4);
                    const int m = m0 + wm * WROWS + c * 32 + row;
                    if (m >= p.Mvalid) continue;
                    int b = qkv_b0, sq = m - qkv_b0 * p.Sp;
                    while (sq >= p.Sp) { sq -= p.Sp; ++b; }
                    const float x1[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]}, x2[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
                    const int d1 = 32 * hf + g4 * 8, d2 = d1 + 64;
                    const f32x4* cp = reinterpret_cast<const f32x4*>(p.rope_cs + ((size_t)sq * 64 + d1) * 2);
                    const f32x4 c0 = cp[0], c1 = cp[1], c2 = cp[2], c3 = cp[3];
                    const float cs[16] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3], c2[0], c2[1], c2[2], c2[3], c3[0], c3[1], c3[2], c3[3]};
                    const float sc = isq ? p.qscale : 1.f;
                    float o1[8], o2[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float co = cs[2 * j], sn = cs[2 * j + 1];
                        o1[j] = (x1[j] * co - x2[j] * sn) * sc;
                        o2[j] = (x2[j] * co + x1[j] * sn) * sc;
                    }
                    const int r = sq & 31, slot = isq ? r : glc_pi32(r);
                    unsigned char* base = isq ? reinterpret_cast<unsigned char*>(p.Qh) + ((size_t)(b * p.nq + head) * ntl + (sq >> 5)) * 16384
                                              : reinterpret_cast<unsigned char*>(p.Kh) + ((size_t)(b * p.nkv + (head - p.nq)) * ntl + (sq >> 5)) * 16384;
                    unsigned* sat = m < p.gx_rows ? p.gx_sat : nullptr;
                    store_mx8(base + (d1 >> 4) * 1024 + (32 * ((d1 >> 3) & 1) + slot) * 16, base + 8192 + (d1 >> 5) * 2048 + (32 * ((d1 >> 4) & 1) + slot) * 32 + 8 * ((d1 >> 3) & 1), o1, isq, sat);
                    store_mx8(base + (d2 >> 4) * 1024 + (32 * ((d2 >> 3) & 1) + slot) * 16, base + 8192 + (d2 >> 5) * 2048 + (32 * ((d2 >> 4) & 1) + slot) * 32 + 8 * ((d2 >> 3) & 1), o2, isq, sat);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int idx = lane + 64 * k, row = idx >> 3, g8 = idx & 7;
                    const f32x4 lo = *reinterpret_cast<const f32x4*>(stg + row * 68 + g8 * 8);
                    const f32x4 hi = *reinterpret_cast<const f32x4*>(stg + row * 68 + g8 * 8 + 4);
                    float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    const int m = m0 + wm * WROWS + c * 32 + row;
                    const int n = n0 + wn * 64 + g8 * 8;
                    if constexpr (EPI == EPI_RESID) {
                        float r[8];
                        if constexpr (RPLAIN) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) { r[e] = pcur[k][0][e]; r[4 + e] = pcur[k][1][e]; }
                        } else
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
                            // raw GX row out + this 64-column block's (sum, squared deviations from the block mean) of the row (gemm256s.hip)
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
                                gx_range_note(v, 1.0f, p.gx_sat && m < p.gx_rows ? p.gx_sat + 1 : nullptr);      // (tiles: the guard's second word; no counter outside a GxScope, padding rows not counted)
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
                            int nl = n;
                            if constexpr (PERM) nl = n < p.perm_cols ? (n & ~127) | glc_rope_perm128(n & 127) : n;      // (W rows in the EPI_QKVR order: back to the logical column)
                            float* cp = reinterpret_cast<float*>(p.C) + (size_t)m * N + nl;
                            *reinterpret_cast<f32x4*>(cp) = (f32x4){v[0], v[1], v[2], v[3]};
                            *reinterpret_cast<f32x4*>(cp + 4) = (f32x4){v[4], v[5], v[6], v[7]};
                        } else
                            gx_store8<false, true>(reinterpret_cast<unsigned char*>(p.C) + (size_t)m * 4 * N, n, v, kHi, kLo, m < p.gx_rows ? p.gx_sat : nullptr);      // FFN1's intermediate: streams (non-temporal)
                    }
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
        for (int c = 0; c < NCHUNK; ++c) {
#pragma unroll
            for (int J = 0; J < 2; ++J)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f32x4 v = {acc[c][J][4 * q], acc[c][J][4 * q + 1], acc[c][J][4 * q + 2], acc[c][J][4 * q + 3]};
                    if (lnf) {      // accumulator rows m0 + WROWS wm + 32 c + 8 q + 4 h + r
                        const float2* sp = p.a_stats + m0 + wm * WROWS + c * 32 + 8 * q + 4 * h;
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
                const int m = m0 + wm * WROWS + c * 32 + kg * 8;           // first of 8 consecutive keys
                if (m < p.Mvalid) {
                    int b = qkv_b0, sq = m - qkv_b0 * p.Sp;
                    while (sq >= p.Sp) { sq -= p.Sp; ++b; }
                    if constexpr (EPI == EPI_QKVR) {      // decoder V^T MX tiles (decoder_mx.hip): D / 32 sub-tiles of 4 KiB per 32-key tile, (lo8 | hi8)
                        const float x8[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                        const int col0 = n0 + wn * 64, g = (col0 >> 7) - p.nq - p.nkv, ddl = 64 * ((col0 >> 6) & 1) + dd, kgt = (sq & 31) >> 3;
                        unsigned char* sub = reinterpret_cast<unsigned char*>(p.Vt) + ((size_t)(b * p.nkv + g) * (p.Sp >> 5) + (sq >> 5)) * 16384 + (ddl >> 5) * 4096;
                        store_mx8(sub + (kgt >> 1) * 1024 + (32 * (kgt & 1) + (ddl & 31)) * 16, sub + 2048 + (32 * (kgt & 1) + (ddl & 31)) * 32 + 8 * (kgt >> 1), x8, false,
                                  m < p.gx_rows ? p.gx_sat : nullptr);
                        continue;
                    }
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

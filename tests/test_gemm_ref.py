"""CPU: the numpy side of the kernel-level GEMM tests (tests/gemm_ref.py) checked on its own — every codec against an encoder written
a second time (element loops straight from the format comments), the accuracy each operand format claims against the exact product
(computed here, in float64: GS ~2^-22, MX ~2^-15 per product), and the checker's sensitivity: the emulation's own output with one
seeded defect of the kinds a wrong tile produces must be flagged, the clean output must pass."""
import math
import struct

import numpy as np
import pytest

import gemm_ref as R


def _rng(seed):
    return np.random.default_rng(seed)


def _f16_bits_slow(x):
    """fp32 -> f16 bits by arithmetic (round to nearest even on the f16 grid), no numpy conversion."""
    x = float(x)
    s = 0x8000 if math.copysign(1.0, x) < 0 else 0
    a = abs(x)
    if a == 0.0:
        return s
    e = max(math.frexp(a)[1] - 1, -14)                 # exponent of the grid: subnormals share 2^-14
    q = a / math.ldexp(1.0, e - 10)                    # in units of the spacing (exact: power of two)
    n = math.floor(q)
    n += 1 if (q - n > 0.5 or (q - n == 0.5 and n % 2 == 1)) else 0
    if n >= 2048:
        n //= 2; e += 1
    if e > 15:
        return s | 0x7C00
    return s | (n if n < 1024 else ((e + 15) << 10) | (n - 1024))


def test_f16_and_bf16_rounding():
    r = _rng(1)
    x = np.concatenate([r.standard_normal(4000).astype(np.float32) * np.float32(10.0) ** r.integers(-7, 5, 4000).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 65504.0, 65519.0, 6.1e-5], np.float32)])
    got = x.astype(np.float16).view(np.uint16)
    want = np.array([_f16_bits_slow(v) for v in x], np.uint16)
    assert np.array_equal(R.encode_T(x, "f16"), got) and np.array_equal(got, want)
    assert np.array_equal(R.decode_T(got, "f16"), R.round_f16(x))
    # bf16: nearest multiple of the 8-bit grid, ties to even, in float64 arithmetic
    e = np.floor(np.log2(np.maximum(np.abs(x.astype(np.float64)), 2.0 ** -126)))
    ulp = 2.0 ** (e - 7)
    want_bf = (np.round(x.astype(np.float64) / ulp) * ulp).astype(np.float32)
    assert np.array_equal(R.round_bf16(x), want_bf)
    assert np.array_equal(R.decode_T(R.encode_T(x, "bf16"), "bf16"), want_bf)


def _e4m3_slow(v, saturate=True):
    s = 0x80 if math.copysign(1.0, v) < 0 else 0
    a = abs(v)
    if a > 448.0:
        if saturate or a <= 464.0:
            return s | 0x7E
        return s | 0x7F
    if a == 0.0:
        return s
    e = max(math.frexp(a)[1] - 1, -6)
    q = a / math.ldexp(1.0, e - 3)
    n = math.floor(q)
    n += 1 if (q - n > 0.5 or (q - n == 0.5 and n % 2 == 1)) else 0
    if n >= 16:
        n //= 2; e += 1
    return s | (n if n < 8 else ((e + 7) << 3) | (n - 8))


def test_e4m3_codec():
    codes = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)
    assert np.array_equal(R.e4m3_encode(R.e4m3_decode(codes)), codes)
    assert R.e4m3_decode(np.uint8(0x7E)) == 448.0 and R.e4m3_decode(np.uint8(0x01)) == 2.0 ** -9 and R.e4m3_decode(np.uint8(0x38)) == 1.0
    r = _rng(2)
    pos = R.E4M3[:127]
    mids = (pos[1:] + pos[:-1]) / 2                       # every tie
    x = np.concatenate([r.uniform(-500, 500, 3000), r.uniform(-1, 1, 3000), r.uniform(-0.02, 0.02, 2000), mids, -mids, [448.0, 449.0, 464.0, 464.5, 1e4]])
    for sat in (True, False):
        want = np.array([_e4m3_slow(v, sat) for v in x], np.uint8)
        assert np.array_equal(R.e4m3_encode(x, sat), want), sat


def test_gs_rows_against_element_loop():
    r = _rng(3)
    M, K = 3, 96
    x = (r.standard_normal((M, K)) * 3).astype(np.float32)
    raw = R.gs_encode(x)
    want = np.zeros((M, 2 * K), np.uint16)
    for m in range(M):
        for e in range(K):
            h = np.float32(x[m, e]).astype(np.float16)
            lo = np.float16(np.float32(x[m, e]) - np.float32(h))
            want[m, (e >> 5) * 64 + (e & 31)] = h.view(np.uint16)             # glc_common.h: halves (e >> 5) * 64 + (e & 31) (hi) and + 32 (lo)
            want[m, (e >> 5) * 64 + (e & 31) + 32] = lo.view(np.uint16)
    assert np.array_equal(raw, want)
    hi, lo = R.gs_decode(raw, M, K)
    assert np.abs((hi.astype(np.float64) + lo) - x).max() <= 2.0 ** -22 * np.abs(x).max()


@pytest.mark.parametrize("worder", (0, 1))
def test_gx_rows_against_element_loop(worder):
    r = _rng(4 + worder)
    M, K, sc = 2, 64, (5 if worder else -5)
    x = (r.standard_normal((M, K)) * (0.05 if worder else 200.0)).astype(np.float32)
    raw = R.gx_encode(x, sc, worder)
    want = np.zeros((M, 4 * K), np.uint8)
    for m in range(M):
        for e in range(K):
            h = np.float32(x[m, e]).astype(np.float16)
            lo = float(np.float32(x[m, e]) - np.float32(h))
            base = (e >> 5) * 128
            want[m, base + 2 * (e & 31): base + 2 * (e & 31) + 2] = np.frombuffer(struct.pack("<e", float(h)), np.uint8)
            j, i = (e & 31) >> 3, e & 7
            lo8, hi8 = _e4m3_slow(lo * 2.0 ** (R.GX_SHIFT + sc), bool(worder)), _e4m3_slow(float(x[m, e]) * 2.0 ** sc, bool(worder))
            want[m, base + 64 + 16 * j + i] = hi8 if worder else lo8          # activations [lo8 | hi8], weights [hi8 | lo8]
            want[m, base + 64 + 16 * j + 8 + i] = lo8 if worder else hi8
    assert np.array_equal(raw, want)
    hi, lo8, hi8 = R.gx_decode(raw, M, K, worder)
    assert np.array_equal(hi, R.round_f16(x))
    v = R.gx_value(hi, lo8, sc)
    assert np.abs(v.astype(np.float64) - x).max() <= np.abs(x).max() * 2.0 ** -15 + 2.0 ** -(10 + R.GX_SHIFT + sc)
    assert np.abs(hi8 * 2.0 ** -sc - x).max() <= np.abs(x).max() * 2.0 ** -4
    assert R.gx_weight_exponent(0.5) == 8 and R.gx_weight_exponent(240.0) == 0 and R.gx_weight_exponent(0.0) == 0 and R.gx_weight_exponent(1e-20) == 40


def test_fragment_major_layouts_against_element_loop():
    r = _rng(6)
    BH, Sp = 3, 64
    Q = r.standard_normal((BH, Sp, 64)).astype(np.float32)
    nt = Sp // 32
    for klayout in (False, True):
        flat = np.zeros(BH * Sp * 64, np.float32)
        for bh in range(BH):
            for row in range(Sp):
                for e in range(0, 64):
                    rr = row & 31
                    if klayout:
                        rr = (rr & 0x13) | ((rr & 4) << 1) | ((rr & 8) >> 1)
                    s, h, j = e >> 4, (e >> 3) & 1, e & 7
                    flat[((((bh * nt + (row >> 5)) * 4 + s) * 64 + 32 * h + rr) * 8) + j] = Q[bh, row, e]
        assert np.array_equal(R.units_from_q(Q, klayout).reshape(-1), flat)
        assert np.array_equal(R.q_from_units(flat.reshape(-1, 8), BH, Sp, klayout), Q)
    Vt = r.standard_normal((BH, 64, Sp)).astype(np.float32)
    flat = np.zeros(BH * Sp * 64, np.float32)
    for bh in range(BH):
        for dd in range(64):
            for key in range(Sp):
                kt, t, h, j = key >> 5, (key >> 4) & 1, (key >> 3) & 1, key & 7
                flat[(((((bh * nt + kt) * 2 + (dd >> 5)) * 2 + t) * 64 + 32 * h + (dd & 31)) * 8) + j] = Vt[bh, dd, key]
    assert np.array_equal(R.units_from_vt(Vt).reshape(-1), flat)
    assert np.array_equal(R.vt_from_units(flat.reshape(-1, 8), BH, Sp), Vt)
    # split-f16 units: [8 hi | 8 lo] halves in the 32 bytes of an fp32 unit
    hi, lo = R.split_f16(Q)
    u = np.concatenate([R.units_from_q(hi), R.units_from_q(lo)], axis=1).astype(np.float16)
    (qa, qb), _, _ = R.qkv_decode([u.tobytes()] * 3, "f32", True, 1, BH, Sp)
    assert np.array_equal(qa, hi) and np.array_equal(qb, lo)


def test_mx_tiles_against_element_loop():
    r = _rng(7)
    BH, Sp = 2, 64
    X = (r.standard_normal((BH, Sp, 64)) * 2).astype(np.float32)
    hi, lo8, hi8 = R.gx_parts(X, 0, saturate=False)
    for hl, klayout in ((True, False), (False, True)):
        buf = np.zeros(BH * (Sp // 32) * 8192, np.uint8)
        for bh in range(BH):
            for row in range(Sp):
                tile, slot = bh * (Sp // 32) + (row >> 5), int(R.pi32(row & 31)) if klayout else row & 31
                for e in range(64):
                    o16 = tile * 8192 + (e >> 4) * 1024 + (32 * ((e >> 3) & 1) + slot) * 16 + 2 * (e & 7)
                    buf[o16:o16 + 2] = np.frombuffer(struct.pack("<e", float(hi[bh, row, e])), np.uint8)
                    y = e & 15
                    omx = tile * 8192 + 4096 + (e >> 5) * 2048 + (32 * ((e >> 4) & 1) + slot) * 32 + y      # lane 32 h + slot, column 32 m + 16 h + y
                    buf[omx] = hi8[bh, row, e] if hl else lo8[bh, row, e]
                    buf[omx + 16] = lo8[bh, row, e] if hl else hi8[bh, row, e]
        dh, dl, dh8 = R.mxt_qk_decode(buf.tobytes(), BH, Sp, hl, klayout)
        assert np.array_equal(dh, hi) and np.array_equal(dl, R.e4m3_decode(lo8)) and np.array_equal(dh8, R.e4m3_decode(hi8))


@pytest.mark.parametrize("D", (64, 128))
def test_mx_tiles_head_dim_and_vt_sub_tiles_against_element_loop(D):
    """Q / K tiles of head_dim D (the decoder's 128) and the V^T sub-tiles, filled byte by byte from the layout comments."""
    r = _rng(8 + D)
    BH, Sp = 2, 64
    nt = Sp // 32
    X = (r.standard_normal((BH, Sp, D)) * 2).astype(np.float32)
    hi, lo8, hi8 = R.gx_parts(X, 0, saturate=False)
    buf = np.zeros(BH * nt * 128 * D, np.uint8)
    for bh in range(BH):
        for row in range(Sp):
            base, slot = (bh * nt + (row >> 5)) * 128 * D, int(R.pi32(row & 31))
            for e in range(D):
                o16 = base + (e >> 4) * 1024 + (32 * ((e >> 3) & 1) + slot) * 16 + 2 * (e & 7)
                buf[o16:o16 + 2] = np.frombuffer(struct.pack("<e", float(hi[bh, row, e])), np.uint8)
                omx = base + (D // 16) * 1024 + (e >> 5) * 2048 + (32 * ((e >> 4) & 1) + slot) * 32 + (e & 15)
                buf[omx], buf[omx + 16] = lo8[bh, row, e], hi8[bh, row, e]
    dh, dl, dh8 = R.mxt_qk_decode(buf.tobytes(), BH, Sp, False, True, D)
    assert np.array_equal(dh, hi) and np.array_equal(dl, R.e4m3_decode(lo8)) and np.array_equal(dh8, R.e4m3_decode(hi8))
    Vt = np.ascontiguousarray(X.transpose(0, 2, 1))                    # [BH, D, Sp]
    vh, vl8, vh8 = R.gx_parts(Vt, 0, saturate=False)
    buf = np.zeros(BH * nt * 128 * D, np.uint8)
    for bh in range(BH):
        for dd in range(D):
            for key in range(Sp):
                sub = ((bh * nt + (key >> 5)) * (D // 32) + (dd >> 5)) * 4096
                ko = key & 31
                t, h, j = ko >> 4, (ko >> 3) & 1, ko & 7
                o16 = sub + t * 1024 + (32 * h + (dd & 31)) * 16 + 2 * j
                buf[o16:o16 + 2] = np.frombuffer(struct.pack("<e", float(vh[bh, dd, key])), np.uint8)
                y = 8 * t + j                                          # key = 16 (y >> 3) + 8 h + (y & 7)
                omx = sub + 2048 + (32 * h + (dd & 31)) * 32 + y
                buf[omx], buf[omx + 16] = vl8[bh, dd, key], vh8[bh, dd, key]
    dh, dl, dh8 = R.mxt_vt_decode(buf.tobytes(), BH, Sp, D)
    assert np.array_equal(dh, vh) and np.array_equal(dl, R.e4m3_decode(vl8)) and np.array_equal(dh8, R.e4m3_decode(vh8))


def test_glu_rows_and_rope_permutation():
    I, K = 64, 4
    g, u = np.arange(I * K, dtype=np.float32).reshape(I, K), -np.arange(I * K, dtype=np.float32).reshape(I, K) - 1
    W = R.glu_interleave(g, u)
    for p in range(2 * I):
        f = 16 * (p // 32) + p % 16
        assert np.array_equal(W[p], (g if (p // 16) % 2 == 0 else u)[f])
    acc = np.arange(2 * 2 * I, dtype=np.float64).reshape(2, 2 * I) / 50 - 2
    out = R.epilogue(acc, R.EPI_SWIGLU)
    assert out.shape == (2, I) and math.isclose(out[1, 17], R.silu(acc[1, 32 + 1]) * acc[1, 32 + 16 + 1])
    p = R.rope_perm128(np.arange(128))
    assert np.array_equal(np.sort(p), np.arange(128)) and np.array_equal(p[p], np.arange(128))
    assert p[0] == 0 and p[32] == 64 and p[64] == 32 and p[96] == 96 and p[37] == 69


# ---- the accuracy each operand format claims, on the GPU sweep's own random operands
def sweep_operands(M, N, K, a_amp=1.0, w_amp=0.05, seed=0):
    r = _rng(1000 + seed)
    return (r.uniform(-a_amp, a_amp, (M, K)).astype(np.float32), r.uniform(-w_amp, w_amp, (N, K)).astype(np.float32))


@pytest.mark.parametrize("K", (32, 96, 768))
def test_emulation_against_exact_within_the_claimed_accuracy(K):
    """GS: x = hi + lo + d with |d| <= 2^-22 |x| (lo rounded to f16), the lo * lo product (<= 2^-22) dropped: |emulated - exact| <= 3 * 2^-22
    (1 + o(1)) sum |a| |w|.  MX: each cross term's two 4-bit operands cost 2^-4 + 2^-4 + 2^-8 of a term that is <= 2^-11 of the product:
    <= 2^-13 (1 + 2^-5) sum |a| |w| in the worst case plus the e4m3 subnormal floor (2^-10 per scaled part) and the GS terms; the claim of
    the kernel header and test_gpu_mx.py — about 2^-15 per product — is the rms figure, asserted as such."""
    A, W = sweep_operands(128, 128, K)
    exact, mag, _ = R.accumulate(R.operands("exact", A, W))
    gs, _, _ = R.accumulate(R.operands("gs", A, W))
    ws = R.gx_weight_exponent(float(np.abs(W).max()))
    mx, _, _ = R.accumulate(R.operands("mx", A, W, sc_a=0, sc_w=ws))
    r_gs = float((np.abs(gs - exact) / mag).max())
    floor = 2.0 ** -(10 + R.GX_SHIFT) * np.abs(W).sum(1)[None, :] + 2.0 ** -(10 + R.GX_SHIFT + ws) * np.abs(A).sum(1)[:, None]
    r_mx = float((np.abs(mx - exact) / mag).max())
    r_mx_b = float((np.abs(mx - exact) / (mag * (2.0 ** -13 * (1 + 2.0 ** -5) + 3 * 2.0 ** -22) + floor)).max())
    rms_mx = float(np.sqrt(((mx - exact) ** 2).mean()) / np.sqrt(K * (A.astype(np.float64) ** 2).mean() * (W.astype(np.float64) ** 2).mean()))
    print(f"K={K}: GS max |emul - exact| / sum|a||w| = 2^{math.log2(r_gs):.2f}; MX max = 2^{math.log2(r_mx):.2f} (worst-case bound ratio {r_mx_b:.3f}), "
          f"MX rms error per rms product * sqrt(K) = 2^{math.log2(rms_mx):.2f}")
    assert r_gs <= 3.01 * 2.0 ** -22
    assert r_mx_b <= 1.0
    assert rms_mx <= 2.0 ** -15


# ---- the checker is sensitive
def _gs_case():
    M, N, K = 256, 256, 96
    A, W = sweep_operands(M, N, K, seed=5)
    bias = _rng(9).uniform(-0.1, 0.1, N).astype(np.float32)
    terms = R.operands("gs", A, W)
    acc, mag, steps = R.accumulate(terms)
    ref = R.epilogue(acc, R.EPI_BIAS, bias=bias)
    bnd = R.bound(mag, steps, extra=R.U24 * (np.abs(acc) + np.abs(bias)[None, :]) + R.out_quant(ref, "gs"))
    return A, W, bias, terms, ref, bnd


def test_checker_passes_clean_output_and_flags_every_seeded_defect():
    A, W, bias, terms, ref, bnd = _gs_case()
    clean = ref.astype(np.float32)                         # what a correct kernel may return: the reference rounded to fp32
    ok, worst, _ = R.check(clean, ref, bnd)
    assert ok and worst < 1.0
    (ah, wh, _), (_, wl, _), (al, _, _) = terms

    def flagged(got, where):
        ok, worst, idx = R.check(got, ref, bnd)
        assert not ok and worst > 1.0, where
        return idx
    # one bias element off by 4x that element's bound
    g = clean.astype(np.float64); g[77, 130] += 4 * bnd[77, 130]
    assert flagged(g, "bias element") == (77, 130)
    # one 32-wide K stage missing from one 128 x 128 tile
    g = clean.astype(np.float64); g[128:, :128] -= (ah[128:, 32:64] @ wh[:128, 32:64].T)
    assert flagged(g, "K stage")[0] >= 128
    # two adjacent 16-column blocks swapped in one tile
    g = clean.astype(np.float64); g[:128, 128 + 32:128 + 48], g[:128, 128 + 48:128 + 64] = clean[:128, 128 + 48:128 + 64], clean[:128, 128 + 32:128 + 48]
    flagged(g, "swapped blocks")
    # lo terms dropped in one wave's 128 x 64 quadrant
    g = clean.astype(np.float64); g[128:, 64:128] = (ah[128:] @ wh[64:128].T) + bias[None, 64:128]
    flagged(g, "lo terms")
    # one V^T unit transposed (8 x 8 block of V^T = one column of 16-byte units)
    Vt = clean[:, :64].T.reshape(1, 64, 256)
    bad = Vt.copy(); bad[0, 8:16, 32:40] = Vt[0, 8:16, 32:40].T
    dec = R.vt_from_units(R.units_from_vt(bad), 1, 256)
    ok, _, _ = R.check(dec[0].T, ref[:, :64], bnd[:, :64])
    assert not ok
    assert R.check(R.vt_from_units(R.units_from_vt(Vt), 1, 256)[0].T, ref[:, :64], bnd[:, :64])[0]
    # one slack row written: rows [Mvalid, Mpad) of a prefilled output must still hold the fill pattern
    fill = 0xA5
    buf = np.full((256, 256), fill * 0x01010101, np.uint32)
    buf[:200] = clean[:200].view(np.uint32)
    assert untouched(buf[200:], fill)
    buf[211] = clean[211].view(np.uint32)
    assert not untouched(buf[200:], fill)


def untouched(raw, fill):
    return bool((np.ascontiguousarray(raw).view(np.uint8) == fill).all())

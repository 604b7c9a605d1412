"""GPU (-m gpu): every GEMM kernel and epilogue against float64 references on operands this file chooses (tests/gemm_ref.py), one
launcher call per case through glc_debug_gemm_run (include/gliclass_hip.h), which returns raw bytes only: the formats are decoded here.

Exact cases.  Operands with few significant bits (integers in {-1, 0, 1}, plus {-1, 0, 1} 2^-12 where a lo half must travel) make every
product and every partial sum a multiple of 2^-12 below 2^12 in magnitude — asserted on the reference alone (sum |a| |w| 2^12 < 2^24,
ref == fp32(ref)) — so fp32 accumulation is exact in ANY order and the kernel's output bytes must EQUAL the encoded emulation.  The values
are seeded random, i.e. position dependent: an index permutation changes the product.

Random cases, every element against its own bound
    C_ACC 2^-24 steps (|A| |W|^T)[m, n]  +  epilogue  +  output format.
Derivation of C_ACC = 2.  A kernel forms `steps` products per output (K for 16-bit operands, 3 K for the GS terms, 3 K for the MX terms:
K f16 products and 2 K fp8 products).  Operand products are exact in fp32 (11 x 11 and 4 x 4 bit significands; the block scales are powers
of two), so the only error is that of adding them in fp32.  Adding n terms in any order and any grouping with correctly rounded additions
has |error| <= (n - 1) 2^-24 sum |terms| to first order (Higham, Accuracy and Stability of Numerical Algorithms, (4.4)); the split-K reduce
is n more additions of the same kind in a fixed order and is covered by the same count.  The MFMA adder is not documented to round every
internal addition to nearest: a truncating alignment loses at most one ulp instead of half of one, hence the factor 2 — chosen before any
kernel output was looked at.  The epilogue adds 2^-24 per fp32 operation on the magnitudes it handles (EPI_OPS operations at most), the
function errors the sources document (Abramowitz-Stegun 7.1.26: 1.5e-7 on erf; glc_gelu2_f32: 5.9e-7; glc_gelu2: 2.6e-5; the hardware
exp2 / rcp approximations: 1 ulp each), and the output format's rounding (gemm_ref.out_quant).  A worst ratio above 1 is a finding.

Worst ratios observed on an MI355X are recorded in DESIGN.md ("Kernel-level tests"); the test prints them (pytest -s)."""
import math

import numpy as np
import pytest

import gemm_ref as R
from gemm_run import FILL, run

pytestmark = pytest.mark.gpu

EPI_OPS = 8
_ENG = {}
RATIOS = {}


def _engine(weights_for, dt):
    from gliclass.c_amd.engine import Engine
    if dt not in _ENG:
        cfg, w = weights_for("tiny")
        _ENG[dt] = Engine(cfg, w, dtype=dt)
    return _ENG[dt]


def ints(shape, seed, lo_part=False, density=0.67):
    """{-1, 0, 1} (+ {-1, 0, 1} 2^-12 with lo_part), seeded."""
    r = np.random.default_rng(seed)
    x = r.integers(-1, 2, shape).astype(np.float32) * (r.random(shape) < density / 0.67)
    if lo_part:      # only beside a non-zero integer: hi = the integer, lo = the 2^-12 part, every product a multiple of 2^-12
        x = x + (x != 0) * r.integers(-1, 2, shape).astype(np.float32) * np.float32(2.0 ** -12)
    return x.astype(np.float32)


def rnd(shape, amp, seed):
    return np.random.default_rng(seed).uniform(-amp, amp, shape).astype(np.float32)


KIND = {R.K128: None, R.K256S: "T", R.KGS: "gs", R.KMX: "mx", R.KAUTO: None}


def emulate(kernel, dt, epi, A, W, o):
    """-> (ref float64, bound, fmt) of the C output of a non-QKV launch, with the operands as that kernel reads them."""
    kind = KIND[kernel] or ("gs" if dt == "f32" else "T")
    sc_a, sc_w = o.get("act_sc", 0), o.get("mx_ws", 0)
    terms = R.operands(kind, A, W, dt, sc_a, sc_w, o.get("prec", 0))
    acc, mag, steps = R.accumulate(terms)
    if o.get("W2") is not None:
        acc2, mag2, _ = R.accumulate(R.operands(kind, A, o["W2"], dt, sc_a, sc_w))
        ms = o["m_split"]
        acc[ms:], mag[ms:] = acc2[ms:], mag2[ms:]
    if o.get("ws_bytes"):
        steps += 8                                            # 128-tile split-K: the reduce adds at most 8 partial tiles in a fixed order
    bias = o.get("bias")
    if o.get("bias2") is not None:                            # two weight groups: a bias per row group, one epilogue addition like the single bias
        bias = np.where(np.arange(len(acc))[:, None] >= o["m_split"], o["bias2"][None, :], o["bias"][None, :])
    resid = o.get("resid")
    if resid is not None:      # the residual as the kernel reads it back
        if kind == "T":
            resid = R.round_T(resid, dt)
        elif kind == "gs" and kernel == R.KGS and not o.get("gs_resid_plain"):
            hi, lo = R.split_f16(resid)
            resid = hi if o.get("prec", 0) & 4 else (hi + lo).astype(np.float32)
        elif kind == "mx":
            hi, lo8, _ = R.gx_parts(resid, sc_a, saturate=False)
            resid = R.gx_value(hi, R.e4m3_decode(lo8), sc_a)
    kw = dict(bias=bias, resid=resid, a_stats=o.get("a_stats"), ln_c=o.get("ln_c"), r_stats=o.get("r_stats"), r_gamma=o.get("r_gamma"), r_beta=o.get("r_beta"))
    ref = R.epilogue(acc, epi, **kw)
    b_acc = R.bound(mag, steps)
    # magnitudes the epilogue's fp32 operations handle, and how the accumulation error passes through it
    amp = np.ones((len(acc), 1))
    emag = np.abs(acc)
    if o.get("a_stats") is not None and epi != R.EPI_RESID:
        st = np.asarray(o["a_stats"], np.float64).reshape(-1, 2)
        amp = np.abs(st[:, 1:2])
        emag = amp * (np.abs(acc) + np.abs(st[:, 0:1]) * (0 if o.get("ln_c") is None else np.abs(o["ln_c"])[None, :]))
    if bias is not None:
        emag = emag + (np.abs(bias) if np.ndim(bias) == 2 else np.abs(bias)[None, :])
    pre = b_acc * amp + EPI_OPS * R.U24 * emag                  # error of the value the activation / residual step receives
    if epi == R.EPI_GELU:
        x = R.epilogue(acc, R.EPI_BIAS, **{**kw, "resid": None})
        if kernel in (R.K128, R.KAUTO):      # glc_gelu: Abramowitz-Stegun erf (1.5e-7) through exp / rcp approximations
            f_err = 0.5 * np.abs(x) * (1.5e-7 + 16 * R.U24) + 4 * R.U24 * np.abs(ref)
        else:                                # glc_gelu2_f32 (GS / MX rows) / glc_gelu2 (16-bit): the deviations their comments state
            f_err = 5.9e-7 if kind != "T" else 2.6e-5
        bnd = 1.13 * pre + f_err                               # |gelu'| <= 1.13
    elif epi in (R.EPI_SWIGLU, R.EPI_GEGLU):
        M, N = acc.shape
        x = R.epilogue(acc, R.EPI_BIAS, a_stats=None if o.get("a_stats") is None else np.stack([np.zeros(M), np.asarray(o["a_stats"]).reshape(-1, 2)[:, 1]], 1))
        sp = lambda v, t: v.reshape(M, N // 32, 2, 16)[:, :, t].reshape(M, N // 2)
        g, u, bg, bu = sp(x, 0), sp(x, 1), sp(pre, 0), sp(pre, 1)
        if epi == R.EPI_SWIGLU:
            bnd = 1.1 * bg * np.abs(u) + np.abs(R.silu(g)) * bu + np.abs(ref) * (16 + 4 * np.abs(g)) * R.U24      # |silu'| <= 1.1
        else:
            bnd = (1.13 * bg + (5.9e-7 if kind != "T" else 2.6e-5)) * np.abs(u) + np.abs(R.gelu(g)) * bu + 4 * R.U24 * np.abs(ref)
    elif epi == R.EPI_RESID:
        r_t = np.abs(R.epilogue(np.zeros_like(acc), R.EPI_RESID, **{**kw, "bias": None}))
        if o.get("r_stats") is not None:
            st = np.asarray(o["r_stats"], np.float64).reshape(-1, 2)
            r_t = (np.abs(resid) + np.abs(st[:, 0:1])) * np.abs(st[:, 1:2] * np.asarray(o["r_gamma"], np.float64)[None, :]) + np.abs(o["r_beta"])[None, :]
        bnd = pre + EPI_OPS * R.U24 * (r_t + np.abs(ref))
    else:
        bnd = pre
    if kernel in (R.KGS, R.KMX):
        plain = o.get("gs_c_plain") or (epi == R.EPI_RESID and not o.get("want_ln_part"))
        fmt = "f32" if plain else ("gs" if kernel == R.KGS else "gx")
    else:
        fmt = dt
    q = R.out_quant(np.abs(ref) + bnd, fmt, sc_a)
    return ref, bnd, q, fmt, mag


def decode_c(res, fmt, dt, rows, cols, sc=0):
    raw = res["out"][0]
    if fmt == "gs":
        hi, lo = R.gs_decode(raw, rows, cols)
        return hi.astype(np.float64) + lo
    if fmt == "gx":
        hi, lo8, _ = R.gx_decode(raw, rows, cols, 0)
        return hi.astype(np.float64) + lo8 * 2.0 ** -(R.GX_SHIFT + sc)
    return R.decode_T(R.raw_T(raw.tobytes(), fmt), fmt).reshape(rows, cols).astype(np.float64)


def encode_c(v32, fmt, sc=0):
    if fmt == "gs":
        return R.gs_encode(v32).view(np.uint8).reshape(-1)
    if fmt == "gx":
        return R.gx_encode(v32, sc, 0).reshape(-1)
    return np.ascontiguousarray(R.encode_T(v32, fmt)).view(np.uint8).reshape(-1)


def check_images(res, kernel, dt, A, W, o):
    """the library's converters against this file's encoders, bit for bit"""
    if kernel == R.KGS:
        assert np.array_equal(res["A_img"].view(np.uint16), R.gs_encode(A).reshape(-1)) and np.array_equal(res["W_img"].view(np.uint16), R.gs_encode(W).reshape(-1))
    elif kernel == R.KMX:
        assert np.array_equal(res["A_img"], R.gx_encode(A, o.get("act_sc", 0), 0).reshape(-1)), "activation GX image"
        Wv = W
        if o.get("w_from_gs"):
            hi, lo = R.split_f16(W)
            Wv = (hi + lo).astype(np.float32)
        assert np.array_equal(res["W_img"], R.gx_encode(Wv, o.get("mx_ws", 0), 1).reshape(-1)), "weight GX image"
    elif dt != "f32":
        assert np.array_equal(res["A_img"].view(np.uint16), R.encode_T(A, dt).reshape(-1)) and np.array_equal(res["W_img"].view(np.uint16), R.encode_T(W, dt).reshape(-1))
    elif o.get("w_presplit"):
        assert np.array_equal(res["W_img"].view(np.uint16), R.gs_encode(W).reshape(-1))


def case(weights_for, dt, kernel, epi, A, W, exact=False, label="", **o):
    eng = _engine(weights_for, dt)
    ref, bnd, q, fmt, mag = emulate(kernel, dt, epi, A, W, o)
    if exact:      # representability, on the reference alone
        assert float(mag.max()) * 2.0 ** 12 < 2.0 ** 24 and np.array_equal(ref, ref.astype(np.float32).astype(np.float64)), "the exact case is not exactly representable"
    res = run(eng, kernel, epi, A, W, **o)
    assert res["rc"] == 0, res["err"]
    assert res["guards_ok"] == 1, "a guard region was written"
    check_images(res, kernel, dt, A, W, o)
    rows, cols = ref.shape
    sc = o.get("act_sc", 0)
    if o.get("perm_cols"):      # columns [0, perm_cols) are computed in the RoPE row order and stored at their logical place
        n = np.arange(cols)
        nl = np.where(n < o["perm_cols"], (n & ~127) | R.rope_perm128(n & 127), n)
        for v in (ref, bnd, q):
            v[:, nl] = v.copy()
    got = decode_c(res, fmt, dt, rows, cols, sc)
    if exact:
        assert np.array_equal(res["out"][0], encode_c(ref.astype(np.float32), fmt, sc)), f"{label}: output bytes differ from the encoded emulation"
    ok, worst, idx = R.check(got, ref, bnd + q)
    key = (("128", "256s", "gs", "mx", "auto")[kernel] + ":" + dt, ("bias", "gelu", "resid", "qkv", "swiglu", "qkvr", "geglu")[epi] + ("+" + label if label else ""))
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    print(f"[gemm] {key[0]:10s} {key[1]:28s} M={rows} N={W.shape[0]} K={A.shape[1]} worst error / bound = {worst:.4f}" + (" (bit-exact)" if exact else ""))
    assert ok, (key, worst, idx, got[idx], ref[idx], (bnd + q)[idx])
    if o.get("want_ln_part"):
        want = R.ln_partials(ref)
        if exact:      # sums of 64 integers, deviations multiples of 2^-6 below 8: every square and partial sum fits 24 bits -> bit for bit
            dev_max = np.abs(ref.reshape(rows, cols // 64, 64) - want[:, :, :1] / 64).max()
            assert np.array_equal(ref, np.round(ref)) and dev_max < 8, "the exact ln_part case is not exactly representable"
            assert np.array_equal(res["ln_part"], want.astype(np.float32)), f"{label}: ln_part differs from the float64 partials"
        pb = 64 * R.U24 * np.abs(ref).reshape(rows, cols // 64, 64).sum(2) + (bnd + q).reshape(rows, cols // 64, 64).sum(2)
        okp, wp, ip = R.check(res["ln_part"][:, :, 0], want[:, :, 0], pb)
        assert okp, ("ln_part sums", wp, ip)
        dev = np.sqrt(want[:, :, 1])
        d = (bnd + q).reshape(rows, cols // 64, 64).max(2) + pb / 64      # error of one deviation v - block mean
        okq, wq, iq = R.check(res["ln_part"][:, :, 1], want[:, :, 1], 2 * dev * 8 * d + 64 * d * d + 200 * R.U24 * want[:, :, 1] + 1e-30)
        assert okq, ("ln_part M2", wq, iq)
    return res, ref, got


def epi_args(epi, M, N, seed, exact, fold=False, rln=False):
    o = {}
    if epi in (R.EPI_BIAS, R.EPI_GELU, R.EPI_RESID):
        o["bias"] = ints(N, seed + 1) * 3 if exact else rnd(N, 0.1, seed + 1)
    if epi == R.EPI_RESID:
        o["resid"] = ints((M, N), seed + 2, lo_part=False) * 2 if exact else rnd((M, N), 1.0, seed + 2)
    if fold:
        o["a_stats"] = np.stack([rnd(M, 0.1, seed + 3), 0.5 + np.abs(rnd(M, 0.4, seed + 4))], 1)
        o["ln_c"] = rnd(N, 0.05, seed + 5)
    if rln:
        o["r_stats"] = np.stack([rnd(M, 0.1, seed + 6), 0.5 + np.abs(rnd(M, 0.4, seed + 7))], 1)
        o["r_gamma"], o["r_beta"] = 1 + rnd(N, 0.3, seed + 8), rnd(N, 0.2, seed + 9)
    return o


# ------------------------------------------------------------------------------------------------ 128-tile
@pytest.mark.parametrize("dt", ("f32", "f16", "bf16"))
@pytest.mark.parametrize("epi", (R.EPI_BIAS, R.EPI_GELU, R.EPI_RESID))
def test_128_tile(weights_for, dt, epi):
    kb = 32 if dt == "f32" else 64                              # one stage = 128 bytes of K
    for (M, N, K, exact) in ((128, 128, kb, True), (256, 384, 3 * kb, True), (128, 256, 5 * kb, False), (256, 128, 12 * kb, False)):
        if epi == R.EPI_GELU and exact:
            continue
        A = ints((M, K), 10, lo_part=dt == "f32") if exact else rnd((M, K), 1.0, 11)
        W = ints((N, K), 12, lo_part=dt == "f32") if exact else rnd((N, K), 0.05, 13)
        for presplit in ((0, 1) if dt == "f32" else (0,)):
            case(weights_for, dt, R.K128, epi, A, W, exact=exact, w_presplit=presplit, **epi_args(epi, M, N, 20, exact))


@pytest.mark.parametrize("dt", ("f32", "f16", "bf16"))
@pytest.mark.parametrize("m_split", (0, 128))
def test_128_tile_split_k_and_two_weight_groups(weights_for, dt, m_split):
    """37 K stages: 8 parts of 5 stages, the last of 2 (no part count from 2 to 8 divides 37); with and without a workspace; with W2 / bias2."""
    kb = 32 if dt == "f32" else 64
    M, N, K = 256, 128, 37 * kb
    for exact in (True, False):
        A = ints((M, K), 30, lo_part=dt == "f32", density=0.3) if exact else rnd((M, K), 1.0, 31)
        W = ints((N, K), 32, lo_part=dt == "f32", density=0.3) if exact else rnd((N, K), 0.05, 33)
        o = epi_args(R.EPI_RESID, M, N, 40, exact)
        if m_split:
            o.update(W2=ints((N, K), 34, density=0.3) if exact else rnd((N, K), 0.05, 35), bias2=ints(N, 36) if exact else rnd(N, 0.1, 37), m_split=m_split)
        with_ws, _, got_ws = case(weights_for, dt, R.K128, R.EPI_RESID, A, W, exact=exact, label="splitk", ws_bytes=8 * M * N * 4, **o)
        # split-K engaged on this device (gemm.hip splitk_parts: tiles * 2 <= CUs, parts = min(8, CUs / tiles, stages / 4) >= 2), and unevenly
        tiles, cus = (M // 128) * (N // 128), with_ws["cus"]
        parts = min(8, cus // tiles, 37 // 4)
        assert tiles * 2 <= cus and parts >= 2 and 37 % parts != 0, (cus, parts)
        without, _, got = case(weights_for, dt, R.K128, R.EPI_RESID, A, W, exact=exact, **o)
        if exact:
            assert np.array_equal(with_ws["out"][0], without["out"][0])


def qkv_case(weights_for, dt, kernel, Mpad, Mvalid, Sp, H, K, exact, label="", **o):
    eng = _engine(weights_for, dt)
    N, nh = 3 * H, H // 64
    lo = kernel != R.K256S and (dt == "f32" or kernel in (R.KGS, R.KMX))
    A = ints((Mpad, K), 50, lo_part=lo) if exact else rnd((Mpad, K), 1.0, 51)
    W = ints((N, K), 52, lo_part=lo) if exact else rnd((N, K), 0.05, 53)
    bias = ints(N, 54) * 2 if exact else rnd(N, 0.1, 54)
    split = kernel in (R.KGS, R.KMX) or (dt == "f32" and o.get("qkv_split"))
    kind = KIND[kernel] or ("gs" if dt == "f32" else "T")
    acc, mag, steps = R.accumulate(R.operands(kind, A, W, dt, 0, o.get("mx_ws", 0)))
    ref = R.epilogue(acc, R.EPI_BIAS, bias=bias, a_stats=o.get("a_stats"), ln_c=o.get("ln_c"))
    amp = 1.0 if o.get("a_stats") is None else np.abs(np.asarray(o["a_stats"]).reshape(-1, 2)[:, 1:2])
    fold_mag = 0.0 if o.get("a_stats") is None else np.abs(np.asarray(o["a_stats"]).reshape(-1, 2)[:, 0:1]) * np.abs(o["ln_c"])[None, :]
    bnd = R.bound(mag, steps) * amp + EPI_OPS * R.U24 * (amp * (np.abs(acc) + fold_mag) + np.abs(bias)[None, :])
    bnd = bnd + R.out_quant(np.abs(ref) + bnd, "gs" if split else dt)
    if exact:
        assert float(mag.max()) * 2.0 ** 12 < 2.0 ** 24 and np.array_equal(ref, ref.astype(np.float32).astype(np.float64))
    res = run(eng, kernel, R.EPI_QKV, A, W, bias=bias, Mvalid=Mvalid, Sp=Sp, nh=nh, H=H, **o)
    assert res["rc"] == 0, res["err"]
    assert res["guards_ok"] == 1, "a guard region (rows beyond the buffers) was written"
    B = -(-Mvalid // Sp)
    rows = B * Sp                                               # rows the buffers hold: [0, Mvalid) written, [Mvalid, B Sp) slack
    fill_word = np.frombuffer(bytes([FILL]) * 4, np.float32)[0] if not split and dt == "f32" else None
    (qa, qb), (ka, kb_), (va, vb) = R.qkv_decode([b.tobytes() for b in res["out"]], dt, split, B, nh, Sp)
    two = lambda a, b: a.astype(np.float64) if b is None else a.astype(np.float64) + b
    Q = two(qa, qb).reshape(B, nh, Sp, 64).transpose(0, 2, 1, 3).reshape(rows, H)
    Kk = two(ka, kb_).reshape(B, nh, Sp, 64).transpose(0, 2, 1, 3).reshape(rows, H)
    V = two(va, vb).reshape(B, nh, 64, Sp).transpose(0, 3, 1, 2).reshape(rows, H)
    flags = o.get("q_tile_flag")
    worst_all = 0.0
    for name, got, c0 in (("Q", Q, 0), ("K", Kk, H), ("V", V, 2 * H)):
        live = np.zeros(rows, bool); live[:Mvalid] = True
        if name == "Q" and o.get("qkv_skip_q"):
            live[:] = False
        if name == "Q" and flags is not None:                  # a 256-row tile of the Q third without a flagged 32-row tile is skipped
            for t in range(Mpad // 256):
                if not flags[8 * t: 8 * t + 8].any():
                    live[256 * t: 256 * t + 256] = False
        raw = res["out"]["QKV".index(name)]
        unit_rows = _row_bytes_untouched(raw, name, B, nh, Sp, split, dt)
        assert unit_rows[~live[:rows]].all(), f"{name}: a row that must stay untouched was written"
        assert not unit_rows[live[:rows]].any(), f"{name}: a live row still holds the fill pattern"
        ok, worst, idx = R.check(got[live], ref[:rows][live][:, c0:c0 + H], bnd[:rows][live][:, c0:c0 + H])
        worst_all = max(worst_all, worst)
        assert ok, (name, worst, idx)
        if exact and live.any():
            v32 = ref[:rows][:, c0:c0 + H].astype(np.float32)
            want = (np.stack(R.split_f16(v32), 0).astype(np.float64).sum(0) if split else R.round_T(v32, dt).astype(np.float64))
            assert np.array_equal(got[live], want[live]), f"{name}: not bit-exact"
    key = (("128", "256s", "gs", "mx", "auto")[kernel] + ":" + dt, "qkv" + ("+" + label if label else ""))
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst_all)
    print(f"[gemm] {key[0]:10s} {key[1]:28s} Mpad={Mpad} Mvalid={Mvalid} Sp={Sp} H={H} K={K} worst error / bound = {worst_all:.4f}" + (" (bit-exact)" if exact else ""))
    return res


def _row_bytes_untouched(raw, name, B, nh, Sp, split, dt):
    """per sequence row: True when every byte that row owns in this fragment-major buffer still holds the fill pattern"""
    per = 4 if split or dt == "f32" else 2
    u = (raw.reshape(-1, 8 * per) == FILL).all(1).astype(np.float32).reshape(-1, 1).repeat(8, 1)     # one flag per unit, as 8 pseudo elements
    if name == "V":
        m = R.vt_from_units(u, B * nh, Sp).reshape(B, nh, 64, Sp).transpose(0, 3, 1, 2).reshape(B * Sp, -1)
    else:
        m = R.q_from_units(u, B * nh, Sp, name == "K").reshape(B, nh, Sp, 64).transpose(0, 2, 1, 3).reshape(B * Sp, -1)
    assert ((m.min(1) == m.max(1))).all() or name == "V", "a row is partly written"
    return m.min(1) == 1.0


@pytest.mark.parametrize("dt", ("f32", "f16", "bf16"))
def test_128_tile_qkv(weights_for, dt):
    kb = 32 if dt == "f32" else 64
    for (Mpad, Mvalid, Sp, H, nk, exact, o) in ((128, 128, 64, 128, 1, True, {}), (384, 384, 192, 384, 3, True, {}), (256, 256, 256, 128, 5, False, {}),
                                                (256, 200, 64, 128, 2, True, {}), (256, 256, 64, 384, 2, True, dict(qkv_skip_q=1))):
        qkv_case(weights_for, dt, R.K128, Mpad, Mvalid, Sp, H, nk * kb, exact, **o)
        if dt == "f32":
            qkv_case(weights_for, dt, R.K128, Mpad, Mvalid, Sp, H, nk * kb, exact, label="split", qkv_split=1, **o)


# ------------------------------------------------------------------------------------------------ 256-tile, 16-bit
@pytest.mark.parametrize("dt", ("f16", "bf16"))
@pytest.mark.parametrize("epi", (R.EPI_BIAS, R.EPI_GELU, R.EPI_RESID, R.EPI_SWIGLU, R.EPI_GEGLU))
def test_256s_16bit(weights_for, dt, epi):
    from gliclass.c_amd import _lib
    shapes = [(256, 256, 32, True), (256, 256, 96, True), (512, 512, 64, True), (256, 512, 160, False), (256, 256, 768, False)]
    for (M, N, K, exact) in shapes:
        exact = exact and epi in (R.EPI_BIAS, R.EPI_RESID)
        A = ints((M, K), 60) if exact else rnd((M, K), 1.0, 61)
        W = ints((N, K), 62) if exact else rnd((N, K), 0.05 if epi < R.EPI_SWIGLU else 0.2, 63)
        o = epi_args(epi, M, N, 70, exact)
        outs = []
        for fl in (1, 0):                                       # the two ring loops: bit-identical
            _lib.hip().glc_debug_set_gemm_full_lines(fl)
            try:
                res, _, _ = case(weights_for, dt, R.K256S, epi, A, W, exact=exact, label="" if fl else "half-lines", **o)
            finally:
                _lib.hip().glc_debug_set_gemm_full_lines(1)
            outs.append(res["out"][0].copy())
        assert np.array_equal(outs[0], outs[1]), "full-line and half-line loops differ"
    if epi == R.EPI_RESID:      # raw rows in T + partials
        A, W = rnd((256, 64), 1.0, 64), rnd((256, 64), 0.05, 65)
        case(weights_for, dt, R.K256S, epi, A, W, label="ln_part", want_ln_part=1, **epi_args(epi, 256, 256, 71, False, rln=True))


@pytest.mark.parametrize("dt", ("f16", "bf16"))
def test_256s_16bit_qkv(weights_for, dt):
    for (Mpad, Mvalid, Sp, H, K, exact, o) in ((256, 256, 64, 256, 32, True, {}), (768, 768, 192, 256, 96, True, {}), (256, 256, 256, 768, 64, False, {}),
                                               (512, 328, 64, 256, 64, True, {}), (256, 256, 64, 256, 64, True, dict(qkv_skip_q=1))):
        qkv_case(weights_for, dt, R.K256S, Mpad, Mvalid, Sp, H, K, exact, **o)
    for nflag, flags in (("none", np.zeros(16, np.uint8)), ("one", np.eye(1, 16, 9, dtype=np.uint8)[0]), ("all", np.ones(16, np.uint8))):
        qkv_case(weights_for, dt, R.K256S, 512, 512, 256, 256, 64, True, label="flags-" + nflag, q_tile_flag=flags)


# ------------------------------------------------------------------------------------------------ 256-tile on GS rows and the MX kernel
GS_MX_SHAPES = [(256, 256, 32, True), (256, 256, 96, True), (512, 256, 64, True), (256, 512, 160, False), (256, 768, 3072 - 32, False), (256, 768, 3072, False)]


_COMMON = ("bias-plain", "bias-rows", "gelu", "gelu-fold", "resid-plain", "resid-raw-ln", "swiglu", "swiglu-fold")
_VARIANTS = [(R.KGS, v) for v in _COMMON + ("geglu", "prec", "resid-plain-in")] + [(R.KMX, v) for v in _COMMON]


@pytest.mark.parametrize("kernel,variant", _VARIANTS, ids=[("gs-" if k == R.KGS else "mx-") + v for k, v in _VARIANTS])
def test_gs_and_mx_epilogues(weights_for, kernel, variant):
    from gliclass.c_amd import _lib
    epi = {"bias": R.EPI_BIAS, "gelu": R.EPI_GELU, "resid": R.EPI_RESID, "swiglu": R.EPI_SWIGLU, "geglu": R.EPI_GEGLU, "prec": R.EPI_RESID}[variant.split("-")[0]]
    for (M, N, K, exact) in GS_MX_SHAPES:
        exact = exact and epi in (R.EPI_BIAS, R.EPI_RESID) and variant != "resid-raw-ln"
        if K > 2000 and variant not in ("bias-rows", "resid-plain", "gelu-fold", "swiglu"):
            continue
        A = ints((M, K), 80, lo_part=True) if exact else rnd((M, K), 1.0, 81)
        W = ints((N, K), 82, lo_part=True) if exact else rnd((N, K), 0.05 if epi not in (R.EPI_SWIGLU, R.EPI_GEGLU) else 0.2, 83)
        o = epi_args(epi, M, N, 90, exact, fold=variant.endswith("fold"), rln=variant == "resid-raw-ln")
        if variant == "swiglu-fold":
            o["ln_c"] = None
        if epi in (R.EPI_SWIGLU, R.EPI_GEGLU):
            o.pop("bias", None)
        if variant == "bias-plain":
            o["gs_c_plain"] = 1
        if variant == "resid-raw-ln":
            o["want_ln_part"] = 1
        if variant == "resid-plain-in":
            o["gs_resid_plain"] = 1
        precs = (1, 2, 4, 7) if variant == "prec" else (0,)
        if kernel == R.KMX:
            o["mx_ws"] = R.gx_weight_exponent(float(np.abs(W).max()))
            if K == 160:
                o["w_from_gs"] = 1
        for prec in precs:
            outs = []
            for fl in ((1, 0) if kernel == R.KGS and not prec else (1,)):
                _lib.hip().glc_debug_set_gemm_full_lines(fl)
                try:
                    res, _, _ = case(weights_for, "f16", kernel, epi, A, W, exact=exact, label=variant + ("" if fl else "/half-lines") + (f"/prec{prec}" if prec else ""), prec=prec, **o)
                finally:
                    _lib.hip().glc_debug_set_gemm_full_lines(1)
                outs.append(res["out"][0].copy())
            assert all(np.array_equal(outs[0], x) for x in outs), "full-line and half-line loops differ"


TILE_ORDER_SHAPES = ((2048, 2048, 32), (2048, 2304, 32), (2048, 2560, 32))
# the launchers' rule (gemm256s.hip launch_e, gemm256x.hip launch_x), a function of the shape alone: N-tiles >= 8 and M-tiles % 8 == 0, then 4 | 3 | 0
assert [(n // 256 >= 8 and (m // 256) % 8 == 0) * (4 if n // 256 % 4 == 0 else 3 if n // 256 % 3 == 0 else 0) for m, n, _ in TILE_ORDER_SHAPES] == [4, 3, 0]
# ... and the MX kernel's wave-tile switch at N K >= 768 * 3072: the last two GS_MX_SHAPES sit just below and at it
assert GS_MX_SHAPES[-2][1] * GS_MX_SHAPES[-2][2] < 768 * 3072 <= GS_MX_SHAPES[-1][1] * GS_MX_SHAPES[-1][2]


@pytest.mark.parametrize("dt", ("f16", "bf16"))
def test_256s_16bit_tile_orders(weights_for, dt):
    """the same three tile orders on the 16-bit kernel (it shares launch_e with the GS kernel)"""
    for (M, N, K) in TILE_ORDER_SHAPES:
        case(weights_for, dt, R.K256S, R.EPI_BIAS, ints((M, K), 100), ints((N, K), 101), exact=True, label="tile-order", bias=ints(N, 102) * 3)


@pytest.mark.parametrize("kernel,dt", ((R.K256S, "f16"), (R.K256S, "bf16"), (R.KGS, "f16"), (R.KMX, "f16")))
def test_exact_residual_with_ln_part(weights_for, kernel, dt):
    """EPI_RESID writing raw rows + ln_part on sparse integer operands: rows AND both words of every partial bit for bit."""
    M, N, K = 256, 256, 32
    A, W = ints((M, K), 110, density=0.12), ints((N, K), 111, density=0.12)
    o = dict(mx_ws=7) if kernel == R.KMX else {}
    case(weights_for, dt, kernel, R.EPI_RESID, A, W, exact=True, label="ln_part-exact", bias=ints(N, 112), resid=ints((M, N), 113), want_ln_part=1, **o)


@pytest.mark.parametrize("kernel", (R.KGS, R.KMX))
def test_gs_and_mx_tile_orders_and_widest_n(weights_for, kernel):
    """n_group 4 (8 N-tiles), 3 (9) and 0 (10) at 8 M-tiles, and N = 73728 with the shortest K: exact operands, GS / GX row outputs."""
    for (M, N, K) in TILE_ORDER_SHAPES + ((256, 73728, 32),):
        A, W = ints((M, K), 100, lo_part=True), ints((N, K), 101, lo_part=True)
        o = dict(mx_ws=R.gx_weight_exponent(float(np.abs(W).max()))) if kernel == R.KMX else {}
        case(weights_for, "f16", kernel, R.EPI_BIAS, A, W, exact=True, label="tile-order", bias=ints(N, 102) * 3, **o)


@pytest.mark.parametrize("kernel", (R.KGS, R.KMX))
def test_gs_and_mx_qkv(weights_for, kernel):
    ws = dict(mx_ws=7) if kernel == R.KMX else {}
    for (Mpad, Mvalid, Sp, H, K, exact, o) in ((256, 256, 64, 256, 32, True, {}), (768, 768, 192, 256, 96, True, {}), (256, 256, 256, 768, 64, False, {}),
                                               (512, 328, 64, 256, 64, True, {}), (256, 256, 64, 256, 64, True, dict(qkv_skip_q=1))):
        if not exact:
            o = dict(o, a_stats=np.stack([rnd(Mpad, 0.1, 3), 0.5 + np.abs(rnd(Mpad, 0.4, 4))], 1), ln_c=rnd(3 * H, 0.05, 5))
            ws = dict(mx_ws=R.gx_weight_exponent(0.05)) if kernel == R.KMX else {}
        qkv_case(weights_for, "f16", kernel, Mpad, Mvalid, Sp, H, K, exact, label="split-units", qkv_split=1, **ws, **o)
    for nflag, flags in (("none", np.zeros(16, np.uint8)), ("one", np.eye(1, 16, 9, dtype=np.uint8)[0]), ("all", np.ones(16, np.uint8))):
        qkv_case(weights_for, "f16", kernel, 512, 512, 256, 256, 64, True, label="flags-" + nflag, qkv_split=1, q_tile_flag=flags, **(dict(mx_ws=7) if kernel == R.KMX else {}))


def test_mx_lowered_activation_exponent_and_weight_exponent_ends(weights_for):
    """act_sc = -5 (rows that hold |x| up to 14336) and mx_ws at both ends of what glc_gx_weight_exponent returns: 40 (tiny weights) and -30.
    -30 answers weights of 2.6e11 and more, which have no f16 hi half; the launcher takes the exponent all the same (glc_kernels.h), so it is
    launched on the largest weights the format holds (their own exponent: -9 / -8): all their fp8 parts are then zero, in the emulation too."""
    M, N, K = 256, 256, 96
    case(weights_for, "f16", R.KMX, R.EPI_RESID, rnd((M, K), 600.0, 1), rnd((N, K), 0.05, 2), label="act_sc-5", act_sc=-5, mx_ws=R.gx_weight_exponent(0.05), want_ln_part=1,
         **epi_args(R.EPI_RESID, M, N, 3, False))
    case(weights_for, "f16", R.KMX, R.EPI_BIAS, rnd((M, K), 1.0, 1), rnd((N, K), 2.0 ** -45, 2), label="mx_ws40", mx_ws=40, gs_c_plain=1, bias=rnd(N, 1e-12, 5))
    assert R.gx_weight_exponent(2.0 ** -45) == 40
    Wbig = rnd((N, K), 60000.0, 4)
    ws = R.gx_weight_exponent(float(np.abs(Wbig).max()))
    case(weights_for, "f16", R.KMX, R.EPI_BIAS, rnd((M, K), 2.0 ** -6, 1), Wbig, label=f"mx_ws{ws}", mx_ws=ws, gs_c_plain=1, bias=rnd(N, 0.1, 5))
    assert R.gx_weight_exponent(65504.0) == -9 and R.gx_weight_exponent(240.0 * 2.0 ** 30) == -30
    case(weights_for, "f16", R.KMX, R.EPI_BIAS, rnd((M, K), 2.0 ** -6, 1), Wbig, label="mx_ws-30", mx_ws=-30, gs_c_plain=1, bias=rnd(N, 0.1, 5))


def test_mx_perm_cols(weights_for):
    """EPI_BIAS, plain fp32 out: columns [0, perm_cols) are computed in the glc_rope_perm128 order and must land at their logical place."""
    M, N, K = 256, 512, 64
    for exact in (True, False):
        A = ints((M, K), 120, lo_part=True) if exact else rnd((M, K), 1.0, 121)
        W = ints((N, K), 122, lo_part=True) if exact else rnd((N, K), 0.05, 123)
        case(weights_for, "f16", R.KMX, R.EPI_BIAS, A, W, exact=exact, label="perm_cols", gs_c_plain=1, perm_cols=256, mx_ws=R.gx_weight_exponent(float(np.abs(W).max())),
             bias=ints(N, 124) * 3 if exact else rnd(N, 0.1, 124))


def _mx_tile_check(name, parts, ref32, bnd, live, exact, label):
    """decoded MX-tile parts (hi, lo8, hi8) [rows, cols] against the fp32 reference values"""
    hi, lo8, hi8 = parts
    got = hi.astype(np.float64) + lo8 * 2.0 ** -R.GX_SHIFT
    ok, worst, idx = R.check(got[live], ref32[live], bnd[live] + R.out_quant(np.abs(ref32[live]) + bnd[live], "gx"))
    assert ok, (label, name, worst, idx)
    # the hi8 part is e4m3 of the same fp32 value: within 2^-4 of it (+ the subnormal floor), whatever rounding the accumulation took
    assert (np.abs(hi8[live] - ref32[live]) <= (np.abs(ref32[live]) + bnd[live]) * 2.0 ** -4 + bnd[live] + 2.0 ** -10).all(), (label, name, "hi8")
    if exact:
        wh, wl8, wh8 = R.gx_parts(ref32.astype(np.float32), 0, saturate=False)
        assert np.array_equal(hi[live], wh[live]) and np.array_equal(lo8[live], R.e4m3_decode(wl8)[live]) and np.array_equal(hi8[live], R.e4m3_decode(wh8)[live]), (label, name, "not bit-exact")
    fill_h, fill_8 = np.frombuffer(bytes([FILL, FILL]), np.float16)[0], R.e4m3_decode(np.uint8(FILL))
    assert (hi[~live] == fill_h).all() and (lo8[~live] == fill_8).all() and (hi8[~live] == fill_8).all(), (label, name, "a row that must stay untouched was written")
    return worst


def test_mx_qkv_mx_tiles_and_second_counter_word(weights_for):
    """EPI_QKV writing MX tiles (qkv_mxt): Q as (hi8 | lo8), K as (lo8 | hi8) at slot pi(r), V^T sub-tiles; the range guard's SECOND word
    counts their out-of-range elements over rows [0, gx_rows) (one Q column pushed to 1000: one element and one store unit per row)."""
    eng = _engine(weights_for, "f16")
    for (Mpad, Mvalid, Sp, H, K, exact, hot) in ((512, 328, 64, 256, 64, True, False), (256, 256, 256, 768, 96, False, False), (512, 512, 192 + 64, 256, 64, True, True)):
        N, nh = 3 * H, H // 64
        A = ints((Mpad, K), 130, lo_part=True) if exact else rnd((Mpad, K), 1.0, 131)
        W = ints((N, K), 132, lo_part=True) if exact else rnd((N, K), 0.05, 133)
        bias = ints(N, 134) * 2 if exact else rnd(N, 0.1, 134)
        if hot:
            bias[77] = 1000.0
        ws = R.gx_weight_exponent(float(np.abs(W).max()))
        acc, mag, steps = R.accumulate(R.operands("mx", A, W, "f16", 0, ws))
        ref = R.epilogue(acc, R.EPI_BIAS, bias=bias)
        bnd = R.bound(mag, steps) + EPI_OPS * R.U24 * (np.abs(acc) + np.abs(bias)[None, :])
        if exact:
            assert float(mag.max()) * 2.0 ** 12 < 2.0 ** 24 and np.array_equal(ref, ref.astype(np.float32).astype(np.float64))
        gx_rows = 400 if hot else 0
        res = run(eng, R.KMX, R.EPI_QKV, A, W, bias=bias, Mvalid=Mvalid, Sp=Sp, nh=nh, H=H, qkv_mxt=1, mx_ws=ws, gx_rows=gx_rows)
        assert res["rc"] == 0 and res["guards_ok"] == 1, res["err"]
        B = -(-Mvalid // Sp)
        rows = B * Sp
        live = np.zeros(rows, bool); live[:Mvalid] = True
        rr = np.zeros((rows, N)); rr[:min(rows, Mpad)] = ref[:rows]
        bb = np.zeros((rows, N)); bb[:min(rows, Mpad)] = bnd[:rows]
        heads = lambda p: tuple(x.reshape(B, nh, Sp, 64).transpose(0, 2, 1, 3).reshape(rows, H) for x in p)
        q = heads(R.mxt_qk_decode(res["out"][0].tobytes(), B * nh, Sp, True, False))
        k = heads(R.mxt_qk_decode(res["out"][1].tobytes(), B * nh, Sp, False, True))
        v = tuple(x.reshape(B, nh, 64, Sp).transpose(0, 3, 1, 2).reshape(rows, H) for x in R.mxt_vt_decode(res["out"][2].tobytes(), B * nh, Sp))
        worst = 0.0
        for name, parts, c0 in (("Q", q, 0), ("K", k, H), ("V", v, 2 * H)):
            if hot and name == "Q":      # the pushed column has no e4m3 image: compare the f16 halves of that column, everything of the others
                keep = np.ones(H, bool); keep[77] = False
                assert np.array_equal(parts[0][live][:, 77], R.round_f16(rr[live][:, 77].astype(np.float32)))
                parts, r_, b_ = tuple(x[:, keep] for x in parts), rr[:, c0:c0 + H][:, keep], bb[:, c0:c0 + H][:, keep]
            else:
                r_, b_ = rr[:, c0:c0 + H], bb[:, c0:c0 + H]
            worst = max(worst, _mx_tile_check(name, parts, r_.astype(np.float32).astype(np.float64) if exact else r_, b_, live, exact, "qkv_mxt"))
        want = int((np.abs(ref[:(gx_rows or Mvalid)]) > 448).sum())
        assert want == (400 if hot else 0) and res["sat"] == (0, want), (res["sat"], want)
        RATIOS[("mx:f16", "qkv+mx-tiles")] = max(RATIOS.get(("mx:f16", "qkv+mx-tiles"), 0.0), worst)
        print(f"[gemm] mx:f16     qkv+mx-tiles                 Mpad={Mpad} Mvalid={Mvalid} Sp={Sp} H={H} K={K} worst error / bound = {worst:.4f}" + (" (bit-exact)" if exact else ""))


def test_mx_qkvr_rope_epilogue(weights_for):
    """EPI_QKVR (decoder QKV): W rows and bias of every Q / K head in the glc_rope_perm128 order, rotate-half RoPE from a cos / sin table,
    qscale on Q, outputs as head_dim-128 MX tiles.  Exact case: cos / sin in {0, 1, -1} by position and feature, qscale 0.5; random case:
    angles pos * 10000^(-i / 64), qscale log2(e) / sqrt(128); Sp a multiple of 32 but not of 64."""
    eng = _engine(weights_for, "f16")
    for (Mpad, Sp, nq, nkv, K, exact) in ((256, 96, 4, 2, 64, True), (256, 32, 2, 2, 96, False), (512, 96, 2, 4, 160, False)):
        B = Mpad // Sp
        Mvalid, N, nqk = B * Sp, (nq + 2 * nkv) * 128, nq + nkv
        A = ints((Mpad, K), 140, lo_part=True) if exact else rnd((Mpad, K), 1.0, 141)
        Wl = ints((N, K), 142, lo_part=True) if exact else rnd((N, K), 0.05, 143)
        bl = ints(N, 144) * 2 if exact else rnd(N, 0.1, 144)
        phys = np.arange(N)
        phys[:nqk * 128] = (phys[:nqk * 128] & ~127) | R.rope_perm128(phys[:nqk * 128] & 127)        # physical row p of a Q / K head holds logical feature perm(p)
        pos, i = np.arange(Sp)[:, None], np.arange(64)[None, :]
        if exact:
            quad = (pos + 3 * i) % 4
            cos, sin, qscale = np.choose(quad, [1.0, 0.0, -1.0, 0.0]), np.choose(quad, [0.0, 1.0, 0.0, -1.0]), 0.5
        else:
            ang = pos * 10000.0 ** (-i / 64.0)
            cos, sin, qscale = np.cos(ang), np.sin(ang), float(np.float32(1.4426950408889634 / math.sqrt(128.0)))
        cs = np.stack([cos, sin], axis=2).astype(np.float32)
        cos, sin = cs[:, :, 0].astype(np.float64), cs[:, :, 1].astype(np.float64)
        ws = R.gx_weight_exponent(float(np.abs(Wl).max()))
        acc, mag, steps = R.accumulate(R.operands("mx", A, Wl, "f16", 0, ws))
        x = acc + bl[None, :]
        bx = R.bound(mag, steps) + EPI_OPS * R.U24 * (np.abs(acc) + np.abs(bl)[None, :])
        ref, bnd = x.copy(), bx.copy()
        p = np.arange(Mpad) % Sp
        for h in range(nqk):
            sc = qscale if h < nq else 1.0
            x1, x2, b1, b2 = x[:, 128 * h:128 * h + 64], x[:, 128 * h + 64:128 * h + 128], bx[:, 128 * h:128 * h + 64], bx[:, 128 * h + 64:128 * h + 128]
            co, sn = cos[p], sin[p]
            ref[:, 128 * h:128 * h + 128] = R.rope_rotate_half(x[:, 128 * h:128 * h + 128], co, sn) * sc
            t1, t2 = np.abs(x1 * co) + np.abs(x2 * sn), np.abs(x2 * co) + np.abs(x1 * sn)
            bnd[:, 128 * h:128 * h + 64] = (b1 * np.abs(co) + b2 * np.abs(sn) + EPI_OPS * R.U24 * t1) * abs(sc)
            bnd[:, 128 * h + 64:128 * h + 128] = (b2 * np.abs(co) + b1 * np.abs(sn) + EPI_OPS * R.U24 * t2) * abs(sc)
        if exact:
            assert float(mag.max()) * 2.0 ** 12 < 2.0 ** 24 and np.array_equal(ref, ref.astype(np.float32).astype(np.float64))
        res = run(eng, R.KMX, R.EPI_QKVR, A, Wl[phys], bias=bl[phys], rope_cs=cs, qscale=qscale, Mvalid=Mvalid, Sp=Sp, nq=nq, nkv=nkv, mx_ws=ws)
        assert res["rc"] == 0, res["err"]
        assert res["guards_ok"] == 1, "rows beyond Mvalid were written"
        assert res["sat"] == (0, 0)
        live = np.ones(Mvalid, bool)
        hq = lambda parts, n: tuple(v.reshape(B, n, Sp, 128).transpose(0, 2, 1, 3).reshape(Mvalid, n * 128) for v in parts)
        q = hq(R.mxt_qk_decode(res["out"][0].tobytes(), B * nq, Sp, True, False, 128), nq)
        k = hq(R.mxt_qk_decode(res["out"][1].tobytes(), B * nkv, Sp, False, True, 128), nkv)
        v = tuple(t.reshape(B, nkv, 128, Sp).transpose(0, 3, 1, 2).reshape(Mvalid, nkv * 128) for t in R.mxt_vt_decode(res["out"][2].tobytes(), B * nkv, Sp, 128))
        worst = 0.0
        for name, parts, c0, c1 in (("Q", q, 0, nq * 128), ("K", k, nq * 128, nqk * 128), ("V", v, nqk * 128, N)):
            r_ = ref[:Mvalid, c0:c1]
            worst = max(worst, _mx_tile_check(name, parts, r_.astype(np.float32).astype(np.float64) if exact else r_, bnd[:Mvalid, c0:c1], live, exact, "qkvr"))
        RATIOS[("mx:f16", "qkvr")] = max(RATIOS.get(("mx:f16", "qkvr"), 0.0), worst)
        print(f"[gemm] mx:f16     qkvr                         Mpad={Mpad} Mvalid={Mvalid} Sp={Sp} nq={nq} nkv={nkv} K={K} worst error / bound = {worst:.4f}" + (" (bit-exact)" if exact else ""))


def test_mx_range_counter(weights_for):
    """The first counter word = the elements of the GX output with |x| 2^sc > 448 in rows [0, gx_rows) (counted per 8-column store unit: the
    overflowing elements here sit in distinct units, so units and elements agree); rows from gx_rows on do not count."""
    eng = _engine(weights_for, "f16")
    M, N, K = 256, 256, 32
    A, W = ints((M, K), 1), ints((N, K), 2)
    acc = A.astype(np.float64) @ W.astype(np.float64).T
    for (gx_rows, rows_hit) in ((200, (3, 77, 199)), (200, (200, 255)), (0, (5, 255))):
        bias = np.zeros(N, np.float32)
        resid = np.zeros((M, N), np.float32)
        for i, m in enumerate(rows_hit):
            resid[m, 8 * (3 * i + 1) + i] = 1000.0                                     # far beyond 448 + |acc|
        ref = acc + resid
        limit = gx_rows if gx_rows else M
        want = int((np.abs(ref[:limit]) > 448).sum())
        units = int((np.abs(ref[:limit]).reshape(limit, N // 8, 8).max(2) > 448).sum())
        assert want == units
        res = run(eng, R.KMX, R.EPI_RESID, A, W, bias=bias, resid=resid, want_ln_part=1, gx_rows=gx_rows, mx_ws=7)
        assert res["rc"] == 0 and res["guards_ok"] == 1, res["err"]
        assert res["sat"] == (want, 0), (gx_rows, rows_hit, res["sat"], want)
        hi, _, _ = R.gx_decode(res["out"][0], M, N, 0)
        assert np.array_equal(hi, R.round_f16(ref.astype(np.float32)))
    # the counter's unit is the 8-element store: two out-of-range elements of one unit count once (the engine only asks whether it is zero)
    resid = np.zeros((M, N), np.float32)
    resid[9, 40], resid[9, 43], resid[9, 48] = 1000.0, -1000.0, 1000.0
    res = run(eng, R.KMX, R.EPI_RESID, A, W, bias=np.zeros(N, np.float32), resid=resid, want_ln_part=1, mx_ws=7)
    assert res["rc"] == 0 and int((np.abs(acc + resid) > 448).sum()) == 3 and res["sat"] == (2, 0), res["sat"]
    # exponent -5: the threshold is |x| 2^-5 > 448, i.e. 14336
    resid = np.zeros((M, N), np.float32)
    resid[4, 8], resid[5, 80], resid[6, 160] = 10000.0, 14000.0, 20000.0
    res = run(eng, R.KMX, R.EPI_RESID, A, W, bias=np.zeros(N, np.float32), resid=resid, want_ln_part=1, mx_ws=7, act_sc=-5)
    assert res["rc"] == 0 and int((np.abs(acc + resid) * 2.0 ** -5 > 448).sum()) == 1 and res["sat"] == (1, 0), res["sat"]


# ------------------------------------------------------------------------------------------------ refusals and ln_stats
REFUSED = [
    ("f16", R.K128, R.EPI_BIAS, dict(Mpad=192), "Mpad must be a positive multiple of 128"),
    ("f16", R.K128, R.EPI_BIAS, dict(N=192), "N must be a multiple of 128"),
    ("f16", R.K128, R.EPI_BIAS, dict(K=96), "K must be a multiple of 128 bytes"),
    ("f32", R.K128, R.EPI_BIAS, dict(K=48), "K must be a multiple of 128 bytes"),
    ("f16", R.K128, R.EPI_RESID, dict(), "null residual"),
    ("f16", R.K128, R.EPI_QKV, dict(N=384, H=128, nh=2, Sp=96, Mvalid=192), "bad QKV epilogue shape"),
    ("f16", R.K128, R.EPI_BIAS, dict(m_split=64, W2=True), "m_split must be a tile-aligned row"),
    ("f16", R.K128, R.EPI_BIAS, dict(want_ln_part=1), "LayerNorm-fold arguments"),
    ("f16", R.K256S, R.EPI_BIAS, dict(Mpad=384), "gemm256s: unsupported shape"),
    ("f16", R.K256S, R.EPI_BIAS, dict(N=384), "gemm256s: unsupported shape"),
    ("f16", R.K256S, R.EPI_BIAS, dict(K=48), "gemm256s: unsupported shape"),
    ("f32", R.K256S, R.EPI_BIAS, dict(), "gemm256s: unsupported shape"),
    ("f16", R.K256S, R.EPI_RESID, dict(), "gemm256s: null residual"),
    ("f16", R.K256S, R.EPI_SWIGLU, dict(bias=True), "the GLU epilogues take no bias"),
    ("f16", R.K256S, R.EPI_QKV, dict(N=768, H=256, nh=4, Sp=96, Mvalid=192), "gemm256s: bad QKV epilogue shape"),
    ("f16", R.KGS, R.EPI_BIAS, dict(Mpad=384), "gemm256s(gs): unsupported shape"),
    ("f16", R.KGS, R.EPI_BIAS, dict(K=48), "gemm256s(gs): unsupported shape"),
    ("f16", R.KGS, R.EPI_RESID, dict(), "gemm256s(gs): null residual"),
    ("f16", R.KGS, R.EPI_SWIGLU, dict(bias=True), "the SwiGLU epilogue takes no bias"),
    ("f16", R.KGS, R.EPI_GEGLU, dict(bias=True), "the GeGLU epilogue takes no bias"),
    ("f16", R.KGS, R.EPI_QKVR, dict(), "gemm256s(gs): unsupported shape"),
    ("f16", R.KMX, R.EPI_BIAS, dict(N=384), "gemm256x: unsupported shape"),
    ("f16", R.KMX, R.EPI_BIAS, dict(K=48), "gemm256x: unsupported shape"),
    ("f16", R.KMX, R.EPI_RESID, dict(), "gemm256x: null residual"),
    ("f16", R.KMX, R.EPI_SWIGLU, dict(bias=True), "the SwiGLU epilogue takes no bias"),
    ("f16", R.KMX, R.EPI_QKVR, dict(N=1024, nq=3, nkv=1, Sp=64, Mvalid=256), "gemm256x: unsupported shape"),
    ("f16", R.KMX, R.EPI_GEGLU, dict(), "gemm256x: unsupported shape"),
    ("f16", R.KMX, R.EPI_QKV, dict(N=768, H=256, nh=4, Sp=96, Mvalid=192), "gemm256x: unsupported shape"),
]


@pytest.mark.parametrize("dt,kernel,epi,o,message", REFUSED, ids=[f"{r[0]}-k{r[1]}-e{r[2]}-{'-'.join(f'{k}{v}' for k, v in r[3].items())}" for r in REFUSED])
def test_refused_shapes_return_the_launchers_message(weights_for, dt, kernel, epi, o, message):
    eng = _engine(weights_for, dt)
    o = dict(o)
    Mpad, N, K = o.pop("Mpad", 256), o.pop("N", 256), o.pop("K", 64)
    A, W = rnd((Mpad, K), 1, 1), rnd((N, K), 1, 2)
    if o.get("bias"):
        o["bias"] = rnd(N, 1, 3)
    if o.get("W2"):
        o["W2"] = W
    res = run(eng, kernel, epi, A, W, out_bytes=[1 << 22] * 3, **o)
    assert res["rc"] == -2 and message in res["err"], (res["rc"], res["err"])


@pytest.mark.parametrize("dt", ("f16", "f32"))
@pytest.mark.parametrize("epi", (R.EPI_SWIGLU, R.EPI_QKVR, R.EPI_GEGLU))
@pytest.mark.parametrize("ws", (0, 1 << 20))
def test_refused_128_tile_unknown_epilogue(weights_for, dt, epi, ws):
    """Regression: glc_launch_gemm took an epilogue it has no build of and returned success without launching anything (with a split-K
    workspace it would have run the residual build on a null residual).  It is refused now, like every other bad argument."""
    eng = _engine(weights_for, dt)
    kb = 32 if dt == "f32" else 64
    res = run(eng, R.K128, epi, rnd((128, 16 * kb), 1, 1), rnd((128, 16 * kb), 1, 2), ws_bytes=ws, out_bytes=[1 << 16] * 3)
    assert res["rc"] == -2 and "gemm: bad epilogue" in res["err"], (res["rc"], res["err"])
    assert (res["out"][0] == 0).all()                          # nothing came back: nothing was launched


@pytest.mark.parametrize("kernel", (R.KGS, R.KMX))
@pytest.mark.parametrize("rms", (0, 1))
def test_ln_stats_on_the_partials_a_gemm_wrote(weights_for, kernel, rms):
    """glc_launch_ln_stats on the ln_part a residual GEMM wrote, against float64 mean and rstd of the rows that GEMM wrote; rows with a large
    mean (no E[x^2] - mean^2 cancellation).  Bound: the partials are fp32 sums of 64 values (64 2^-24 relative), merged in double."""
    eng = _engine(weights_for, "f16")
    M, N, K, eps = 256, 768, 64, 1e-5
    A, W = rnd((M, K), 1.0, 1), rnd((N, K), 0.05, 2)
    resid = rnd((M, N), 1.0, 3) + np.linspace(-50, 50, M, dtype=np.float32)[:, None]
    o = dict(mx_ws=R.gx_weight_exponent(0.05)) if kernel == R.KMX else {}
    res, ref, got = case(weights_for, "f16", kernel, R.EPI_RESID, A, W, label="ln_stats", bias=rnd(N, 0.1, 4), resid=resid, want_ln_part=1, **o)
    stats = np.zeros((M, 2), np.float32)
    part = np.ascontiguousarray(res["ln_part"])
    assert eng.L.glc_debug_ln_stats_run(eng.h, part.ctypes.data, N // 64, M, eps, rms, stats.ctypes.data) == 0, eng.L.glc_last_error().decode()
    # the statistics describe the fp32 values the epilogue held; `got` is their GS / GX image (2^-22 / 2^-15 away)
    want = R.ln_stats(got, eps, bool(rms))
    rel = 2.0 ** -14 if kernel == R.KMX else 2.0 ** -20
    mean_b = np.abs(got).mean(1) * (rel + 256 * R.U24)
    assert (np.abs(stats[:, 0] - want[:, 0]) <= mean_b + 1e-30).all(), float(np.abs(stats[:, 0] - want[:, 0]).max())
    sd = 1.0 / want[:, 1]
    rstd_b = want[:, 1] * ((np.abs(got).max(1) * rel + 256 * R.U24 * np.abs(got).max(1)) * 2 / sd + 4 * R.U24)
    assert (np.abs(stats[:, 1] - want[:, 1]) <= rstd_b).all(), float((np.abs(stats[:, 1] - want[:, 1]) / rstd_b).max())


def test_auto_picks_a_kernel_that_computes_the_same(weights_for):
    for dt in ("f16", "f32"):
        kb = 32 if dt == "f32" else 64
        for (M, N, K) in ((256, 256, 2 * kb), (4096, 4096, 2 * kb)):       # few tiles: the 128-tile kernel; enough for every CU: the 256-tile one (16-bit)
            A, W = ints((M, K), 1, lo_part=dt == "f32"), ints((N, K), 2, lo_part=dt == "f32")
            case(weights_for, dt, R.KAUTO, R.EPI_BIAS, A, W, exact=True, bias=ints(N, 3))


def test_zz_print_ratio_table():
    print("\n| kernel | epilogue | worst error / bound |\n|---|---|---|")
    for (k, e), v in sorted(RATIOS.items()):
        print(f"| {k} | {e} | {v:.4f} |")

"""numpy references for the GEMM kernels (no GPU): the operand / output formats read a second time, two float64 references per
case, and the checker of tests/test_gpu_gemm_kernels.py.

The codecs follow the format COMMENTS of gliclass/c_amd/csrc/glc_common.h ("GS" / "GX" rows, split-f16 units, e4m3 parts) and
glc_layout.h (fragment-major Q / K / V^T, MX tiles); none of them is a port of a kernel or of the offset helpers — the layouts are
written as reshapes of the index tuples the comments give ([bh][qt][s][lane = 32 h + r][8] holds Q[32 qt + r][16 s + 8 h + j], ...).

References (float64 accumulation):
  exact     the mathematical epilogue of A W^T on the fp32 operands
  emulated  the same with the rounding points the format documents: 16-bit operands rounded to T; GS a_hi w_hi + a_hi w_lo + a_lo w_hi;
            MX a_hi w_hi + (a_lo8 w_hi8 + a_hi8 w_lo8) 2^-(SHIFT + sc_a + sc_w)

Error model of the checker (bound(); derivation in test_gpu_gemm_kernels.py's docstring): a kernel sums `steps` exactly formed products in
fp32 in an order of its own, so |kernel - emulated| <= C_ACC 2^-24 steps (|A| |W|^T)[m, n] before the epilogue."""
import math

import numpy as np

GX_SHIFT = 11
EPI_BIAS, EPI_GELU, EPI_RESID, EPI_QKV, EPI_SWIGLU, EPI_QKVR, EPI_GEGLU = range(7)
K128, K256S, KGS, KMX, KAUTO = range(5)
U24 = 2.0 ** -24
C_ACC = 2.0            # one fp32 ulp (not half) per accumulation step: the MFMA adder's internal alignment may truncate


# ---------------------------------------------------------------- scalar formats
def round_f16(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def bf16_bits(x):
    """fp32 -> bf16 bit patterns, round to nearest even."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_from_bits(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def round_bf16(x):
    return bf16_from_bits(bf16_bits(x))


def round_T(x, dt):
    x = np.asarray(x, np.float32)
    return x if dt == "f32" else round_f16(x) if dt == "f16" else round_bf16(x)


def encode_T(x, dt):
    """fp32 values -> the raw array a buffer of T holds."""
    x = np.ascontiguousarray(x, np.float32)
    return x if dt == "f32" else x.astype(np.float16).view(np.uint16) if dt == "f16" else bf16_bits(x)


def decode_T(raw, dt):
    raw = np.asarray(raw)
    return raw.view(np.float32) if dt == "f32" else raw.view(np.float16).astype(np.float32) if dt == "f16" else bf16_from_bits(raw.view(np.uint16))


def raw_T(buf, dt):
    """bytes -> array of T's storage words."""
    return np.frombuffer(buf, np.float32 if dt == "f32" else np.uint16)


def _e4m3_table():
    t = np.zeros(256, np.float64)
    for b in range(256):
        s, e, m = b >> 7, (b >> 3) & 15, b & 7
        v = math.ldexp(m, -9) if e == 0 else math.ldexp(8 + m, e - 10)      # bias 7, 3 mantissa bits; subnormals m 2^-9
        if e == 15 and m == 7:
            v = float("nan")                                                # the only NaN pattern; no infinities, 448 = 0x7e is the largest
        t[b] = -v if s else v
    return t


E4M3 = _e4m3_table()
_E4M3_POS = E4M3[:127]          # 0 .. 448, ascending, code = index


def e4m3_decode(b):
    return E4M3[np.asarray(b, np.uint8)]


def e4m3_encode(x, saturate=True):
    """Nearest e4m3 code, ties to the even code.  saturate: |x| > 448 -> 448 (weights, tables); else (activations, unclamped conversion)
    448 up to 464 and the NaN code beyond."""
    x = np.asarray(x, np.float64)
    a = np.abs(x)
    ac = np.minimum(a, 448.0)
    hi = np.clip(np.searchsorted(_E4M3_POS, ac, side="left"), 0, 126)
    lo = np.maximum(hi - 1, 0)
    dlo, dhi = ac - _E4M3_POS[lo], _E4M3_POS[hi] - ac
    code = np.where((dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0)), hi, lo).astype(np.uint8)
    if not saturate:
        code = np.where(a > 464.0, 0x7F, code).astype(np.uint8)
    code = np.where(np.isnan(x), 0x7F, code).astype(np.uint8)
    return (code | (np.signbit(x).astype(np.uint8) << 7)).astype(np.uint8)


# ---------------------------------------------------------------- row formats
def split_f16(x):
    """x = hi + lo, hi = f16(x), lo = f16(x - hi) (fp32 subtraction: exact)."""
    x = np.asarray(x, np.float32)
    hi = round_f16(x)
    return hi, round_f16(x - hi)


def gs_encode(x):
    """[M, K] fp32 -> uint16 [M, 2 K]: per 32 elements [32 hi halves | 32 lo halves]."""
    M, K = x.shape
    hi, lo = split_f16(x)
    g = np.stack([hi.reshape(M, K // 32, 32), lo.reshape(M, K // 32, 32)], axis=2)      # [M, group, (hi | lo), 32]
    return g.astype(np.float16).view(np.uint16).reshape(M, 2 * K)


def gs_decode(raw, M, K):
    g = np.asarray(raw).view(np.float16).reshape(M, K // 32, 2, 32).astype(np.float32)
    return g[:, :, 0].reshape(M, K), g[:, :, 1].reshape(M, K)


def gx_parts(x, sc, saturate):
    """hi (f16 value), lo8 and hi8 codes of GX elements with fp8 exponent sc."""
    x = np.asarray(x, np.float32)
    hi = round_f16(x)
    lo = (x - hi).astype(np.float64)
    return hi, e4m3_encode(lo * 2.0 ** (GX_SHIFT + sc), saturate), e4m3_encode(x.astype(np.float64) * 2.0 ** sc, saturate)


def gx_encode(x, sc, worder):
    """[M, K] fp32 -> uint8 [M, 4 K]: per 32 elements [32 f16 hi | 4 x 16 bytes], the 16 bytes of elements 8 j .. 8 j + 7 as
    [lo8 x 8 | hi8 x 8] (activations) or [hi8 x 8 | lo8 x 8] (weights: worder, saturating)."""
    M, K = x.shape
    hi, lo8, hi8 = gx_parts(x, sc, saturate=bool(worder))
    out = np.zeros((M, K // 32, 128), np.uint8)
    out[:, :, :64] = hi.astype(np.float16).view(np.uint16).reshape(M, K // 32, 32).view(np.uint8).reshape(M, K // 32, 64)
    l8, h8 = lo8.reshape(M, K // 32, 4, 8), hi8.reshape(M, K // 32, 4, 8)
    pair = np.concatenate([h8, l8] if worder else [l8, h8], axis=3)                       # [M, group, j, 16]
    out[:, :, 64:] = pair.reshape(M, K // 32, 64)
    return out.reshape(M, 4 * K)


def gx_decode(raw, M, K, worder):
    """-> hi (fp32), lo8, hi8 (decoded e4m3 values, float64), each [M, K]."""
    g = np.asarray(raw).view(np.uint8).reshape(M, K // 32, 128)
    hi = np.ascontiguousarray(g[:, :, :64]).view(np.float16).astype(np.float32).reshape(M, K)
    pair = g[:, :, 64:].reshape(M, K // 32, 4, 2, 8)
    first, second = e4m3_decode(pair[:, :, :, 0]).reshape(M, K), e4m3_decode(pair[:, :, :, 1]).reshape(M, K)
    return (hi, second, first) if worder else (hi, first, second)


def gx_value(hi, lo8, sc):
    """what a reader of a GX row gets back: hi + lo8 2^-(SHIFT + sc), formed in fp32."""
    return (hi.astype(np.float32) + (lo8 * 2.0 ** -(GX_SHIFT + sc)).astype(np.float32)).astype(np.float32)


def gx_weight_exponent(maxabs):
    """2^sc maxabs <= 240."""
    if not maxabs > 0:
        return 0
    return int(min(40, max(-30, math.floor(math.log2(240.0 / maxabs)))))


# ---------------------------------------------------------------- fragment-major attention operands
def pi32(r):
    """slot permutation of the K layouts: bits 2 and 3 trade places."""
    r = np.asarray(r)
    return (r & 0x13) | ((r & 4) << 1) | ((r & 8) >> 1)


def _units(raw, n_units, split):
    """storage words -> (value [n_units, 8] fp32 of the first part, second part or None); split: a unit is [8 hi | 8 lo] halves."""
    if split:
        u = np.asarray(raw).view(np.float16).reshape(n_units, 16).astype(np.float32)
        return u[:, :8], u[:, 8:]
    return np.asarray(raw).reshape(n_units, 8), None


def q_from_units(u, BH, Sp, klayout=False):
    """[bh][qt][s][lane = 32 h + r][8] holds Q[32 qt + r][16 s + 8 h + j] (K: row 32 kt + pi(r)) -> [BH, Sp, 64]."""
    nt = Sp // 32
    a = u.reshape(BH, nt, 4, 2, 32, 8)
    if klayout:
        a = a[:, :, :, :, pi32(np.arange(32)), :]          # row r' sits in slot pi(r') (pi is its own inverse)
    return a.transpose(0, 1, 4, 2, 3, 5).reshape(BH, Sp, 64)


def vt_from_units(u, BH, Sp):
    """[bh][kt][dt][t][lane = 32 h + r][8] holds V^T[32 dt + r][32 kt + 16 t + 8 h + j] -> V^T [BH, 64, Sp]."""
    nt = Sp // 32
    a = u.reshape(BH, nt, 2, 2, 2, 32, 8)
    return a.transpose(0, 2, 5, 1, 3, 4, 6).reshape(BH, 64, Sp)


def units_from_q(Q, klayout=False):
    """inverse of q_from_units, written on its own (scatter by the element's index tuple): [BH, Sp, 64] -> [BH * Sp * 8, 8]."""
    BH, Sp, _ = Q.shape
    out = np.zeros((BH, Sp // 32, 4, 64, 8), Q.dtype)
    row, e = np.meshgrid(np.arange(Sp), np.arange(64), indexing="ij")
    slot = pi32(row & 31) if klayout else (row & 31)
    out[:, row >> 5, e >> 4, 32 * ((e >> 3) & 1) + slot, e & 7] = Q
    return out.reshape(-1, 8)


def units_from_vt(Vt):
    BH, _, Sp = Vt.shape
    out = np.zeros((BH, Sp // 32, 2, 2, 64, 8), Vt.dtype)
    dd, key = np.meshgrid(np.arange(64), np.arange(Sp), indexing="ij")
    ko = key & 31
    out[:, key >> 5, dd >> 5, ko >> 4, 32 * ((ko >> 3) & 1) + (dd & 31), ko & 7] = Vt
    return out.reshape(-1, 8)


def qkv_decode(bufs, dt, split, B, nh, Sp):
    """raw Qh / Kh / Vt bytes -> (Q, K [B nh, Sp, 64], V^T [B nh, 64, Sp]) as (first part, second part or None) pairs."""
    BH, n_units = B * nh, B * nh * Sp * 8
    out = []
    for i, buf in enumerate(bufs):
        raw = np.frombuffer(buf, np.uint16 if split else (np.float32 if dt == "f32" else np.uint16))
        a, b = _units(raw if split else decode_T(raw, dt), n_units, split)
        f = (lambda u: vt_from_units(u, BH, Sp)) if i == 2 else (lambda u, k=(i == 1): q_from_units(u, BH, Sp, k))
        out.append((f(a), None if b is None else f(b)))
    return out


def mxt_qk_decode(buf, BH, Sp, hl, klayout, D=64):
    """MX tiles of Q / K (32 rows x D columns, 128 D bytes): D / 16 f16 units of 1 KiB (unit s, lane 32 h + slot: columns 16 s + 8 h + j), then
    D / 32 steps m of 2 KiB: lane 32 h + slot holds 32 bytes = [16 first parts | 16 second parts] of columns 32 m + 16 h + y; (hi8 | lo8) when
    hl, else (lo8 | hi8); K rows sit at slot pi(r).  D = 64: glc_layout.h; D = 128: the decoder's tiles (decoder_mx.hip).
    -> hi [BH, Sp, D] fp32, lo8, hi8 (decoded, float64)."""
    nt, ns, nm = Sp // 32, D // 16, D // 32
    t = np.frombuffer(buf, np.uint8).reshape(BH * nt, 128 * D)
    inv = pi32(np.arange(32)) if klayout else np.arange(32)
    f = np.ascontiguousarray(t[:, :ns * 1024]).view(np.float16).astype(np.float32).reshape(BH * nt, ns, 2, 32, 8)      # [tile][s][h][slot][j]
    hi = f[:, :, :, inv].transpose(0, 3, 1, 2, 4).reshape(BH, Sp, D)
    mx = t[:, ns * 1024:].reshape(BH * nt, nm, 2, 32, 2, 16)[:, :, :, inv]                                             # [tile][m][h][slot][first | second][y]
    parts = e4m3_decode(mx).transpose(4, 0, 3, 1, 2, 5).reshape(2, BH, Sp, D)
    return (hi, parts[1], parts[0]) if hl else (hi, parts[0], parts[1])


def mxt_vt_decode(buf, BH, Sp, D=64):
    """MX tiles of V^T: per 32-key tile D / 32 sub-tiles of 4 KiB (rows dd = 32 a .. 32 a + 31): [f16 unit t = 0 | t = 1 | one MX step over the
    32 keys]; f16 unit t, lane 32 h + dd: keys 16 t + 8 h + j; MX byte y of lane (dd, h): key 16 (y >> 3) + 8 h + (y & 7), 32 bytes per lane
    = [16 lo8 | 16 hi8].  -> hi [BH, D, Sp] fp32, lo8, hi8 (decoded, float64)."""
    nt, na = Sp // 32, D // 32
    t = np.frombuffer(buf, np.uint8).reshape(BH, nt, na, 4096)
    f = np.ascontiguousarray(t[..., :2048]).view(np.float16).astype(np.float32).reshape(BH, nt, na, 2, 2, 32, 8)       # [bh][kt][a][t][h][dd][j]
    hi = f.transpose(0, 2, 5, 1, 3, 4, 6).reshape(BH, D, Sp)
    mx = e4m3_decode(t[..., 2048:].reshape(BH, nt, na, 2, 32, 2, 2, 8))                                                # [bh][kt][a][h][dd][part][y >> 3][y & 7]
    parts = mx.transpose(5, 0, 2, 4, 1, 6, 3, 7).reshape(2, BH, D, Sp)                                                 # key = 32 kt + 16 (y >> 3) + 8 h + (y & 7)
    return hi, parts[0], parts[1]


def glu_interleave(W_first, W_second):
    """[I, K] x 2 -> [2 I, K]: rows alternate 16 features of the first projection (the gated one) / the same 16 of the second."""
    I, K = W_first.shape
    return np.stack([W_first.reshape(I // 16, 16, K), W_second.reshape(I // 16, 16, K)], axis=1).reshape(2 * I, K)


def rope_perm128(p):
    """physical row p of a 128-feature head holds logical feature: the 32-blocks 1 and 2 trade places."""
    p = np.asarray(p)
    b = (p >> 5) & 3
    return (p & 31) | (np.array([0, 2, 1, 3])[b] << 5)


# ---------------------------------------------------------------- references
def _erf(x):
    return np.frompyfunc(math.erf, 1, 1)(x).astype(np.float64)


def gelu(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def silu(x):
    x = np.asarray(x, np.float64)
    return x / (1.0 + np.exp(-x))


def operands(kind, A, W, dt="f16", sc_a=0, sc_w=0, prec=0):
    """The product terms a kernel forms, as float64 matrices: list of (a_part [M, K], w_part [N, K], factor)."""
    A, W = np.asarray(A, np.float32), np.asarray(W, np.float32)
    if kind == "exact":
        return [(A.astype(np.float64), W.astype(np.float64), 1.0)]
    if kind == "T":
        return [(round_T(A, dt).astype(np.float64), round_T(W, dt).astype(np.float64), 1.0)]
    if kind == "gs":
        ah, al = split_f16(A)
        wh, wl = split_f16(W)
        if prec & 1:
            al = np.zeros_like(al)
        if prec & 2:
            wl = np.zeros_like(wl)
        ah, al, wh, wl = (v.astype(np.float64) for v in (ah, al, wh, wl))
        return [(ah, wh, 1.0), (ah, wl, 1.0), (al, wh, 1.0)]
    if kind == "mx":
        ah, al8, ah8 = gx_parts(A, sc_a, saturate=False)
        wh, wl8, wh8 = gx_parts(W, sc_w, saturate=True)
        f = 2.0 ** -(GX_SHIFT + sc_a + sc_w)
        return [(ah.astype(np.float64), wh.astype(np.float64), 1.0), (e4m3_decode(al8), e4m3_decode(wh8), f), (e4m3_decode(ah8), e4m3_decode(wl8), f)]
    raise ValueError(kind)


def accumulate(terms):
    """(sum of the terms' products, sum of their magnitudes, number of products per output)."""
    acc = sum(f * (a @ w.T) for a, w, f in terms)
    mag = sum(f * (np.abs(a) @ np.abs(w).T) for a, w, f in terms)
    return acc, mag, sum(a.shape[1] for a, _, _ in terms)


def epilogue(acc, epi, bias=None, resid=None, a_stats=None, ln_c=None, r_stats=None, r_gamma=None, r_beta=None):
    """float64 epilogue of acc [M, N]: the LayerNorm fold rstd (acc - mean ln_c) + bias, then GELU / residual (raw residual rows
    normalised on the fly with r_stats) / silu(g) u / gelu(x) g on 16 / 16 interleaved columns."""
    v = np.asarray(acc, np.float64)
    if a_stats is not None and epi != EPI_RESID:
        st = np.asarray(a_stats, np.float64).reshape(-1, 2)
        if epi in (EPI_SWIGLU, EPI_GEGLU):
            v = v * st[:, 1:2]
        else:
            v = st[:, 1:2] * (v - st[:, 0:1] * (0.0 if ln_c is None else np.asarray(ln_c, np.float64)[None, :]))
    if bias is not None:      # [N], or [M, N] (two weight groups: a bias per row group)
        b = np.asarray(bias, np.float64)
        v = v + (b if b.ndim == 2 else b[None, :])
    if epi == EPI_GELU:
        v = gelu(v)
    elif epi == EPI_RESID:
        r = np.asarray(resid, np.float64)
        if r_stats is not None:
            st = np.asarray(r_stats, np.float64).reshape(-1, 2)
            r = (r - st[:, 0:1]) * st[:, 1:2] * np.asarray(r_gamma, np.float64)[None, :] + np.asarray(r_beta, np.float64)[None, :]
        v = v + r
    elif epi in (EPI_SWIGLU, EPI_GEGLU):
        M, N = v.shape
        g = v.reshape(M, N // 32, 2, 16)
        first, second = g[:, :, 0].reshape(M, N // 2), g[:, :, 1].reshape(M, N // 2)
        v = (silu(first) if epi == EPI_SWIGLU else gelu(first)) * second
    return v


def ln_partials(v):
    """(sum, squared deviations from the block mean) of every 64-column block: [M, N / 64, 2]."""
    M, N = v.shape
    b = np.asarray(v, np.float64).reshape(M, N // 64, 64)
    s = b.sum(2)
    return np.stack([s, ((b - s[:, :, None] / 64.0) ** 2).sum(2)], axis=2)


def ln_stats(rows, eps, rms=False):
    rows = np.asarray(rows, np.float64)
    if rms:
        return np.stack([np.zeros(len(rows)), 1.0 / np.sqrt((rows ** 2).mean(1) + eps)], axis=1)
    return np.stack([rows.mean(1), 1.0 / np.sqrt(rows.var(1) + eps)], axis=1)


def rope_rotate_half(x, cos, sin):
    """x [.., Sp, 128], cos / sin [Sp, 64]: (x1 cos - x2 sin | x2 cos + x1 sin)."""
    x1, x2 = x[..., :64], x[..., 64:]
    return np.concatenate([x1 * cos - x2 * sin, x2 * cos + x1 * sin], axis=-1)


# ---------------------------------------------------------------- bounds and the checker
def out_quant(ref, fmt, sc=0):
    """error of writing the fp32 value ref in the output format: half an ulp of the 16-bit types; GS rows lo = f16(v - hi): 2^-11 of
    |v - hi| <= 2^-11 |v|; GX rows lo8 = e4m3(..): 2^-4 of it; both with the floor of their subnormal spacing."""
    a = np.abs(np.asarray(ref, np.float64))
    if fmt == "f32":
        return np.zeros_like(a)
    if fmt == "f16":
        return a * 2.0 ** -11 + 2.0 ** -25
    if fmt == "bf16":
        return a * 2.0 ** -8
    if fmt == "gs":
        return a * 2.0 ** -22 + 2.0 ** -25
    if fmt == "gx":
        return a * 2.0 ** -15 + 2.0 ** -(10 + GX_SHIFT + sc)
    raise ValueError(fmt)


def bound(mag, steps, extra=0.0, c=C_ACC):
    return c * U24 * steps * np.asarray(mag, np.float64) + extra


def check(got, ref, bnd):
    """every element: |got - ref| against its own bound.  -> (ok, worst ratio, index of the worst element)."""
    got, ref, bnd = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.broadcast_to(np.asarray(bnd, np.float64), np.shape(ref))
    if got.shape != ref.shape:
        return False, float("inf"), None
    err = np.abs(got - ref)
    ratio = np.where(np.isfinite(err), err / np.maximum(bnd, 1e-300), np.inf)
    ratio = np.where(err == 0, 0.0, ratio)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else None
    worst = float(ratio[i]) if ratio.size else 0.0
    return worst <= 1.0, worst, i

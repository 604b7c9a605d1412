"""GPU (-m gpu): the 128 x 128 tile of the MX cross-term GEMM (csrc/gemm128x.hip) through glc_debug_gemm_run (kernel GLC_GEMM_RUN_MX128 = 5)
on an fp32 engine.  The arithmetic is that of the 256 tile, so the float64 emulation and the bound are the ones tests/test_gpu_gemm_kernels.py
applies to R.KMX (its docstring derives them); on shapes both tiles take, outputs, ln_part partials and the range counter must be EQUAL to the
256 tile's, byte for byte — the same products are added in the same order (f16 k 0-15, f16 k 16-31, the scaled fp8 MFMA; groups ascending)."""
import numpy as np
import pytest

import gemm_ref as R
import test_gpu_gemm_kernels as G
from gemm_run import FILL, run

pytestmark = pytest.mark.gpu

K128X = 5                                                       # GLC_GEMM_RUN_MX128 (include/gliclass_hip.h)
# (Mpad, N, K): one group (nothing requested ahead) | two | odd tile counts both ways, rows the 256 tile refuses, 3 groups on a 2-group ring | 24 groups
SHAPES = ((128, 128, 32), (128, 128, 64), (384, 384, 96), (256, 256, 768))
VARIANTS = ("bias", "gelu", "gelu-fold", "resid-raw-ln")
EPI = {"bias": R.EPI_BIAS, "gelu": R.EPI_GELU, "resid": R.EPI_RESID}


def _eng(weights_for):
    return G._engine(weights_for, "f32")


def _operands(variant, M, N, K):
    epi = EPI[variant.split("-")[0]]
    A, W = G.rnd((M, K), 1.0, 81), G.rnd((N, K), 0.05, 83)
    o = G.epi_args(epi, M, N, 90, False, fold=variant.endswith("fold"), rln=variant == "resid-raw-ln")
    if variant == "resid-raw-ln":
        o["want_ln_part"] = 1
    o["mx_ws"] = R.gx_weight_exponent(float(np.abs(W).max()))
    return epi, A, W, o


@pytest.mark.parametrize("variant", VARIANTS)
def test_epilogues(weights_for, variant):
    eng = _eng(weights_for)
    for (M, N, K) in SHAPES:
        epi, A, W, o = _operands(variant, M, N, K)
        ref, bnd, q, fmt, _ = G.emulate(R.KMX, "f32", epi, A, W, o)
        res = run(eng, K128X, epi, A, W, **o)
        assert res["rc"] == 0, res["err"]
        assert res["guards_ok"] == 1, "a guard region was written"
        G.check_images(res, R.KMX, "f32", A, W, o)             # the operand images GLC_GEMM_RUN_MX produces (the encoders that test checks them against)
        got = G.decode_c(res, fmt, "f32", M, N)
        ok, worst, idx = R.check(got, ref, bnd + q)
        print(f"[gemm128x] {variant:14s} M={M} N={N} K={K} worst error / bound = {worst:.4f}")
        assert ok, (variant, (M, N, K), worst, idx, got[idx], ref[idx], (bnd + q)[idx])
        assert res["sat"] == (0, 0)
        if o.get("want_ln_part"):                               # the partials against float64, with the bounds of test_gpu_gemm_kernels.case
            want = R.ln_partials(ref)
            pb = 64 * R.U24 * np.abs(ref).reshape(M, N // 64, 64).sum(2) + (bnd + q).reshape(M, N // 64, 64).sum(2)
            okp, wp, ip = R.check(res["ln_part"][:, :, 0], want[:, :, 0], pb)
            assert okp, ("ln_part sums", wp, ip)
            d = (bnd + q).reshape(M, N // 64, 64).max(2) + pb / 64
            okq, wq, iq = R.check(res["ln_part"][:, :, 1], want[:, :, 1], 2 * np.sqrt(want[:, :, 1]) * 8 * d + 64 * d * d + 200 * R.U24 * want[:, :, 1] + 1e-30)
            assert okq, ("ln_part M2", wq, iq)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("K", (32, 96, 768))
def test_bit_identical_to_the_256_tile(weights_for, variant, K):
    eng = _eng(weights_for)
    epi, A, W, o = _operands(variant, 256, 256, K)
    a, b = run(eng, R.KMX, epi, A, W, **o), run(eng, K128X, epi, A, W, **o)
    assert a["rc"] == 0 and b["rc"] == 0, (a["err"], b["err"])
    assert np.array_equal(a["A_img"], b["A_img"]) and np.array_equal(a["W_img"], b["W_img"])
    assert np.array_equal(a["out"][0], b["out"][0]), f"{int((a['out'][0] != b['out'][0]).sum())} output bytes differ"
    if o.get("want_ln_part"):
        assert np.array_equal(a["ln_part"].view(np.uint32), b["ln_part"].view(np.uint32))
    assert a["sat"] == b["sat"]


def _qkv_operands(Mpad, H, K):
    N = 3 * H
    A, W, bias = G.rnd((Mpad, K), 1.0, 51), G.rnd((N, K), 0.05, 53), G.rnd(N, 0.1, 54)
    ws = R.gx_weight_exponent(0.05)
    acc, mag, steps = R.accumulate(R.operands("mx", A, W, "f32", 0, ws))
    ref = R.epilogue(acc, R.EPI_BIAS, bias=bias)
    bnd = R.bound(mag, steps) + G.EPI_OPS * R.U24 * (np.abs(acc) + np.abs(bias)[None, :])
    return A, W, bias, ws, ref, bnd


@pytest.mark.parametrize("Mpad,Mvalid,Sp", ((256, 256, 64), (512, 384, 128)))
@pytest.mark.parametrize("mxt", (0, 1))
@pytest.mark.parametrize("skip_q", (0, 1))
def test_qkv(weights_for, Mpad, Mvalid, Sp, mxt, skip_q):
    """Q / K / V^T (split-f16 units, or MX tiles with qkv_mxt) equal to the 256 tile's, a skipped Q and the rows from Mvalid on untouched,
    and every live element within the float64 bound of test_gpu_gemm_kernels (qkv_case / _mx_tile_check)."""
    eng = _eng(weights_for)
    H, K, nh = 256, 96, 4
    A, W, bias, ws, ref, bnd = _qkv_operands(Mpad, H, K)
    o = dict(bias=bias, Mvalid=Mvalid, Sp=Sp, nh=nh, H=H, mx_ws=ws, qkv_skip_q=skip_q)
    o.update(dict(qkv_mxt=1) if mxt else dict(qkv_split=1))
    a, b = run(eng, R.KMX, R.EPI_QKV, A, W, **o), run(eng, K128X, R.EPI_QKV, A, W, **o)
    assert a["rc"] == 0 and b["rc"] == 0, (a["err"], b["err"])
    assert b["guards_ok"] == 1
    for i, name in enumerate("QKV"):
        assert np.array_equal(a["out"][i], b["out"][i]), f"{name}: {int((a['out'][i] != b['out'][i]).sum())} bytes differ from the 256 tile's"
    assert a["sat"] == b["sat"] == (0, 0)
    if skip_q:
        assert (b["out"][0] == FILL).all(), "a skipped Q was written"
    B = -(-Mvalid // Sp)
    rows = B * Sp
    live = np.zeros(rows, bool); live[:Mvalid] = True
    rr, bb = ref[:rows], bnd[:rows]
    if mxt:
        heads = lambda p: tuple(x.reshape(B, nh, Sp, 64).transpose(0, 2, 1, 3).reshape(rows, H) for x in p)
        q = heads(R.mxt_qk_decode(b["out"][0].tobytes(), B * nh, Sp, True, False))
        k = heads(R.mxt_qk_decode(b["out"][1].tobytes(), B * nh, Sp, False, True))
        v = tuple(x.reshape(B, nh, 64, Sp).transpose(0, 3, 1, 2).reshape(rows, H) for x in R.mxt_vt_decode(b["out"][2].tobytes(), B * nh, Sp))
        for name, parts, c0 in (("Q", q, 0), ("K", k, H), ("V", v, 2 * H)):
            if name == "Q" and skip_q:                          # (every byte still the fill pattern: asserted above)
                continue
            lv = live
            worst = G._mx_tile_check(name, parts, rr[:, c0:c0 + H], bb[:, c0:c0 + H], lv, False, "gemm128x qkv_mxt")
            print(f"[gemm128x] qkv mx-tiles {name} Mpad={Mpad} Sp={Sp} skip_q={skip_q} worst error / bound = {worst:.4f}")
        return
    (qa, qb), (ka, kb_), (va, vb) = R.qkv_decode([x.tobytes() for x in b["out"]], "f32", True, B, nh, Sp)
    two = lambda x, y: x.astype(np.float64) + y
    Q = two(qa, qb).reshape(B, nh, Sp, 64).transpose(0, 2, 1, 3).reshape(rows, H)
    Kk = two(ka, kb_).reshape(B, nh, Sp, 64).transpose(0, 2, 1, 3).reshape(rows, H)
    V = two(va, vb).reshape(B, nh, 64, Sp).transpose(0, 3, 1, 2).reshape(rows, H)
    bq = bb + R.out_quant(np.abs(rr) + bb, "gs")
    for name, got, c0 in (("Q", Q, 0), ("K", Kk, H), ("V", V, 2 * H)):
        lv = live & (not (name == "Q" and skip_q))
        untouched = G._row_bytes_untouched(b["out"]["QKV".index(name)], name, B, nh, Sp, True, "f32")
        assert untouched[~lv].all(), f"{name}: a row that must stay untouched was written"
        assert not untouched[lv].any(), f"{name}: a live row still holds the fill pattern"
        if lv.any():
            ok, worst, idx = R.check(got[lv], rr[lv][:, c0:c0 + H], bq[lv][:, c0:c0 + H])
            print(f"[gemm128x] qkv split-units {name} Mpad={Mpad} Sp={Sp} skip_q={skip_q} worst error / bound = {worst:.4f}")
            assert ok, (name, worst, idx)


def test_range_counter(weights_for):
    """one activation element at 500.0 (beyond the e4m3 range, 448): the first counter word as on the 256 tile; the same for a Q / K / V tile
    and the second word"""
    eng = _eng(weights_for)
    M = N = 256
    K = 32
    A, W = G.ints((M, K), 1), G.ints((N, K), 2)
    resid = np.zeros((M, N), np.float32)
    resid[131, 77] = 500.0 - float(A[131].astype(np.float64) @ W[77].astype(np.float64))      # the sum itself is 500.0
    o = dict(bias=np.zeros(N, np.float32), resid=resid, want_ln_part=1, mx_ws=7)
    a, b = run(eng, R.KMX, R.EPI_RESID, A, W, **o), run(eng, K128X, R.EPI_RESID, A, W, **o)
    assert a["rc"] == 0 and b["rc"] == 0, (a["err"], b["err"])
    assert a["sat"] == (1, 0) and b["sat"] == a["sat"], (a["sat"], b["sat"])
    assert np.array_equal(a["out"][0], b["out"][0])
    H, nh, Sp = 256, 4, 64
    Wq = G.ints((3 * H, K), 3)
    bias = np.zeros(3 * H, np.float32)
    o = dict(Mvalid=M, Sp=Sp, nh=nh, H=H, qkv_mxt=1, mx_ws=7)
    # a Q, a K and a V column pushed beyond the range in every row.  The counter's unit is the 8-element store: 8 columns of a row for Q / K (one
    # unit per row), 8 keys of a column for V^T (one unit per 8 rows)
    for col, units in ((77, M), (H + 5, M), (2 * H + 200, M // 8)):
        bq = bias.copy(); bq[col] = 1000.0
        assert int((np.abs(A.astype(np.float64) @ Wq.astype(np.float64).T + bq) > 448).sum()) == M
        a, b = run(eng, R.KMX, R.EPI_QKV, A, Wq, bias=bq, **o), run(eng, K128X, R.EPI_QKV, A, Wq, bias=bq, **o)
        assert a["rc"] == 0 and b["rc"] == 0, (a["err"], b["err"])
        assert b["sat"] == a["sat"] and b["sat"] == (0, units), (col, units, a["sat"], b["sat"])


REFUSED = [(dict(Mpad=192), R.EPI_BIAS), (dict(N=192), R.EPI_BIAS), (dict(K=48), R.EPI_BIAS), (dict(), R.EPI_RESID), (dict(), R.EPI_SWIGLU)]


@pytest.mark.parametrize("o,epi", REFUSED, ids=["Mpad192", "N192", "K48", "resid-without-residual", "swiglu"])
def test_refusals(weights_for, o, epi):
    eng = _eng(weights_for)
    o = dict(o)
    Mpad, N, K = o.pop("Mpad", 256), o.pop("N", 256), o.pop("K", 64)
    res = run(eng, K128X, epi, G.rnd((Mpad, K), 1, 1), G.rnd((N, K), 1, 2), out_bytes=[1 << 20] * 3, **o)
    assert res["rc"] == -2 and res["err"].startswith("gemm128x:"), (res["rc"], res["err"])
    assert all((x == 0).all() for x in res["out"]), "an output came back from a refused launch"

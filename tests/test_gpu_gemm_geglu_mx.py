"""GPU (-m gpu): the GeGLU epilogue of the MX cross-term GEMM (gemm256x.hip EPI_GEGLU, the FFN input projection of ModernBERT's MX
pipeline), one launcher call per case through glc_debug_gemm_run.  W rows interleave 16 input / 16 gate features; the output
[Mpad, N / 2] = gelu_erf(input) * gate is written as GX rows.

The emulation, the encoders and the per-element bound are those of tests/test_gpu_gemm_kernels.py (`case` / `emulate`): the bound it
derives for `mx ... swiglu` with the silu function-error term replaced by the erf-GELU one of `256s ... geglu` — glc_gelu2_f32's
documented 5.9e-7 on GS / MX rows — which is what `emulate` returns for (KMX, EPI_GEGLU).  Nothing is fitted to an output.

Exact case.  A = {-1, 0, 1} (+ 2^-12 parts), its first 16 columns all 1.  An input row of W is either zero (GELU argument 0 -> 0) or ones
on those 16 columns (argument 16: erf(16 / sqrt 2) == 1 in float64 and 1 + 2^(16 P(36)) == 1 in fp32, so gelu(16) == 16 in both); the gate
rows carry the values (sparse, so that 16 * gate stays inside the e4m3 range).  Output bytes must equal the encoded emulation.

Every launch states `glu_interleaved` (GemmArgs: the caller vouches for W's row order); a launch without it is refused as before
(tests/test_gpu_gemm_kernels.py keeps that case).

Shapes: Mpad = 256, N = 512 and K = 32 (one K-group), 96 (an odd group count), 256 (the four-slot ring wraps twice); one Mpad = 512 case."""
import numpy as np
import pytest

import gemm_ref as R
import test_gpu_gemm_kernels as G
from gemm_run import run

pytestmark = pytest.mark.gpu

SHAPES = ((256, 512, 32), (256, 512, 96), (256, 512, 256), (512, 512, 96))


def exact_operands(M, N, K, seed):
    A = G.ints((M, K), seed, lo_part=True)
    A[:, :16] = 1.0
    W = G.ints((N, K), seed + 1, lo_part=True, density=0.08)                  # gate rows (and the input rows, overwritten below)
    on = np.random.default_rng(seed + 2).random(N // 32 * 16) < 0.5
    rows_in = (np.arange(N).reshape(N // 32, 2, 16)[:, 0]).reshape(-1)        # the input rows: 16 of every 32
    W[rows_in] = 0.0
    W[rows_in[on], :16] = 1.0
    return A, W, rows_in, on


@pytest.mark.parametrize("M,N,K", SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in SHAPES])
def test_exact(weights_for, M, N, K):
    A, W, _, on = exact_operands(M, N, K, 300 + K)
    assert on.any() and not on.all()
    ws = R.gx_weight_exponent(float(np.abs(W).max()))
    res, ref, got = G.case(weights_for, "f16", R.KMX, R.EPI_GEGLU, A, W, exact=True, label="exact", mx_ws=ws, glu_interleaved=1)     # bytes == encoded emulation, guards untouched
    assert ref.shape == (M, N // 2) and (ref != 0).any() and np.abs(ref).max() < 448
    assert res["sat"] == (0, 0)


@pytest.mark.parametrize("M,N,K", SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in SHAPES])
def test_random_against_float64(weights_for, M, N, K):
    A, W = G.rnd((M, K), 1.0, 81), G.rnd((N, K), 0.2, 83)
    ws = R.gx_weight_exponent(float(np.abs(W).max()))
    res, ref, got = G.case(weights_for, "f16", R.KMX, R.EPI_GEGLU, A, W, exact=False, mx_ws=ws, glu_interleaved=1)      # prints worst error / bound, asserts <= 1
    assert res["sat"] == (0, 0)


def test_range_counter(weights_for):
    """One product pushed beyond 448 (input 32 x gate 32 in one row and column) must count: the first counter word = the 8-column store
    units of rows [0, gx_rows) that hold |x| > 448, from the reference alone."""
    M, N, K = 256, 512, 32
    A, W, rows_in, on = exact_operands(M, N, K, 410)
    m_hot, f_hot = 77, 40                                        # output feature 40: input row 32 * 2 + 8, gate row 32 * 2 + 16 + 8
    A[m_hot, :16] = 2.0
    W[32 * (f_hot // 16) + f_hot % 16] = 0.0
    W[32 * (f_hot // 16) + f_hot % 16, :16] = 1.0
    W[32 * (f_hot // 16) + 16 + f_hot % 16, :16] = 1.0
    ws = R.gx_weight_exponent(float(np.abs(W).max()))
    eng = G._engine(weights_for, "f16")
    ref, _, _, fmt, _ = G.emulate(R.KMX, "f16", R.EPI_GEGLU, A, W, dict(mx_ws=ws))
    assert fmt == "gx" and abs(ref[m_hot, f_hot]) > 448
    for gx_rows in (0, 200, 64):
        limit = gx_rows or M
        want = int((np.abs(ref[:limit]).reshape(limit, N // 16, 8).max(2) > 448).sum())
        assert want >= (1 if limit > m_hot else 0) and (want == 0) == (limit <= m_hot)
        res = run(eng, R.KMX, R.EPI_GEGLU, A, W, mx_ws=ws, gx_rows=gx_rows, glu_interleaved=1)
        assert res["rc"] == 0 and res["guards_ok"] == 1, res["err"]
        assert res["sat"] == (want, 0), (gx_rows, res["sat"], want)


@pytest.mark.parametrize("o,message", [(dict(bias=True), "the GeGLU epilogue takes no bias"), (dict(a_stats=True), "the GeGLU epilogue takes no bias and no folded norm")],
                         ids=["bias", "a_stats"])
def test_refusals(weights_for, o, message):
    eng = G._engine(weights_for, "f16")
    M, N, K = 256, 512, 64
    A, W = G.rnd((M, K), 1, 1), G.rnd((N, K), 1, 2)
    kw = {}
    if o.get("bias"):
        kw["bias"] = G.rnd(N, 1, 3)
    if o.get("a_stats"):
        kw["a_stats"] = np.stack([G.rnd(M, 0.1, 4), 0.5 + np.abs(G.rnd(M, 0.4, 5))], 1)
    res = run(eng, R.KMX, R.EPI_GEGLU, A, W, glu_interleaved=1, **kw)
    assert res["rc"] == -2 and message in res["err"], (res["rc"], res["err"])
    assert (res["out"][0] == 0).all()                            # nothing came back: nothing was launched


@pytest.mark.parametrize("exact", (True, False), ids=["exact", "random"])
def test_mx_residual_from_plain_fp32_rows(weights_for, exact):
    """EPI_RESID with gs_resid_plain on the MX kernel (the o-projection and the down projection of ModernBERT's MX pipeline: the residual
    stream stays plain fp32 in and out).  `emulate` reads an MX residual back through its GX image, so the residual here is one that
    image holds exactly (integers; random values rounded through the GX parts once): the same bound then covers the plain rows."""
    for (M, N, K) in ((256, 256, 32), (512, 512, 96)):
        A = G.ints((M, K), 500, lo_part=True) if exact else G.rnd((M, K), 1.0, 501)
        W = G.ints((N, K), 502, lo_part=True) if exact else G.rnd((N, K), 0.05, 503)
        o = G.epi_args(R.EPI_RESID, M, N, 510, exact)
        if not exact:
            hi, lo8, _ = R.gx_parts(o["resid"], 0, saturate=False)
            o["resid"] = R.gx_value(hi, R.e4m3_decode(lo8), 0).astype(np.float32)
            hi2, lo82, _ = R.gx_parts(o["resid"], 0, saturate=False)
            assert np.array_equal(R.gx_value(hi2, R.e4m3_decode(lo82), 0).astype(np.float32), o["resid"])
        res, ref, got = G.case(weights_for, "f16", R.KMX, R.EPI_RESID, A, W, exact=exact, label="resid-plain-in", gs_resid_plain=1,
                               mx_ws=R.gx_weight_exponent(float(np.abs(W).max())), **o)
        assert np.array_equal(res["resid_img"][:M * N * 4].view(np.float32), o["resid"].reshape(-1)), "the residual travelled as plain fp32 rows"
    eng = G._engine(weights_for, "f16")
    res = run(eng, R.KMX, R.EPI_RESID, A, W, gs_resid_plain=1, want_ln_part=1, mx_ws=0, resid=o["resid"])
    assert res["rc"] == -2 and "plain fp32 residual" in res["err"], (res["rc"], res["err"])

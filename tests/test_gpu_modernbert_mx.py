"""GPU (-m gpu): the opt-in MX pipeline of the ModernBERT backbone (Engine.enable_mx / GLICLASS_MX_MODERNBERT=1): GX rows, the MX
cross-term GEMM with the GeGLU epilogue, attention on MX tiles (ring kernel on the global layers, windowed per-wave kernel on the local
ones), against the CPU restatement tests/modernbert_ref.py in float64.

Tolerance on probabilities: 5e-4 for the MX arithmetic — the bar DESIGN.md §2 holds the MX forwards of the other backbones to on
short-row shapes — and the existing 1e-4 for the split-f16 arithmetic of the same engine (set_mx(False)).  Every test prints the worst
error it saw (pytest -s); DESIGN.md §4c records them."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import modernbert_ref

pytestmark = pytest.mark.gpu

TOL_MX, TOL_SPLIT = 5e-4, 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sig(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def perr(a, b):
    return float(np.abs(sig(a) - sig(b)).max()) if np.size(a) else 0.0


def ref_logits(cfg, w, ids, mask):
    return modernbert_ref.forward(cfg, w, ids, mask, dtype=torch.float64)


def mx_engine(cfg, w):
    from gliclass.c_amd.engine import Engine
    eng = Engine(cfg, w, dtype="f32")
    try:
        eng.enable_mx()
        eng.set_group_split(2)
    except Exception:
        eng.close()
        raise
    return eng


def first_pooled(cfg):
    from gliclass.c_amd.config import POOL_FIRST
    return dataclasses.replace(cfg, pooling=POOL_FIRST)


@pytest.mark.parametrize("pooling", ["avg", "first"])
def test_sweep(pooling, weights_for):
    """S in {1, 33, 129, 515} with 0 - 4 labels: MX with the attention on MX tiles, MX with the attention on split units, split arithmetic."""
    from gliclass.c_amd import synth
    cfg, w = weights_for("mb-mini")
    if pooling == "first":
        cfg = first_pooled(cfg)
    eng = mx_engine(cfg, w)
    worst = {"mx": 0.0, "mx, split-unit attention": 0.0, "split": 0.0}
    try:
        for S, Cn in ((1, 0), (33, 2), (129, 3), (515, 4)):
            ids, mask, _ = synth.make_inputs(cfg, 1, S, Cn, seed=S, ragged=False)
            ref = ref_logits(cfg, w, ids, mask)
            got = eng.forward(ids, mask, c_alloc=ref.shape[1])
            assert got.shape == ref.shape and np.isfinite(got).all()
            assert eng.last_group_split() == 1 and eng.last_mx() == 1 and eng.last_mx_attention() == 1, S
            assert eng.last_pruned() == (1 if pooling == "first" else 0)
            worst["mx"] = max(worst["mx"], perr(got, ref))
            eng.set_mx_attention(False)
            got = eng.forward(ids, mask, c_alloc=ref.shape[1])
            eng.set_mx_attention(True)
            assert eng.last_mx() == 1 and eng.last_mx_attention() == 0 and np.isfinite(got).all(), S
            worst["mx, split-unit attention"] = max(worst["mx, split-unit attention"], perr(got, ref))
            eng.set_mx(False)
            got = eng.forward(ids, mask, c_alloc=ref.shape[1])
            eng.set_mx(True)
            assert eng.last_mx() == 0 and eng.last_group_split() == 1 and np.isfinite(got).all(), S
            worst["split"] = max(worst["split"], perr(got, ref))
        assert eng.fp8_range_retries() == 0 and eng.activation_exponent() == 0
    finally:
        eng.close()
    print(f"[mb-mx] sweep ({pooling} pooling): worst probability error " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["mx"] <= TOL_MX and worst["mx, split-unit attention"] <= TOL_MX and worst["split"] <= TOL_SPLIT, worst


@pytest.mark.parametrize("W", [8, 50, 64, 200])
def test_window_edges(W, weights_for):
    """Ragged batches where the window crosses the key length inside a tile: the windowed MX kernel against the reference and against
    the straightforward kernel (impl 1: plain fp32 rows, no MX) of the same engine."""
    from gliclass.c_amd import synth, weights
    base, _ = weights_for("mb-mini")
    cfg = dataclasses.replace(base, layers=3, local_window=W, global_every=3)
    w = weights.make_weights(cfg, 21)
    eng = mx_engine(cfg, w)
    worst = 0.0
    try:
        for S, seed in ((100, 1), (1000, 2)):
            ids, mask, _ = synth.make_inputs(cfg, 3, S, 3, seed=seed, ragged=True)
            ref = ref_logits(cfg, w, ids, mask)
            got = eng.forward(ids, mask)
            assert eng.last_mx() == 1 and eng.last_mx_attention() == 1
            eng.set_attention_impl(1)
            simple = eng.forward(ids, mask)
            eng.set_attention_impl(0)
            assert eng.last_mx() == 0
            e_ref, e_simple = perr(got, ref), perr(got, simple)
            worst = max(worst, e_ref, e_simple)
            assert e_ref <= TOL_MX and e_simple <= TOL_MX and perr(simple, ref) <= TOL_SPLIT, (W, S, e_ref, e_simple)
    finally:
        eng.close()
    print(f"[mb-mx] window {W}: worst probability error {worst:.2e}")


def test_window_covering_the_sequence_equals_global(weights_for):
    """W = S - 1 (every key inside the window: the windowed kernel walks all tiles) against W = 0 (the ring kernel on every layer), one
    RoPE base for both layer kinds.  Two kernels walk the keys: within the tolerance, not bit for bit."""
    from gliclass.c_amd import synth, weights
    base, _ = weights_for("mb-mini")
    cfg = dataclasses.replace(base, layers=3, global_every=3)
    w = weights.make_weights(cfg, 21)
    S = 1000
    ids, mask, _ = synth.make_inputs(cfg, 3, S, 3, seed=2, ragged=True)
    outs = []
    for W in (S - 1, 0):
        c2 = dataclasses.replace(cfg, local_window=W, rope_theta_local=cfg.rope_theta)
        eng = mx_engine(c2, w)
        try:
            outs.append(eng.forward(ids, mask))
            assert eng.last_mx() == 1 and eng.last_mx_attention() == 1
        finally:
            eng.close()
    err = perr(outs[0], outs[1])
    print(f"[mb-mx] window S - 1 against global: probability difference {err:.2e}")
    assert err <= TOL_MX


def test_pruned_last_layer(weights_for):
    from gliclass.c_amd import synth
    base, w = weights_for("mb-mini")
    cfg = first_pooled(base)
    eng = mx_engine(cfg, w)
    try:
        for S, Cn, ragged in ((200, 3, True), (515, 4, False)):
            ids, mask, _ = synth.make_inputs(cfg, 3, S, Cn, seed=S, ragged=ragged)
            ref = ref_logits(cfg, w, ids, mask)
            for mxa in (True, False):
                eng.set_mx_attention(mxa)
                pruned = eng.forward(ids, mask)
                assert eng.last_pruned() == 1 and eng.last_mx() == 1 and eng.last_mx_attention() == int(mxa)
                eng.set_prune_last_layer(False)
                full = eng.forward(ids, mask)
                eng.set_prune_last_layer(True)
                assert eng.last_pruned() == 0 and eng.last_mx() == 1
                e1, e2, e3 = perr(pruned, ref), perr(full, ref), perr(pruned, full)
                print(f"[mb-mx] pruned S={S} mx attention {mxa}: pruned / reference {e1:.2e}, full / reference {e2:.2e}, pruned / full {e3:.2e}")
                assert e1 <= TOL_MX and e2 <= TOL_MX and e3 <= TOL_MX
            eng.set_mx_attention(True)
    finally:
        eng.close()


def test_length_buckets_same_rows(weights_for):
    """The shapes of test_gpu_modernbert.py::test_length_bucketing_rows_identical (the planner splits them), first-token pooling, MX on:
    every group runs the pruned MX forward, and a row's answer does not depend on the group it ran in."""
    from gliclass.c_amd import synth
    base, w = weights_for("mb-mini")
    cfg = first_pooled(base)
    ids, mask, _ = synth.make_inputs(cfg, 96, 2048, 3, seed=31)
    for b in range(32, 96):
        n = 100 + b
        ids[b, n:] = cfg.pad_id
        mask[b, n:] = 0
    eng = mx_engine(cfg, w)
    try:
        eng.set_length_buckets(4)
        a = eng.forward(ids, mask)
        groups = eng.L.glc_debug_last_forward_groups(eng.h)
        assert eng.last_mx() == 1 and eng.last_pruned() == 1
        eng.set_length_buckets(1)
        b = eng.forward(ids, mask)
        assert eng.last_mx() == 1 and eng.last_pruned() == 1
        assert groups > 1
        err = perr(a, b)
        print(f"[mb-mx] buckets 4 against 1: {groups} groups, probability difference {err:.2e}")
        assert err <= 1e-5
    finally:
        eng.close()


def outlier_model(weights_for, gain):
    """mb-mini with channel 5 of layer 1's mlp_norm gain multiplied by `gain` and column 5 of that layer's Wi divided by it: the same
    function, with normalised rows that hold |x| ~ 3 gain in one channel."""
    base, w0 = weights_for("mb-mini")
    w = dict(w0)
    g = w0["layers.1.mlp_norm.weight"].copy()
    g[5] *= gain
    wi = w0["layers.1.mlp.Wi.weight"].copy()
    wi[:, 5] /= gain
    w["layers.1.mlp_norm.weight"], w["layers.1.mlp.Wi.weight"] = g, wi
    return base, w


def test_fp8_range_guard(weights_for):
    """Mirror of test_gpu_decoder.py::test_decoder_outlier_tokens_fp8_range_guard.  The gain puts the bound max |gamma| sqrt(H) beyond 448,
    so enable_mx starts the engine at activation exponent -5; rows of ~ 2e4 leave that range too (> 14336): the host-buffer forward
    counts them, repeats itself on the split-f16 kernels and returns exactly what the split arithmetic returns."""
    from gliclass.c_amd import synth
    from gliclass.c_amd.engine import Engine
    cfg, w = outlier_model(weights_for, 6000.0)
    ids, mask, _ = synth.make_inputs(cfg, 3, 200, 3, seed=91, ragged=True)
    ref = ref_logits(cfg, w, ids, mask)
    eng = Engine(cfg, w, dtype="f32")
    try:
        eng.set_group_split(2)
        split = eng.forward(ids, mask)
        assert eng.last_mx() == 0 and eng.fp8_range_retries() == 0
        eng.enable_mx()
        assert eng.activation_exponent() == -5
        got = eng.forward(ids, mask)
        assert np.isfinite(got).all() and eng.range_retries() == 0
        assert eng.fp8_range_retries() == 1 and eng.last_mx() == 0 and eng.last_group_split() == 1
        assert np.array_equal(got, split), "the repeated forward is the split-f16 forward"
        err = perr(got, ref)
        print(f"[mb-mx] range guard: probability error of the repeated (split-f16) forward {err:.2e}")
        assert err <= 1e-3
        got = eng.forward(ids, mask)                     # the second in a row: the engine leaves the MX pipeline for good
        assert eng.fp8_range_retries() == 2 and eng.fp8_range_sticky() and np.array_equal(got, split)
        got = eng.forward(ids, mask)
        assert eng.fp8_range_retries() == 2 and eng.last_mx() == 0 and np.array_equal(got, split)
    finally:
        eng.close()


def test_fp8_range_guard_first_answer_and_device_resident_path(weights_for):
    """Rows of ~ 1e3 (gain 300).  enable_mx picks exponent -5 from the gains: no forward is repeated.  With the exponent put back to 0
    (set_mx(True) clears the guard's verdict) the host-buffer forward finds it again (one repeat, still MX), and the device-resident
    forward reports through glc_engine_sync: it fails once with the message, the next forward is good."""
    from gliclass.c_amd import synth
    cfg, w = outlier_model(weights_for, 300.0)
    B, S, Cn = 3, 200, 3
    ids, mask, _ = synth.make_inputs(cfg, B, S, Cn, seed=91, ragged=True)
    ref = ref_logits(cfg, w, ids, mask)
    eng = mx_engine(cfg, w)
    d_ids = d_mask = d_out = None
    try:
        assert eng.activation_exponent() == -5
        got = eng.forward(ids, mask)
        assert eng.last_mx() == 1 and eng.fp8_range_retries() == 0
        e0 = perr(got, ref)
        eng.set_mx(True)
        assert eng.activation_exponent() == 0
        got = eng.forward(ids, mask)
        assert eng.fp8_range_retries() == 1 and eng.last_mx() == 1 and eng.activation_exponent() == -5
        e1 = perr(got, ref)
        eng.set_mx(True)
        d_ids, d_mask, d_out = eng.dev_alloc(ids.nbytes), eng.dev_alloc(mask.nbytes), eng.dev_alloc(B * Cn * 4)
        eng.h2d(d_ids, ids); eng.h2d(d_mask, mask)
        eng.forward_device(d_ids, d_mask, B, S, Cn, d_out)
        assert eng.last_mx() == 1
        with pytest.raises(RuntimeError, match="fp8 range"):
            eng.sync()
        assert eng.activation_exponent() == -5 and not eng.fp8_range_sticky()
        eng.forward_device(d_ids, d_mask, B, S, Cn, d_out)
        eng.sync()
        assert eng.last_mx() == 1
        dev = np.zeros((B, Cn), np.float32)
        eng.d2h(dev, d_out)
        e2 = perr(dev, ref)
        print(f"[mb-mx] outlier rows at exponent -5: probability error {e0:.2e} (proactive), {e1:.2e} (after the repeat), {e2:.2e} (device-resident)")
        assert max(e0, e1, e2) <= 1e-3
    finally:
        for p in (d_ids, d_mask, d_out):
            if p:
                eng.dev_free(p)
        eng.close()


def test_refusals(weights_for):
    from gliclass.c_amd import synth
    from gliclass.c_amd.engine import Engine
    cfg, w = weights_for("mb-tiny")                      # hidden 128
    eng = Engine(cfg, w, dtype="f32")
    try:
        with pytest.raises(RuntimeError, match="multiple of 256"):
            eng.enable_mx()
        with pytest.raises(RuntimeError):
            eng.set_mx(True)
    finally:
        eng.close()
    cfg, w = weights_for("mb-mini")
    eng = Engine(cfg, w, dtype="f16")
    try:
        with pytest.raises(RuntimeError, match="fp32"):
            eng.enable_mx()
    finally:
        eng.close()
    eng = Engine(cfg, w, dtype="f32")                    # created without the switch: as before
    try:
        eng.set_group_split(2)
        ids, mask, _ = synth.make_inputs(cfg, 1, 129, 3, seed=129, ragged=False)
        eng.forward(ids, mask)
        assert eng.last_group_split() == 1 and eng.last_mx() == 0 and eng.last_mx_attention() == 0
        with pytest.raises(RuntimeError):
            eng.set_mx(True)
        eng.enable_mx()
        eng.enable_mx()                                  # a second call changes nothing
        eng.forward(ids, mask)
        assert eng.last_mx() == 1
    finally:
        eng.close()


def test_environment_switch():
    code = ("import numpy as np\n"
            "from gliclass.c_amd import synth, weights\n"
            "from gliclass.c_amd.config import CONFIGS\n"
            "from gliclass.c_amd.engine import Engine\n"
            "cfg = CONFIGS['mb-mini']\n"
            "eng = Engine(cfg, weights.make_weights(cfg, 42), dtype='f32')\n"
            "eng.set_group_split(2)\n"
            "ids, mask, _ = synth.make_inputs(cfg, 1, 129, 3, seed=129, ragged=False)\n"
            "got = eng.forward(ids, mask)\n"
            "print('LAST_MX', int(eng.last_mx()), int(eng.last_mx_attention()), int(np.isfinite(got).all()))\n"
            "eng.close()\n")
    env = dict(os.environ, GLICLASS_MX_MODERNBERT="1", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-s", "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "LAST_MX 1 1 1" in out.stdout, (out.stdout, out.stderr[-2000:])

"""GPU (-m gpu): the ModernBERT backbone — fixtures (tests/golden/modernbert, made by transformers' ModernBertModel), a shape sweep
and the window's edges against the CPU restatement tests/modernbert_ref.py, long context, length bucketing, and a full-size model.
Tolerances are the decoder suite's (fp32 is the parity-grade mode; the 16-bit modes are held to their measured envelope)."""
import dataclasses
import glob
import os

import numpy as np
import pytest
import torch

import modernbert_ref

pytestmark = pytest.mark.gpu

TOL_PROB = {"f32": 1e-4, "f16": 1e-2, "bf16": 6e-2}
MB_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "modernbert")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(MB_GOLDEN, "*.npz")))


def sig(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def ref_logits(cfg, w, ids, mask):
    return modernbert_ref.forward(cfg, w, ids, mask, dtype=torch.float64)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("case", CASES)
def test_fixtures(case, dtype, weights_for):
    from gliclass.c_amd.engine import Engine
    g = np.load(os.path.join(MB_GOLDEN, case + ".npz"))
    cfg, w = weights_for(str(g["config"]))
    ids, mask = g["ids"].astype(np.int64), g["mask"].astype(np.int64)
    B, S = ids.shape
    eng = Engine(cfg, w, dtype=dtype)
    try:
        if dtype == "f32":
            eng.keep_hidden(True)
        got = eng.forward(ids, mask)
        assert got.shape == g["logits"].shape and np.isfinite(got).all()
        assert np.abs(sig(got) - g["probs"].astype(np.float64)).max() <= TOL_PROB[dtype]
        assert eng.last_mx() == 0
        if dtype == "f32":
            pos, hs = g["sample_pos"], g["hidden_samples"]
            att = mask[:, pos].astype(bool)
            for which in range(cfg.layers + 1):
                h = eng.hidden(which, B, S)[:, pos, : hs.shape[-1]]
                assert np.abs(h - hs[which])[att].max() <= 3e-4, which
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_sweep_against_reference(dtype, weights_for):
    """S in {1, 33, 129, 515} at B = 1, rows without labels, on both small configs; mb-mini in f32 with the group-split pipeline forced
    (it must run) and off."""
    from gliclass.c_amd import synth
    from gliclass.c_amd.engine import Engine
    for cname in ("mb-tiny", "mb-mini"):
        cfg, w = weights_for(cname)
        eng = Engine(cfg, w, dtype=dtype)
        try:
            modes = (2, 0) if (dtype == "f32" and cname == "mb-mini") else (1,)
            for S, Cn in ((1, 0), (33, 2), (129, 3), (515, 4)):
                ids, mask, _ = synth.make_inputs(cfg, 1, S, Cn, seed=S, ragged=False)
                ref = ref_logits(cfg, w, ids, mask)
                for mode in modes:
                    eng.set_group_split(mode)
                    got = eng.forward(ids, mask, c_alloc=ref.shape[1])
                    assert got.shape == ref.shape and np.isfinite(got).all()
                    if ref.size:
                        assert np.abs(sig(got) - sig(ref)).max() <= TOL_PROB[dtype], (cname, S, mode)
                    if mode == 2:
                        assert eng.last_group_split() == 1, (cname, S)
                    assert eng.last_mx() == 0 and eng.last_mx_attention() == 0
            with pytest.raises(RuntimeError):
                eng.set_mx(True)                   # no MX pipeline for this backbone
        finally:
            eng.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("W", [8, 50, 64, 200])
def test_window_edges(W, dtype, weights_for):
    """Ragged batches where the window crosses the key length inside a tile; the straightforward kernel (impl 1) agrees."""
    from gliclass.c_amd import synth, weights
    from gliclass.c_amd.engine import Engine
    base, _ = weights_for("mb-tiny")
    cfg = dataclasses.replace(base, layers=3, local_window=W, global_every=3)
    w = weights.make_weights(cfg, 21)
    eng = Engine(cfg, w, dtype=dtype)
    try:
        for S, seed in ((100, 1), (1000, 2)):
            ids, mask, _ = synth.make_inputs(cfg, 3, S, 3, seed=seed, ragged=True)
            ref = ref_logits(cfg, w, ids, mask)
            eng.set_attention_impl(0)
            got = eng.forward(ids, mask)
            assert np.abs(sig(got) - sig(ref)).max() <= TOL_PROB[dtype], (W, S)
            eng.set_attention_impl(1)
            simple = eng.forward(ids, mask)
            eng.set_attention_impl(0)
            assert np.abs(sig(simple) - sig(ref)).max() <= TOL_PROB[dtype], (W, S)
            assert np.abs(sig(simple) - sig(got)).max() <= TOL_PROB[dtype], (W, S)
    finally:
        eng.close()


def test_long_context(weights_for):
    """2 layers (full, sliding) of mb-mini at S = 8192; a window >= S - 1 gives the all-global answer (with one RoPE base for both layer
    kinds: W = 0 also puts the global base on every layer)."""
    from gliclass.c_amd import synth, weights
    from gliclass.c_amd.engine import Engine
    base, _ = weights_for("mb-mini")
    cfg = dataclasses.replace(base, layers=2, global_every=2)
    w = weights.make_weights(cfg, 5)
    ids, mask, _ = synth.make_inputs(cfg, 1, 8192, 4, seed=9)
    eng = Engine(cfg, w, dtype="f32")
    try:
        got = eng.forward(ids, mask)
        ref = modernbert_ref.forward(cfg, w, ids, mask, dtype=torch.float32)      # (fp64 scores at S = 8192 would take 4 GB per layer)
        assert np.abs(sig(got) - sig(ref)).max() <= 1e-4
    finally:
        eng.close()
    outs = []
    for W in (8191, 0):
        c2 = dataclasses.replace(cfg, local_window=W, rope_theta_local=cfg.rope_theta)
        eng = Engine(c2, w, dtype="f32")
        try:
            outs.append(eng.forward(ids, mask))
        finally:
            eng.close()
    assert np.abs(sig(outs[0]) - sig(outs[1])).max() <= 1e-5


def test_length_bucketing_rows_identical(weights_for):
    from gliclass.c_amd import synth
    from gliclass.c_amd.engine import Engine
    cfg, w = weights_for("mb-mini")
    ids, mask, _ = synth.make_inputs(cfg, 96, 2048, 3, seed=31)
    for b in range(32, 96):                  # 32 rows of 2048 tokens, 64 of 100 - 163: the planner splits the batch (3 waves of tiles -> 2)
        n = 100 + b
        ids[b, n:] = cfg.pad_id
        mask[b, n:] = 0
    eng = Engine(cfg, w, dtype="f32")
    try:
        eng.set_length_buckets(4)
        a = eng.forward(ids, mask)
        groups = eng.L.glc_debug_last_forward_groups(eng.h)
        eng.set_length_buckets(1)
        b = eng.forward(ids, mask)
        assert groups > 1
        assert np.abs(sig(a) - sig(b)).max() <= 1e-5
    finally:
        eng.close()


def test_full_size_base(c_generated_weights):
    from gliclass.c_amd import synth
    from gliclass.c_amd.config import CONFIGS
    from gliclass.c_amd.engine import Engine
    cfg = CONFIGS["modernbert-base"]
    w = c_generated_weights("synthetic:modernbert-base:42", cfg)
    ids, mask, _ = synth.make_inputs(cfg, 4, 1024, 4, seed=3, ragged=True)
    eng = Engine(cfg, w, dtype="f32")
    try:
        got = eng.forward(ids, mask)
        assert eng.last_mx() == 0
    finally:
        eng.close()
    ref = ref_logits(cfg, w, ids, mask)
    assert np.abs(sig(got) - sig(ref)).max() <= 1e-4


def test_large_falls_back_cleanly():
    """modernbert-large: 2I = 5248 is not a multiple of 256 — no fused GeGLU epilogue; the unfused path runs (one layer, small batch)."""
    from gliclass.c_amd import synth, weights
    from gliclass.c_amd.config import CONFIGS
    from gliclass.c_amd.engine import Engine
    cfg = dataclasses.replace(CONFIGS["modernbert-large"], vocab=1027, class_token_index=1025, text_token_index=1026, layers=2)
    w = weights.make_weights(cfg, 2)
    ids, mask, _ = synth.make_inputs(cfg, 2, 300, 3, seed=4, ragged=True)
    ref = ref_logits(cfg, w, ids, mask)
    for dtype in ("f32", "bf16"):
        eng = Engine(cfg, w, dtype=dtype)
        try:
            eng.set_group_split(2)
            got = eng.forward(ids, mask)
            assert np.abs(sig(got) - sig(ref)).max() <= TOL_PROB[dtype], dtype
        finally:
            eng.close()

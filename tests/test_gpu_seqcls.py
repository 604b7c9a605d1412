"""GPU (-m gpu): the sequence-classification head (head_kind = 1) — the transformers fixtures of tests/golden/seqcls through the engine in
every dtype, a shape sweep over six backbones against tests/seqcls_ref.py (pinned on those fixtures by tests/test_seqcls_host.py), the
head's variants, last-layer pruning, length buckets, graph replay, the zero-shot NLI reduction and the shape contract of the C-ABI.

Bars: softmax(logits) (sigmoid for K = 1) against the float64 reference within the BERT suite's 1e-4 / 1e-2 / 6e-2 (tests/test_gpu_bert.py);
the DeBERTa MX pipeline within the 5e-4 MX bar of DESIGN.md §2.  Run with -s for the worst errors (DESIGN.md §4i records them)."""
import ctypes as C
import dataclasses
import importlib.util
import os

import numpy as np
import pytest

import seqcls_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_PROB = {"f32": 1e-4, "f16": 1e-2, "bf16": 6e-2}
TOL_MX = 5e-4
FAMILIES = ("deberta", "bert", "roberta", "modernbert", "modernbert_mean")
# (config name, head fields): the arithmetic each backbone's HF class has
HEADS = {
    "tiny": dict(cls_act=2, cls_norm=0, cls_dense=1), "mini": dict(cls_act=2, cls_norm=0, cls_dense=1),
    "bert-tiny": dict(cls_act=1, cls_norm=0, cls_dense=1), "bert-mini": dict(cls_act=1, cls_norm=0, cls_dense=1),
    "mb-tiny": dict(cls_act=2, cls_norm=1, cls_dense=1), "mb-mini": dict(cls_act=2, cls_norm=1, cls_dense=1),      # (mb-mini pools 'avg')
}

_spec = importlib.util.spec_from_file_location("gen_seqcls_golden", os.path.join(ROOT, "scripts", "gen_seqcls_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

_HIDDEN = {}
_WORST = {}


def _cfg(cname, K, **over):
    from gliclass.c_amd.config import CONFIGS
    return dataclasses.replace(CONFIGS[cname], head_kind=1, cls_labels=K, **{**HEADS[cname], **over})


def _weights(cfg, seed=11, drop=()):
    from gliclass.c_amd import weights
    w = weights.make_weights(cfg, seed)
    for n in drop:
        del w[n]
    return w


def _inputs(cfg, B, S, ragged_pads=False):
    """ragged rows; ragged_pads: a left-padded row with 'avg' pooling, pad runs inside rows 0 and 2 on the BERT backbone"""
    from gliclass.c_amd.config import BACKBONE_BERT, POOL_AVG
    on = ragged_pads and B > 1 and S > 20
    return gen.make_case(cfg, B, S, 100 * B + S, left=(1, 9) if on and cfg.pooling == POOL_AVG else None,
                         holes=((0, 10, 15), (2, 5, 8)) if on and cfg.backbone == BACKBONE_BERT else ())


def _hidden(cname, cfg, w, B, S, lpad=False):
    """the reference backbone's rows, once per (config, shape): every K and every head variant shares them"""
    key = (cname, B, S, lpad)
    if key not in _HIDDEN:
        ids, mask = _inputs(cfg, B, S, lpad)
        _HIDDEN[key] = (ids, mask, seqcls_ref.last_hidden(cfg, w, ids, mask))
    return _HIDDEN[key]


def _err(got, ref):
    return float(np.abs(seqcls_ref.probs(got) - seqcls_ref.probs(ref)).max())


def _note(tag, err):
    _WORST[tag] = max(_WORST.get(tag, 0.0), err)
    print(f"worst |prob - ref| so far, {tag}: {_WORST[tag]:.2e}")


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("family", FAMILIES)
def test_fixtures(family, dtype, golden_dir):
    """The transformers fixture models through the engine: against the reference (the asserted bar) and, printed, HF's own float32 logits."""
    from gliclass.c_amd.engine import Engine
    z = np.load(os.path.join(golden_dir, "seqcls", family + ".npz"))
    cfg = gen.family_config(family)
    w = gen.family_weights(family, cfg, int(z["seed"]))
    eng = Engine(cfg, w, dtype=dtype)
    try:
        assert eng.num_labels() == cfg.cls_labels
        for name in z["case_names"]:
            ids, mask = z[name + ".ids"].astype(np.int64), z[name + ".mask"].astype(np.int64)
            ref = seqcls_ref.forward(cfg, w, ids, mask)
            got = eng.forward(ids, mask)
            assert got.shape == ref.shape == z[name + ".logits"].shape and np.isfinite(got).all() and eng.last_c == cfg.cls_labels
            err = _err(got, ref)
            print(f"{family} {name} {dtype}: |prob - ref| = {err:.2e}, |prob - HF| = {_err(got, z[name + '.logits']):.2e}")
            _note(f"fixtures {dtype}", err)
            assert err <= TOL_PROB[dtype], (family, name, dtype, err)
    finally:
        eng.close()


@pytest.mark.parametrize("K", [1, 2, 3, 7, 65, 1024])
@pytest.mark.parametrize("cname", list(HEADS))
def test_shape_sweep(cname, K):
    """B in {1, 3} x S in {1, 33, 130} (one row, a tile edge, two query tiles), ragged rows; on mb-mini a left-padded row under the masked
    mean; on the BERT configs (RoBERTa position ids) pad runs inside two rows, which move the position ids of everything behind them while
    the pooled token stays attended; K up to the cap; H = 128 on the plain pipeline and H = 256 on the plain and the group-split pipeline
    (bert-mini, mb-mini: split-f16 arithmetic, the f32 bar; mini: its group-split pipeline is the MX arithmetic, held to the MX bar)."""
    from gliclass.c_amd.engine import Engine
    cfg = _cfg(cname, K)
    w = _weights(cfg)
    eng = Engine(cfg, w, dtype="f32")
    try:
        for B in (1, 3):
            for S in (1, 33, 130):
                ids, mask, hid = _hidden(cname, cfg, w, B, S, True)
                ref = seqcls_ref.head(cfg, w, hid, mask)
                for mode in ((1, 2) if cfg.hidden == 256 else (1,)):
                    eng.set_group_split(mode)
                    got = eng.forward(ids, mask)
                    assert got.shape == (B, K) and np.isfinite(got).all()
                    err = _err(got, ref)
                    _note(f"sweep f32 {cname} {'MX' if eng.last_mx() else 'group-split' if eng.last_group_split() else 'plain'}", err)
                    # (mini with the group-split pipeline forced runs the MX pipeline: its own bar)
                    assert err <= (TOL_MX if eng.last_mx() else TOL_PROB["f32"]), (cname, K, B, S, mode, err)
    finally:
        eng.close()


def test_deberta_mx_pipeline():
    """mini at B = 3, S = 100 with the group-split pipeline forced takes the MX pipeline (tests/test_gpu_mx_small.py reaches it the same way)"""
    from gliclass.c_amd.engine import Engine
    cfg = _cfg("mini", 3)
    w = _weights(cfg)
    ids, mask = _inputs(cfg, 3, 100)
    ref = seqcls_ref.forward(cfg, w, ids, mask)
    eng = Engine(cfg, w, dtype="f32")
    try:
        eng.set_length_buckets(1)
        eng.set_group_split(2)
        got = eng.forward(ids, mask)
        assert eng.last_mx() == 1 and eng.last_pruned() == 1
        err = _err(got, ref)
        _note("mini MX pipeline", err)
        assert err <= TOL_MX
    finally:
        eng.close()


@pytest.mark.parametrize("variant", ["no_dense", "no_dense_no_act", "norm_without_bias", "no_classifier_bias", "no_dense_bias"])
def test_variants(variant):
    from gliclass.c_amd.engine import Engine
    over, drop = {
        "no_dense": (dict(cls_dense=0), ()), "no_dense_no_act": (dict(cls_dense=0, cls_act=0), ()),
        "norm_without_bias": ({}, ("cls.norm.bias",)), "no_classifier_bias": ({}, ("cls.classifier.bias",)), "no_dense_bias": ({}, ("cls.dense.bias",)),
    }[variant]
    cfg = _cfg("mb-tiny", 7, **over)
    w = _weights(cfg, drop=drop)
    ids, mask, hid = _hidden("mb-tiny", cfg, w, 3, 33)
    ref = seqcls_ref.head(cfg, w, hid, mask)
    full = seqcls_ref.head(_cfg("mb-tiny", 7), _weights(_cfg("mb-tiny", 7)), hid, mask)
    assert np.abs(ref - full).max() > 1e-2, "the variant does not change the reference: the test would show nothing"
    eng = Engine(cfg, w, dtype="f32")
    try:
        err = _err(eng.forward(ids, mask), ref)
        _note("variants f32", err)
        assert err <= TOL_PROB["f32"], (variant, err)
    finally:
        eng.close()


@pytest.mark.parametrize("cname,pruned", [("tiny", 1), ("mb-tiny", 1), ("mb-mini", 0), ("bert-tiny", 0)])
def test_pruning(cname, pruned):
    """'first' pooling on DeBERTa and ModernBERT: the last layer runs on the B pooled rows (the existing pruned path with no class rows) and
    agrees with the unpruned forward; 'avg' pooling (mb-mini) and the BERT backbone: never pruned."""
    from gliclass.c_amd.engine import Engine
    cfg = _cfg(cname, 3)
    w = _weights(cfg)
    ids, mask = _inputs(cfg, 3, 130)
    eng = Engine(cfg, w, dtype="f32")
    try:
        a = eng.forward(ids, mask)
        assert eng.last_pruned() == pruned
        eng.set_prune_last_layer(False)
        b = eng.forward(ids, mask)
        assert eng.last_pruned() == 0
        assert _err(a, b) <= TOL_PROB["f32"]
    finally:
        eng.close()


def _bucket_batch(cfg):
    """32 rows of 2048 tokens, 64 of 132 - 195: the planner splits the batch (the shape tests/test_gpu_bert.py and test_gpu_modernbert_mx.py use)"""
    rng = np.random.default_rng(5)
    B, S = 96, 2048
    ids = rng.integers(3, cfg.vocab - 2, (B, S)).astype(np.int64)
    mask = np.ones((B, S), np.int64)
    ids[:, 0] = cfg.cls_id
    for b in range(32, B):
        mask[b, 100 + b:] = 0
    ids[mask == 0] = cfg.pad_id
    return ids, mask


def _bucketed_against_single(eng, ids, mask):
    """-> (probability distance between the bucketed and the single forward, group-split flags of the two runs)"""
    eng.set_length_buckets(4)
    a = eng.forward(ids, mask)
    assert eng.L.glc_debug_last_forward_groups(eng.h) > 1
    gs_a = eng.last_group_split()
    eng.set_length_buckets(1)
    b = eng.forward(ids, mask)
    return _err(a, b), (gs_a, eng.last_group_split())


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("cname", ["mini", "bert-mini", "mb-mini"])
def test_length_buckets_rows_identical(cname, mode):
    """A row's logits do not depend on the group it ran in: 1e-5, the bar of tests/test_gpu_modernbert_mx.py::test_length_buckets_same_rows,
    and arranged as that test arranges it — every group on ONE pipeline (there: set_group_split(2) with MX on).  Here both pinned pipelines
    run: mode 0, every group on the plain split-f16 kernels; mode 2, every group on the group-split pipeline (mini: the MX arithmetic)."""
    from gliclass.c_amd.engine import Engine
    cfg = _cfg(cname, 3)
    eng = Engine(cfg, _weights(cfg), dtype="f32")
    try:
        eng.set_group_split(mode)
        err, gs = _bucketed_against_single(eng, *_bucket_batch(cfg))
        print(f"buckets 4 against 1, {cname}, group split {mode}: {err:.2e}")
        assert gs == (mode == 2, mode == 2)
        assert err <= 1e-5
    finally:
        eng.close()


# the default mode picks the pipeline by the size of each forward (the fill rule, include/gliclass_hip.h): the project's own bars for the
# distance between the pipelines a group may land on
AUTO_BUCKET_TOL = {"mini": TOL_MX, "bert-mini": TOL_PROB["f32"], "mb-mini": TOL_PROB["f32"]}


@pytest.mark.parametrize("cname", ["mini", "bert-mini", "mb-mini"])
def test_length_buckets_default_mode(cname):
    """The same batch with the pipeline left on auto, the mode users run.  The groups of one batch then pick their pipeline by their own size:
    the 32 long rows (and all 96 together) fill the device and run the group-split pipeline, the 64 short rows run the plain kernels, so a
    short row is compared across two arithmetics.  The bar is the project's bar for that distance, not for bucket membership: on the DeBERTa
    backbone the group-split pipeline of an fp32 engine is the MX arithmetic (~4e-5 from the reference against the split-f16 kernels'
    ~1e-5), and tests/test_gpu_parity.py::test_length_bucketing_preserves_results holds exactly this comparison to TOL_MX =
    5e-4; on the BERT and ModernBERT backbones both pipelines are split-f16 arithmetic with different rounding points, and
    tests/test_gpu_bert.py::_check holds "the two pipelines agree with each other" to the f32 bar, 1e-4.  (Measured at these shapes: 7.2e-5
    on mini, 1.1e-5 on bert-mini, 6e-6 on mb-mini; the GLiClass-head tests of the two latter backbones happen to stay under 1e-5.)"""
    from gliclass.c_amd.engine import Engine
    cfg = _cfg(cname, 3)
    eng = Engine(cfg, _weights(cfg), dtype="f32")
    try:
        err, gs = _bucketed_against_single(eng, *_bucket_batch(cfg))
        print(f"buckets 4 against 1, {cname}, default mode (group split of the last group / the single forward: {gs}): {err:.2e}")
        assert err <= AUTO_BUCKET_TOL[cname]
    finally:
        eng.close()


@pytest.mark.parametrize("cname,dtype", [("tiny", "f32"), ("bert-tiny", "f32"), ("mb-mini", "f32"), ("mb-tiny", "bf16")])
def test_graph_replay_bit_identical(cname, dtype):
    from gliclass.c_amd.engine import Engine
    cfg = _cfg(cname, 7)
    w = _weights(cfg)
    ids, mask = _inputs(cfg, 3, 70)
    eng = Engine(cfg, w, dtype=dtype)
    try:
        eager = eng.forward(ids, mask)
        eng.set_graph_replay(True)
        states = []
        for _ in range(3):
            got = eng.forward(ids, mask)
            states.append(eng.last_graph())
            assert np.array_equal(got, eager)
        assert states == [0, 1, 2]
    finally:
        eng.close()


def test_profiler_head_class():
    from gliclass.c_amd.engine import Engine
    cfg = _cfg("bert-tiny", 3)
    eng = Engine(cfg, _weights(cfg), dtype="f16")
    try:
        eng.profile(True)
        eng.forward(*_inputs(cfg, 3, 33))
        assert eng.profile_read()["head"][1] == 1
    finally:
        eng.close()


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)])        # (entailment, neutral, contradiction) ids, both ways round
@pytest.mark.parametrize("Lb", [1, 4])
@pytest.mark.parametrize("multi_label", [0, 1])
def test_nli_scores(order, Lb, multi_label):
    """T = 3 texts x Lb labels as one pair batch through an NLI-shaped engine (K = 3), then the device reduction against the float64
    restatement of the pipeline's postprocess.  Bar 1e-6: an fp32 softmax over at most four values — the exp2 arguments are (x - max) log2(e)
    <= 0, rounded to <= 2^-24 relative, |x - max| <= ~10 for these logits, so each exponential is within ~1e-6 relative of the exact one and
    every probability (<= 1, a ratio of such terms) within a few 1e-7 absolute.
    The max subtraction: logits of magnitude 100 and more (fp32 exp overflows above 88.7 and flushes below -103), with entailment and
    contradiction columns that differ by 0.5 .. 1.25 in every row and label logits 0.75 apart — without the subtraction every result is
    inf / inf or 0 / 0; with it the probabilities are ordinary numbers (0.05 .. 0.78), held to the same bar."""
    from gliclass.c_amd.engine import Engine
    T, (en, _, co) = 3, order
    cfg = _cfg("bert-tiny", 3)
    eng = Engine(cfg, _weights(cfg), dtype="f32")
    try:
        ids, mask = _inputs(cfg, T * Lb, 33)
        logits = eng.forward(ids, mask)
        got = eng.nli_scores(logits, T, Lb, en, co, multi_label)
        ref = seqcls_ref.nli_scores(logits, T, Lb, en, co, multi_label)
        assert got.shape == (T, Lb) and np.abs(got - ref).max() <= 1e-6
        if not multi_label:
            assert np.abs(got.sum(1) - 1).max() <= 1e-6
        r = np.arange(T * Lb, dtype=np.float64)
        for sign in (1.0, -1.0):
            big = np.zeros((T * Lb, 3), np.float32)
            big[:, en] = sign * 120.0 - 0.75 * (r % Lb)
            big[:, co] = big[:, en] + np.where(r % 3 == 0, -1.25, 0.5)
            big[:, 1] = -sign * 150.0
            got = eng.nli_scores(big, T, Lb, en, co, multi_label)
            ref = seqcls_ref.nli_scores(big, T, Lb, en, co, multi_label)
            assert np.isfinite(got).all() and np.abs(got - ref).max() <= 1e-6
            assert 0.03 < ref.min() and (Lb == 1 and not multi_label or ref.max() < 0.95)      # ordinary probabilities, not saturated ones
    finally:
        eng.close()


def test_shape_contract_and_no_shared_state(weights_for):
    from gliclass.c_amd import synth
    from gliclass.c_amd.engine import Engine
    import bert_ref
    cfg = _cfg("bert-tiny", 3)
    eng = Engine(cfg, _weights(cfg), dtype="f32")
    try:
        ids, mask = _inputs(cfg, 2, 33)
        with pytest.raises(RuntimeError, match="c_alloc = 2 is too small"):
            eng.forward(ids, mask, c_alloc=2)
        wide = eng.forward(ids, mask, c_alloc=5)
        assert eng.last_c == 3 and wide.shape == (2, 5) and np.array_equal(wide[:, :3], eng.forward(ids, mask))
        d = eng.dev_alloc(8 * ids.size)
        try:
            with pytest.raises(RuntimeError, match="must equal cls_labels"):
                eng.forward_device(d, d, 2, 33, 2, d)
        finally:
            eng.dev_free(d)
        one = Engine(_cfg("bert-tiny", 1), _weights(_cfg("bert-tiny", 1)), dtype="f32")
        try:
            with pytest.raises(RuntimeError, match="cls_labels >= 2"):
                one.nli_scores(np.zeros((2, 1), np.float32), 2, 1, 0, 0)
        finally:
            one.close()
        with pytest.raises(RuntimeError, match="must name one of the K labels"):
            eng.nli_scores(np.zeros((2, 3), np.float32), 2, 1, 3, 0)
        # a GLiClass-head engine of the same backbone, created afterwards: refuses nli_scores, and still agrees with its reference
        base, w = weights_for("bert-tiny")
        gl = Engine(base, w, dtype="f32")
        try:
            assert gl.num_labels() == 0
            dl = gl.dev_alloc(64)
            try:
                assert gl.L.glc_engine_nli_scores(gl.h, dl, 1, 1, 0, 1, 0, dl) == -1 and b"GLiClass head" in gl.L.glc_last_error()
            finally:
                gl.dev_free(dl)
            gi, gm, _ = synth.make_inputs(base, 3, 65, 2, seed=65, ragged=True)
            gi[gm == 0] = base.pad_id
            ref = bert_ref.forward(base, w, gi, gm)
            got = gl.forward(gi, gm, c_alloc=ref.shape[1])
            sig = lambda x: 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))
            assert np.abs(sig(got) - sig(ref)).max() <= TOL_PROB["f32"]
        finally:
            gl.close()
    finally:
        eng.close()


@pytest.mark.parametrize("cname,word", [("dec-tiny", "decoder"), ("t5-tiny", "T5")])
def test_decoder_and_t5_refused(cname, word, weights_for):
    """(also in tests/test_seqcls_host.py: the refusal comes before the engine looks for a device)"""
    from gliclass.c_amd import _lib
    from gliclass.c_amd.engine import to_c_config
    base, _ = weights_for(cname)
    cc = to_c_config(base)
    cc.head_kind, cc.cls_labels, cc.cls_act, cc.cls_dense = 1, 3, 1, 1
    L = _lib.hip()
    ptrs = (C.c_void_p * 1)()
    assert not L.glc_engine_create(C.byref(cc), ptrs, 1, 0, 0)
    assert word.encode() in L.glc_last_error() and b"head_kind" in L.glc_last_error()


@pytest.mark.parametrize("family", FAMILIES)
def test_checkpoint_directory_through_the_c_host_layer(family, tmp_path, golden_dir):
    """The directory an HF *ForSequenceClassification model saves, through the C host layer: create_ort_session on the directory (the C
    checkpoint reader), prepare_input_tensors, run_inference -> an OrtValue [B, K] within the f32 bar of the reference; a version-7 blob of
    the same model and Engine.from_spec on both give bit-identical logits (one weight source, one engine)."""
    pytest.importorskip("safetensors")
    from gliclass.c_amd import _lib, weights
    from gliclass.c_amd.engine import Engine
    z = np.load(os.path.join(golden_dir, "seqcls", family + ".npz"))
    cfg = gen.family_config(family)
    w = gen.family_weights(family, cfg, int(z["seed"]))
    model = gen.build_hf(family, cfg, w)
    model.config.architectures = [type(model).__name__]
    ckpt = tmp_path / "ckpt"
    model.save_pretrained(str(ckpt), safe_serialization=True)
    blob = str(tmp_path / "model.glcw")
    weights.write_blob(blob, cfg, w)
    name = str(z["case_names"][1])
    ids, mask = z[name + ".ids"].astype(np.int64), z[name + ".mask"].astype(np.int64)
    B, S = ids.shape
    ref = seqcls_ref.forward(cfg, w, ids, mask)
    m = _lib.model()
    os.environ["GLICLASS_DTYPE"] = "f32"
    try:
        m.initialize_ort_api()
        outs = []
        for spec in (str(ckpt), blob):
            sess = m.create_ort_session(m.initialize_ort_environment(), spec.encode(), 8)
            assert sess, spec
            i32, m32 = ids.astype(np.int32), mask.astype(np.int32)
            rows_i = (C.POINTER(C.c_int) * B)(*[i32[b].ctypes.data_as(C.POINTER(C.c_int)) for b in range(B)])
            rows_m = (C.POINTER(C.c_int) * B)(*[m32[b].ctypes.data_as(C.POINTER(C.c_int)) for b in range(B)])
            tok = _lib.TokenizedInputs(rows_i, rows_i, rows_m, B, S)
            a, b = C.POINTER(_lib.OrtValue)(), C.POINTER(_lib.OrtValue)()
            assert m.prepare_input_tensors(C.byref(tok), C.byref(a), C.byref(b)) == 0
            out = m.run_inference(sess, a, b)
            assert out and list(out.contents.dims[:2]) == [B, cfg.cls_labels], spec
            got = np.ctypeslib.as_array(C.cast(out.contents.data, C.POINTER(C.c_float)), shape=ref.shape).copy()
            assert _err(got, ref) <= TOL_PROB["f32"], (spec, _err(got, ref))
            assert _err(got, z[name + ".logits"]) <= TOL_PROB["f32"]          # ... and of transformers' own logits
            outs.append(got)
        for spec in (str(ckpt), blob):
            eng = Engine.from_spec(cfg, spec, dtype="f32")
            try:
                assert eng.num_labels() == cfg.cls_labels
                outs.append(eng.forward(ids, mask))
            finally:
                eng.close()
        assert all(np.array_equal(o, outs[0]) for o in outs[1:])
    finally:
        del os.environ["GLICLASS_DTYPE"]

"""GPU (-m gpu): exact pruning of the last layer on the decoder and ModernBERT backbones (engine.hip run_pruned_tail): the rows the head
reads — the pooled row of every sequence and its class tokens — go through attention output, o-projection, gated FFN and final norm as
R = B (1 + C) compact rows; the attention runs on the 32-query tiles that hold one (the tile flag of the grouped-query kernels).

Three answers must agree everywhere: the forward with the switch on (Engine.last_pruned() == 1), with it off (== 0) and the CPU
restatements tests/decoder_ref.py / tests/modernbert_ref.py in float64.  Every bound is one the decoder, Qwen3 and ModernBERT suites
already hold the engine to against those references — TOL_PROB per operand type, and for f32 forwards that ran the MX pipeline the
decoder suite's 5e-4 — and pruned against unpruned uses the same figure: nothing here is taken from the code under test.

mb-mini pools by average, which is never pruned; where a test needs mb-mini's shapes on the pruned path it runs them with first-token
pooling (the tensors do not depend on the pooling)."""
import dataclasses

import numpy as np
import pytest
import torch

import decoder_ref
import modernbert_ref

pytestmark = pytest.mark.gpu

TOL_PROB = {"f32": 1e-4, "f16": 1e-2, "bf16": 6e-2}      # tests/test_gpu_decoder.py, test_gpu_qwen3.py, test_gpu_modernbert.py
TOL_PROB_MX = 5e-4                                       # tests/test_gpu_decoder.py: f32 forwards on the MX pipeline against the oracle
SMALL = ("dec-tiny", "q3-mini", "ll-tiny", "mb-tiny", "mb-mini")


def sig(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def perr(a, b):
    return float(np.abs(sig(a) - sig(b)).max()) if np.size(a) else 0.0


def small(cname, weights_for):
    from gliclass.c_amd.config import POOL_AVG, POOL_FIRST
    cfg, w = weights_for(cname)
    if cfg.pooling == POOL_AVG:
        cfg = dataclasses.replace(cfg, pooling=POOL_FIRST)
    return cfg, w


_REFS = {}


def reference(cfg, w, ids, mask):
    """float64 logits of the CPU restatement, computed once per (config, tensors, batch) and shared by the operand types"""
    from gliclass.c_amd.config import BACKBONE_DECODER
    key = (cfg, float(np.asarray(w["text_projector.linear_1.weight"]).ravel()[:64].sum()), ids.tobytes(), mask.tobytes())
    if key not in _REFS:
        mod = decoder_ref if cfg.backbone == BACKBONE_DECODER else modernbert_ref
        _REFS[key] = mod.forward(cfg, w, ids, mask, dtype=torch.float64)
    return _REFS[key]


def place(cfg, S, lens, cls_pos, seed):
    """Rows with their class tokens at chosen positions: [CLS] at 0, <<LABEL>> at cls_pos[b], [SEP] at lens[b] - 1, padding behind."""
    from gliclass.c_amd import prng
    B = len(lens)
    ids = prng.randint(seed, "ids", B * S, 3, cfg.vocab - 2).reshape(B, S).astype(np.int64)
    mask = np.zeros((B, S), np.int64)
    for b in range(B):
        n = lens[b]
        assert all(0 < p < n - 1 for p in cls_pos[b]) or n <= 2
        ids[b, 0] = cfg.cls_id
        ids[b, list(cls_pos[b])] = cfg.class_token_index
        ids[b, n - 1] = cfg.sep_id
        ids[b, n:] = cfg.pad_id
        mask[b, :n] = 1
    return ids, mask


def three_way(eng, cfg, w, ids, mask, tol, ref=None, c_alloc=None, what=""):
    """pruned, unpruned and the reference agree within tol; the getter says which forward ran.  -> (pruned, unpruned)"""
    if ref is None:
        ref = reference(cfg, w, ids, mask)
    eng.set_prune_last_layer(True)
    on = eng.forward(ids, mask, c_alloc=c_alloc)
    assert eng.last_pruned() == 1, what
    eng.set_prune_last_layer(False)
    off = eng.forward(ids, mask, c_alloc=c_alloc)
    assert eng.last_pruned() == 0, what
    eng.set_prune_last_layer(True)
    assert np.isfinite(on).all() and np.isfinite(off).all(), what
    k = ref.shape[1]
    e_on, e_off, e_oo = perr(on[:, :k], ref), perr(off[:, :k], ref), perr(on, off)
    print(what, "pruned vs reference", e_on, "unpruned vs reference", e_off, "pruned vs unpruned", e_oo)
    assert e_on <= tol and e_off <= tol and e_oo <= tol, what
    return on, off


_RAGGED = {}


def ragged_cases(cname, weights_for):
    """B = 3, C = 3, S in {1, 33, 100, 1000}, ragged, rows with 3 / 1 / 2 class tokens; the float64 reference once per config."""
    from gliclass.c_amd import synth
    if cname not in _RAGGED:
        cfg, w = small(cname, weights_for)
        out = []
        for S in (1, 33, 100, 1000):
            ids, mask, _ = synth.make_inputs(cfg, 3, S, 3, seed=100 + S, ragged=True, labels_per_row=[3, 1, 2])
            out.append((ids, mask, reference(cfg, w, ids, mask)))
        _RAGGED[cname] = (cfg, w, out)
    return _RAGGED[cname]


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("cname", SMALL)
def test_pruned_equals_unpruned_equals_reference(cname, dtype, weights_for):
    """Every small config and operand type.  S = 1 holds no class token (the reference has no column there): the engine runs it with
    C = 3 absent classes, pruned against unpruned."""
    from gliclass.c_amd.engine import Engine
    cfg, w, cases = ragged_cases(cname, weights_for)
    eng = Engine(cfg, w, dtype=dtype)
    try:
        for (ids, mask, ref) in cases:
            S = ids.shape[1]
            assert S == 1 or (ids == cfg.class_token_index).sum(1).min() < 3
            three_way(eng, cfg, w, ids, mask, TOL_PROB[dtype], ref=ref, c_alloc=3, what=f"{cname} {dtype} S={S}")
    finally:
        eng.close()


@pytest.mark.parametrize("variant", ["decoder-last", "decoder-first", "modernbert-first", "modernbert-last"])
def test_pooling_first_and_last(variant, weights_for):
    from gliclass.c_amd import synth, weights
    from gliclass.c_amd.config import POOL_FIRST, POOL_LAST
    from gliclass.c_amd.engine import Engine
    dec, mb = weights_for("dec-tiny")[0], weights_for("mb-tiny")[0]
    cfg = {"decoder-last": dec, "decoder-first": dataclasses.replace(dec, pooling=POOL_FIRST, causal=0),
           "modernbert-first": mb, "modernbert-last": dataclasses.replace(mb, pooling=POOL_LAST)}[variant]
    w = weights.make_weights(cfg, 7)
    ids, mask, _ = synth.make_inputs(cfg, 3, 300, 3, seed=3, ragged=True, labels_per_row=[3, 0, 2])
    assert mask.sum(1).min() < 300
    for dtype in ("f32", "f16"):
        eng = Engine(cfg, w, dtype=dtype)
        try:
            three_way(eng, cfg, w, ids, mask, TOL_PROB[dtype], what=f"{variant} {dtype}")
        finally:
            eng.close()


@pytest.mark.parametrize("cname", ["dec-tiny", "mb-mini"])
def test_average_pooling_and_keep_hidden_are_never_pruned(cname, weights_for):
    from gliclass.c_amd import synth
    from gliclass.c_amd.config import POOL_AVG
    from gliclass.c_amd.engine import Engine
    base, w = weights_for(cname)
    avg = dataclasses.replace(base, pooling=POOL_AVG)
    ids, mask, _ = synth.make_inputs(avg, 3, 100, 3, seed=5, ragged=True)
    eng = Engine(avg, w, dtype="f32")
    try:
        outs = []
        for on in (True, False):
            eng.set_prune_last_layer(on)
            outs.append(eng.forward(ids, mask))
            assert eng.last_pruned() == 0
        assert np.array_equal(outs[0], outs[1])
        assert perr(outs[0], reference(avg, w, ids, mask)) <= TOL_PROB["f32"]
    finally:
        eng.close()
    cfg, w = small(cname, weights_for)
    eng = Engine(cfg, w, dtype="f32")
    try:
        eng.set_prune_last_layer(True)
        eng.forward(ids, mask)
        assert eng.last_pruned() == 1
        eng.keep_hidden(True)
        kept = eng.forward(ids, mask)
        assert eng.last_pruned() == 0
        eng.keep_hidden(False)
        assert perr(kept, reference(cfg, w, ids, mask)) <= TOL_PROB["f32"]
    finally:
        eng.close()


# S = 1000 (32 query tiles): where the selected rows fall.  (lens, class-token positions per row)
_SCATTER = {
    "one-tile": ((1000, 517, 770), ((1, 4, 7), (2, 30), (5, 9, 31))),                 # first pooling: every selected row in tile 0
    "several-tiles": ((1000, 640, 333), ((5, 200, 700), (40, 333, 600), (100, 320))),
    "last-tile-only": ((1000, 1000, 999), ((993, 995, 997), (992, 996), (994, 995, 996))),     # last pooling: nothing outside rows 992 .. 999
    "tile-boundaries": ((1000, 32, 33, 64), ((31, 32, 63), (3, 7), (31,), (32, 33, 62))),      # pooled rows klen - 1 = 31, 32, 63; class tokens on both sides
}


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("case", sorted(_SCATTER))
@pytest.mark.parametrize("cname", ["dec-tiny", "mb-tiny"])
def test_scattered_tiles(cname, case, dtype, weights_for):
    """dec-tiny pools the last attended token (causal: a late row walks every key tile before it), mb-tiny the first token (tile 0 is
    always flagged; its last layer is global)."""
    from gliclass.c_amd.engine import Engine
    cfg, w = small(cname, weights_for)
    lens, cls_pos = _SCATTER[case]
    ids, mask = place(cfg, 1000, lens, cls_pos, seed=17)
    eng = Engine(cfg, w, dtype=dtype)
    try:
        three_way(eng, cfg, w, ids, mask, TOL_PROB[dtype], what=f"{cname} {case} {dtype}")
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("W", [8, 64])
@pytest.mark.parametrize("layers", [3, 4])
def test_modernbert_windows(layers, W, dtype, weights_for):
    """layers = 3, global_every = 3: the pruned last layer is a local one (windowed kernel with the flag); layers = 4: a global one."""
    from gliclass.c_amd import synth, weights
    from gliclass.c_amd.engine import Engine
    base, _ = weights_for("mb-tiny")
    cfg = dataclasses.replace(base, layers=layers, local_window=W, global_every=3)
    assert cfg.is_global_layer(layers - 1) == (layers == 4)
    w = weights.make_weights(cfg, 21)
    eng = Engine(cfg, w, dtype=dtype)
    try:
        for S, seed in ((100, 1), (1000, 2)):
            ids, mask, _ = synth.make_inputs(cfg, 3, S, 3, seed=seed, ragged=True, labels_per_row=[3, 2, 3])
            three_way(eng, cfg, w, ids, mask, TOL_PROB[dtype], what=f"layers={layers} W={W} S={S} {dtype}")
        # class tokens deep in the sequence: their windows lie inside it, and across the key length of the short rows
        ids, mask = place(cfg, 1000, (1000, 530, 77), ((300, 511, 990), (520, 527), (70, 75)), seed=23)
        three_way(eng, cfg, w, ids, mask, TOL_PROB[dtype], what=f"layers={layers} W={W} placed {dtype}")
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cname", ["dec-tiny", "mb-tiny"])
def test_more_than_one_compact_tile(cname, dtype, weights_for):
    """B = 40, C = 7, S = 64: R = 320 compact rows on a 512-row grid."""
    from gliclass.c_amd import synth
    from gliclass.c_amd.engine import Engine
    cfg, w = small(cname, weights_for)
    lpr = [7 - (b % 3) for b in range(40)]
    ids, mask, _ = synth.make_inputs(cfg, 40, 64, 7, seed=29, ragged=True, labels_per_row=lpr)
    eng = Engine(cfg, w, dtype=dtype)
    try:
        three_way(eng, cfg, w, ids, mask, TOL_PROB[dtype], what=f"{cname} R=320 {dtype}")
    finally:
        eng.close()


@pytest.mark.parametrize("head_dim", [64, 128])
def test_every_flagged_kernel_is_reached(head_dim, weights_for):
    """fp32 decoder at both head dimensions, the shapes at which tests/test_gpu_decoder.py gets the MX attention: the split-f16
    kernel off and on the group-split pipeline, the MX ring kernel, the MX projections with split-f16 attention, and the
    straightforward kernel (unpruned attention, compact rows behind it).  The 16-bit forms and the windowed kernel run in the tests above;
    the per-wave MX kernel is reachable in developer builds only."""
    from gliclass.c_amd import synth, weights
    from gliclass.c_amd.engine import Engine
    base, _ = weights_for("dec-tiny")
    cfg = dataclasses.replace(base, head_dim=64, heads=4, kv_heads=2, layers=2) if head_dim == 64 else base
    w = weights.make_weights(cfg, 11)
    B, S = (3, 150) if head_dim == 64 else (3, 100)
    ids, mask, _ = synth.make_inputs(cfg, B, S, 3, seed=1, ragged=True, labels_per_row=[3, 1, 2])
    ref = reference(cfg, w, ids, mask)
    eng = Engine(cfg, w, dtype="f32")
    try:
        eng.set_group_split(0)
        three_way(eng, cfg, w, ids, mask, TOL_PROB["f32"], ref=ref, what="plain rows, split-f16 attention")
        assert not eng.last_group_split() and not eng.last_mx()
        eng.set_group_split(2)
        eng.set_mx(False)
        three_way(eng, cfg, w, ids, mask, TOL_PROB["f32"], ref=ref, what="group split, folded norms")
        assert eng.last_group_split() and eng.last_ln_folded() and not eng.last_mx()
        eng.set_ln_fused(False)
        three_way(eng, cfg, w, ids, mask, TOL_PROB["f32"], ref=ref, what="group split, norms unfused")
        assert eng.last_group_split() and not eng.last_ln_folded()
        eng.set_ln_fused(True)
        eng.set_mx(True)
        three_way(eng, cfg, w, ids, mask, TOL_PROB_MX, ref=ref, what="MX pipeline, ring attention")
        assert eng.last_mx() and eng.last_mx_attention()
        eng.set_mx_attention(False)
        three_way(eng, cfg, w, ids, mask, TOL_PROB_MX, ref=ref, what="MX projections, split-f16 attention")
        assert eng.last_mx() and not eng.last_mx_attention()
        eng.set_mx_attention(True)
        eng.set_group_split(1)
        eng.set_attention_impl(1)
        three_way(eng, cfg, w, ids, mask, TOL_PROB["f32"], ref=ref, what="straightforward attention")
        eng.set_attention_impl(0)
    finally:
        eng.close()


def test_length_buckets_prune_each_group():
    """The shape idea of test_gpu_modernbert.py::test_length_bucketing_rows_identical at about a quarter of its rows (40 x 1024 against
    96 x 2048), on a decoder wide enough for the planner to split it (hidden 2048: 8 rows of 1024 tokens fill one wave of tiles); its bound.
    The comparison is about bucketing, so both sides run one arithmetic: the split-f16 projections (a group below the MX pipeline's size
    threshold would otherwise differ from the whole batch by the MX format's rounding), and a short group (32 rows of <= 163 tokens, 6144
    padded rows) that is still large enough for the group-split pipeline with the folded norms which the whole batch takes — the plain
    small-forward path keeps the residual stream in another format and is held to 1e-4 against it by tests/test_gpu_decoder.py, not 1e-5."""
    from gliclass.c_amd import synth, weights
    from gliclass.c_amd.config import CONFIGS
    from gliclass.c_amd.engine import Engine
    cfg = dataclasses.replace(CONFIGS["dec-tiny"], hidden=2048)
    w = weights.make_weights(cfg, 3)
    ids, mask, _ = synth.make_inputs(cfg, 40, 1024, 3, seed=31)
    for b in range(8, 40):
        n = 100 + b
        ids[b, n:] = cfg.pad_id
        mask[b, n:] = 0
    eng = Engine(cfg, w, dtype="f32")
    try:
        eng.set_mx(False)
        eng.set_length_buckets(4)
        a = eng.forward(ids, mask)
        groups = eng.L.glc_debug_last_forward_groups(eng.h)
        assert eng.last_pruned() == 1 and eng.last_group_split(), "the short group left the group-split pipeline"
        eng.set_length_buckets(1)
        b = eng.forward(ids, mask)
        assert eng.last_pruned() == 1 and eng.last_group_split()
        assert groups > 1
        err = perr(a, b)
        print("buckets 4 against 1:", groups, "groups, probability difference", err)
        assert err <= 1e-5
    finally:
        eng.close()


@pytest.mark.parametrize("cname", ["dec-tiny", "mb-tiny"])
def test_device_resident_forward(cname, weights_for):
    from gliclass.c_amd import synth
    from gliclass.c_amd.engine import Engine
    cfg, w = small(cname, weights_for)
    B, S, Cn = 3, 200, 3
    ids, mask, _ = synth.make_inputs(cfg, B, S, Cn, seed=91, ragged=True, labels_per_row=[3, 1, 2])
    eng = Engine(cfg, w, dtype="f32")
    d_ids = d_mask = d_out = None
    try:
        eng.set_length_buckets(1)
        host = eng.forward(ids, mask, c_alloc=Cn)
        assert eng.last_pruned() == 1
        d_ids, d_mask, d_out = eng.dev_alloc(ids.nbytes), eng.dev_alloc(mask.nbytes), eng.dev_alloc(B * Cn * 4)
        eng.h2d(d_ids, ids); eng.h2d(d_mask, mask)
        eng.forward_device(d_ids, d_mask, B, S, Cn, d_out)
        eng.sync()
        assert eng.last_pruned() == 1
        got = np.zeros((B, Cn), np.float32)
        eng.d2h(got, d_out)
        assert np.array_equal(got, host)
        assert perr(got, reference(cfg, w, ids, mask)) <= TOL_PROB["f32"]
    finally:
        for p in (d_ids, d_mask, d_out):
            if p:
                eng.dev_free(p)
        eng.close()


def test_getter_on_the_encoder_and_on_null(weights_for):
    from gliclass.c_amd import synth
    from gliclass.c_amd.engine import Engine
    cfg, w = weights_for("tiny")
    ids, mask, _ = synth.make_inputs(cfg, 2, 96, 3, seed=7, ragged=True)
    eng = Engine(cfg, w, dtype="f32")
    try:
        assert eng.L.glc_debug_last_forward_pruned(None) == -1
        on = eng.forward(ids, mask)
        assert eng.last_pruned() == 1
        eng.set_prune_last_layer(False)
        off = eng.forward(ids, mask)
        assert eng.last_pruned() == 0
        assert perr(on, off) <= TOL_PROB["f32"]
    finally:
        eng.close()

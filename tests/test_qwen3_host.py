"""Host side (no GPU) of the Qwen3 / Llama decoder variants: the CPU restatement tests/decoder_ref.py against the transformers fixtures of
tests/golden/qwen3 and a live model, the two config fields in the blob header and the C-ABI, the named configs, the C weight source and
the checkpoint importer with its refusals."""
import ctypes as C
import dataclasses
import glob
import json
import os
import struct

import numpy as np
import pytest
import torch

import decoder_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q3_GOLDEN = os.path.join(ROOT, "tests", "golden", "qwen3")
Q3_CONFIGS = ("q3-tiny", "q3-mini", "ll-tiny", "qwen3-0.6b")
REF_TOL = 1e-5          # what the decoder oracle is pinned at


@pytest.fixture(scope="module")
def libs():
    from gliclass.c_amd import _lib
    return _lib, _lib.model()


def _fixtures():
    return sorted(glob.glob(os.path.join(Q3_GOLDEN, "*.npz")))


def _gen():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_q3", os.path.join(ROOT, "scripts", "gen_qwen3_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_fixture_set_is_complete():
    names = {os.path.basename(f)[:-4] for f in _fixtures()}
    assert names == {"q3_tiny_b2_s7", "q3_tiny_b3_s200", "q3_mini_b1_s7", "q3_mini_b2_s96", "q3_mini_b3_s200",
                     "ll_tiny_b2_s7", "ll_tiny_b2_s96", "ll_tiny_b3_s200"}


@pytest.mark.parametrize("path", _fixtures(), ids=lambda p: os.path.basename(p)[:-4])
def test_reference_matches_fixtures(path, weights_for):
    z = np.load(path)
    cfg, w = weights_for(str(z["config"]))
    ids, mask = z["ids"].astype(np.int64), z["mask"].astype(np.int64)
    logits, hs = decoder_ref.forward(cfg, w, ids, mask, dtype=torch.float64, want_hidden=True)
    pos = z["sample_pos"]
    got = hs[:, :, pos, : z["hidden_samples"].shape[-1]]
    att = mask[:, pos].astype(bool)                       # attended positions only
    e_h, e_l = np.abs(got - z["hidden_samples"])[:, att].max(), np.abs(logits - z["logits"]).max()
    print(os.path.basename(path), "hidden", e_h, "logits", e_l)
    assert e_h <= REF_TOL and e_l <= REF_TOL


@pytest.mark.parametrize("name", ["q3_tiny_b3_s200", "q3_mini_b2_s96"])
def test_fixtures_see_the_qk_norm(name, weights_for):
    """With the norm switched off the reference misses a Qwen3 fixture by more than 100 x its bound: the fixtures pin the norm."""
    z = np.load(os.path.join(Q3_GOLDEN, name + ".npz"))
    cfg, w = weights_for(str(z["config"]))
    ids, mask = z["ids"].astype(np.int64), z["mask"].astype(np.int64)
    logits, hs = decoder_ref.forward(cfg, w, ids, mask, want_hidden=True, qk_norm=0)
    pos = z["sample_pos"]
    att = mask[:, pos].astype(bool)
    assert np.abs(hs[:, :, pos, : z["hidden_samples"].shape[-1]] - z["hidden_samples"])[:, att].max() > 100 * REF_TOL
    assert np.abs(logits - z["logits"])[:, : 1].max() > 100 * REF_TOL or z["counts"][0] == 0


@pytest.mark.parametrize("kind", ["qwen3", "llama"])
def test_reference_matches_live_hf_model(kind):
    """A shape no fixture has: 3 layers, 4 query / 4 kv heads of 64 on hidden 128 (nq d = 256 != H), another RoPE base, a ragged batch."""
    pytest.importorskip("transformers")
    gen = _gen()
    from gliclass.c_amd import synth, weights
    from gliclass.c_amd.config import CONFIGS
    cfg = dataclasses.replace(CONFIGS["q3-tiny"], layers=3, heads=4, kv_heads=4, rope_theta=50000.0, qk_norm=int(kind == "qwen3"))
    w = weights.make_weights(cfg, 3)
    ids, mask, _ = synth.make_inputs(cfg, 3, 130, 3, seed=5, ragged=True, labels_per_row=[3, 1, 2])
    model = gen.build_hf_model(cfg, w)
    assert type(model).__name__ == ("Qwen3Model" if kind == "qwen3" else "LlamaModel")
    ref_logits, ref_hs = gen.hf_forward(cfg, w, ids, mask, model)
    logits, hs = decoder_ref.forward(cfg, w, ids, mask, dtype=torch.float64, want_hidden=True)
    att = mask.astype(bool)
    e_h, e_l = np.abs(hs - ref_hs)[:, att].max(), np.abs(logits - ref_logits).max()
    print(kind, "hidden", e_h, "logits", e_l)
    assert e_l <= REF_TOL and e_h <= REF_TOL


def test_named_configs_and_tensor_specs_match_python(libs):
    _lib, model = libs
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS, BACKBONE_DECODER, POOL_LAST
    for cname in Q3_CONFIGS + ("dec-tiny", "dec-mini", "qwen-1.5b"):
        cfg = CONFIGS[cname]
        assert cfg.backbone == BACKBONE_DECODER and cfg.pooling == POOL_LAST and cfg.causal == 1
        cc = _lib.ModelConfig()
        assert model.glc_named_config(cname.encode(), C.byref(cc)) == 0
        assert abs(cc.ln_eps - 1e-6) < 1e-12 and abs(cc.ln_eps - cfg.ln_eps) < 1e-12 and abs(cc.rope_theta - cfg.rope_theta) < 1.0
        for f in ("vocab", "hidden", "layers", "heads", "head_dim", "inter", "class_token_index", "text_token_index", "pos_buckets",
                  "backbone", "kv_heads", "causal", "pooling", "qk_norm", "attn_bias"):
            assert getattr(cc, f) == getattr(cfg, f), (cname, f)
        specs = weights.tensor_specs(cfg)
        buf = C.create_string_buffer(96)
        shp = (C.c_uint64 * 4)()
        amp, mean = C.c_double(), C.c_double()
        for i, (n, shape, a, m) in enumerate(specs):
            nd = model.glc_tensor_spec(C.byref(cc), i, buf, shp, C.byref(amp), C.byref(mean))
            assert nd == len(shape) and buf.value.decode() == n and tuple(shp[:nd]) == tuple(shape), (cname, i, n)
            assert abs(amp.value - a) < 1e-15 and mean.value == m
        assert model.glc_tensor_spec(C.byref(cc), len(specs), buf, shp, C.byref(amp), C.byref(mean)) == -1
        assert len(specs) == 2 + (12 - 3 * (1 - cfg.attn_bias) + 2 * cfg.qk_norm) * cfg.layers + 8
    q3, ll = CONFIGS["q3-mini"], CONFIGS["ll-tiny"]
    assert (q3.qk_norm, q3.attn_bias, q3.heads * q3.head_dim) == (1, 0, 512) and q3.hidden == 256
    assert dataclasses.replace(ll, attn_bias=1, name="dec-tiny") == CONFIGS["dec-tiny"]
    z = CONFIGS["qwen3-0.6b"]
    assert (z.hidden, z.layers, z.heads, z.kv_heads, z.head_dim, z.inter, z.rope_theta) == (1024, 28, 16, 8, 128, 3072, 1e6)
    # every other named config keeps (0, 1), in both tables
    for cname, cfg in CONFIGS.items():
        cc = _lib.ModelConfig()
        assert model.glc_named_config(cname.encode(), C.byref(cc)) == 0
        assert (cc.qk_norm, cc.attn_bias) == (cfg.qk_norm, cfg.attn_bias)
        if cname not in Q3_CONFIGS:
            assert (cfg.qk_norm, cfg.attn_bias) == (0, 1), cname


def test_qk_norm_gains_are_not_ones():
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    w = weights.make_weights(CONFIGS["q3-mini"], 42)
    q, k = w["layers.1.self_attn.q_norm.weight"], w["layers.1.self_attn.k_norm.weight"]
    assert q.shape == k.shape == (128,) and q.std() > 0.1 and k.std() > 0.1 and abs(q.mean() - k.mean()) > 0.1
    assert 0.5 < q.min() and q.max() < 1.6 and 0.5 < k.min() and k.max() < 1.6


@pytest.mark.parametrize("cname", ["q3-tiny", "ll-tiny"])
def test_synthetic_weights_bit_identical_to_python(cname, libs, c_generated_weights):
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = CONFIGS[cname]
    ref = weights.make_weights(cfg, 9)
    got = c_generated_weights("synthetic:%s:9" % cname, cfg)
    assert list(got) == list(ref) and all(np.array_equal(got[k], ref[k]) for k in ref)


def test_blob_v4_round_trip_and_older_blobs_mean_no_norm_with_bias(libs, tmp_path):
    _lib, model = libs
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    for cname, want in (("q3-mini", (1, 0)), ("ll-tiny", (0, 0))):
        cfg = CONFIGS[cname]
        ref = weights.make_weights(cfg, 7)
        path = str(tmp_path / (cname + ".glcw"))
        weights.write_blob(path, cfg, ref)
        with open(path, "rb") as f:
            assert struct.unpack_from("<I", f.read(16), 8)[0] == 4
        cfg2, back = weights.read_blob(path)
        assert (cfg2.backbone, cfg2.qk_norm, cfg2.attn_bias, cfg2.head_dim, cfg2.kv_heads) == (cfg.backbone,) + want + (cfg.head_dim, cfg.kv_heads)
        assert all(np.array_equal(back[n], ref[n]) for n in ref)
        W = _lib.Weights()
        assert model.glc_weights_load(path.encode(), C.byref(W)) == 0
        try:
            assert (W.cfg.backbone, W.cfg.qk_norm, W.cfg.attn_bias) == (cfg.backbone,) + want
            assert W.n_tensors == len(ref)
            for i, (n, shape, _, _) in enumerate(weights.tensor_specs(cfg)):
                assert np.array_equal(np.ctypeslib.as_array(W.tensors[i], shape=shape), ref[n])
        finally:
            model.glc_weights_free(C.byref(W))
    # older versions: byte-identical headers as before, and both readers take them as (qk_norm, attn_bias) = (0, 1)
    for cname, ver, slots in (("dec-tiny", 2, 23), ("tiny", 2, 23), ("mb-tiny", 3, 26)):
        cfg = CONFIGS[cname]
        path = str(tmp_path / (cname + ".glcw"))
        weights.write_blob(path, cfg, weights.make_weights(cfg, 7))
        with open(path, "rb") as f:
            hdr = f.read(256)
        assert struct.unpack_from("<I", hdr, 8)[0] == ver
        assert hdr[16 + 4 * slots:] == b"\x00" * (256 - 16 - 4 * slots)
        cfg2, _ = weights.read_blob(path)
        assert (cfg2.qk_norm, cfg2.attn_bias) == (0, 1)
        W = _lib.Weights()
        assert model.glc_weights_load(path.encode(), C.byref(W)) == 0
        try:
            assert (W.cfg.qk_norm, W.cfg.attn_bias) == (0, 1)
        finally:
            model.glc_weights_free(C.byref(W))


def _hf_dir(tmp_path, cfg, tensors, kind, prefix="decoder_model.model.", enc_extra=None, drop=(), drop_tensors=(), extra_tensors=None):
    from safetensors.numpy import save_file
    enc = dict(model_type=kind, vocab_size=cfg.vocab - 2, hidden_size=cfg.hidden, intermediate_size=cfg.inter,
               num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads, num_key_value_heads=cfg.kv_heads, head_dim=cfg.head_dim,
               rms_norm_eps=cfg.ln_eps, attention_bias=bool(cfg.attn_bias), hidden_act="silu", tie_word_embeddings=True,
               rope_parameters={"rope_type": "default", "rope_theta": cfg.rope_theta}, pad_token_id=cfg.pad_id,
               bos_token_id=cfg.cls_id, eos_token_id=cfg.sep_id)
    if kind == "qwen3":
        enc.update(use_sliding_window=False, sliding_window=None, layer_types=["full_attention"] * cfg.layers)
    else:
        enc.update(mlp_bias=False)
    enc.update(enc_extra or {})
    for k in drop:
        enc.pop(k, None)
    root = dict(encoder_config=enc, architecture_type="uni-encoder", scorer_type="simple", class_token_index=cfg.class_token_index,
                text_token_index=cfg.text_token_index, embed_class_token=True, normalize_features=False)
    d = tmp_path / f"ckpt_{kind}_{len(list(tmp_path.iterdir()))}"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(root))
    sd = {(prefix if "projector" not in k else "") + k: np.ascontiguousarray(v) for k, v in tensors.items() if k not in drop_tensors}
    sd.update({prefix + k: v for k, v in (extra_tensors or {}).items()})
    save_file(sd, str(d / "model.safetensors"))
    return str(d)


@pytest.mark.parametrize("kind,cname,prefix,drop", [("qwen3", "q3-mini", "decoder_model.model.", ()), ("llama", "ll-tiny", "model.", ("head_dim",)),
                                                    ("llama", "dec-tiny", "", ())])
def test_checkpoint_import(libs, tmp_path, kind, cname, prefix, drop):
    """Qwen3 (head_dim from the file: nq d != hidden), Llama without head_dim in the file (hidden / heads), Llama with attention_bias."""
    pytest.importorskip("safetensors")
    _lib, model = libs
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS, POOL_LAST
    cfg = dataclasses.replace(CONFIGS[cname], rope_theta=250000.0)
    ref = weights.make_weights(cfg, 4)
    # (Llama / Qwen3 with attention_bias carry an o_proj bias too; a checkpoint of that form without one is what the tensor order can hold)
    path = _hf_dir(tmp_path, cfg, ref, kind, prefix, drop=drop)
    W = _lib.Weights()
    assert model.glc_weights_load(path.encode(), C.byref(W)) == 0
    try:
        c = W.cfg
        assert (c.backbone, c.vocab, c.hidden, c.layers, c.heads, c.kv_heads, c.head_dim, c.inter) == \
               (cfg.backbone, cfg.vocab, cfg.hidden, cfg.layers, cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.inter)
        assert (c.qk_norm, c.attn_bias, c.causal, c.pooling) == (int(kind == "qwen3"), cfg.attn_bias, 1, POOL_LAST)
        assert abs(c.rope_theta - 250000.0) < 1.0 and abs(c.ln_eps - 1e-6) < 1e-12 and c.class_token_index == cfg.class_token_index
        specs = weights.tensor_specs(cfg)
        assert W.n_tensors == len(specs)
        for i, (n, shape, _, _) in enumerate(specs):
            assert np.array_equal(np.ctypeslib.as_array(W.tensors[i], shape=shape), ref[n]), n
    finally:
        model.glc_weights_free(C.byref(W))


_ONES = np.ones(128, np.float32)


@pytest.mark.parametrize("kind,cname,kw,msg", [
    ("llama", "ll-tiny", dict(enc_extra={"rope_scaling": {"rope_type": "llama3", "factor": 8.0}}), "rope_scaling type 'llama3' is not implemented"),
    ("qwen3", "q3-mini", dict(enc_extra={"rope_parameters": {"rope_type": "yarn", "rope_theta": 1e6, "factor": 4.0}}), "rope_parameters type 'yarn' is not implemented"),
    ("llama", "ll-tiny", dict(enc_extra={"rope_scaling": {"type": "linear", "factor": 2.0}}), "rope_scaling type 'linear' is not implemented"),
    ("qwen3", "q3-mini", dict(enc_extra={"use_sliding_window": True}), "use_sliding_window=true is not implemented"),
    ("qwen3", "q3-mini", dict(enc_extra={"layer_types": ["full_attention", "sliding_attention", "full_attention"]}), "'sliding_attention' entry is not implemented"),
    ("llama", "ll-tiny", dict(enc_extra={"mlp_bias": True}), "mlp_bias=true is not implemented"),
    ("qwen3", "q3-mini", dict(enc_extra={"mlp_bias": True}), "mlp_bias=true is not implemented"),
    ("qwen3", "q3-mini", dict(drop_tensors=("layers.0.self_attn.k_norm.weight",)), "layers.0.self_attn.k_norm.weight' is missing"),
    ("llama", "ll-tiny", dict(extra_tensors={"layers.0.self_attn.q_norm.weight": _ONES, "layers.0.self_attn.k_norm.weight": _ONES}),
     "layers.0.self_attn.q_norm.weight' is present"),
    ("llama", "ll-tiny", dict(extra_tensors={"layers.0.self_attn.o_proj.bias": np.zeros(256, np.float32)}), "an output-projection bias) is not implemented"),
    ("qwen3", "q3-mini", dict(enc_extra={"head_dim": 96}), "head_dim 96 is not implemented"),
    ("qwen3_moe", "q3-mini", dict(), "model_type 'qwen3_moe' is not implemented"),
])
def test_checkpoint_rejections(libs, tmp_path, kind, cname, kw, msg):
    """Everything the engine does not build fails loudly, naming the field (the importer prints to stderr; checked in a child)."""
    pytest.importorskip("safetensors")
    import subprocess
    import sys
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = CONFIGS[cname]
    path = _hf_dir(tmp_path, cfg, weights.make_weights(cfg, 4), kind, **kw)
    code = ("import ctypes as C, sys; sys.path.insert(0, %r); from gliclass.c_amd import _lib; W = _lib.Weights(); "
            "sys.exit(0 if _lib.model().glc_weights_load(%r, C.byref(W)) != 0 else 3)") % (ROOT, path.encode())
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert msg in r.stderr, r.stderr


def test_tensor_count_follows_the_two_fields():
    """include/gliclass_hip.h glc_num_tensors_cfg, restated: 12 per layer for Qwen2, 9 for Llama, 11 for Qwen3."""
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    base = CONFIGS["dec-mini"]
    for qkn, ab, per in ((0, 1, 12), (0, 0, 9), (1, 0, 11), (1, 1, 14)):
        cfg = dataclasses.replace(base, qk_norm=qkn, attn_bias=ab)
        names = [s[0] for s in weights.tensor_specs(cfg)]
        assert len(names) == 2 + per * cfg.layers + 8
        i = names.index("layers.1.self_attn.o_proj.weight")
        assert (names[i - 1] == "layers.1.self_attn.k_norm.weight") == bool(qkn) and (names[i - 2] == "layers.1.self_attn.q_norm.weight") == bool(qkn)
        assert ("layers.1.self_attn.v_proj.bias" in names) == bool(ab)

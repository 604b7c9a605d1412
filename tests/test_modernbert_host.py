"""ModernBERT backbone, host side (no GPU): the CPU restatement against the committed fixtures (and a live HF model where
transformers is importable), the C config / tensor-spec mirror, the v3 blob header, and the checkpoint importer."""
import ctypes as C
import dataclasses
import glob
import json
import os
import struct

import numpy as np
import pytest
import torch

import modernbert_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB_GOLDEN = os.path.join(ROOT, "tests", "golden", "modernbert")
MB_CONFIGS = ("mb-tiny", "mb-mini", "modernbert-base", "modernbert-large")


@pytest.fixture(scope="module")
def libs():
    from gliclass.c_amd import _lib
    return _lib, _lib.model()


def _fixtures():
    return sorted(glob.glob(os.path.join(MB_GOLDEN, "*.npz")))


def test_fixture_set_is_complete():
    names = {os.path.basename(f)[:-4] for f in _fixtures()}
    assert names == {"mb_tiny_b3_s200", "mb_tiny_b2_s700", "mb_mini_b2_s333", "mb_mini_b2_s1100"}


@pytest.mark.parametrize("path", _fixtures(), ids=lambda p: os.path.basename(p)[:-4])
def test_reference_matches_fixtures(path, weights_for):
    z = np.load(path)
    cfg, w = weights_for(str(z["config"]))
    ids, mask = z["ids"].astype(np.int64), z["mask"].astype(np.int64)
    logits, hs = modernbert_ref.forward(cfg, w, ids, mask, dtype=torch.float32, want_hidden=True)
    assert np.abs(logits - z["logits"]).max() <= 1e-5
    pos = z["sample_pos"]
    got = hs[:, :, pos, : z["hidden_samples"].shape[-1]]
    att = mask[:, pos].astype(bool)                       # attended positions only
    assert np.abs(got - z["hidden_samples"])[:, att].max() <= 1e-5


def test_reference_window_is_effective(weights_for):
    """The local layers' window changes the answer (a restatement that ignored it would pass the fixtures only by luck)."""
    z = np.load(os.path.join(MB_GOLDEN, "mb_tiny_b2_s700.npz"))
    cfg, w = weights_for("mb-tiny")
    ids, mask = z["ids"].astype(np.int64), z["mask"].astype(np.int64)
    glob_only = modernbert_ref.forward(dataclasses.replace(cfg, local_window=0), w, ids, mask, dtype=torch.float32)
    assert np.abs(glob_only - z["logits"]).max() > 1e-3


def test_reference_matches_live_hf_model():
    """A fresh config: W = 50 (not a multiple of 32), every 2nd layer global, the legacy config keys, a ragged batch."""
    pytest.importorskip("transformers")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_mb", os.path.join(ROOT, "scripts", "gen_modernbert_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    from gliclass.c_amd import synth, weights
    from gliclass.c_amd.config import CONFIGS
    cfg = dataclasses.replace(CONFIGS["mb-tiny"], layers=4, local_window=50, global_every=2, rope_theta=80000.0, rope_theta_local=5000.0)
    w = weights.make_weights(cfg, 3)
    ids, mask, _ = synth.make_inputs(cfg, 3, 300, 3, seed=5, ragged=True, labels_per_row=[3, 1, 2])
    model = gen.build_hf_model(cfg, w, legacy=True)
    assert model.config.layer_types == ["full_attention", "sliding_attention"] * 2
    ref_logits, ref_hs = gen.hf_forward(cfg, w, ids, mask, model)
    logits, hs = modernbert_ref.forward(cfg, w, ids, mask, dtype=torch.float32, want_hidden=True)
    assert np.abs(logits - ref_logits).max() <= 1e-5
    att = mask.astype(bool)
    assert np.abs(hs - ref_hs)[:, att].max() <= 1e-4


def test_named_configs_and_tensor_specs_match_python(libs):
    _lib, model = libs
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS, BACKBONE_MODERNBERT
    for cname in MB_CONFIGS:
        cfg = CONFIGS[cname]
        assert cfg.backbone == BACKBONE_MODERNBERT and cfg.head_dim == 64
        cc = _lib.ModelConfig()
        assert model.glc_named_config(cname.encode(), C.byref(cc)) == 0
        assert abs(cc.ln_eps - cfg.ln_eps) < 1e-12 and abs(cc.rope_theta - cfg.rope_theta) < 1.0
        assert abs(cc.rope_theta_local - cfg.rope_theta_local) < 1.0
        for f in ("vocab", "hidden", "layers", "heads", "head_dim", "inter", "class_token_index", "text_token_index", "pos_buckets",
                  "backbone", "kv_heads", "causal", "pooling", "local_window", "global_every"):
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
        assert len(specs) == 3 + 6 * cfg.layers - 1 + 8


def test_synthetic_weights_bit_identical_to_python(libs, c_generated_weights):
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = CONFIGS["mb-tiny"]
    ref = weights.make_weights(cfg, 9)
    got = c_generated_weights("synthetic:mb-tiny:9", cfg)
    assert list(got) == list(ref) and all(np.array_equal(got[k], ref[k]) for k in ref)


def test_blob_v3_round_trip_and_v2_unchanged(libs, tmp_path):
    _lib, model = libs
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = dataclasses.replace(CONFIGS["mb-mini"], local_window=40, global_every=2, rope_theta_local=2500.0)
    ref = weights.make_weights(cfg, 7)
    path = str(tmp_path / "mb.glcw")
    weights.write_blob(path, cfg, ref)
    with open(path, "rb") as f:
        assert struct.unpack_from("<I", f.read(16), 8)[0] == 3
    cfg2, back = weights.read_blob(path)
    assert (cfg2.backbone, cfg2.local_window, cfg2.global_every, cfg2.rope_theta_local) == (cfg.backbone, 40, 2, 2500.0)
    assert all(np.array_equal(back[n], ref[n]) for n in ref)
    W = _lib.Weights()
    assert model.glc_weights_load(path.encode(), C.byref(W)) == 0
    try:
        assert (W.cfg.backbone, W.cfg.local_window, W.cfg.global_every, W.cfg.rope_theta_local) == (cfg.backbone, 40, 2, 2500.0)
        assert W.n_tensors == len(ref)
        for i, (n, shape, _, _) in enumerate(weights.tensor_specs(cfg)):
            assert np.array_equal(np.ctypeslib.as_array(W.tensors[i], shape=shape), ref[n])
    finally:
        model.glc_weights_free(C.byref(W))
    tiny = str(tmp_path / "tiny.glcw")
    weights.write_blob(tiny, CONFIGS["tiny"], weights.make_weights(CONFIGS["tiny"], 7))
    with open(tiny, "rb") as f:
        hdr = f.read(256)
    assert struct.unpack_from("<I", hdr, 8)[0] == 2
    assert hdr[16 + 4 * 23:] == b"\x00" * (256 - 16 - 4 * 23)        # nothing behind the v2 slots


def _hf_dir(tmp_path, cfg, tensors, form="v5", prefix="encoder_model.", enc_extra=None, drop=()):
    from safetensors.numpy import save_file
    enc = dict(model_type="modernbert", vocab_size=cfg.vocab - 2, hidden_size=cfg.hidden, intermediate_size=cfg.inter,
               num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads, norm_eps=cfg.ln_eps, norm_bias=False,
               attention_bias=False, mlp_bias=False, hidden_activation="gelu", local_attention=2 * cfg.local_window,
               pad_token_id=cfg.pad_id, cls_token_id=cfg.cls_id, sep_token_id=cfg.sep_id)
    if form == "v5":
        enc["layer_types"] = ["full_attention" if cfg.is_global_layer(l) else "sliding_attention" for l in range(cfg.layers)]
        enc["rope_parameters"] = {"full_attention": {"rope_type": "default", "rope_theta": cfg.rope_theta},
                                  "sliding_attention": {"rope_type": "default", "rope_theta": cfg.rope_theta_local}}
    else:
        enc.update(global_attn_every_n_layers=cfg.global_every, global_rope_theta=cfg.rope_theta, local_rope_theta=cfg.rope_theta_local)
    enc.update(enc_extra or {})
    for k in drop:
        enc.pop(k, None)
    root = dict(encoder_config=enc, architecture_type="uni-encoder", scorer_type="simple",
                pooling_strategy={0: "first", 1: "avg", 2: "last"}[cfg.pooling], class_token_index=cfg.class_token_index,
                text_token_index=cfg.text_token_index, embed_class_token=True, normalize_features=False)
    d = tmp_path / f"ckpt_{form}_{len(list(tmp_path.iterdir()))}"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(root))
    sd = {(prefix if "projector" not in k else "") + k: np.ascontiguousarray(v) for k, v in tensors.items()}
    save_file(sd, str(d / "model.safetensors"))
    return str(d)


@pytest.mark.parametrize("form,prefix", [("v5", "encoder_model."), ("legacy", "model.encoder_model."), ("v5", "")])
def test_checkpoint_import(libs, tmp_path, form, prefix):
    pytest.importorskip("safetensors")
    _lib, model = libs
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = dataclasses.replace(CONFIGS["mb-tiny"], layers=5, local_window=24, global_every=2)
    ref = weights.make_weights(cfg, 4)
    path = _hf_dir(tmp_path, cfg, ref, form, prefix)
    W = _lib.Weights()
    assert model.glc_weights_load(path.encode(), C.byref(W)) == 0
    try:
        c = W.cfg
        assert (c.backbone, c.vocab, c.hidden, c.layers, c.heads, c.head_dim, c.inter) == (cfg.backbone, cfg.vocab, 128, 5, 2, 64, cfg.inter)
        assert (c.local_window, c.global_every, c.causal, c.kv_heads, c.pooling) == (24, 2, 0, 2, cfg.pooling)
        assert abs(c.rope_theta - cfg.rope_theta) < 1.0 and abs(c.rope_theta_local - cfg.rope_theta_local) < 1e-3
        assert abs(c.ln_eps - 1e-5) < 1e-12 and c.class_token_index == cfg.class_token_index
        specs = weights.tensor_specs(cfg)
        assert W.n_tensors == len(specs)
        for i, (n, shape, _, _) in enumerate(specs):
            assert np.array_equal(np.ctypeslib.as_array(W.tensors[i], shape=shape), ref[n]), n
    finally:
        model.glc_weights_free(C.byref(W))


@pytest.mark.parametrize("extra,drop,msg", [
    ({"attention_bias": True}, (), "attention_bias=true is not implemented"),
    ({"mlp_bias": True}, (), "mlp_bias=true is not implemented"),
    ({"norm_bias": True}, (), "norm_bias=true is not implemented"),
    ({"hidden_activation": "silu"}, (), "hidden_activation 'silu' is not implemented"),
    ({"num_attention_heads": 4}, (), "head_dim 32 is not implemented"),
    ({"local_attention": 17}, (), "local_attention 17 is not implemented"),
    ({"layer_types": ["full_attention", "sliding_attention", "full_attention", "full_attention"]}, (), "layer_types is not periodic"),
    ({"layer_types": ["sliding_attention", "full_attention", "sliding_attention", "full_attention"]}, (), "layer_types is not periodic"),
])
def test_checkpoint_rejections(libs, tmp_path, extra, drop, msg):
    """Everything the engine does not build fails loudly, with its message (the importer prints to stderr; checked in a child)."""
    pytest.importorskip("safetensors")
    import subprocess
    import sys
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = CONFIGS["mb-tiny"]
    path = _hf_dir(tmp_path, cfg, weights.make_weights(cfg, 4), "v5", "encoder_model.", extra, drop)
    code = ("import ctypes as C, sys; sys.path.insert(0, %r); from gliclass.c_amd import _lib; W = _lib.Weights(); "
            "sys.exit(0 if _lib.model().glc_weights_load(%r, C.byref(W)) != 0 else 3)") % (ROOT, path.encode())
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert msg in r.stderr, r.stderr


def test_flops_per_seq():
    from gliclass.c_amd.config import CONFIGS
    cfg = CONFIGS["modernbert-base"]
    H, I, L, W = 768, 1152, 22, 64
    for S, C_ in ((1024, 4), (8192, 2), (100, 1)):
        keys = sum(S if l % 3 == 0 else min(S, 2 * W + 1) for l in range(L))
        want = L * S * (8 * H * H + 6 * H * I) + 4 * S * H * keys + 8 * H * H * (1 + C_)
        assert cfg.flops_per_seq(S, C_) == want

"""GPU (-m gpu): opt-in captured-graph replay of forwards (glc_engine_set_graph_replay; engine.hip graph_forward).

Per key — shape, pipeline switches, workspace generation, the three device pointers — the first forward runs eagerly, the second is
captured as a HIP graph and launched, later ones replay it: Engine.last_graph() reads 0, 1, 2, 2.  The graph holds the launches the eager
forward makes, on the same buffers, so every comparison here is np.array_equal against a second engine that never replays (same tensors,
same switches, same entry point): no tolerance is involved anywhere.

Shapes: the mini configs of the three backbones (hidden 256, so that the fp32 mode's group-split and MX pipelines exist), B <= 8 and
S <= 200 — except the length-bucket case: the planner's cost model (whole waves of 256-row tiles over the CUs) never splits a batch of
fewer rows than one wave, so that case takes the smallest batch it does split at S = 200 (768 rows of a 3-layer model)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BACKBONES = ("mini", "mb-mini", "dec-mini", "q3-mini")      # DeBERTa, ModernBERT, decoder (Qwen2 / Qwen3 flavours)


def place(cfg, S, lens, cls_pos, seed):
    """Rows with their class tokens at chosen positions: [CLS] at 0, <<LABEL>> at cls_pos[b], [SEP] at lens[b] - 1, padding behind."""
    from gliclass.c_amd import prng
    B = len(lens)
    ids = prng.randint(seed, "ids", B * S, 3, cfg.vocab - 2).reshape(B, S).astype(np.int64)
    mask = np.zeros((B, S), np.int64)
    for b in range(B):
        n = lens[b]
        assert all(0 < p < n - 1 for p in cls_pos[b])
        ids[b, 0] = cfg.cls_id
        ids[b, list(cls_pos[b])] = cfg.class_token_index
        ids[b, n - 1] = cfg.sep_id
        ids[b, n:] = cfg.pad_id
        mask[b, :n] = 1
    return ids, mask


class Pair:
    """An engine that replays and one that never does, on the same tensors; switches go to both."""

    def __init__(self, cname, dtype, weights_for):
        from gliclass.c_amd.engine import Engine
        self.cfg, w = weights_for(cname)
        self.eager = Engine(self.cfg, w, dtype=dtype)
        self.replay = Engine(self.cfg, w, dtype=dtype)
        self.replay.set_graph_replay(True)

    def both(self, fn):
        fn(self.eager)
        fn(self.replay)

    def forward(self, ids, mask, c_alloc=None):
        """the replaying engine's logits and its last_graph(); asserted equal to the eager engine's logits"""
        want = self.eager.forward(ids, mask, c_alloc=c_alloc)
        assert self.eager.last_graph() == 0 and self.eager.graph_cache_size() == 0
        got = self.replay.forward(ids, mask, c_alloc=c_alloc)
        assert np.isfinite(want).all()
        assert np.array_equal(got, want), "replay differs from the eager forward"
        return got, self.replay.last_graph()

    def sequence(self, ids, mask, n, c_alloc=None):
        return [self.forward(ids, mask, c_alloc)[1] for _ in range(n)]

    def close(self):
        self.eager.close()
        self.replay.close()


@pytest.fixture
def pair(weights_for):
    made = []

    def get(cname, dtype):
        made.append(Pair(cname, dtype, weights_for))
        return made[-1]
    yield get
    for p in made:
        p.close()


class DevBufs:
    """device-resident entry: ids / mask / logits buffers of one shape on one engine"""

    def __init__(self, eng, B, S, Cn):
        self.eng, self.B, self.S, self.Cn = eng, B, S, Cn
        self.ids, self.mask, self.logits = eng.dev_alloc(B * S * 8), eng.dev_alloc(B * S * 8), eng.dev_alloc(B * Cn * 4)

    def run(self, ids, mask, logits=None):
        e = self.eng
        e.h2d(self.ids, ids)
        e.h2d(self.mask, mask)
        dst = self.logits if logits is None else logits
        e.forward_device(self.ids, self.mask, self.B, self.S, self.Cn, dst)
        state = e.last_graph()
        e.sync()
        out = np.zeros((self.B, self.Cn), np.float32)
        e.d2h(out, dst)
        return out, state

    def free(self):
        for p in (self.ids, self.mask, self.logits):
            self.eng.dev_free(p)


# ---- 1. bit identity on every backbone --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("cname", BACKBONES)
def test_bit_identical_and_0_1_2_2(cname, dtype, pair):
    from gliclass.c_amd import synth
    p = pair(cname, dtype)
    ids, mask, _ = synth.make_inputs(p.cfg, 3, 100, 3, seed=31, ragged=True, labels_per_row=[3, 1, 2])
    assert p.sequence(ids, mask, 4) == [0, 1, 2, 2]
    assert p.replay.graph_cache_size() == 1


def test_environment_switch(weights_for, monkeypatch):
    """GLICLASS_GRAPH_REPLAY=1 at creation makes the call; without it the engine never captures"""
    from gliclass.c_amd import synth
    from gliclass.c_amd.engine import Engine
    cfg, w = weights_for("tiny")
    ids, mask, _ = synth.make_inputs(cfg, 2, 64, 2, seed=5, ragged=True)
    monkeypatch.setenv("GLICLASS_GRAPH_REPLAY", "1")
    on = Engine(cfg, w, dtype="f16")
    monkeypatch.delenv("GLICLASS_GRAPH_REPLAY")
    off = Engine(cfg, w, dtype="f16")
    try:
        want = [off.forward(ids, mask) for _ in range(3)]
        assert off.last_graph() == 0 and off.graph_cache_size() == 0
        states = []
        for i in range(3):
            assert np.array_equal(on.forward(ids, mask), want[i])
            states.append(on.last_graph())
        assert states == [0, 1, 2]
    finally:
        on.close()
        off.close()


# ---- 2. the graph reads buffers, not baked values ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("cname,dtype", [("mini", "f32"), ("mb-mini", "f16"), ("q3-mini", "f32"), ("dec-mini", "f16")])
def test_replay_reads_new_inputs_host_entry(cname, dtype, pair):
    from gliclass.c_amd import synth
    p = pair(cname, dtype)
    S = 100
    ids, mask, _ = synth.make_inputs(p.cfg, 3, S, 3, seed=31, ragged=True, labels_per_row=[3, 1, 2])
    assert p.sequence(ids, mask, 3) == [0, 1, 2]
    first = p.replay.forward(ids, mask)
    # other tokens, other lengths, other class-token positions (and counts per row), the same maximum label count
    ids2, mask2 = place(p.cfg, S, [61, 100, 37], [[7, 30, 55], [2, 90], [11]], seed=77)
    got, state = p.forward(ids2, mask2)
    assert state == 2
    assert not np.array_equal(got, first)
    # ... and back
    again, state = p.forward(ids, mask)
    assert state == 2 and np.array_equal(again, first)


@pytest.mark.parametrize("cname,dtype", [("mini", "f16"), ("dec-mini", "f32")])
def test_replay_reads_new_inputs_device_entry(cname, dtype, pair):
    from gliclass.c_amd import synth
    p = pair(cname, dtype)
    B, S, Cn = 3, 100, 3
    ids, mask, _ = synth.make_inputs(p.cfg, B, S, Cn, seed=31, ragged=True, labels_per_row=[3, 1, 2])
    ids2, mask2 = place(p.cfg, S, [61, 100, 37], [[7, 30, 55], [2, 90], [11]], seed=77)
    de, dr = DevBufs(p.eager, B, S, Cn), DevBufs(p.replay, B, S, Cn)
    try:
        want, _ = de.run(ids, mask)
        want2, _ = de.run(ids2, mask2)
        assert np.isfinite(want).all() and not np.array_equal(want, want2)
        states = []
        for _ in range(3):
            got, st = dr.run(ids, mask)
            assert np.array_equal(got, want)
            states.append(st)
        assert states == [0, 1, 2]
        got2, st = dr.run(ids2, mask2)              # the same device buffers, rewritten
        assert st == 2 and np.array_equal(got2, want2)
        got, st = dr.run(ids, mask)
        assert st == 2 and np.array_equal(got, want)
    finally:
        de.free()
        dr.free()


# ---- 3. keys ----------------------------------------------------------------------------------------------------------------------------

def test_each_shape_is_a_key_of_its_own(pair):
    from gliclass.c_amd import synth
    p = pair("tiny", "f16")

    def batch(B, S, Cn):
        ids, mask, _ = synth.make_inputs(p.cfg, B, S, Cn, seed=B * 1000 + S + Cn, ragged=True)
        return ids, mask
    p.forward(*batch(8, 200, 3))                    # the largest shape first: a workspace that grows later would drop the cache
    size = 0
    for shape in ((4, 128, 2), (4, 64, 2), (2, 128, 2), (4, 128, 3), (4, 100, 2)):      # base, new S, new B, new C, new S under the same padded S
        assert p.sequence(*batch(*shape), 3) == [0, 1, 2], shape
        size += 1
        assert p.replay.graph_cache_size() == size, shape
    assert p.forward(*batch(4, 128, 2))[1] == 2     # the first key is still there


def test_device_pointers_are_part_of_the_key(pair):
    from gliclass.c_amd import synth
    p = pair("tiny", "f16")
    B, S, Cn = 3, 100, 3
    ids, mask, _ = synth.make_inputs(p.cfg, B, S, Cn, seed=31, ragged=True, labels_per_row=[3, 1, 2])
    de, dr = DevBufs(p.eager, B, S, Cn), DevBufs(p.replay, B, S, Cn)
    other = p.replay.dev_alloc(B * Cn * 4)
    try:
        want, _ = de.run(ids, mask)
        assert [dr.run(ids, mask)[1] for _ in range(3)] == [0, 1, 2]
        p.replay.h2d(other, np.full((B, Cn), 123.0, np.float32))
        got, st = dr.run(ids, mask, logits=other)
        assert st == 0, "a graph captured for another d_logits was replayed"
        assert np.array_equal(got, want)            # ... and the logits landed in the new buffer
        assert dr.run(ids, mask)[1] == 2            # the old pointers still find their graph
    finally:
        p.replay.set_graph_replay(False)            # (no cached graph names `other` any more)
        p.replay.dev_free(other)
        de.free()
        dr.free()


def test_cache_holds_16_graphs(pair):
    from gliclass.c_amd import synth
    p = pair("tiny", "f16")
    shapes = [(B, S) for B in range(1, 7) for S in (64, 128, 200)][:17]
    batches = [synth.make_inputs(p.cfg, B, S, 2, seed=B * 1000 + S, ragged=True)[:2] for B, S in shapes]
    p.replay.forward(*synth.make_inputs(p.cfg, 8, 200, 2, seed=1, ragged=True)[:2])      # size the workspace once
    for i, (ids, mask) in enumerate(batches):
        assert p.sequence(ids, mask, 2) == [0, 1], shapes[i]
        assert p.replay.graph_cache_size() == min(i + 1, 16)
    assert p.replay.graph_cache_size() == 16
    assert p.forward(*batches[16])[1] == 2          # the newest is there
    assert p.forward(*batches[0])[1] == 0           # the least recently used one went


# ---- 4. invalidation --------------------------------------------------------------------------------------------------------------------

SWITCHES = [("prune off", lambda e: e.set_prune_last_layer(False)),
            ("group split 0", lambda e: e.set_group_split(0)),
            ("group split 2", lambda e: e.set_group_split(2)),
            ("attention impl 1", lambda e: e.set_attention_impl(1)),
            ("length buckets 1", lambda e: e.set_length_buckets(1))]


@pytest.mark.parametrize("cname", ["mini", "dec-mini"])
def test_switches_drop_the_cache(cname, pair):
    from gliclass.c_amd import synth
    p = pair(cname, "f32")
    ids, mask, _ = synth.make_inputs(p.cfg, 3, 100, 3, seed=31, ragged=True, labels_per_row=[3, 1, 2])
    assert p.sequence(ids, mask, 3) == [0, 1, 2]
    for what, switch in SWITCHES:
        assert p.replay.graph_cache_size() == 1, what
        p.both(switch)
        assert p.replay.graph_cache_size() == 0, what
        assert p.sequence(ids, mask, 3) == [0, 1, 2], what       # (each forward equal to the eager engine under the same switch)


def test_workspace_growth_drops_the_cache(pair):
    from gliclass.c_amd import synth
    p = pair("mini", "f32")
    small = synth.make_inputs(p.cfg, 2, 64, 2, seed=3, ragged=True)[:2]
    large = synth.make_inputs(p.cfg, 8, 200, 4, seed=4, ragged=True)[:2]
    assert p.sequence(*small, 3) == [0, 1, 2]
    assert p.forward(*large)[1] == 0                 # every workspace buffer moves
    assert p.replay.graph_cache_size() == 0
    assert p.sequence(*small, 3) == [0, 1, 2]        # not the graph captured on the old buffers
    assert p.sequence(*large, 2) == [1, 2]           # (nothing moved since its eager forward)
    assert p.replay.graph_cache_size() == 2


# ---- 5. eager fall-backs ----------------------------------------------------------------------------------------------------------------

def test_profile_keep_hidden_and_off_run_eagerly(pair):
    from gliclass.c_amd import synth
    p = pair("mini", "f16")
    ids, mask, _ = synth.make_inputs(p.cfg, 3, 100, 3, seed=31, ragged=True, labels_per_row=[3, 1, 2])
    assert p.sequence(ids, mask, 3) == [0, 1, 2]
    base = p.replay.forward(ids, mask)
    p.both(lambda e: e.profile(True))
    for _ in range(3):
        got, st = p.forward(ids, mask)
        assert st == 0 and np.array_equal(got, base)
    assert sum(n for _, n in p.replay.profile_read().values()) > 0      # the events were recorded
    p.both(lambda e: e.profile(False))
    assert p.sequence(ids, mask, 3) == [0, 1, 2]
    p.both(lambda e: e.keep_hidden(True))
    for _ in range(3):
        assert p.forward(ids, mask)[1] == 0
    assert p.replay.graph_cache_size() == 0
    p.both(lambda e: e.keep_hidden(False))
    assert p.sequence(ids, mask, 3) == [0, 1, 2]
    assert p.replay.graph_cache_size() == 1
    p.replay.set_graph_replay(False)
    assert p.replay.graph_cache_size() == 0
    for _ in range(3):
        got, st = p.forward(ids, mask)
        assert st == 0 and np.array_equal(got, base)
    assert p.replay.graph_cache_size() == 0


# ---- 6. length buckets ------------------------------------------------------------------------------------------------------------------

def test_length_bucketed_forward_replays_every_group(pair):
    """256 rows of 200 tokens and 512 of 60: one wave of 256-row tiles each when split, three when padded together (the planner's
    cost model, glc_plan_length_buckets), so the plan has two groups; each is a key of its own."""
    p = pair("mini", "f16")
    B, S = 768, 200
    lens = [200] * 256 + [60] * 512
    ids, mask = place(p.cfg, S, lens, [[2, 5]] * B, seed=9)
    order, cuts, n = (C.c_int * B)(), (C.c_int * (B + 1))(), C.c_int(0)
    assert p.replay.L.glc_plan_length_buckets((C.c_int * B)(*lens), B, 4, p.cfg.hidden, order, cuts, C.byref(n)) == 0
    assert n.value >= 2, "the planner does not split this batch"
    assert p.sequence(ids, mask, 3) == [0, 1, 2]
    assert p.replay.L.glc_debug_last_forward_groups(p.replay.h) == n.value
    assert p.replay.graph_cache_size() == n.value


# ---- 7. MX pipeline ---------------------------------------------------------------------------------------------------------------------

def test_mx_pipeline_under_replay(pair):
    from gliclass.c_amd import synth
    p = pair("q3-mini", "f32")
    p.both(lambda e: (e.set_group_split(2), e.set_mx(True)))
    ids, mask, _ = synth.make_inputs(p.cfg, 3, 100, 3, seed=31, ragged=True, labels_per_row=[3, 1, 2])
    states = []
    for _ in range(4):
        states.append(p.forward(ids, mask)[1])
        assert p.eager.last_mx() and p.eager.last_mx_attention(), "the MX pipeline did not run"
        assert p.replay.last_mx() and p.replay.last_mx_attention(), "the replayed forward does not report the MX pipeline"
        assert p.replay.last_group_split() and p.replay.last_ln_folded() == p.eager.last_ln_folded()
        assert p.replay.fp8_range_retries() == p.eager.fp8_range_retries()
    assert p.eager.fp8_range_retries() == 0, "the range guard repeated a forward of this case: its 0 / 1 / 2 sequence is another"
    assert states == [0, 1, 2, 2]

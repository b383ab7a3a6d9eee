"""GPU: LoRA adapters merged into the device-resident weights (falcon_hip_model_apply_lora, csrc/kernels_lora.hip) and the tensor read-back
(falcon_hip_model_get_tensor). Bytes against the composed expectation of tests/lora_ref.py (proved against the real reference by tests/gen_lora_golden.py),
logits against the reference's own after its merge (tests/golden/lora.npz), a live context across the merge, and every refusal leaving the model as it was."""
import os

import numpy as np
import pytest

import ggllm_cpp_amd as g
import lora_ref as lr
import synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

N_CTX, N_BATCH = 32, 16
ALL_TYPES = ob.WEIGHT_TYPES + [lr.F16]
# 4 x n_embd as every Falcon; rows of 768 and 3072 weights: whole 1 KiB columns of the interleaved layout AND a partial last one in every format
# (Q4_0: 24 | 64 + 32 blocks, Q8_0: 24 | 3 x 32, Q4_K: 3 | 8 + 4 super-blocks); 896 / 768 / 96 rows: 7-row chunks end ragged for lm_head (13 x 7 + 5) and down (109 x 7 + 5)
HP_WIDE = dict(n_vocab=96, n_embd=768, n_head=12, n_head_kv=1, n_layer=1, n_ff=3072, two_norms=False)


@pytest.fixture(scope="module")
def L():
    L = g.load()
    L.ggml_hip_init(0)
    return L


@pytest.fixture(scope="module")
def wide(oracle):
    """{type: weights} of HP_WIDE, made once"""
    cache = {}

    def get(t):
        if t not in cache:
            cache[t] = synth.make_model_float(HP_WIDE, seed=4321, f16=True) if t == lr.F16 else synth.make_model(oracle, HP_WIDE, t, seed=4321)
        return cache[t]
    return get


@pytest.fixture(scope="module")
def gold(golden):
    d = golden["lora"]
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    """lora_ref.build_case per recorded case, files included, made once"""
    d, cache = str(tmp_path_factory.mktemp("lora_cases")), {}

    def get(name):
        if name not in cache:
            cache[name] = lr.build_case(oracle, name, d)
        return cache[name]
    return get


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).ravel()


def _assert_matrices(m, hp, want, what, keys=None):
    for key in (keys or lr.matrix_keys(hp)):
        got, exp = m.get_tensor(lr.tensor_name(key)), _bytes(lr.get_matrix(want, key))
        assert got.size == exp.size, (what, key)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, "%s: %s differs in %d of %d bytes, first at %d" % (what, lr.tensor_name(key), bad.size, exp.size, bad[0])


def _evaluate_12(m, tok):
    """a 9-token prompt and three single-token steps: [12][n_vocab]"""
    rows = [m.eval(tok[:lr.N_PROMPT], 0, logits_all=True)]
    for i in range(lr.N_PROMPT, lr.N_TOKENS):
        rows.append(m.eval(tok[i:i + 1], i, logits_all=True))
    return np.concatenate(rows)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---------------------------------------------------------------------------------------------- 1. read-back alone
@pytest.mark.parametrize("t", ALL_TYPES)
def test_get_tensor_returns_the_uploaded_bytes(L, wide, t):
    w = wide(t)
    m = g.FalconModel(w, n_ctx=N_CTX, n_batch=N_BATCH)
    try:
        _assert_matrices(m, HP_WIDE, w, "round trip of type %d" % t)
        with pytest.raises(KeyError):
            m.get_tensor("transformer.h.1.mlp.dense_4h_to_h.weight")
        with pytest.raises(KeyError):
            m.get_tensor("transformer.h.0.input_layernorm.weight")
    finally:
        m.free()


# ---------------------------------------------------------------------------------------------- 2. bytes
@pytest.mark.parametrize("rows", [None, 7])
@pytest.mark.parametrize("t", ALL_TYPES)
def test_merged_bytes_are_the_composed_expectation(L, wide, t, rows, tmp_path, monkeypatch):
    """every kind of target, one of them twice, r = 5 with scaling 3.2; the default chunk (one per matrix) and chunks of 7 rows (ragged last one);
    every matrix that is no target keeps its bytes"""
    w = wide(t)
    keys = [(0, "qkv"), (0, "down"), "lm_head", "tok_emb"]
    ad = lr.draw_adapter(HP_WIDE, keys, 5, seed=21 + t)
    again = lr.draw_adapter(HP_WIDE, keys[1:2], 5, seed=321 + t)
    pairs = [(k,) + ad[k] for k in keys] + [(keys[1],) + again[keys[1]]]
    path = str(tmp_path / "adapter.bin")
    lr.write_ggla(path, 5, 16, lr.adapter_records(pairs))
    want = lr.compose(w, pairs, 5, 16)
    if rows is None:
        monkeypatch.delenv("FALCON_HIP_LORA_ROWS", raising=False)
    else:
        monkeypatch.setenv("FALCON_HIP_LORA_ROWS", str(rows))
    m = g.FalconModel(w, n_ctx=N_CTX, n_batch=N_BATCH)
    try:
        before = m.weight_bytes()
        m.apply_lora(path)
        assert m.weight_bytes() == before
        for key in keys:
            assert not np.array_equal(_bytes(lr.get_matrix(want, key)), _bytes(lr.get_matrix(w, key)))
        _assert_matrices(m, HP_WIDE, want, "type %d, rows per chunk %s" % (t, rows))
    finally:
        m.free()


@pytest.mark.parametrize("r,a_f16", [(40, False), (41, False), (64, True)])
@pytest.mark.parametrize("t", [ob.Q8_0, lr.F16])
def test_rank_on_both_sides_of_the_lds_threshold(L, wide, t, r, a_f16, tmp_path):
    """k_lora_add keeps its A tile in LDS up to r = 40 and reads A through the cache beyond: the last r of the one form, the first of the other, and a
    larger one with an F16 loraA; scaling exactly 1 (alpha = r: no multiply) for r = 41"""
    w = wide(t)
    keys = [(0, "wo"), "lm_head"]
    ad = lr.draw_adapter(HP_WIDE, keys, r, seed=70 + r, a_f16=a_f16)
    pairs = [(k,) + ad[k] for k in keys]
    alpha = r if r == 41 else 16
    path = str(tmp_path / "adapter.bin")
    lr.write_ggla(path, r, alpha, lr.adapter_records(pairs))
    want = lr.compose(w, pairs, r, alpha)
    m = g.FalconModel(w, n_ctx=N_CTX, n_batch=N_BATCH)
    try:
        m.apply_lora(path)
        _assert_matrices(m, HP_WIDE, want, "type %d, r %d" % (t, r))
    finally:
        m.free()


# ---------------------------------------------------------------------------------------------- 3. the reference's logits after its own merge
@pytest.mark.parametrize("name", sorted(lr.CASES))
def test_reference_order_logits_are_the_references(L, cases, gold, name):
    c = cases(name)
    assert lr.sha256_file(c["model"]) == str(gold[name + ".model_sha256"]) and lr.sha256_file(c["adapter"]) == str(gold[name + ".adapter_sha256"]), "the inputs are not the recorded ones"
    if c["base"]:
        assert lr.sha256_file(c["base"]) == str(gold[name + ".base_sha256"])
    assert np.array_equal(c["tokens"], gold[name + ".tokens"])
    m = g.FalconModel(c["weights"], n_ctx=N_CTX, n_batch=N_BATCH)
    try:
        m.apply_lora(c["adapter"], base=c["base"])
        for key in dict.fromkeys(k for k, _, _ in c["pairs"]):
            n = lr.tensor_name(key)
            assert lr.sha256_bytes(m.get_tensor(n)) == str(gold["%s.sha.%s" % (name, n)]), "%s: %s is not the matrix the reference's merge leaves" % (name, n)
        L.ggml_hip_reference_order(1)
        try:
            got = _evaluate_12(m, c["tokens"])
        finally:
            L.ggml_hip_reference_order(0)
        assert _same_bits(got, gold[name + ".logits"]), "%s: worst difference %g" % (name, np.abs(got - gold[name + ".logits"]).max())
    finally:
        m.free()


# ---------------------------------------------------------------------------------------------- 4. default order: a model built from the composed weights
@pytest.mark.parametrize("name", ["q4_0", "q5_1", "q4_k", "f16", "base_f16_q4_0", "base_f32_q5_1"])
def test_default_order_logits_equal_a_model_of_the_composed_weights(L, cases, name):
    c = cases(name)
    composed = lr.compose_case(c)
    direct = g.FalconModel(composed, n_ctx=N_CTX, n_batch=N_BATCH)
    want = _evaluate_12(direct, c["tokens"])
    direct.free()
    plain = g.FalconModel(c["weights"], n_ctx=N_CTX, n_batch=N_BATCH)
    untouched = _evaluate_12(plain, c["tokens"])
    plain.apply_lora(c["adapter"], base=c["base"])
    got = _evaluate_12(plain, c["tokens"])
    plain.free()
    assert not np.array_equal(untouched, want)
    assert _same_bits(got, want)
    loaded = g.FalconModel.from_ggcc(c["model"], n_ctx=N_CTX, n_batch=N_BATCH)
    try:
        loaded.apply_lora(c["adapter"], base=c["base"])
        _assert_matrices(loaded, c["hp"], composed, name + " from its file")
        assert _same_bits(_evaluate_12(loaded, c["tokens"]), want)
    finally:
        loaded.free()


# ---------------------------------------------------------------------------------------------- 5. a live context
def test_contexts_and_captured_steps_survive_the_merge(L, cases):
    c = cases("q4_0")
    tok = c["tokens"]
    fresh = g.FalconModel(lr.compose_case(c), n_ctx=N_CTX, n_batch=N_BATCH)
    want_prompt = fresh.eval(tok[:9], 0, logits_all=True)
    want_ids = fresh.decode_greedy(tok[9], 9, 6, use_graph=True)
    m = g.FalconModel(c["weights"], n_ctx=N_CTX, n_batch=N_BATCH)
    try:
        before_prompt = m.eval(tok[:9], 0, logits_all=True)
        m.decode_greedy(tok[9], 9, 6, use_graph=True)
        captures = L.falcon_hip_context_graph_captures(m.ctx)
        assert captures >= 1
        m.apply_lora(c["adapter"])
        got_prompt = m.eval(tok[:9], 0, logits_all=True)
        got_ids = m.decode_greedy(tok[9], 9, 6, use_graph=True)
        assert L.falcon_hip_context_graph_captures(m.ctx) == captures, "the step captured before the merge was not replayed after it"
        assert not np.array_equal(before_prompt, got_prompt)
        assert _same_bits(got_prompt, want_prompt) and np.array_equal(got_ids, want_ids)
        # three lock-step sequences on the patched model against the fresh model's single context, sequence by sequence
        streams = [synth.tokens(4, c["hp"]["n_vocab"], seed=300 + t) for t in range(3)]
        sc = g.SeqContext(m, N_CTX, 3)
        rows = [sc.eval([s[i] for s in streams], i) for i in range(4)]
        for t, s in enumerate(streams):
            for i in range(4):
                assert _same_bits(rows[i][t], fresh.eval(s[i:i + 1], i, logits_all=True)[0]), (t, i)
        L.falcon_hip_context_free(sc.ctx)
    finally:
        m.free()
        fresh.free()


# ---------------------------------------------------------------------------------------------- 6. refusals change nothing
def test_refused_adapters_leave_the_model_untouched(L, cases, oracle, tmp_path):
    import ggcc_writer
    c = cases("q4_0")
    hp, w, tok = c["hp"], c["weights"], c["tokens"]
    corpus = [(label, path, code) for label, path, code in lr.damaged_corpus(str(tmp_path), hp) if code != 0]
    assert any(label == "second_pair_wrong_m" for label, _, _ in corpus)
    other = lr.build_case(oracle, "q5_1", str(tmp_path))                   # (a GQA model's adapter: every name exists here, no shape fits)
    corpus.append(("another_models_adapter", other["adapter"], lr.E_SHAPE))
    quantized_base, float_base = str(tmp_path / "base_q.bin"), str(tmp_path / "base_f.bin")
    ggcc_writer.write_ggcc(quantized_base, w)
    ggcc_writer.write_ggcc(float_base, synth.make_model_float(hp, seed=5, f16=True))
    m = g.FalconModel(w, n_ctx=N_CTX, n_batch=N_BATCH)
    f16m = g.FalconModel(cases("f16")["weights"], n_ctx=N_CTX, n_batch=N_BATCH)
    try:
        before = _evaluate_12(m, tok)
        for label, path, code in corpus:
            with pytest.raises(g.LoraError) as e:
                m.apply_lora(path)
            assert e.value.code == code, label
        for base, code in ((quantized_base, lr.E_BASE_TENSOR), (str(tmp_path / "no_such_base.bin"), lr.E_BASE_OPEN), (other["model"], lr.E_BASE_TENSOR)):
            with pytest.raises(g.LoraError) as e:
                m.apply_lora(c["adapter"], base=base)
            assert e.value.code == code, base
        with pytest.raises(g.LoraError) as e:
            f16m.apply_lora(cases("f16")["adapter"], base=float_base)
        assert e.value.code == lr.E_BASE_F16_DST
        _assert_matrices(m, hp, w, "after the refusals")
        _assert_matrices(f16m, hp, cases("f16")["weights"], "after the refusal (F16)")
        assert _same_bits(_evaluate_12(m, tok), before)
    finally:
        m.free()
        f16m.free()


# ---------------------------------------------------------------------------------------------- 7. a pipeline stage
def test_a_stage_patches_its_own_blocks_only(L, cases, tmp_path):
    c = cases("q4_0")
    hp, w = c["hp"], c["weights"]
    keys = [(0, "qkv"), (1, "qkv"), (1, "down"), "tok_emb", "lm_head"]
    ad = lr.draw_adapter(hp, keys, 3, seed=8)
    pairs = [(k,) + ad[k] for k in keys]
    path = str(tmp_path / "stage.bin")
    lr.write_ggla(path, 3, 16, lr.adapter_records(pairs))
    want = lr.compose(w, pairs, 3, 16)
    m = g.FalconModel(w, n_ctx=N_CTX, n_batch=N_BATCH, layer_begin=1)
    try:
        m.apply_lora(path)                                                  # block 0 and the embedding belong to another stage: skipped, no error
        _assert_matrices(m, hp, want, "stage [1, 2)", keys=[(1, "qkv"), (1, "wo"), (1, "up"), (1, "down"), "lm_head"])
        for key in ((0, "qkv"), "tok_emb"):
            with pytest.raises(KeyError):
                m.get_tensor(lr.tensor_name(key))
    finally:
        m.free()

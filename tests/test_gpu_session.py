"""GPU: session files on the device path. The staging kernels alone against the numpy restatement of the layout (tests/session_ref.py), bit for bit;
files written by the device against golden files the reference itself wrote (tests/golden/session.npz, scripts/gen_session_golden.py): the same
bytes in reference orders 1 and 2, loaded back into plain contexts and lock-step slots, continued greedily and sampled, loaded by the reference;
and every refusal at model level leaving the context as it was."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import ggllm_cpp_amd as g
import session_ref as sr
import synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libfalcon_ref.so")
MODELS = {"mqa_q4_0": (synth.HP_TINY_MQA, ob.Q4_0), "gqa_q5_1": (synth.HP_TINY_GQA, ob.Q5_1)}
N_CTX, N_BATCH, N_TOK = 32, 16, 12


@pytest.fixture(scope="module")
def L():
    L = g.load()
    L.ggml_hip_init(0)
    return L


@pytest.fixture(scope="module")
def weights(oracle):
    """the two golden models, made once (the drop-in tests' recipe)"""
    return {name: synth.make_model(oracle, hp, t, seed=4321) for name, (hp, t) in MODELS.items()}


@pytest.fixture(scope="module")
def gold(golden):
    d = golden["session"]
    return {k: d[k] for k in d.files}


def _golden_file(gold, name, tmp_path):
    path = str(tmp_path / (name + ".golden.session"))
    gold[name + "_file"].tofile(path)
    return path


def _model(weights, name, n_ctx=N_CTX, n_batch=N_BATCH, **kw):
    return g.FalconModel(weights[name], n_ctx=n_ctx, n_batch=n_batch, **kw)


def _evaluate_12(m, tokens):
    """what the reference did before it saved: 9 tokens in one call with every row's logits, then 3 single-token steps"""
    m.eval(tokens[:9], 0, logits_all=True)
    for i in range(9, N_TOK):
        m.eval_token(tokens[i], i)
    return m.logits()


# ---------------------------------------------------------------------------------------------- 1. the kernels alone
CANARY_STAGE, CANARY_CACHE = np.float32(-7.0), np.float32(-3.0)


@pytest.mark.parametrize("slots", [False, True])
@pytest.mark.parametrize("n_tok", [1, 3, 63, 64, 65, 130])
@pytest.mark.parametrize("n_head_kv", [1, 8])
def test_pack_and_unpack_against_the_layout(L, n_head_kv, n_tok, slots):
    """n_ctx 160 (the source pitch differs from n_tok), 2 layers, plain or slot 1 of 3: the first partial tile, the tile edge from both sides, an odd
    n_tok, more than one tile, the slot pitch. Every element distinct; canaries behind the staging floats, in the rows at and beyond n_tok and in
    the other slots"""
    n_ctx, n_layer, R = 160, 2, n_head_kv * 64
    n_seq, seq = (3, 1) if slots else (1, 0)
    rows, first = n_seq * n_ctx, seq * n_ctx
    n = n_layer * rows * R
    k = np.arange(n, dtype=np.float32).reshape(n_layer, rows, R)              # (< 2^24: every value exact and distinct)
    v = (np.arange(n, dtype=np.float32) + np.float32(8e6)).reshape(n_layer, rows, R)
    want = sr.staging(k, v, n_tok, first)
    assert want.size == 2 * n_layer * n_tok * R
    tail = 1024
    kb, vb = g.DevBuf(host=k), g.DevBuf(host=v)
    sb = g.DevBuf(host=np.full(want.size + tail, CANARY_STAGE, np.float32))
    assert g.kv_pack(kb, vb, sb, n_layer, n_head_kv, n_tok, rows, first) == 0
    got = sb.to_host(np.float32, (want.size + tail,))
    assert np.array_equal(got[:want.size].view(np.uint32), want.view(np.uint32))
    assert (got[want.size:] == CANARY_STAGE).all()
    # back: into caches full of canaries
    kd, vd = g.DevBuf(host=np.full(k.shape, CANARY_CACHE, np.float32)), g.DevBuf(host=np.full(v.shape, CANARY_CACHE, np.float32))
    assert g.kv_unpack(kd, vd, sb, n_layer, n_head_kv, n_tok, rows, first) == 0
    for dev, src in ((kd, k), (vd, v)):
        back = dev.to_host(np.float32, src.shape)
        exp = np.full(src.shape, CANARY_CACHE, np.float32)
        exp[:, first:first + n_tok] = src[:, first:first + n_tok]
        assert np.array_equal(back.view(np.uint32), exp.view(np.uint32))        # the rows, and nothing at or beyond n_tok or in slots 0 and 2
    # refusals launch nothing
    assert g.kv_pack(kb, vb, sb, n_layer, n_head_kv, n_tok, first + n_tok - 1, first) == 1
    assert g.kv_unpack(kd, vd, sb, 0, n_head_kv, n_tok, rows, first) == 1
    for b in (kb, vb, sb, kd, vd):
        b.free()


def test_sampler_generator_get_and_set(L):
    """ggml_hip_sampler_get_rng / set_rng: a row's 624 words and position, std::mt19937's after seeding; set moves one row only"""
    s = L.ggml_hip_sampler_create(2, 512, 32)
    p = g.sampling(seed=1)
    assert L.ggml_hip_sampler_set_row(s, 0, p, None, 0) == 0 and L.ggml_hip_sampler_set_row(s, 1, p, None, 0) == 0
    mt, pos = np.zeros(sr.MT_N, np.uint32), np.zeros(1, np.int32)
    assert L.ggml_hip_sampler_get_rng(s, 1, mt.ctypes.data, pos.ctypes.data) == 0
    seeded, at = sr.mt_seeded(1)
    assert pos[0] == at and np.array_equal(mt, seeded)
    other, _ = sr.mt_seeded(9)
    assert L.ggml_hip_sampler_set_rng(s, 1, other.ctypes.data, 17) == 0
    assert L.ggml_hip_sampler_get_rng(s, 1, mt.ctypes.data, pos.ctypes.data) == 0 and pos[0] == 17 and np.array_equal(mt, other)
    assert L.ggml_hip_sampler_get_rng(s, 0, mt.ctypes.data, pos.ctypes.data) == 0 and pos[0] == at and np.array_equal(mt, seeded)
    assert L.ggml_hip_sampler_set_rng(s, 1, other.ctypes.data, 625) == 1 and L.ggml_hip_sampler_set_rng(s, 2, other.ctypes.data, 0) == 1
    L.ggml_hip_sampler_free(s)


# ---------------------------------------------------------------------------------------------- 2. the same bytes as the reference
def _device_file(L, weights, gold, name, order, path):
    """the reference's run on the device in reference order `order`, saved"""
    tokens = gold[name + "_tokens"]
    L.ggml_hip_reference_order(order)
    try:
        m = _model(weights, name)
        _evaluate_12(m, tokens)
        m.set_sampling(g.sampling(seed=1))                           # the reference context's generator: seed 1, nothing drawn
        m.save_session(path, tokens[:N_TOK], logits_all=True)
        m.free()
    finally:
        L.ggml_hip_reference_order(0)
    return np.fromfile(path, np.uint8)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", list(MODELS))
def test_device_writes_the_bytes_the_reference_writes(L, weights, gold, tmp_path, name, order):
    got = _device_file(L, weights, gold, name, order, str(tmp_path / "s.session"))
    want = gold[name + "_file"]
    if got.size == want.size and not np.array_equal(got, want):      # say which section differs before failing
        _, _, a, off = sr.split_file(got)
        _, _, b, _ = sr.split_file(want)
        diff = [key for key in ("rng_text", "logits_cap", "kv_size", "n_tok") if a[key] != b[key]]
        diff += [key for key in ("logits", "k", "v") if not np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32))]
        print("sections that differ:", diff, "header equal:", np.array_equal(got[:off], want[:off]))
    assert got.size == want.size and np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------- 3. round trip
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", list(MODELS))
def test_reference_file_continues_on_the_device(L, weights, gold, tmp_path, name, order):
    """the reference's file into a fresh plain context and into slot 2 of three: the next step's logits are the reference's next step's"""
    path, tokens = _golden_file(gold, name, tmp_path), gold[name + "_tokens"]
    L.ggml_hip_reference_order(order)
    try:
        m = _model(weights, name)
        assert np.array_equal(m.load_session(path), tokens[:N_TOK])
        want_logits = sr.split_file(gold[name + "_file"])[2]["logits"]
        assert np.array_equal(m.logits().view(np.uint32), want_logits.view(np.uint32))       # the file's last row is what get_logits returns
        got = m.eval(tokens[N_TOK:N_TOK + 1], N_TOK)[0]
        assert np.array_equal(got.view(np.uint32), gold[name + "_next_logits"].view(np.uint32))
        sc = g.SeqContext(m, N_CTX, 3)
        assert np.array_equal(sc.load_session(2, path), tokens[:N_TOK])
        rows = sc.eval([tokens[0], tokens[0], tokens[N_TOK]], [0, 0, N_TOK])
        assert np.array_equal(rows[2].view(np.uint32), gold[name + "_next_logits"].view(np.uint32))
        sc.free()
        m.free()
    finally:
        L.ggml_hip_reference_order(0)


@pytest.mark.parametrize("name", list(MODELS))
def test_loaded_context_decodes_what_the_unstopped_one_does(L, weights, gold, tmp_path, name):
    """eight greedy tokens after a load equal those of the context that never stopped, with and without the captured step; a second load into the
    captured context moves no buffer: no new capture"""
    tokens, path = gold[name + "_tokens"], str(tmp_path / "s.session")
    m = _model(weights, name)
    _evaluate_12(m, tokens)
    m.save_session(path, tokens[:N_TOK])
    want = m.decode_greedy(tokens[N_TOK], N_TOK, 8)
    m.free()
    for use_graph in (False, True):
        m2 = _model(weights, name)
        assert np.array_equal(m2.load_session(path), tokens[:N_TOK])
        assert np.array_equal(m2.decode_greedy(tokens[N_TOK], N_TOK, 8, use_graph=use_graph), want)
        if use_graph:
            captures = g.graph_captures(m2)
            assert captures >= 1
            m2.load_session(path)
            assert np.array_equal(m2.decode_greedy(tokens[N_TOK], N_TOK, 8, use_graph=True), want)
            assert g.graph_captures(m2) == captures
        m2.free()


def test_state_blob_is_the_file_without_its_header(L, weights, gold, tmp_path):
    """copy_state / set_state: the blob is the file's tail, its size the announced one; a decode loop leaves no logits to save"""
    name, path = "mqa_q4_0", str(tmp_path / "s.session")
    tokens = gold[name + "_tokens"]
    m = _model(weights, name)
    _evaluate_12(m, tokens)
    m.save_session(path, tokens[:N_TOK], logits_all=True)
    blob = m.copy_state(N_TOK, logits_all=True)
    raw = np.fromfile(path, np.uint8)
    assert blob.size == L.falcon_hip_state_size(m.ctx, N_TOK, 1) and np.array_equal(raw[raw.size - blob.size:], blob)
    assert sr.split_state(bytes(blob), 2, 64)["logits"].size == 512
    want = m.decode_greedy(tokens[N_TOK], N_TOK, 4)
    assert sr.split_state(bytes(m.copy_state(N_TOK)), 2, 64)["logits"].size == 0
    m2 = _model(weights, name)
    assert m2.set_state(blob) == N_TOK
    assert np.array_equal(m2.decode_greedy(tokens[N_TOK], N_TOK, 4), want)
    m.free()
    m2.free()


# ---------------------------------------------------------------------------------------------- 4. sampled continuation
@pytest.mark.parametrize("name", list(MODELS))
def test_sampled_stream_continues_across_a_session(L, weights, gold, tmp_path, name):
    """default chain at temperature 0.8, seed 7: 6 tokens, save, load into a fresh context, set_sampling with the history (it keeps the loaded
    generator instead of seeding), 6 more: the 12 of the uninterrupted run"""
    prompt, path = [int(t) for t in gold[name + "_tokens"][:9]], str(tmp_path / "s.session")
    p = g.sampling(temp=0.8, seed=7)

    def start():
        m = _model(weights, name)
        m.eval(prompt, 0)
        m.set_sampling(p, history=prompt)
        return m, int(m.sample())
    m, t0 = start()
    whole = [t0] + [int(t) for t in m.decode_sample(t0, 9, 11)]
    m.free()
    m, t0b = start()
    first = [t0b] + [int(t) for t in m.decode_sample(t0b, 9, 5)]
    assert first == whole[:6]
    evaluated = prompt + first[:5]                                    # (the sixth is drawn, not evaluated yet)
    m.save_session(path, evaluated)
    m.free()
    m2 = _model(weights, name)
    assert [int(t) for t in m2.load_session(path)] == evaluated
    m2.set_sampling(p, history=prompt + first)
    rest = [int(t) for t in m2.decode_sample(first[5], len(evaluated), 6)]
    m2.free()
    assert first + rest == whole
    # ... and the generator is what made the difference: seeded afresh, the stream is another one
    m3 = _model(weights, name)
    m3.eval(evaluated, 0)
    m3.set_sampling(p, history=prompt + first)
    assert [int(t) for t in m3.decode_sample(first[5], len(evaluated), 6)] != rest
    m3.free()


# ---------------------------------------------------------------------------------------------- 5. the reference loads ours
_REF_LOADS = r"""
import ctypes as C, sys, numpy as np
so, model, nv, sess, out = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5]
nxt = np.array([int(sys.argv[6])], np.int32)
L = C.CDLL(so)
L.reff_load.restype = C.c_void_p; L.reff_load.argtypes = [C.c_char_p, C.c_int, C.c_int]
L.reff_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
L.reff_free.argtypes = [C.c_void_p]
L.llama_load_session_file.restype = C.c_bool; L.llama_load_session_file.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_void_p]
ctx = L.reff_load(model.encode(), 32, 16)
assert ctx
got, n = np.zeros(32, np.int32), C.c_size_t(0)
ok = bool(L.llama_load_session_file(ctx, sess.encode(), got.ctypes.data, 32, C.byref(n)))
lg = np.zeros((1, nv), np.float32)
if ok:
    assert L.reff_eval(ctx, nxt.ctypes.data, 1, int(n.value), 1, lg.ctypes.data) == 0
np.savez(out, ok=np.int64(ok), tokens=got[:n.value], logits=lg[0])
L.reff_free(ctx)
"""


@pytest.mark.parametrize("name", list(MODELS))
def test_the_reference_loads_a_device_written_file(L, weights, gold, tmp_path, name):
    """llama_load_session_file of the real reference (a child process) on the device's file: true, the 12 tokens, and its next step's logits are
    the golden ones"""
    if not os.path.exists(REF_SO):
        pytest.skip("oracle/_ref/libfalcon_ref.so was not built (make -C oracle ref_falcon in the dev container)")
    import ggcc_writer
    sess, model = str(tmp_path / "device.session"), str(tmp_path / (name + ".ggcc"))
    _device_file(L, weights, gold, name, 1, sess)
    ggcc_writer.write_ggcc(model, weights[name])
    script, out = str(tmp_path / "run.py"), str(tmp_path / "out.npz")
    open(script, "w").write(_REF_LOADS)
    tokens = gold[name + "_tokens"]
    r = subprocess.run([sys.executable, script, REF_SO, model, str(MODELS[name][0]["n_vocab"]), sess, out, str(int(tokens[N_TOK]))],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = np.load(out)
    assert res["ok"] == 1 and np.array_equal(res["tokens"], tokens[:N_TOK])
    assert np.array_equal(res["logits"].view(np.uint32), gold[name + "_next_logits"].view(np.uint32))


# ---------------------------------------------------------------------------------------------- 6. prefix sharing
def test_one_session_in_two_slots_next_to_another_prompt(L, weights, gold, tmp_path):
    """the session in slots 0 and 2, another prompt prefilled into slot 1, 6 lock-step greedy steps: slots 0 and 2 agree with each other and with
    the single stream that loaded the session, slot 1 with its own single stream"""
    name = "mqa_q4_0"
    path, tokens = _golden_file(gold, name, tmp_path), gold[name + "_tokens"]
    other = synth.tokens(7, 512, seed=5)
    m = _model(weights, name)
    m.load_session(path)
    own = m.decode_greedy(tokens[N_TOK], N_TOK, 6)
    sc = g.SeqContext(m, N_CTX, 3)
    for slot in (0, 2):
        sc.load_session(slot, path)
    m.eval(other[:6], 0)                                             # (the model's own context again: copy_seq wants contexts of one model)
    assert g.copy_seq(sc, 1, m, 0, 6) == 0
    others = m.decode_greedy(other[6], 6, 6)
    out = sc.decode_greedy([tokens[N_TOK], other[6], tokens[N_TOK]], [N_TOK, 6, N_TOK], 6)
    assert np.array_equal(out[:, 0], own) and np.array_equal(out[:, 2], own) and np.array_equal(out[:, 1], others)
    sc.free()
    m.free()


# ---------------------------------------------------------------------------------------------- 7. refusals at model level
def _pair(weights, name, n_ctx, tokens, n_eval):
    """two contexts in the same state: n_eval tokens evaluated, a sampler row seeded"""
    out = []
    for _ in range(2):
        m = _model(weights, name, n_ctx=n_ctx, n_batch=8)
        m.eval(tokens[:n_eval], 0, logits_all=False)
        m.set_sampling(g.sampling(temp=0.8, seed=3), history=tokens[:n_eval])
        out.append(m)
    return out


def _same_afterwards(a, b, token, n_past):
    """logits, cache and generator: the row get_logits returns, then three sampled steps"""
    assert np.array_equal(a.logits().view(np.uint32), b.logits().view(np.uint32))
    assert np.array_equal(a.decode_sample(token, n_past, 3), b.decode_sample(token, n_past, 3))


def test_refusals_return_their_code_and_change_nothing(L, weights, gold, tmp_path):
    name = "mqa_q4_0"
    path, tokens = _golden_file(gold, name, tmp_path), gold[name + "_tokens"]
    file_hp = g.SessionHParams(*struct.unpack_from("<9i", gold[name + "_file"].tobytes(), 8))
    # a session of 12 tokens into a context of 8: by its own record the hparams differ; with the file's record its 12 tokens exceed the 8 the
    # Python layer makes room for (n_ctx, as falcon_main does); with room for them, kv_ntok exceeds n_ctx
    a, b = _pair(weights, name, 8, tokens, 4)
    with pytest.raises(g.SessionError) as e:
        a.load_session(path)
    assert e.value.code == 2
    with pytest.raises(g.SessionError) as e:
        a.load_session(path, hparams=file_hp)
    assert e.value.code == 3
    got, n = np.full(N_CTX, -5, np.int32), np.zeros(1, np.int32)
    assert L.falcon_hip_session_load(a.ctx, 0, os.fsencode(path), file_hp, got.ctypes.data, N_CTX, n.ctypes.data) == 5
    assert (got == -5).all() and n[0] == 0
    blob = gold[name + "_file"][48 + 4 * N_TOK:]
    with pytest.raises(g.SessionError) as e:
        a.set_state(blob)                                            # (the blob alone: kv_ntok 12 of a context of 8 again)
    assert e.value.code == 5
    _same_afterwards(a, b, tokens[4], 4)
    a.free()
    b.free()
    # a record with another n_layer; a sequence out of range; both on a context the file would fit
    a, b = _pair(weights, name, N_CTX, tokens, 4)
    wrong = g.SessionHParams(*struct.unpack_from("<9i", gold[name + "_file"].tobytes(), 8))
    wrong.n_layer += 1
    with pytest.raises(g.SessionError) as e:
        a.load_session(path, hparams=wrong)
    assert e.value.code == 2
    for seq in (-1, 1):
        n = np.zeros(1, np.int32)
        got = np.full(N_CTX, -5, np.int32)
        assert L.falcon_hip_session_load(a.ctx, seq, os.fsencode(path), file_hp, got.ctypes.data, N_CTX, n.ctypes.data) == 18
        assert (got == -5).all() and n[0] == 0
        assert L.falcon_hip_session_save(a.ctx, seq, os.fsencode(str(tmp_path / "no.session")), file_hp, got.ctypes.data, 4, 0) == 18
        assert not os.path.exists(str(tmp_path / "no.session"))
    short = str(tmp_path / "short.session")
    gold[name + "_file"][:-5].tofile(short)
    with pytest.raises(g.SessionError) as e:
        a.load_session(short)
    assert e.value.code == 4
    _same_afterwards(a, b, tokens[4], 4)
    sc = g.SeqContext(a, N_CTX, 3)
    with pytest.raises(g.SessionError) as e:
        sc.load_session(3, path)
    assert e.value.code == 18
    sc.free()
    a.free()
    b.free()
    # a pipeline stage holds part of the layers: refused whichever part it is
    for lb, le in ((0, 1), (1, 2)):
        stage = g.FalconModel(weights[name], n_ctx=N_CTX, n_batch=1, layer_begin=lb, layer_end=le)
        with pytest.raises(g.SessionError) as e:
            stage.load_session(path)
        assert e.value.code == 17
        with pytest.raises(g.SessionError) as e:
            stage.save_session(str(tmp_path / "stage.session"), tokens[:4])
        assert e.value.code == 17 and not os.path.exists(str(tmp_path / "stage.session"))
        stage.free()


# ---------------------------------------------------------------------------------------------- 8. the examples
def _example(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def bpe_model(oracle, tmp_path_factory):
    """the tiny model with a real BPE vocabulary that the other example tests build"""
    import bpe_fixture
    import ggcc_writer
    vocab, merges = bpe_fixture.build(n_merges=308)
    hp = dict(synth.HP_TINY_MQA)
    hp["n_vocab"] = len(vocab)
    path = str(tmp_path_factory.mktemp("bpe") / "tiny_bpe.ggcc")
    ggcc_writer.write_ggcc(path, synth.make_model(oracle, hp, ob.Q4_0, seed=321), vocab, merges)
    return path


SYSTEM = "Once upon a time, in a land far away,"
PROMPTS = [SYSTEM + " there lived", SYSTEM + " a fox didn't jump", "hello world", SYSTEM[:-1]]


def test_generate_example_with_a_prompt_cache(L, bpe_model, tmp_path):
    """--prompt-cache: the first run writes the file, later runs load it and evaluate only what it does not hold -- the same tokens; the record of
    a GGCC file (falcon_hip_session_hparams_ggcc) is the one the file carries; -ro leaves the file alone, -all appends the generation"""
    gen = _example("falcon_generate")
    cache, n = str(tmp_path / "prompt.session"), 8
    want = gen.generate(bpe_model, PROMPTS[0], n, n_ctx=64)[1].tolist()
    ids, out, _ = gen.generate(bpe_model, PROMPTS[0], n, n_ctx=64, prompt_cache=cache)
    assert out.tolist() == want
    raw = open(cache, "rb").read()
    hp, tokens, st, _ = sr.split_file(raw)
    assert np.array_equal(tokens, ids) and st["n_tok"] == ids.size
    rec = g.session_hparams(path=bpe_model, n_ctx=64)
    assert tuple(getattr(rec, f) for f in sr.HP_FIELDS) == tuple(hp) and rec.n_bpe_merges == 308 and rec.ftype == 2 and rec.n_falcon_type == 7
    # the whole prompt is in the file: its last token is evaluated again, nothing is written
    assert gen.generate(bpe_model, PROMPTS[0], n, n_ctx=64, prompt_cache=cache)[1].tolist() == want
    assert open(cache, "rb").read() == raw
    # another prompt with the same beginning: the common prefix comes from the file; read-only keeps the file
    other = gen.generate(bpe_model, PROMPTS[1], n, n_ctx=64)[1].tolist()
    assert gen.generate(bpe_model, PROMPTS[1], n, n_ctx=64, prompt_cache=cache, prompt_cache_ro=True)[1].tolist() == other
    assert open(cache, "rb").read() == raw
    # -all: the file then holds the prompt and every generated token but the last (drawn, not evaluated), and continues from there
    no_eos = g.sampling(temp=0.0, repeat_penalty=1.0, seed=0, logit_bias={int(L.falcon_hip_token_eos()): float("-inf")})
    ids, out, _ = gen.generate(bpe_model, PROMPTS[0], n, n_ctx=64, prompt_cache=cache, prompt_cache_all=True, ignore_eos=True, sampling=no_eos)
    _, tokens, st, _ = sr.split_file(open(cache, "rb").read())
    assert out.size == n and tokens.tolist() == ids.tolist() + out.tolist()[:-1] and st["n_tok"] == tokens.size
    # a file of another n_ctx is refused by its record, whatever the prompt
    with pytest.raises(g.SessionError) as e:
        gen.generate(bpe_model, PROMPTS[0], n, n_ctx=48, prompt_cache=cache)
    assert e.value.code == 2


def test_batch_example_with_a_prefix_cache(L, bpe_model, tmp_path):
    """--prefix-cache: prompts that begin with the session's tokens prefill only their remainder behind its rows, the others whole: every
    continuation is the one without the flag"""
    gen, bat = _example("falcon_generate"), _example("falcon_batch_generate")
    cache, n = str(tmp_path / "system.session"), 6
    vocab = g.Vocab(bpe_model)
    try:
        sys_ids = vocab.tokenize(SYSTEM)
        assert all(np.array_equal(vocab.tokenize(p)[:sys_ids.size], sys_ids) for p in PROMPTS[:2])      # (the fixture's premise)
    finally:
        vocab.free()
    gen.generate(bpe_model, SYSTEM, 1, n_ctx=64, prompt_cache=cache)
    assert np.array_equal(sr.split_file(open(cache, "rb").read())[1], sys_ids)
    want = [r[1].tolist() for r in bat.generate_batch(bpe_model, PROMPTS, n, n_seq=3, n_ctx=64)]
    got = [r[1].tolist() for r in bat.generate_batch(bpe_model, PROMPTS, n, n_seq=3, n_ctx=64, prefix_cache=cache)]
    assert got == want

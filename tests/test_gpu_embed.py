"""GPU: embeddings on the device. The pooling kernels alone (ggml_hip_embed_pool_accum / _finish, csrc/kernels_embed.hip) against the numpy statement
of csrc/fq_embed.h (tests/embed_ref.py), bit for bit; then the model level: falcon_hip_get_embeddings against what the REAL reference returned from
falcon_get_embeddings (tests/golden/embedding.npz) in reference orders 1 and 2, against the oracle's LayerNorm of the device's own last hidden plane in
the default order, falcon_hip_embed, pooled vectors, the session file that carries the row, mode 0 launching what it always launched, and refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

import embed_ref as er
import ggllm_cpp_amd as g
import synth
from embed_ref import MODELS, bits, golden_model, oracle_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CTX, N_BATCH, N_PROMPT, N_TOK = 32, 16, 9, 12
GUARD = 64                 # canary values behind out[n_embd] and acc[n_embd]


@pytest.fixture(scope="module")
def L():
    L = g.load()
    L.ggml_hip_init(0)
    return L


# ---------------------------------------------------------------------------------------------- 1. the kernels alone
def _pool(L, x, splits, normalize):
    """(rc, out with its guard, acc with its guard, count) after the rows went in over the calls `splits` and one finish"""
    n_rows, E = x.shape
    xb = g.DevBuf(host=x)
    acc = g.DevBuf(host=np.concatenate([np.zeros(E, np.float64), np.full(GUARD, -7.0, np.float64)]))
    cnt = g.DevBuf(host=np.array([0, 0x5A5A5A5A5A5A5A5A], np.int64))
    out = g.DevBuf(host=np.full(E + GUARD, -3.0, np.float32))
    at = 0
    for k in splits:
        assert L.ggml_hip_embed_pool_accum(xb.ptr + 4 * at * E, k, E, acc.ptr, cnt.ptr) == 0
        at += k
    rc = L.ggml_hip_embed_pool_finish(acc.ptr, cnt.ptr, E, 1 if normalize else 0, out.ptr)
    L.ggml_hip_synchronize()
    res = rc, out.to_host(np.float32, (E + GUARD,)), acc.to_host(np.float64, (E + GUARD,)), cnt.to_host(np.int64, (2,))
    for b in (xb, acc, cnt, out):
        b.free()
    return res


@pytest.fixture(scope="module")
def cases():
    """every operator case's rows and expectation, made once: {(n_embd, n_rows): (rows, acc, mean, unit)}"""
    out = {}
    for E, n in er.CASE_SHAPES:
        x = er.case_rows(E, n, er.case_seed(E, n))
        acc, cnt = er.accumulate(x)
        m = er.mean(acc, cnt)
        assert er.order_free(m)                        # (chosen on the CPU: tests/test_embed_cpu.py::test_operator_cases_are_order_free)
        out[(E, n)] = (x, acc, m, er.unit(m))
    return out


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("n_embd,n_rows", er.CASE_SHAPES)
def test_pool_kernels_against_the_reference_statement(L, cases, n_embd, n_rows, split):
    x, acc_want, mean_want, unit_want = cases[(n_embd, n_rows)]
    splits = er.case_splits(n_rows) if split else [n_rows]
    for normalize, want in ((False, mean_want), (True, unit_want)):
        rc, out, acc, cnt = _pool(L, x, splits, normalize)
        assert rc == 0 and cnt[0] == n_rows and cnt[1] == 0x5A5A5A5A5A5A5A5A
        assert np.array_equal(acc[:n_embd].view(np.uint64), acc_want.view(np.uint64))
        assert np.array_equal(bits(out[:n_embd]), bits(want))
        assert (out[n_embd:] == -3.0).all() and (acc[n_embd:] == -7.0).all()       # the guard regions
    if n_rows >= 3:                                    # the order-sensitive column: 0 in row order (1 / n_rows in another)
        for col in {0, 63, 64, n_embd - 1} & set(range(n_embd)):
            assert acc_want[col] == 0.0 and mean_want[col] == 0.0


def test_pool_finish_refuses_nothing_pooled_and_the_zero_vector(L, capfd):
    E = 256
    acc = g.DevBuf(host=np.zeros(E, np.float64))
    cnt = g.DevBuf(host=np.zeros(1, np.int64))
    out = g.DevBuf(host=np.full(E, -3.0, np.float32))
    for normalize in (0, 1):
        assert L.ggml_hip_embed_pool_finish(acc.ptr, cnt.ptr, E, normalize, out.ptr) == 1              # count == 0
    zeros = g.DevBuf(host=np.zeros((3, E), np.float32))
    assert L.ggml_hip_embed_pool_accum(zeros.ptr, 3, E, acc.ptr, cnt.ptr) == 0
    assert L.ggml_hip_embed_pool_finish(acc.ptr, cnt.ptr, E, 1, out.ptr) == 2                          # s == 0: refused, not divided
    assert (out.to_host(np.float32, (E,)) == -3.0).all()
    assert L.ggml_hip_embed_pool_finish(acc.ptr, cnt.ptr, E, 0, out.ptr) == 0                          # the mean of zeros is fine
    assert (out.to_host(np.float32, (E,)) == 0.0).all()
    assert L.ggml_hip_embed_pool_accum(None, 3, E, acc.ptr, cnt.ptr) == 1 and L.ggml_hip_embed_pool_accum(zeros.ptr, 0, E, acc.ptr, cnt.ptr) == 1
    err = capfd.readouterr().err
    assert "no rows were pooled" in err and "zero vector" in err
    for b in (acc, cnt, out, zeros):
        b.free()


# ---------------------------------------------------------------------------------------------- 2. the model level
@pytest.fixture(scope="module")
def weights(oracle):
    return {name: golden_model(oracle, name)[1] for name in MODELS}


@pytest.fixture(scope="module")
def gold(golden):
    d = golden["embedding"]
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def text25(oracle, weights):
    """a 25-token text per model and the reference-order ln_f rows of its positions, evaluated as 16 + 9 (the oracle, which test_embed_cpu.py pins on the
    reference's rows), made once"""
    out = {}
    for name, w in weights.items():
        toks = synth.tokens(25, w["hparams"]["n_vocab"], seed=77)
        out[name] = (toks, oracle_rows(oracle, w, toks, [16, 9], N_CTX))
    return out


def _model(weights, name, **kw):
    return g.FalconModel(weights[name], n_ctx=N_CTX, n_batch=N_BATCH, **kw)


def _rows_of_run(m, tokens, step):
    """the golden run: the embedding after the 9-token eval and after each single-token step (`step`: FalconModel.eval or eval_token)"""
    m.eval(tokens[:N_PROMPT], 0, logits_all=True)
    rows = [m.embeddings()]
    for i in range(N_PROMPT, N_TOK):
        if step == "eval":
            m.eval(tokens[i:i + 1], i, logits_all=True)
        else:
            m.eval_token(tokens[i], i)
        rows.append(m.embeddings())
    return np.stack(rows)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_embedding_is_the_reference_row(L, weights, gold, name, order):
    """falcon_hip_eval's default forms, the captured single-token step (falcon_hip_eval_token), use_graph off and on, and the op-list step"""
    tokens, want = gold[name + "_tokens"], gold[name + "_emb"]
    L.ggml_hip_reference_order(order)
    try:
        for step, use_graph, fused in (("eval", 0, None), ("eval", 1, None), ("token", 1, None), ("eval", 0, 0), ("token", 0, 0)):
            m = _model(weights, name)
            assert m.embeddings() is None
            m.set_embedding(last=True)
            assert m.embeddings() is None              # on, but nothing evaluated yet
            L.falcon_hip_context_use_graph(m.ctx, use_graph)
            if fused is not None:
                m.set_fused(fused)
            got = _rows_of_run(m, tokens, step)
            m.free()
            assert np.array_equal(bits(got), bits(want)), (step, use_graph, fused)
    finally:
        L.ggml_hip_reference_order(0)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_embedding_in_the_default_order_is_ln_f_of_the_last_plane(L, oracle, weights, gold, name):
    """... of the device's own last hidden plane, through the oracle's LayerNorm; every single-token form leaves the same row"""
    tokens, w = gold[name + "_tokens"], weights[name]
    m = _model(weights, name)
    m.set_embedding(last=True)
    _, hid = m.eval(tokens[:N_PROMPT], 0, want_hidden=True)
    want = oracle.layer_norm(hid[-1], w["out_norm_w"], w["out_norm_b"])[-1]
    assert np.array_equal(bits(m.embeddings()), bits(want))
    _, hid = m.eval(tokens[N_PROMPT:N_PROMPT + 1], N_PROMPT, want_hidden=True)
    want1 = oracle.layer_norm(hid[-1], w["out_norm_w"], w["out_norm_b"])[-1]
    assert np.array_equal(bits(m.embeddings()), bits(want1))
    for fused in (0, 1, 2, 3):                         # op list, three, two and one launch per block: the same step again
        m.set_fused(fused)
        m.eval(tokens[N_PROMPT:N_PROMPT + 1], N_PROMPT)
        assert np.array_equal(bits(m.embeddings()), bits(want1)), fused
        m.eval_token(tokens[N_PROMPT], N_PROMPT)
        assert np.array_equal(bits(m.embeddings()), bits(want1)), fused
    assert m.sync_error() == 0
    m.free()


def _kv_bytes(m, n_tok):
    """the K and V sections of the state blob: the cache rows [0, n_tok) as ggml_hip_kv_pack's kernel reads them (the caches' addresses are the context's own)"""
    hp = m.hp
    kvb = hp["n_layer"] * n_tok * hp["n_head_kv"] * 64 * 4
    return bytes(m.copy_state(n_tok)[-2 * kvb:])


@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_embed_is_eval_without_the_head(L, weights, gold, name, order):
    tokens = gold[name + "_tokens"]
    L.ggml_hip_reference_order(order)
    try:
        a, b = _model(weights, name), _model(weights, name)
        for m in (a, b):
            m.set_embedding(last=True)
        a.eval(tokens[:N_PROMPT], 0)
        b.embed_tokens(tokens[:N_PROMPT], 0)
        assert np.array_equal(bits(a.embeddings()), bits(b.embeddings()))
        assert not L.falcon_hip_get_logits(b.ctx)      # NULL, as after falcon_hip_eval_score
        for i in range(N_PROMPT, N_TOK):
            a.eval(tokens[i:i + 1], i)
            b.embed_tokens(tokens[i:i + 1], i)
            assert np.array_equal(bits(a.embeddings()), bits(b.embeddings()))
            assert not L.falcon_hip_get_logits(b.ctx)
        assert _kv_bytes(a, N_TOK) == _kv_bytes(b, N_TOK)
        if order == 2:
            assert np.array_equal(bits(b.embeddings()), bits(gold[name + "_emb"][-1]))
        # ... and the cache it wrote serves a later eval: the next logits are those behind falcon_hip_eval's cache
        la, lb = a.eval(tokens[N_TOK:N_TOK + 1], N_TOK), b.eval(tokens[N_TOK:N_TOK + 1], N_TOK)
        assert np.array_equal(bits(la), bits(lb))
        b.set_embedding(last=False)
        t = np.ascontiguousarray(tokens[:2], np.int32)
        assert L.falcon_hip_embed(b.ctx, t.ctypes.data, 2, 0) == 1         # no mode set: refused
        a.free(); b.free()
    finally:
        L.ggml_hip_reference_order(0)


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_pooled_vector_of_a_text_in_two_calls(L, oracle, weights, text25, name, order):
    toks, ref_rows = text25[name]
    w = weights[name]
    L.ggml_hip_reference_order(order)
    try:
        m = _model(weights, name)
        if order == 0:                                 # the default order: the device's own last planes through the oracle's LayerNorm
            planes = [m.eval(toks[:16], 0, want_hidden=True)[1][-1], m.eval(toks[16:], 16, want_hidden=True)[1][-1]]
            rows = oracle.layer_norm(np.concatenate(planes), w["out_norm_w"], w["out_norm_b"])
        else:
            rows = ref_rows
        m.set_embedding(last=True, pool=True)
        assert m.pool_count() == 0
        with pytest.raises(ValueError):
            m.pooled(False)                            # nothing pooled yet
        m.embed_tokens(toks[:16], 0)
        m.embed_tokens(toks[16:], 16)
        assert m.pool_count() == 25
        assert np.array_equal(bits(m.pooled(False)), bits(er.pooled(rows, False, [16, 9])))
        assert np.array_equal(bits(m.pooled(True)), bits(er.pooled(rows, True, [16, 9])))
        assert np.array_equal(bits(m.embeddings()), bits(rows[-1]))
        m.pool_reset()
        assert m.pool_count() == 0
        m.eval(toks[:16], 0)                           # falcon_hip_eval pools as well
        if order == 0:
            m.eval(toks[16:], 16)
            assert m.pool_count() == 25
            assert np.array_equal(bits(m.pooled(True)), bits(er.pooled(rows, True, [16, 9])))
        else:                                          # ... and a single-token step adds its one row (the reference's orders: a row does not depend on its batch)
            m.eval(toks[16:17], 16)
            assert m.pool_count() == 17
            assert np.array_equal(bits(m.pooled(True)), bits(er.pooled(rows[:17], True, [16, 1])))
        # FalconModel.embed: chunks of n_batch from an empty context
        assert np.array_equal(bits(m.embed(toks, pool="mean", normalize=True)), bits(er.pooled(rows, True, [16, 9])))
        assert np.array_equal(bits(m.embed(toks, pool="last", normalize=False)), bits(rows[-1]))
        m.free()
    finally:
        L.ggml_hip_reference_order(0)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_session_file_carries_the_row(L, weights, gold, tmp_path, name, order):
    tokens, want_file = gold[name + "_tokens"], gold[name + "_file"]
    E = weights[name]["hparams"]["n_embd"]
    golden_path, path = str(tmp_path / "golden.session"), str(tmp_path / "device.session")
    want_file.tofile(golden_path)
    L.ggml_hip_reference_order(order)
    try:
        m = _model(weights, name)
        size0 = L.falcon_hip_state_size(m.ctx, N_TOK, 1)
        m.set_embedding(last=True)
        assert L.falcon_hip_state_size(m.ctx, N_TOK, 1) == size0 + 4 * E
        _rows_of_run(m, tokens, "eval")
        m.set_sampling(g.sampling(seed=1))             # the reference context's generator: seed 1, nothing drawn
        m.save_session(path, tokens[:N_TOK], logits_all=True)
        got = np.fromfile(path, np.uint8)
        assert got.size == want_file.size and np.array_equal(got, want_file)
        m.free()
        # the reference's file into a fresh context: the row without an eval, then the reference's next step
        m = _model(weights, name)
        m.set_embedding(last=True)
        assert np.array_equal(m.load_session(golden_path), tokens[:N_TOK])
        assert np.array_equal(bits(m.embeddings()), bits(gold[name + "_emb"][-1]))
        nxt = m.eval(tokens[N_TOK:N_TOK + 1], N_TOK)[0]
        assert np.array_equal(bits(nxt), bits(gold[name + "_next_logits"]))
        assert np.array_equal(bits(m.embeddings()), bits(gold[name + "_next_emb"]))
        # ... and the state blob alone
        blob = m.copy_state(N_TOK + 1, logits_all=True)
        m2 = _model(weights, name)
        with pytest.raises(g.SessionError) as e:
            m2.set_state(blob)                         # a context that keeps no row takes no blob with one
        assert e.value.code == 7
        m2.set_embedding(last=True)
        assert m2.set_state(blob) == N_TOK + 1
        assert np.array_equal(bits(m2.embeddings()), bits(gold[name + "_next_emb"]))
        m2.free()
        # mode 0: refused with code 7, nothing changed
        m.set_embedding(last=False)
        before = m.copy_state(N_TOK + 1, logits_all=True).tobytes()
        with pytest.raises(g.SessionError) as e:
            m.load_session(golden_path)
        assert e.value.code == 7
        assert m.copy_state(N_TOK + 1, logits_all=True).tobytes() == before
        # a file without the row is refused while the mode is set
        m.save_session(path, tokens[:N_TOK], logits_all=True)
        m.set_embedding(last=True)
        with pytest.raises(g.SessionError) as e:
            m.load_session(path)
        assert e.value.code == 7
        m.free()
    finally:
        L.ggml_hip_reference_order(0)


def test_off_is_off(L, weights, gold):
    """mode 0: no row, and the captured graphs of an eval / step sequence are those of a context that never had a mode: one capture for the single-token
    step (the batch eval is plain launches), not one more after the mode went on and off again"""
    name = "mqa_q4_0"
    tokens = gold[name + "_tokens"]

    def run(m):
        m.eval(tokens[:N_PROMPT], 0)
        for i in range(N_PROMPT, N_TOK):
            m.eval_token(tokens[i], i)
        return m.logits()

    fresh, m = _model(weights, name), _model(weights, name)
    want = run(fresh)
    assert g.graph_captures(fresh) == 1 and fresh.embeddings() is None
    m.set_embedding(last=True); m.set_embedding(last=False)                # on and off before anything ran
    assert np.array_equal(bits(run(m)), bits(want)) and g.graph_captures(m) == 1 and m.embeddings() is None
    m.set_embedding(last=True, pool=True)
    assert np.array_equal(bits(run(m)), bits(want)) and g.graph_captures(m) == 2      # the step with the row: a graph of its own
    assert m.embeddings() is not None
    m.set_embedding(last=False)
    assert np.array_equal(bits(run(m)), bits(want)) and g.graph_captures(m) == 2      # back to the graph captured first
    assert m.embeddings() is None and m.pool_count() == N_TOK                          # (what was pooled stays until pool_reset)
    m.set_embedding(last=True, pool=True)
    assert np.array_equal(bits(run(m)), bits(want)) and g.graph_captures(m) == 2      # ... and to the one with the row
    fresh.free(); m.free()


def test_refusals(L, weights, gold, capfd):
    name = "mqa_q4_0"
    tokens = gold[name + "_tokens"]
    m = _model(weights, name)
    # a lock-step context, a pipeline stage, an unknown bit: 1, a message, the mode stays 0
    sc = g.SeqContext(m, N_CTX, 3)
    assert L.falcon_hip_context_set_embedding(sc.ctx, 1) == 1
    assert "lock-step" in capfd.readouterr().err
    sc.free()
    stage = g.FalconModel(weights[name], n_ctx=N_CTX, n_batch=N_BATCH, layer_begin=0, layer_end=1)
    assert L.falcon_hip_context_set_embedding(stage.ctx, 1) == 1
    assert "pipeline stage" in capfd.readouterr().err
    stage.free()
    assert L.falcon_hip_context_set_embedding(m.ctx, 4) == 1 and not L.falcon_hip_get_embeddings(m.ctx)
    capfd.readouterr()
    # the decode loops, the swap and perplexity while a mode is set: their code, a message, nothing evaluated
    m.eval(tokens[:N_PROMPT], 0)
    m.set_embedding(last=True)
    m.set_sampling(g.sampling(seed=1))
    before = m.copy_state(N_PROMPT + 3).tobytes()
    out = np.full(3, -5, np.int32)
    t = np.ascontiguousarray(tokens, np.int32)
    for use_graph in (0, 1):
        L.falcon_hip_context_use_graph(m.ctx, use_graph)
        assert L.falcon_hip_decode_greedy(m.ctx, int(tokens[N_PROMPT]), N_PROMPT, 3, out.ctypes.data) == 1
        assert L.falcon_hip_decode_sample(m.ctx, int(tokens[N_PROMPT]), N_PROMPT, 3, out.ctypes.data) == 1
    assert L.falcon_hip_context_swap(m.ctx, 0, 4, t.ctypes.data, 2, 2) == 1
    nll = np.zeros(1, np.float64)
    assert L.falcon_hip_perplexity(m.ctx, t.ctypes.data, 12, 12, 12, nll.ctypes.data) == -1
    n_out = np.zeros(1, np.int32)
    assert L.falcon_hip_decode_spec(m.ctx, int(tokens[N_PROMPT]), N_PROMPT, 3, out.ctypes.data, n_out.ctypes.data) == 1      # (not on, or refused: 1 either way)
    err = capfd.readouterr().err
    assert err.count("refused while an embedding mode is set") == 6
    assert (out == -5).all() and m.copy_state(N_PROMPT + 3).tobytes() == before and m.embeddings() is None
    m.set_embedding(last=False)
    assert L.falcon_hip_decode_greedy(m.ctx, int(tokens[N_PROMPT]), N_PROMPT, 3, out.ctypes.data) == 0 and (out >= 0).all()
    m.free()


# ---------------------------------------------------------------------------------------------- 3. the link-time wrap
_WRAP_SCRIPT = r"""
import ctypes as C, os, sys, numpy as np
so, path, nv, ne, out = sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), sys.argv[7]
toks = np.ascontiguousarray(np.load(sys.argv[6]), np.int32)
L = C.CDLL(so)
# (the linker's --wrap redirects the calls made inside the library; from outside the wrapped entries are reached by their own names)
init, get_emb = getattr(L, "__wrap_falcon_init_from_file"), getattr(L, "__wrap_falcon_get_embeddings")
class Params(C.Structure):
    # falcon_context_params of a -DGGML_USE_CUBLAS build: LLAMA_MAX_DEVICES is GGML_CUDA_MAX_DEVICES, 16 (libfalcon.h:6-10, :92-113)
    _fields_ = [(n, C.c_int) for n in ("n_ctx", "n_batch", "n_gpu_layers", "i_gpu_start", "i_gpu_last", "main_gpu")] + [("tensor_split", C.c_float * 16), ("seed", C.c_int)] + \
               [(n, C.c_bool) for n in ("f16_kv", "logits_all", "vocab_only", "use_mmap", "use_mlock", "embedding")] + [("progress_callback", C.c_void_p), ("progress_callback_user_data", C.c_void_p)]
L.falcon_context_default_params.restype = Params
init.restype = C.c_void_p; init.argtypes = [C.c_char_p, Params]
L.reff_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
L.reff_free.argtypes = [C.c_void_p]
get_emb.restype = C.POINTER(C.c_float); get_emb.argtypes = [C.c_void_p]
L.falcon_init_backend()
p = L.falcon_context_default_params()
got = (p.n_ctx, p.n_batch, p.n_gpu_layers, p.i_gpu_start, p.i_gpu_last, p.main_gpu, sum(p.tensor_split), p.seed, p.f16_kv, p.logits_all, p.vocab_only,
       p.use_mmap, p.use_mlock, p.embedding, p.progress_callback, p.progress_callback_user_data)
assert got == (512, 512, 0, -1, -1, 0, 0.0, -1, False, False, False, True, False, False, None, None), got      # the mirror's layout (libfalcon.cpp:1387-1405)
p.n_ctx, p.n_batch, p.n_gpu_layers, p.seed = 32, 16, 100, 1
p.f16_kv, p.logits_all, p.embedding = False, True, sys.argv[8] == "1"
ctx = init(os.fsencode(path), p)
assert ctx
def ev(t, n_past):
    lg = np.zeros((len(t), nv), np.float32)
    assert L.reff_eval(ctx, t.ctypes.data, len(t), n_past, 1, lg.ctypes.data) == 0
    e = get_emb(ctx)
    return np.ctypeslib.as_array(e, (ne,)).copy() if e else None
rows = [ev(toks[:9], 0)] + [ev(toks[i:i + 1], i) for i in range(9, 12)]
if rows[0] is None:
    print("no embeddings")
else:
    np.save(out, np.stack(rows))
L.reff_free(ctx)
"""


@pytest.mark.parametrize("order", ["1", "2"])
def test_wrap_returns_the_reference_row(oracle, weights, gold, tmp_path, order):
    """the reference's falcon_init_from_file / falcon_eval / falcon_get_embeddings with csrc/falcon_wrap.cpp linked in (oracle/_ref/libfalcon_ref_hip.so):
    a context prepared with params.embedding returns the golden rows; one without it is refused with a message, as before"""
    import ggcc_writer
    lib = os.path.join(ROOT, "oracle", "_ref", "libfalcon_ref_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libfalcon_ref_hip.so was not built (make -C oracle ref_falcon_hip in the dev container)")
    if b"falcon_hip_context_set_embedding" not in open(lib, "rb").read():
        # (the objects are built where the reference's sources are and shipped; ones linked with an earlier csrc/falcon_wrap.cpp never ask the library for the mode)
        pytest.skip("oracle/_ref/libfalcon_ref_hip.so predates the embedding wrap (make -C oracle ref_falcon_hip)")
    name = "gqa_q5_1"
    hp = weights[name]["hparams"]
    path, toks, out, script = (str(tmp_path / n) for n in ("m.ggcc", "toks.npy", "emb.npy", "run.py"))
    ggcc_writer.write_ggcc(path, weights[name])
    np.save(toks, gold[name + "_tokens"])
    open(script, "w").write(_WRAP_SCRIPT)
    env = dict(os.environ, GGML_HIP_REFERENCE_ORDER=order)
    r = subprocess.run([sys.executable, script, ROOT, lib, path, str(hp["n_vocab"]), str(hp["n_embd"]), toks, out, "1"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "resident on the device" in r.stderr
    assert "no embeddings" not in r.stdout, r.stderr[-3000:]           # falcon_get_embeddings answered NULL for a context made with params.embedding
    assert np.array_equal(bits(np.load(out)), bits(gold[name + "_emb"]))
    if order == "1":
        r = subprocess.run([sys.executable, script, ROOT, lib, path, str(hp["n_vocab"]), str(hp["n_embd"]), toks, out, "0"], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "no embeddings" in r.stdout and "falcon_get_embeddings is not supported for a context evaluated on the device" in r.stderr

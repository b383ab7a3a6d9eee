"""GPU: constrained decoding on the device (csrc/fq_grammar.h: the index built by k_grammar_index, k_sample_rows' MASK instantiations).
The contract is "as if the row had a -inf bias on every token its state forbids": a sampler with grammars is compared, draw for draw,
with one that has none and is given the same logits rows with -inf written where tests/grammar_ref.py says the token is forbidden."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ggllm_cpp_amd as g
import grammar_ref as ref
import sample_ref
import stop_text_ref
import synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

V, R, N_DRAWS, EOS = 300, 5, 24, 0           # EOS: the token without bytes


@pytest.fixture(scope="module")
def L():
    L = g.load()
    L.ggml_hip_init(0)
    return L


@pytest.fixture(scope="module")
def vocab():
    return ref.vocab300(np.random.default_rng(11))


# ---------------------------------------------------------------------------------------------- 1. the index
@pytest.mark.parametrize("n_vocab", [300, 65])
def test_index_equals_restatement(L, vocab, n_vocab):
    """automata of 2, 3, 65 and 700 states (whole and partial tiles of 16 states, 5 and 2 index words: whole and partial workgroups, a
    partial last word)"""
    voc = vocab[:n_vocab]
    for pattern, n_states in ((b"[abcd]*", 2), (b"a", 3), (b"[abcd]{63}", 65), (b"[ab]{698}", 700)):
        d = g.regex_dfa(pattern)
        assert d.n_states == n_states
        gr = g.Grammar.make(voc, d, EOS)
        try:
            got = gr.index()
            want = ref.index(d.trans, d.accept, EOS, voc)
            assert got.shape == want.shape == (n_states, (n_vocab + 63) // 64)
            assert np.array_equal(got, want), pattern
            assert np.array_equal(gr.index(1, 1), want[1:2]) and not got[0].any()
        finally:
            gr.free()


# ---------------------------------------------------------------------------------------------- 2. the sampler against -inf rows
SPARSE = [b"(ab|cd)+", b"[abcd]{0,70}", b"a(b|c)d*", b"\\xff\\x00"]       # the last: exactly one token allowed, then one, then only EOS
DENSE = [b"[abcd]*", b"([abcd][abcd])*", b"[abcd]*d[abcd]*", b"[abcd]*a[abcd]"]  # every state allows every token over a..d (>= 128), the states still move
PEN = dict(repeat_penalty=1.3, repeat_last_n=16, frequency_penalty=0.25, presence_penalty=0.5)
CONFIGS = {
    "greedy": (SPARSE, lambda i: g.sampling_ext(temp=0.0, seed=10 + i, **PEN)),
    "top_k_top_p": (SPARSE, lambda i: g.sampling_ext(temp=0.8, top_k=40, top_p=0.95, seed=20 + i, logit_bias={7: 1.5, 30: float("-inf")}, **PEN)),
    "hbm_sort": (SPARSE, lambda i: g.sampling_ext(temp=0.9, top_k=0, top_p=0.9, seed=30 + i, **PEN)),
    "tfs_typical": (DENSE, lambda i: g.sampling_ext(tfs_z=0.9, typical_p=0.8, temp=0.8, top_k=40, top_p=0.95, seed=40 + i, **PEN)),
    "mirostat2": (DENSE, lambda i: g.sampling_ext(mirostat=2, mirostat_tau=4.0, mirostat_eta=0.2, temp=0.9, seed=50 + i, **PEN)),
}


def rng_of(L, s, row):
    w, p = np.zeros(624, np.uint32), C.c_int32(0)
    assert L.ggml_hip_sampler_get_rng(s, row, w.ctypes.data, C.byref(p)) == 0
    return w.tolist(), p.value


def states_of(L, s, n=R):
    st = np.zeros(n, np.int32)
    assert L.ggml_hip_sampler_get_grammar_state(s, st.ctypes.data) == 0
    return st.tolist()


class Allow:
    """grammar_ref.allowed_row per (automaton, state), computed once"""

    def __init__(self, vocab):
        self.vocab, self.memo = vocab, {}

    def __call__(self, k, d, state):
        if (k, state) not in self.memo:
            self.memo[(k, state)] = ref.allowed_row(d.trans, d.accept, state, EOS, self.vocab)
        return self.memo[(k, state)]


@pytest.mark.parametrize("config", list(CONFIGS))
def test_sampler_equals_plain_sampler_on_minus_inf_rows(L, vocab, config):
    """rows 0..3 of sampler A hold grammars, row 4 none; sampler B holds none and gets A's rows with the forbidden entries at -inf. 24 draws:
    tokens, A's states, then the generators and mu. (The window has no getter: with penalties over 16 tokens its effects are in the draws.)"""
    patterns, params = CONFIGS[config]
    dfas = [g.regex_dfa(p) for p in patterns]
    grammars = [g.Grammar.make(vocab, d, EOS) for d in dfas]
    allow = Allow(vocab)
    rng = np.random.default_rng(len(config))
    A, B = L.ggml_hip_sampler_create(R, V, 32), L.ggml_hip_sampler_create(R, V, 32)
    lgA, lgB, tkA, tkB = g.DevBuf(R * V * 4), g.DevBuf(R * V * 4), g.DevBuf(R * 4), g.DevBuf(R * 4)
    try:
        for r in range(R):
            h = np.ascontiguousarray(rng.integers(3, V, 16), np.int32)
            p = params(r)
            for s in (A, B):
                assert L.ggml_hip_sampler_set_row_ext(s, r, C.byref(p), h.ctypes.data, h.size) == 0
        assert states_of(L, A) == [-1] * R
        for r in range(4):
            assert L.ggml_hip_sampler_set_grammar(A, r, grammars[r].h, -1) == 0
        state = [d.start for d in dfas]
        assert states_of(L, A) == state + [-1] and states_of(L, B) == [-1] * R
        one_allowed = only_eos = 0
        for draw in range(N_DRAWS):
            x = np.stack([sample_ref.tie_free_row(rng, V, 3.0) for _ in range(R)])
            y = x.copy()
            for r in range(4):
                ok = allow(r, dfas[r], state[r])
                assert ok.any() and (config not in ("tfs_typical", "mirostat2") or ok.sum() >= 128)
                one_allowed += int(ok.sum() == 1 and not ok[EOS])
                only_eos += int(ok.sum() == 1 and ok[EOS])
                y[r] = ref.masked(x[r], ok)
            L.ggml_hip_memcpy_h2d(lgA.ptr, x.ctypes.data, x.nbytes)
            L.ggml_hip_memcpy_h2d(lgB.ptr, y.ctypes.data, y.nbytes)
            L.ggml_hip_sampler_sample(A, lgA.ptr, V, tkA.ptr)
            L.ggml_hip_sampler_sample(B, lgB.ptr, V, tkB.ptr)
            a, b = tkA.to_host(np.int32, (R,)).tolist(), tkB.to_host(np.int32, (R,)).tolist()
            assert a == b, (config, draw, a, b)
            for r in range(4):
                assert allow(r, dfas[r], state[r])[a[r]], (config, draw, r)
                state[r] = ref.advance(dfas[r].trans, state[r], a[r], EOS, vocab)
            assert states_of(L, A) == state + [-1], (config, draw)
        if patterns is SPARSE:
            assert one_allowed >= 2 and only_eos >= 1          # row 3: \xff, then \0, then EOS for good
        muA, muB = np.zeros(R, np.float32), np.zeros(R, np.float32)
        assert L.ggml_hip_sampler_get_mu(A, muA.ctypes.data) == 0 and L.ggml_hip_sampler_get_mu(B, muB.ctypes.data) == 0
        assert muA.tobytes() == muB.tobytes()
        for r in range(R):
            assert rng_of(L, A, r) == rng_of(L, B, r), (config, r)
        # free while bound is refused and changes nothing; the binding travels with copy_row; unbound, the grammar goes
        assert L.ggml_hip_grammar_free(grammars[0].h) == 1 and states_of(L, A) == state + [-1]
        assert L.ggml_hip_sampler_copy_row(B, 2, A, 0) == 0 and states_of(L, B) == [-1, -1, state[0], -1, -1]
        assert L.ggml_hip_sampler_set_grammar(A, 0, None, 0) == 0 and L.ggml_hip_grammar_free(grammars[0].h) == 1       # (B's row 2 holds it)
        assert L.ggml_hip_sampler_copy_row(B, 2, B, 4) == 0 and states_of(L, B) == [-1] * R
        grammars[0].free()
    finally:
        L.ggml_hip_sampler_free(A)
        L.ggml_hip_sampler_free(B)
        for x in (lgA, lgB, tkA, tkB):
            x.free()
        for gr in grammars:
            gr.free()


def test_frozen_row_keeps_the_state_of_its_last_draw(L, vocab):
    """row 0 ends by a budget at its third draw: its state includes that draw and later launches leave it alone. ggml_hip_sampler_resume takes
    rows that ended at the end of their cache only, so it refuses this one (nothing moves); with its stops set again the row goes on as
    its unstopped twin (row 1) does"""
    d = g.regex_dfa(b"([abcd][abcd])*")
    gr = g.Grammar.make(vocab, d, EOS)
    rng = np.random.default_rng(3)
    s = L.ggml_hip_sampler_create(2, V, 32)
    lg, tk = g.DevBuf(2 * V * 4), g.DevBuf(2 * 4)
    try:
        p = g.sampling(temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_last_n=8, seed=5)
        for r in range(2):
            assert L.ggml_hip_sampler_set_row(s, r, C.byref(p), None, 0) == 0 and L.ggml_hip_sampler_set_grammar(s, r, gr.h, -1) == 0
        assert L.ggml_hip_sampler_set_stops(s, 0, C.byref(g.stops(max_tokens=3))) == 0
        rows = [sample_ref.tie_free_row(rng, V, 3.0) for _ in range(8)]

        def launch(x0, x1):
            x = np.stack([x0, x1])
            L.ggml_hip_memcpy_h2d(lg.ptr, x.ctypes.data, x.nbytes)
            L.ggml_hip_sampler_sample(s, lg.ptr, V, tk.ptr)
            return tk.to_host(np.int32, (2,)).tolist()

        state = d.start
        for k in range(3):
            a = launch(rows[k], rows[k])
            assert a[0] == a[1]
            state = ref.advance(d.trans, state, a[0], EOS, vocab)
        reason = np.zeros(2, np.int32)
        assert L.ggml_hip_sampler_get_stops(s, None, reason.ctypes.data) == 0 and reason[0] == g.STOP_BUDGET
        assert states_of(L, s, 2) == [state, state]
        keep0 = rng_of(L, s, 0)
        # frozen: row 1 is copied aside and put back, so the twin does not move while row 0 rides two launches
        twin = L.ggml_hip_sampler_create(1, V, 32)
        try:
            assert L.ggml_hip_sampler_copy_row(twin, 0, s, 1) == 0
            for k in (3, 4):
                assert launch(rows[k], rows[k])[0] == a[0]                  # (its token stays)
            assert states_of(L, s, 2)[0] == state and rng_of(L, s, 0) == keep0
            assert L.ggml_hip_sampler_resume(s, 0) == 1 and states_of(L, s, 2)[0] == state
            assert L.ggml_hip_sampler_copy_row(s, 1, twin, 0) == 0 and states_of(L, s, 2) == [state, state]
        finally:
            L.ggml_hip_sampler_free(twin)
        assert L.ggml_hip_sampler_set_stops(s, 0, None) == 0 and states_of(L, s, 2) == [state, state]
        for k in range(5, 8):
            a = launch(rows[k], rows[k])
            assert a[0] == a[1]
            state = ref.advance(d.trans, state, a[0], EOS, vocab)
            assert states_of(L, s, 2) == [state, state]
        assert rng_of(L, s, 0) == rng_of(L, s, 1)
    finally:
        L.ggml_hip_sampler_free(s)
        lg.free()
        tk.free()
        gr.free()


def test_operator_refusals_change_nothing(L, vocab):
    d = g.regex_dfa(b"(ab|cd)+")
    with pytest.raises(g.GrammarError) as e:                 # no token holds a z: the state after a allows nothing
        g.Grammar.make(vocab, g.regex_dfa(b"az"), EOS)
    assert (e.value.code, e.value.state) == (g.GRAMMAR_DEAD_END, g.regex_dfa(b"az").walk(1, b"a"))
    with pytest.raises(g.GrammarError) as e:                 # an accepting state without transitions and no EOS token
        g.Grammar.make(vocab, g.regex_dfa(b"ab"), None)
    assert (e.value.code, e.value.state) == (g.GRAMMAR_DEAD_END, 3)
    bad = g.Dfa(d.trans.copy(), d.accept, d.start)
    bad.trans[2, 9] = d.n_states
    with pytest.raises(g.GrammarError) as e:
        g.Grammar.make(vocab, bad, EOS)
    assert (e.value.code, e.value.state) == (g.GRAMMAR_BAD_TRANS, 2)
    with pytest.raises(g.GrammarError) as e:
        g.Grammar.make(vocab, g.Dfa(d.trans, d.accept, d.n_states), EOS)
    assert e.value.code == g.GRAMMAR_BAD_ARGS
    gr = g.Grammar.make(vocab, d, EOS)
    s, other = L.ggml_hip_sampler_create(2, V, 32), L.ggml_hip_sampler_create(1, V + 1, 32)
    try:
        assert L.ggml_hip_sampler_set_grammar(s, 0, gr.h, 2) == 0 and states_of(L, s, 2) == [2, -1]
        for row, state in ((0, d.n_states), (0, -2), (2, 1), (-1, 1)):
            assert L.ggml_hip_sampler_set_grammar(s, row, gr.h, state) == 1
        assert L.ggml_hip_sampler_set_grammar(other, 0, gr.h, -1) == 1          # another n_vocab
        assert states_of(L, s, 2) == [2, -1]
        assert L.ggml_hip_grammar_free(gr.h) == 1 and states_of(L, s, 2) == [2, -1]
        lg, out = g.DevBuf(2 * V * 4), g.DevBuf(64)
        try:
            assert L.ggml_hip_memset(lg.ptr, 0, 2 * V * 4) is None
            assert L.ggml_hip_sampler_verify_rows(s, lg.ptr, V, 1, None, out.ptr, out.ptr + 32) == 1         # row 0 holds a grammar
            assert states_of(L, s, 2) == [2, -1]
        finally:
            lg.free()
            out.free()
    finally:
        L.ggml_hip_sampler_free(s)                           # (frees the binding)
        L.ggml_hip_sampler_free(other)
    gr.free()


# ---------------------------------------------------------------------------------------------- 3. the model loops
HP = synth.HP_TINY_MQA
N_CTX, STEPS, FIRST = 64, 24, 5
BYTE_VOCAB = [bytes([t]) for t in range(256)] + [bytes([97 + k // 16, 97 + k % 16]) for k in range(256)]      # every byte, then the pairs over a..p
PATTERN = b"(ab|cd)+x"
P_MODES = {"greedy": dict(temp=0.0, repeat_penalty=1.1, repeat_last_n=64), "sampled": dict(temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64)}


@pytest.fixture(scope="module")
def model(L, tmp_path_factory):
    """the tiny model with a byte vocabulary and the grammar of PATTERN with EOS (token 0) allowed at the end; first the refusal without one"""
    path = str(tmp_path_factory.mktemp("grammar_vocab") / "bytes.ggcc")
    stop_text_ref.write_vocab_ggcc(path, BYTE_VOCAB)
    v = g.Vocab(path)
    assert [v.token_bytes(t) for t in range(HP["n_vocab"])] == BYTE_VOCAB
    m = g.FalconModel(synth.make_model(ob.Oracle(), HP, ob.Q4_0, seed=77), n_ctx=N_CTX, n_batch=8)
    d = g.regex_dfa(PATTERN)
    with pytest.raises(g.GrammarError):                      # no vocabulary on the model
        m.grammar(d, eos_id=EOS)
    assert m.grammar_state == -1
    m.set_vocab(v)
    gr = m.grammar(d, eos_id=EOS)
    assert np.array_equal(gr.index(), ref.index(d.trans, d.accept, EOS, BYTE_VOCAB))
    yield m, d, gr
    m.set_grammar(None)
    gr.free()
    m.free()
    v.free()


@pytest.fixture(scope="module")
def host_loops(L, model):
    """per mode: the tokens and the final state of a host loop -- falcon_hip_eval of one token, the row masked on the host, the plain
    operator sampler -- computed once"""
    m, d, gr = model
    nv = HP["n_vocab"]
    out = {}
    allow = Allow(BYTE_VOCAB)
    lg, tk = g.DevBuf(nv * 4), g.DevBuf(4)
    try:
        for mode, kw in P_MODES.items():
            p = g.sampling(seed=4321, **kw)
            plain = L.ggml_hip_sampler_create(1, nv, N_CTX)
            h = np.array([FIRST], np.int32)
            assert L.ggml_hip_sampler_set_row(plain, 0, C.byref(p), h.ctypes.data, 1) == 0
            tok, state, toks = FIRST, d.start, []
            for step in range(STEPS):
                m.eval_token(tok, step)
                x = ref.masked(np.array(m.logits(), np.float32).reshape(-1)[:nv], allow(0, d, state))
                L.ggml_hip_memcpy_h2d(lg.ptr, x.ctypes.data, x.nbytes)
                L.ggml_hip_sampler_sample(plain, lg.ptr, nv, tk.ptr)
                tok = int(tk.to_host(np.int32, (1,))[0])
                toks.append(tok)
                state = ref.advance(d.trans, state, tok, EOS, BYTE_VOCAB)
            L.ggml_hip_sampler_free(plain)
            out[mode] = (p, toks, state)
    finally:
        lg.free()
        tk.free()
    return out


def check_text(toks):
    text = b"".join(BYTE_VOCAB[t] for t in toks if t != EOS)
    if EOS in toks:
        assert re.fullmatch(PATTERN, text) and all(t == EOS for t in toks[toks.index(EOS):])      # EOS only where the match is complete, and only EOS behind it
    else:
        assert re.fullmatch(b"(ab|cd)*(a|c|(ab|cd)x)?", text)                                      # a live prefix


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("mode", list(P_MODES))
def test_decode_sample_equals_host_masked_loop(model, host_loops, mode, use_graph):
    m, d, gr = model
    p, want, want_state = host_loops[mode]
    m.set_sampling(p, [FIRST])
    m.set_grammar(gr)
    assert m.grammar_state == d.start
    got = m.decode_sample(FIRST, 0, STEPS, use_graph=use_graph).tolist()
    assert got == want and m.grammar_state == want_state
    check_text(got)
    # in two calls the state is carried; setting the state a row has, or another grammar and back, does not capture the step again
    m.set_sampling(p, [FIRST])
    m.set_grammar(gr)
    c0 = g.graph_captures(m)
    a = m.decode_sample(FIRST, 0, 10, use_graph=use_graph).tolist()
    c1 = g.graph_captures(m)
    m.set_grammar(gr, state=m.grammar_state)
    b = m.decode_sample(a[-1], 10, STEPS - 10, use_graph=use_graph).tolist()
    assert a + b == want and m.grammar_state == want_state
    assert g.graph_captures(m) == c1 and c1 <= c0 + 1
    if use_graph:
        m.set_grammar(None)                                  # the last grammar off: another instantiation, one capture
        m.set_sampling(p, [FIRST])
        m.decode_sample(FIRST, 0, 4, use_graph=True)
        assert g.graph_captures(m) == c1 + 1 and m.grammar_state == -1
        m.set_grammar(gr)                                    # ... and on again
        m.decode_sample(FIRST, 0, 4, use_graph=True)
        assert g.graph_captures(m) == c1 + 2
    m.set_grammar(None)


def test_lockstep_slots_equal_their_single_runs(model):
    """three slots -- two grammars and none -- each against its single-context run; copy_sampling carries binding and state"""
    m, d, gr = model
    d2 = g.choice_dfa([b"yes", b"no", b"maybe"])
    gr2 = m.grammar(d2, eos_id=EOS)
    firsts, n = [5, 77, 300], 12
    ps = [g.sampling(seed=90 + s, **P_MODES["sampled"]) for s in range(3)]
    grs = [gr, gr2, None]
    sc = g.SeqContext(m, N_CTX, 3)
    try:
        want, states = [], []
        for s in range(3):
            m.set_sampling(ps[s], [firsts[s]])
            m.set_grammar(grs[s])
            want.append(m.decode_sample(firsts[s], 0, n, use_graph=False).tolist())
            states.append(m.grammar_state)
        assert states[2] == -1 and states[0] > 0 and states[1] > 0
        text = b"".join(BYTE_VOCAB[t] for t in want[1] if t != EOS)
        assert text in (b"yes", b"no", b"maybe") if EOS in want[1] else any(w.startswith(text) for w in (b"yes", b"no", b"maybe"))
        for s in range(3):
            sc.set_sampling(s, ps[s], [firsts[s]])
            sc.set_grammar(s, grs[s])
        assert sc.grammar_state.tolist() == [d.start, d2.start, -1]
        got = sc.decode_sample(firsts, [0, 0, 0], n, use_graph=True)
        for s in range(3):
            assert got[:, s].tolist() == want[s], s
        assert sc.grammar_state.tolist() == states
        # m still holds slot 2's row (no grammar); give it gr at a state of its own and copy that into slot 2
        m.set_grammar(gr, state=2)
        assert g.copy_sampling(sc, 2, m, 0) == 0 and sc.grammar_state.tolist() == [states[0], states[1], 2]
        assert g.copy_sampling(sc, 1, sc, 2) == 0 and sc.grammar_state.tolist() == [states[0], 2, 2]
        with pytest.raises(ValueError):
            gr.free()                                        # bound by m and the slots
    finally:
        sc.free()
        m.set_grammar(None)
    gr2.free()


def test_model_refusals_change_nothing(model):
    m, d, gr = model
    m.set_sampling(g.sampling(seed=1, **P_MODES["greedy"]), [FIRST])
    m.set_grammar(gr, state=3)
    with pytest.raises(ValueError):
        m.set_grammar(gr, state=d.n_states)                  # a state out of range
    assert m.grammar_state == 3
    with pytest.raises(ValueError):
        gr.free()                                            # free while bound
    assert m.grammar_state == 3
    with pytest.raises(ValueError):
        m.set_spec(4, history=[1, 2, 3, FIRST])              # draft-and-verify on a context with a grammar
    assert m.grammar_state == 3
    m.set_grammar(None)
    m.set_spec(4, history=[1, 2, 3, FIRST])
    try:
        with pytest.raises(ValueError):
            m.set_grammar(gr)                                # a grammar while draft-and-verify is on
        assert m.grammar_state == -1
    finally:
        m.set_spec(0)


# ---------------------------------------------------------------------------------------------- 4. the examples, end to end
@pytest.fixture(scope="module")
def bpe_model(tmp_path_factory):
    """the tiny model with a real BPE vocabulary that tests/test_gpu_sample.py's example tests build"""
    import bpe_fixture
    import ggcc_writer
    vocab, merges = bpe_fixture.build(n_merges=308)
    hp = dict(synth.HP_TINY_MQA)
    hp["n_vocab"] = len(vocab)
    path = str(tmp_path_factory.mktemp("bpe") / "tiny_bpe.ggcc")
    ggcc_writer.write_ggcc(path, synth.make_model(ob.Oracle(), hp, ob.Q4_0, seed=321), vocab, merges)
    return path


def _example(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_examples_generate_what_the_grammar_allows(L, bpe_model):
    """--choice and --regex with the real tokenizer: whatever the tiny model prefers, the printed continuation is one of the choices, or
    matches the pattern, and ends there (end-of-text is the only token allowed behind a complete match, and it is a stop)"""
    gen, bat = _example("falcon_generate"), _example("falcon_batch_generate")
    prompt, choices = "Is the sky blue? Answer: ", [b"yes", b"no", b"maybe so"]
    for seed in (1, 2):
        res = gen.generate(bpe_model, prompt, 12, n_ctx=64, sampling=g.sampling(seed=seed), grammar=g.choice_dfa(choices))
        assert res[2] in choices, res[2]
    res = gen.generate(bpe_model, prompt, 12, n_ctx=64, grammar=g.regex_dfa("-?[0-9]{2,3}(\\.[0-9])?"))       # greedy
    assert re.fullmatch(b"-?[0-9]{2,3}(\\.[0-9])?", res[2]), res[2]
    got = bat.generate_batch(bpe_model, [prompt, "A", "B c"], 12, n_seq=2, n_ctx=64, sampling=g.sampling(seed=0), seeds=[3, 4, 5], grammar=g.choice_dfa(choices))
    assert all(r[2] in choices for r in got), [r[2] for r in got]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "falcon_generate.py"), "--model", bpe_model, "--prompt", prompt, "-n", "12",
                        "--n-ctx", "64", "--seed", "1", "--choice", "yes", "--choice", "no"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout in (prompt + "yes\n", prompt + "no\n")
    with pytest.raises(ValueError):
        gen.generate(bpe_model, prompt, 12, n_ctx=64, grammar=g.choice_dfa(choices), draft=4)

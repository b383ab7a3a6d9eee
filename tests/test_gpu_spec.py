"""GPU: draft-and-verify decode at the model level (falcon_hip_context_set_spec / falcon_hip_decode_spec, csrc/fq_spec.h) against the
plain sampled loop on the same model: the SAME tokens, the same state behind them, and the passes tests/spec_ref.py predicts from the
token ids alone.

Which rows of a verify pass are promised the bits of the single-token step -- checked with the CPU oracle before this file was written
(batches of 2, 4, 8 and 16 rows at positions 4.. against 16 single-token evals, Q4_0 / Q5_1 / Q8_0 / Q4_K at the sizes used here):
  oracle sum order 0 (the device's ggml_hip_reference_order 1 and 2): every row of every batch == the single-token row, all formats;
  oracle sum order 2 (the device's default order): rows of batches of 2 and 4 == the single-token rows, batches of 8 and 16 differ.
So equality with falcon_hip_decode_sample IS asserted for: the default order at K = 1 and 3, all five legacy formats; order 2 at K = 1, 3, 7
and 15 for Q4_0 and Q4_K; order 1 at K = 3; every LOOKUP, end-of-cache, budget, stale-row and graph case below (K <= 3 in the default
order, or order 2). It is NOT asserted for the default order at K = 7: there the draws must equal a host replay of the reference's sampling
functions over the logits falcon_hip_eval(..., logits_all) gives for the same rows (test_default_order_wide_pass_equals_host_replay)."""
import ctypes as C
import os

import numpy as np
import pytest

import ggllm_cpp_amd as g
import sample_ref
import spec_ref as sr
import synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

HP = dict(n_vocab=512, n_embd=256, n_head=4, n_head_kv=1, n_layer=2, n_ff=1024, two_norms=False)      # tests/test_gpu_sample.py's
P_LOOP = dict(temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64)
PROMPT = [11, 200, 37, 4, 99]
N, TAIL = 24, 8
CONTEXT = g.STOP_CONTEXT


@pytest.fixture(scope="module")
def L():
    L = g.load()
    L.ggml_hip_init(0)
    return L


_weights = {}


def weights(t):
    if t not in _weights:
        _weights[t] = synth.make_model(ob.Oracle(), HP, t, seed=77)
    return _weights[t]


class order:
    def __init__(self, L, mode):
        self.L, self.mode = L, mode

    def __enter__(self):
        self.L.ggml_hip_reference_order(self.mode)

    def __exit__(self, *a):
        self.L.ggml_hip_reference_order(0)


def start(m, p, prompt=PROMPT):
    """the prompt evaluated, the sampler set, the first token drawn: where both loops begin"""
    m.eval(prompt, 0, logits_all=False)
    m.set_sampling(p, prompt)
    return m.sample()


_plain = {}


def plain_run(L, t, mode, p, key, n_ctx=64, prompt=PROMPT, n=N + TAIL, context_stop=False):
    """falcon_hip_decode_sample's n tokens from the prompt (computed once per case and shared), with the session blob behind them"""
    k = (t, mode, key, n_ctx, tuple(prompt), n, context_stop)
    if k not in _plain:
        with order(L, mode):
            m = g.FalconModel(weights(t), n_ctx=n_ctx, n_batch=max(16, len(prompt)))
            try:
                first = start(m, p, prompt)
                if context_stop:
                    m.set_context_stop(True)
                s = m.decode_sample(first, len(prompt), n).tolist()
                n_rows = min(len(prompt) + len([x for x in s if x >= 0]), n_ctx)
                _plain[k] = (first, s, m.copy_state(n_rows).tobytes(), m.stop_state() if context_stop else None)
            finally:
                m.free()
    return _plain[k]


def corrupt(s, at):
    q = list(s)
    for i in at:
        q[i] = (q[i] + 1) % HP["n_vocab"]
    return q


def hist16(h, K):
    return h + [0] * (16 - len(h)) if len(h) == K + 1 else None


def given_cases(L, t, mode, K, use_graph=False):
    """guess == the plain continuation, the same with draws 5 and 6 corrupted, and a guess that is wrong everywhere: each yields the plain
    tokens, the predicted passes, and the plain run's next TAIL tokens when the plain loop goes on from there (generator, window, cache --
    the stale rows of the rejected drafts included); in reference order also the plain run's session blob, byte for byte"""
    p = g.sampling(seed=1234, **P_LOOP)
    first, s, _, _ = plain_run(L, t, mode, p, "given")
    _, _, blob24, _ = plain_run(L, t, mode, p, "given", n=N)
    assert min(s) >= 0
    with order(L, mode):
        m = g.FalconModel(weights(t), n_ctx=64, n_batch=16)
        try:
            for name, guess in (("all", s[:N]), ("some", corrupt(s[:N], (5, 6))), ("none", corrupt(s[:N], range(N)))):
                assert start(m, p) == first
                m.set_spec(K, g.SPEC_GIVEN)
                m.set_spec_guess(guess)
                out = m.decode_spec(first, len(PROMPT), N, use_graph=use_graph).tolist()
                assert out == s[:N], (name, K)
                per, hist = sr.simulate(s[:N], K, sr.GIVEN, guess=guess)
                passes, draws, h = m.spec_stats()
                assert (passes, draws, h.tolist()) == (len(per), N, hist16(hist, K)), (name, K)
                if name == "all":
                    assert passes == -(-N // (K + 1))
                if name == "none":
                    assert passes == N
                if mode:
                    assert m.copy_state(len(PROMPT) + N).tobytes() == blob24, (name, K)
                assert m.decode_sample(out[-1], len(PROMPT) + N, TAIL).tolist() == s[N:], (name, K)
        finally:
            m.free()


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("t", ob.LEGACY, ids=[g.TYPE_NAME[t] for t in ob.LEGACY])
def test_given_default_order(L, t, K):
    given_cases(L, t, 0, K)


@pytest.mark.parametrize("K", [1, 3, 7, 15])
@pytest.mark.parametrize("t", [ob.Q4_0, ob.Q4_K], ids=["q4_0", "q4_K"])
def test_given_reference_order_2(L, t, K):
    given_cases(L, t, 2, K)


def test_given_reference_order_1(L):
    given_cases(L, ob.Q4_0, 1, 3)


@pytest.mark.parametrize("temp", [0.0, 0.8], ids=["greedy", "sampled"])
def test_lookup(L, temp):
    """prompt lookup, 40 tokens, K = 3, from a prompt that repeats itself: the plain loop's tokens, and the passes and the histogram of the
    reference simulation run on those tokens"""
    prompt = [11, 200, 37, 4, 99, 11, 200, 37, 4, 99, 11, 200]
    p = g.sampling(seed=77, **dict(P_LOOP, temp=temp))
    first, s, _, _ = plain_run(L, ob.Q4_0, 0, p, ("lookup", temp), prompt=prompt, n=40 + TAIL)
    m = g.FalconModel(weights(ob.Q4_0), n_ctx=64, n_batch=16)
    try:
        assert start(m, p, prompt) == first
        m.set_spec(3, g.SPEC_LOOKUP, ngram=(1, 3), history=prompt + [first])
        out = m.decode_spec(first, len(prompt), 40).tolist()
        assert out == s[:40]
        per, hist = sr.simulate(s[:40], 3, sr.LOOKUP, history=prompt + [first], ngram=(1, 3))
        passes, draws, h = m.spec_stats()
        assert (passes, draws, h.tolist()) == (len(per), 40, hist16(hist, 3))
        assert m.decode_sample(out[-1], len(prompt) + 40, TAIL).tolist() == s[40:]
    finally:
        m.free()


def test_end_of_the_cache(L):
    """n_ctx 32, a prompt of 20, K = 7, the context stop on, every draft right (in reference order 2): the row ends with STOP_CONTEXT at
    the plain loop's draw, the pass that reaches the end evaluates and writes no position >= n_ctx -- a second context made right behind
    this one keeps its cache --, and the session saved afterwards is the plain run's, byte for byte"""
    prompt = [int(x) for x in synth.tokens(20, HP["n_vocab"], seed=5)]
    p = g.sampling(seed=4321, **P_LOOP)
    first, s, blob, st = plain_run(L, ob.Q4_0, 2, p, "end", n_ctx=32, prompt=prompt, n=32, context_stop=True)
    n = 32 - len(prompt)
    assert min(s[:n]) >= 0 and s[n:] == [-1] * (32 - n) and st == (n, CONTEXT)
    with order(L, 2):
        m = g.FalconModel(weights(ob.Q4_0), n_ctx=32, n_batch=20)
        canary = g.FalconModel(weights(ob.Q4_0), n_ctx=32, n_batch=16)
        try:
            canary.eval(prompt[:16], 0, logits_all=False)
            canary.eval(prompt[4:20], 16, logits_all=False)
            before = canary.copy_state(32).tobytes()
            assert start(m, p, prompt) == first
            m.set_context_stop(True)
            m.set_spec(7, g.SPEC_GIVEN)
            m.set_spec_guess(s[:n] + [5, 6, 7, 8])              # (guesses for draws that are never made)
            out = m.decode_spec(first, len(prompt), 32).tolist()
            assert out == s[:n]
            assert m.stop_state() == st
            per, hist = sr.simulate(s[:n], 7, sr.GIVEN, guess=s[:n] + [5, 6, 7, 8], pos=len(prompt), n_ctx=32)
            assert per == [8, 4]
            passes, draws, h = m.spec_stats()
            assert (passes, draws, h.tolist()) == (2, n, hist16(hist, 7))
            assert m.copy_state(32).tobytes() == blob
            assert canary.copy_state(32).tobytes() == before
            # the row has ended: called again where it stands (the token at position 31 is the draw before the last), nothing is drawn, nothing moves
            assert m.decode_spec(s[n - 2], 31, 4).size == 0
            assert m.copy_state(32).tobytes() == blob and m.stop_state() == st
            assert canary.copy_state(32).tobytes() == before
        finally:
            canary.free()
            m.free()


def test_budget(L):
    """n_tokens 10 at K = 3 with every draft right: exactly 10 draws in passes of 4, 4 and 2 -- the third pass stops at the budget although
    its next draft is right --, and the state is the plain loop's after 10: it goes on with the plain run's next tokens"""
    p = g.sampling(seed=1234, **P_LOOP)
    first, s, _, _ = plain_run(L, ob.Q4_0, 0, p, "given")
    m = g.FalconModel(weights(ob.Q4_0), n_ctx=64, n_batch=16)
    try:
        assert start(m, p) == first
        m.set_spec(3, g.SPEC_GIVEN)
        m.set_spec_guess(s[:N])
        out = np.full(12, -1, np.int32)
        n = C.c_int(0)
        assert L.falcon_hip_decode_spec(m.ctx, first, len(PROMPT), 10, out.ctypes.data, C.addressof(n)) == 0
        assert n.value == 10 and out.tolist() == s[:10] + [-1, -1]
        passes, draws, h = m.spec_stats()
        assert (passes, draws, h[:4].tolist()) == (3, 10, [0, 1, 0, 2])
        # the guess stays aligned with the draw's number: the next call picks up at draw 10
        assert m.decode_spec(s[9], len(PROMPT) + 10, 6).tolist() == s[10:16]
        assert m.spec_stats()[:2] == (5, 16)
        assert m.decode_sample(s[15], len(PROMPT) + 16, TAIL).tolist() == s[16:16 + TAIL]
    finally:
        m.free()


def test_stops_end_a_pass(L):
    """a stop sequence the 6th draw completes, every draft right at K = 3: 6 draws (4 + 2), reason 0, as the plain loop"""
    p = g.sampling(seed=1234, **P_LOOP)
    first, s, _, _ = plain_run(L, ob.Q4_0, 0, p, "given")
    m = g.FalconModel(weights(ob.Q4_0), n_ctx=64, n_batch=16)
    try:
        assert start(m, p) == first
        m.set_stops(g.stops([[s[4], s[5]]]))
        m.set_spec(3, g.SPEC_GIVEN)
        m.set_spec_guess(s[:N])
        m.set_stop_poll(2)
        assert m.decode_spec(first, len(PROMPT), N).tolist() == s[:6]
        assert m.stop_state() == (6, 0)
        assert m.spec_stats()[:2] == (2, 6)
        assert m.loop_steps() <= 2 + 2 * 2                      # at most two poll intervals of passes past the end
    finally:
        m.free()


def test_graph(L):
    """the pass is captured once over all passes of a call and over later calls; turning spec off and on re-captures; same tokens"""
    p = g.sampling(seed=1234, **P_LOOP)
    first, s, _, _ = plain_run(L, ob.Q4_0, 0, p, "given")
    m = g.FalconModel(weights(ob.Q4_0), n_ctx=64, n_batch=16)
    try:
        assert start(m, p) == first
        m.set_spec(3, g.SPEC_GIVEN)
        m.set_spec_guess(corrupt(s[:N], (5, 6)))
        c0 = g.graph_captures(m)
        assert m.decode_spec(first, len(PROMPT), 12, use_graph=True).tolist() == s[:12]
        assert g.graph_captures(m) == c0 + 1
        assert m.decode_spec(s[11], len(PROMPT) + 12, 12, use_graph=True).tolist() == s[12:N]
        assert g.graph_captures(m) == c0 + 1
        m.set_spec(0)
        assert m.decode_sample(s[N - 1], len(PROMPT) + N, 2, use_graph=True).tolist() == s[N:N + 2]
        c1 = g.graph_captures(m)
        m.set_spec(3, g.SPEC_GIVEN)
        assert m.decode_spec(s[N + 1], len(PROMPT) + N + 2, 3, use_graph=True).tolist() == s[N + 2:N + 5]
        assert g.graph_captures(m) == c1 + 1
    finally:
        m.free()
    given_cases(L, ob.Q5_0, 0, 3, use_graph=True)


def test_default_order_wide_pass_equals_host_replay(L, tmp_path):
    """the default order at K = 7 (a pass of 8 rows: the small-batch mat-mul, whose rows are not promised the single-token bits): every draw
    is the reference's own sampling functions' draw from the logits falcon_hip_eval(..., logits_all) gives for the rows of the pass"""
    if not os.path.exists(sample_ref.REF_SO):
        pytest.skip("oracle/_ref/libfalcon_ref.so is not built (make -C oracle ref_falcon)")
    ref = sample_ref.RefSampler(sample_ref.tiny_ggcc(str(tmp_path / "tiny.ggcc")))
    K, n = 7, 20
    p = g.sampling(seed=99, **P_LOOP)
    _, s, _, _ = plain_run(L, ob.Q4_0, 0, p, "replay")
    guess = corrupt(s[:n], (9,))                                 # (a guess: the plain loop's tokens with one wrong; nothing depends on its being right)
    m, e = g.FalconModel(weights(ob.Q4_0), n_ctx=64, n_batch=16), g.FalconModel(weights(ob.Q4_0), n_ctx=64, n_batch=16)
    try:
        first = start(m, p)
        m.set_spec(K, g.SPEC_GIVEN)
        m.set_spec_guess(guess)
        got = m.decode_spec(first, len(PROMPT), n).tolist()
        _, _, hist = m.spec_stats()
        # the host replay: the same passes on a second context through falcon_hip_eval, the reference's sampler with falcon_main's window
        lg = e.eval(PROMPT, 0, logits_all=False)[-1]
        ref.seed(p.seed)
        h = list(PROMPT)
        t0 = ref.draw(lg, p, g.sampling_window(h, 64, p.repeat_last_n))
        assert t0 == first
        h.append(t0)
        want, per, pos = [], [], len(PROMPT)
        while len(want) < n:
            d = sr.given(guess, len(want), K)
            rows = e.eval([h[-1]] + [x if x >= 0 else 0 for x in d], pos, logits_all=True)
            j = 0
            while True:
                t = ref.draw(rows[j], p, g.sampling_window(h, 64, p.repeat_last_n))
                want.append(t)
                h.append(t)
                if not (j < K and len(want) < n and d[j] == t):
                    break
                j += 1
            per.append(j + 1)
            pos += j + 1
        assert got == want
        assert hist.tolist() == [per.count(d) for d in range(1, 17)]
    finally:
        ref.free()
        m.free()
        e.free()


def test_example_draft_flag_generates_the_same_bytes(L, tmp_path):
    """examples/falcon_generate.py with draft=3 on a model with a real BPE vocabulary: ids and bytes of the run without it, sampled and greedy"""
    import importlib.util
    import bpe_fixture
    import ggcc_writer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("falcon_generate", os.path.join(root, "examples", "falcon_generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    vocab, merges = bpe_fixture.build(n_merges=308)
    hp = dict(synth.HP_TINY_MQA)
    hp["n_vocab"] = len(vocab)
    path = str(tmp_path / "tiny_bpe.ggcc")
    ggcc_writer.write_ggcc(path, synth.make_model(ob.Oracle(), hp, ob.Q4_0, seed=321), vocab, merges)
    prompt = "the fox and the dog and the fox and the dog and the"
    for p in (g.sampling(seed=7), None):
        a = gen.generate(path, prompt, 24, n_ctx=64, sampling=p)
        b = gen.generate(path, prompt, 24, n_ctx=64, sampling=p, draft=3)
        assert np.array_equal(a[0], b[0]) and a[1].tolist() == b[1].tolist() and a[2] == b[2]


def test_refusals(L):
    """every documented refusal returns non-zero, and the context goes on working"""
    p = g.sampling(seed=1234, **P_LOOP)
    first, s, _, _ = plain_run(L, ob.Q4_0, 0, p, "given")
    w = weights(ob.Q4_0)
    m = g.FalconModel(w, n_ctx=64, n_batch=8)
    try:
        assert start(m, p) == first
        out, n = np.zeros(8, np.int32), C.c_int(0)
        assert L.falcon_hip_decode_spec(m.ctx, first, len(PROMPT), 4, out.ctypes.data, C.addressof(n)) == 1       # spec is off
        for bad in (dict(n_draft=16), dict(n_draft=-1), dict(n_draft=8), dict(n_draft=3, source=3), dict(n_draft=3, ngram=(0, 3)), dict(n_draft=3, ngram=(3, 2)),
                    dict(n_draft=3, ngram=(1, 33)), dict(n_draft=3, history=[0] * 65), dict(n_draft=3, history=[1, 512])):
            with pytest.raises(ValueError):
                m.set_spec(**bad)
        with pytest.raises(ValueError):
            m.set_spec_guess([1, 2, 3])                           # spec is off
        m.set_logprobs(0)
        with pytest.raises(ValueError):
            m.set_spec(3, g.SPEC_GIVEN)                           # records are on
        m.set_logprobs(-1)
        m.set_spec(3, g.SPEC_LOOKUP, history=PROMPT + [first])
        with pytest.raises(ValueError):
            m.set_logprobs(0)                                     # ... and the reverse
        with pytest.raises(ValueError):
            m.set_spec_guess([1, 2, 3])                           # the source is the lookup
        for tok, n_past, n_tok in ((first, 64, 1), (first, -1, 1), (512, 5, 1), (first, 5, 0), (first, 60, 5)):
            assert L.falcon_hip_decode_spec(m.ctx, tok, n_past, n_tok, out.ctypes.data, C.addressof(n)) == 1
        assert m.decode_spec(first, len(PROMPT), 8).tolist() == s[:8]
        assert m.decode_sample(s[7], len(PROMPT) + 8, 4).tolist() == s[8:12]       # spec on: the plain loop stays the plain loop
        sc = g.SeqContext(m, 32, 2)
        try:
            assert L.falcon_hip_context_set_spec(sc.ctx, 3, g.SPEC_GIVEN, 1, 3, None, 0) == 1                   # a lock-step context
        finally:
            sc.free()
    finally:
        m.free()
    st = g.FalconModel(w, n_ctx=32, n_batch=8, layer_begin=0, layer_end=1)
    try:
        assert L.falcon_hip_context_set_spec(st.ctx, 3, g.SPEC_GIVEN, 1, 3, None, 0) == 1                       # a pipeline stage
    finally:
        st.free()

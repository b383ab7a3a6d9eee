"""GPU: the captured steps of the Falcon driver (csrc/falcon_ctx.h: one step_slot per entry point and per batch shape, keyed by the mode
signature, the config epoch and the named parts the step bakes in). Every case runs the same calls on two contexts of one model -- one replaying graphs,
one with plain launches -- and asks for the same bits, and reads falcon_hip_context_graph_captures to pin WHEN a step is captured:
once in steady state, again after a mode change, a global switch or a moved buffer, and never otherwise. Host logic: the tiny
model of tests/test_gpu_sample.py is as good as any."""
import numpy as np
import pytest

import ggllm_cpp_amd as g
import synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

HP = dict(n_vocab=512, n_embd=256, n_head=4, n_head_kv=1, n_layer=2, n_ff=1024, two_norms=False)
N_CTX = 64
PROMPT = synth.tokens(16, HP["n_vocab"], seed=5)           # fills KV rows [0, 16) of every context: the loops below start inside them
P_LOOP = dict(temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64)
FIRST = 7
FIRSTS, POS = [7, 300, 42], [0, 5, 11]


@pytest.fixture(scope="module")
def L():
    L = g.load()
    L.ggml_hip_init(0)
    return L


@pytest.fixture(scope="module")
def weights():
    return synth.make_model(ob.Oracle(), HP, ob.Q4_0, seed=77)


@pytest.fixture(scope="module")
def weights_q4k():
    return synth.make_model(ob.Oracle(), HP, ob.Q4_K, seed=77)


class Pair:
    """two contexts of one model with the same KV rows: .graph replays captured steps, .plain launches"""

    def __init__(self, weights, n_seq=0):
        self.models = [g.FalconModel(weights, n_ctx=N_CTX, n_batch=16) for _ in range(2)]
        for m in self.models:
            m.eval(PROMPT, 0, logits_all=False)
        self.seqs = []
        if n_seq:
            for m in self.models:
                sc = g.SeqContext(m, N_CTX, n_seq)
                for t in range(n_seq):
                    assert g.copy_seq(sc, t, m, 0, len(PROMPT)) == 0
                self.seqs.append(sc)
        self.graph, self.plain = self.seqs if n_seq else self.models

    def captures(self):
        return g.graph_captures(self.graph)

    def both(self, call):
        """call(context, use_graph) on both contexts; asserts the same bits, returns (result, captures the call added)"""
        before = self.captures()
        got, want = call(self.graph, True), call(self.plain, False)
        assert g.graph_captures(self.plain) == 0
        for a, b in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        return got, self.captures() - before

    def free(self):
        for sc in self.seqs:
            sc.free()
        for m in self.models:
            m.free()


# ---- the calls: (context, use_graph) -> array(s). The sampled ones re-seed first, so a repeated call repeats its tokens
def greedy(n_past, steps=4):
    return lambda m, ug: m.decode_greedy(FIRST, n_past, steps, use_graph=ug)


def sample(n_past, steps=4, records=False):
    def call(m, ug):
        m.set_sampling(g.sampling(seed=1234, **P_LOOP), [FIRST])
        out = m.decode_sample(FIRST, n_past, steps, use_graph=ug)
        return (out,) + tuple(m.logprobs()) if records else out
    return call


def seqs_greedy(pos, steps=4, firsts=FIRSTS):
    return lambda sc, ug: sc.decode_greedy(firsts, pos, steps, use_graph=ug)


def seqs_sample(pos, steps=4, records=False, firsts=FIRSTS):
    def call(sc, ug):
        for t in range(sc.n_seq):
            sc.set_sampling(t, g.sampling(seed=50 + t, **P_LOOP), [firsts[t]])
        out = sc.decode_sample(firsts, pos, steps, use_graph=ug)
        return (out,) + tuple(sc.logprobs()) if records else out
    return call


def token(n_past):
    """falcon_hip_eval_token has no switch: it replays wherever it may. Its plain form is falcon_hip_eval of the one token"""
    def call(m, ug):
        if not ug:
            return m.eval([FIRST], n_past, logits_all=False)[-1]
        m.eval_token(FIRST, n_past)
        return m.logits()
    return call


# ---------------------------------------------------------------------------------------------- 1. steady state
@pytest.mark.parametrize("name", ["decode_greedy", "decode_sample", "seqs_greedy", "seqs_sample", "eval_token"])
def test_steady_state_captures_once(L, weights, name):
    """first call: one capture; the same call again: none; from other positions: none -- but falcon_hip_decode_greedy, whose base
    position is an argument of its last launch: one capture per change of base (one slot: coming back captures again)"""
    seqs = name.startswith("seqs")
    make = dict(decode_greedy=greedy, decode_sample=sample, seqs_greedy=seqs_greedy, seqs_sample=seqs_sample, eval_token=token)[name]
    here, there = (POS, [3, 9, 2]) if seqs else (5, 9)
    p = Pair(weights, 3 if seqs else 0)
    try:
        assert p.both(make(here))[1] == 1
        assert p.both(make(here))[1] == 0
        moved = 1 if name == "decode_greedy" else 0
        assert p.both(make(there))[1] == moved
        assert p.both(make(here))[1] == moved
        assert p.both(make(here))[1] == 0
    finally:
        p.free()


# ---------------------------------------------------------------------------------------------- 2. moved buffers
def test_grown_output_buffer_recaptures(L, weights):
    """the lock-step loops' [step][seq] output grows under a captured greedy step: the step is captured again for the new buffer
    (its address is in the key), the sampled step -- captured after the growth -- is not"""
    p = Pair(weights, 3)
    try:
        assert p.both(seqs_greedy(POS, 2))[1] == 1
        assert p.both(seqs_sample(POS, 40))[1] == 1                # 40 x 3 ids: the buffer of 2 x 3 is replaced
        assert p.both(seqs_greedy(POS, 2))[1] == 1                 # the growth: captured for the new address
        assert p.both(seqs_sample(POS, 3))[1] == 0
        assert p.both(seqs_greedy(POS, 2))[1] == 0
    finally:
        p.free()


@pytest.mark.parametrize("lockstep", [False, True])
def test_logprob_settings_recapture(L, weights, lockstep):
    """set_logprobs -1 -> 3 -> 0 -> -1 between sampled calls: the step gains, changes and loses its record launch and its record
    buffers, so every change captures once; tokens and records are the plain context's, bit for bit"""
    p = Pair(weights, 3 if lockstep else 0)
    try:
        for n_top in (-1, 3, 0, -1):
            p.graph.set_logprobs(n_top)
            p.plain.set_logprobs(n_top)
            call = seqs_sample(POS, 4, records=n_top >= 0) if lockstep else sample(5, 4, records=n_top >= 0)
            got, grew = p.both(call)
            assert grew == 1
            if n_top >= 0:
                assert got[2].shape[-1] == n_top and np.all(got[1] > 0)
            assert p.both(call)[1] == 0
    finally:
        p.free()


# ---------------------------------------------------------------------------------------------- 3. set_fused
def test_set_fused_drops_every_step(L, weights):
    """set_fused between modes 2, 1, 0, 2: every loop's step is captured once per mode change and not otherwise; eval_token as
    well, where it replays at all (mode 0 has no fused step: plain launches, no capture)"""
    pm, ps = Pair(weights), Pair(weights, 3)
    try:
        for mode in (2, 1, 0, 2):
            for m in pm.models:
                m.set_fused(mode)
            for sc in ps.seqs:                                     # (a SeqContext has a context of its own)
                L.falcon_hip_context_set_fused(sc.ctx, mode)
            for rnd in (0, 1):
                fresh = 1 if rnd == 0 else 0
                assert pm.both(greedy(5))[1] == fresh
                assert pm.both(sample(5))[1] == fresh
                assert pm.both(token(5))[1] == (fresh if mode != 0 else 0)
                assert ps.both(seqs_greedy(POS))[1] == fresh
                assert ps.both(seqs_sample(POS))[1] == fresh
    finally:
        pm.free()
        ps.free()


# ---------------------------------------------------------------------------------------------- 4. the config epoch
def test_reference_order_change_recaptures_kquant(L, weights_q4k):
    """a Q4_K model in reference order 1, then 2: the mode signature is the same, the launch lists are not (one thread per output
    against the wave-speed mat-vec). Both orders give the reference's bits, so the tokens agree; the second call must capture
    its own step (the key holds fq_config_epoch)"""
    p = Pair(weights_q4k)
    try:
        L.ggml_hip_reference_order(1)
        first, grew = p.both(greedy(5))
        assert grew == 1
        L.ggml_hip_reference_order(2)
        second, grew = p.both(greedy(5))
        assert grew == 1
        assert first.tolist() == second.tolist()
    finally:
        L.ggml_hip_reference_order(0)
        p.free()


def test_force_gemv_recaptures_lockstep(L, weights):
    """6 lock-step sequences, then ggml_hip_debug_force_gemv(1), which sends their mat-muls through other kernels: the same call
    captures again and gives what plain launches give under the same switch"""
    firsts, pos = [7, 300, 42, 9, 111, 256], [0, 5, 11, 3, 15, 8]
    p = Pair(weights, 6)
    try:
        assert p.both(seqs_greedy(pos, firsts=firsts))[1] == 1
        L.ggml_hip_debug_force_gemv(1)
        assert p.both(seqs_greedy(pos, firsts=firsts))[1] == 1
        assert p.both(seqs_greedy(pos, firsts=firsts))[1] == 0
    finally:
        L.ggml_hip_debug_force_gemv(0)
        p.free()


# ---------------------------------------------------------------------------------------------- 5. the pipeline step's pointers
def test_stage_step_keyed_by_its_pointers(L, weights, monkeypatch):
    """falcon_hip_stage_step on a whole-model context: three steps with one set of device buffers capture once, another set of
    buffers captures once more; the tokens are falcon_hip_decode_greedy's for the same positions"""
    monkeypatch.setenv("FALCON_HIP_STAGE_GRAPH", "1")
    p = Pair(weights)
    bufs = [(g.DevBuf(4), g.DevBuf(4)) for _ in range(2)]
    try:
        want = p.plain.decode_greedy(FIRST, 5, 6)
        got, cur = [], FIRST
        for i, grew in enumerate((1, 0, 0, 1, 0, 0)):
            tok, nxt = bufs[i // 3]
            before = p.captures()
            one = np.array([cur], np.int32)
            L.ggml_hip_memcpy_h2d(tok.ptr, one.ctypes.data, 4)
            assert L.falcon_hip_stage_step(p.graph.ctx, tok.ptr, None, 5 + i, None, nxt.ptr) == 0
            cur = int(nxt.to_host(np.int32, (1,))[0])
            got.append(cur)
            assert p.captures() - before == grew
        assert got == want.tolist()
    finally:
        for pair in bufs:
            for b in pair:
                b.free()
        p.free()


# ---------------------------------------------------------------------------------------------- 6. captured batches
HP_GQA = synth.HP_TINY_GQA


@pytest.fixture(scope="module")
def weights_gqa():
    return synth.make_model(ob.Oracle(), HP_GQA, ob.Q4_0, seed=78)


class BatchPair:
    """two models of the same weights: .graph replays its batches (FALCON_HIP_PREFILL_GRAPH=1, read when a context is made), .plain launches them"""

    def __init__(self, weights, monkeypatch):
        monkeypatch.setenv("FALCON_HIP_PREFILL_GRAPH", "1")
        self.graph = g.FalconModel(weights, n_ctx=N_CTX, n_batch=16)
        monkeypatch.setenv("FALCON_HIP_PREFILL_GRAPH", "0")
        self.plain = g.FalconModel(weights, n_ctx=N_CTX, n_batch=16)

    def eval(self, n, n_past, want_hidden=False):
        """n tokens at n_past on both; asserts the same bits (logits of every row, and the hidden rows when kept); returns the captures it added"""
        tok = synth.tokens(n, HP_GQA["n_vocab"], seed=100 + n)
        before = g.graph_captures(self.graph)
        got, want = (m.eval(tok, n_past, logits_all=True, want_hidden=want_hidden) for m in (self.graph, self.plain))
        for a, b in zip(got if want_hidden else (got,), want if want_hidden else (want,)):
            assert a.shape == b.shape and a.tobytes() == b.tobytes()
        assert g.graph_captures(self.plain) == 0
        return g.graph_captures(self.graph) - before

    def free(self):
        self.graph.free()
        self.plain.free()


def test_batch_graphs_key(L, weights_gqa, monkeypatch):
    """a batch is captured once per (tokens, keys, keep_hidden, mode signature, config epoch) and replayed otherwise; the logits are those of
    plain launches, bit for bit, at every step"""
    p = BatchPair(weights_gqa, monkeypatch)
    try:
        assert [p.eval(6, 0) for _ in range(3)] == [1, 0, 0]
        assert p.eval(6, 6) == 1                                   # max_kv differs
        assert p.eval(9, 0) == 1
        assert p.eval(6, 0, want_hidden=True) == 1                 # keep_hidden: a graph of its own for a shape already seen
        assert p.eval(6, 0) == 0 and p.eval(6, 0, want_hidden=True) == 0
        L.ggml_hip_debug_force_gemv(1)
        assert p.eval(6, 0) == 1                                   # the config epoch moved
        assert p.eval(6, 0) == 0
    finally:
        L.ggml_hip_debug_force_gemv(0)
        p.free()


def test_batch_graphs_eviction(L, weights_gqa, monkeypatch):
    """eight batch graphs are kept, the oldest goes first; set_fused drops them all"""
    p = BatchPair(weights_gqa, monkeypatch)
    shapes = [(5 + i, i % 3) for i in range(9)]                    # nine distinct (N, n_past), N = 5..13
    try:
        assert [p.eval(*s) for s in shapes] == [1] * 9
        assert p.eval(*shapes[0]) == 1                             # the ninth pushed the first out
        assert p.eval(*shapes[8]) == 0
        for m in (p.graph, p.plain):
            m.set_fused(2)
        assert [p.eval(*s) for s in shapes] == [1] * 9
    finally:
        p.free()


# ---------------------------------------------------------------------------------------------- 7. the sampler part of the key, both callers
def test_sampler_key_both_callers(L, weights_gqa):
    """what the sampler's launch takes is in the key of falcon_hip_decode_sample's step and of falcon_hip_decode_spec's pass alike: turning stops on, off,
    mirostat on and the context stop on each capture once, and a repeated call does not; the draws are an ungraphed context's in every phase.
    (decode_sample with stops on / off: tests/test_gpu_stop.py has those two deltas)"""
    n0 = len(PROMPT)
    base = dict(seed=1234, **P_LOOP)
    state = dict(ext=False)

    def seed_row(m):
        if state["ext"]:
            m.set_sampling_ext(g.sampling_ext(mirostat=2, **base), [FIRST])
        else:
            m.set_sampling(g.sampling(**base), [FIRST])

    def sample_call(m, ug):
        seed_row(m)
        return m.decode_sample(FIRST, n0, 4, use_graph=ug)

    def spec_call(m, ug):
        seed_row(m)
        m.set_spec_guess([3, 5, 8, 13, 21, 34])
        return m.decode_spec(FIRST, n0, 6, use_graph=ug)

    def stops_on(m):
        m.set_stops(g.stops(max_tokens=40))

    def stops_off(m):
        m.set_stops(None)

    def mirostat_on(m):
        state["ext"] = True

    def context_stop_on(m):
        m.set_context_stop(True)

    for call, spec, switches in ((sample_call, False, (mirostat_on, context_stop_on)),
                                 (spec_call, True, (stops_on, stops_off, mirostat_on, context_stop_on))):
        state["ext"] = False
        p = Pair(weights_gqa)
        try:
            if spec:
                for m in p.models:
                    seed_row(m)
                    m.set_spec(2, g.SPEC_GIVEN)
            assert p.both(call)[1] == 1
            assert p.both(call)[1] == 0                            # steady state
            for switch in switches:
                for m in p.models:
                    switch(m)
                assert p.both(call)[1] == 1, switch.__name__
                assert p.both(call)[1] == 0, switch.__name__
        finally:
            p.free()


# ---------------------------------------------------------------------------------------------- 8. what a context makes late goes with it
def test_lifecycle_of_late_made_resources(L, weights_gqa):
    """three rounds of: a plain and a 3-sequence lock-step context, every buffer and event a context makes after its creation touched once
    (eval_score, eval_token, log-prob records that grow, a polled lock-step loop, draft-and-verify, embeddings, a context swap), both freed.
    Every round gives the first round's outputs exactly. (No memory figure is asserted: free-memory readings of a shared device measure nothing.)"""
    n0, V = len(PROMPT), HP_GQA["n_vocab"]

    def one_round():
        out = []
        m = g.FalconModel(weights_gqa, n_ctx=N_CTX, n_batch=16)
        sc = g.SeqContext(m, N_CTX, 3)
        try:
            m.eval(PROMPT, 0, logits_all=False)
            out.append(m.score(PROMPT[:8], 0, list(PROMPT[1:8]) + [-1])[:7])           # score_tgt / score_prob
            m.eval_token(FIRST, n0)                                                   # logits_pinned
            out.append(m.logits())
            for t in range(3):
                assert g.copy_seq(sc, t, m, 0, n0) == 0
                sc.set_sampling(t, g.sampling(seed=50 + t, **P_LOOP), [FIRSTS[t]])
            sc.set_logprobs(2)                                                        # lp_*: made for 2 x 3 records, then for 8 x 3
            for steps in (2, 8):
                out.append(sc.decode_sample(FIRSTS, [n0] * 3, steps, use_graph=True))  # (seq_out_dev grows with them)
                out += list(sc.logprobs())
            sc.set_logprobs(-1)
            for t in range(3):
                sc.set_stops(t, g.stops(max_tokens=3 + t))
            sc.set_stop_poll(2)                                                       # stop images and events: every row has stops, the loop polls
            out.append(sc.decode_sample(FIRSTS, [n0] * 3, 16, use_graph=True))
            assert sc.loop_steps() < 16
            m.set_sampling(g.sampling(seed=1234, **P_LOOP), [FIRST])
            m.set_spec(2, g.SPEC_GIVEN)                                               # spec images and events
            m.set_spec_guess([3, 5, 8, 13])
            out.append(m.decode_spec(FIRST, n0, 6, use_graph=True))
            m.set_spec(0)
            m.set_embedding(last=True, pool=True)
            m.eval(PROMPT[:8], 0, logits_all=False)
            out += [m.embeddings(), m.pooled()]
            m.set_embedding(last=False, pool=False)
            for t in range(3):                                                        # swap_ctx: sequence 0 runs into the end of its cache and is swapped
                sc.set_stops(t, None)
                sc.set_sampling(t, g.sampling(seed=70 + t, **P_LOOP), [FIRSTS[t]])
            sc.set_context_stop(True)
            out.append(sc.decode_sample(FIRSTS, [N_CTX - 3, n0, n0], 5, use_graph=True))
            assert sc.stop_state()[1][0] == g.STOP_CONTEXT
            sc.context_swap(0, 8, PROMPT[8:14], n_batch=4)
            out.append(sc.decode_sample([FIRST, 0, 0], [14, n0 + 5, n0 + 5], 3, use_graph=True))
        finally:
            sc.free()
            m.free()
        return out

    first = one_round()
    for _ in range(2):
        again = one_round()
        assert len(again) == len(first)
        for a, b in zip(again, first):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()

"""GPU: stop strings on the device (csrc/fq_stop_text.h in k_sample_rows' TEXT instantiations). The bare sampler draws scripted tokens
(temp <= 0 over one-hot logits rows) and every draw's reason, n_drawn and cut_bytes is compared with the rule's restatement in
tests/stop_text_ref.py; the model loops are compared with their own unstopped runs, as tests/test_gpu_stop.py compares the id stops."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ggllm_cpp_amd as g
import stop_text_ref as ref
import synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNING, BUDGET, TEXT0 = g.STOP_RUNNING, g.STOP_BUDGET, g.STOP_TEXT0
HP = synth.HP_TINY_MQA
P_LOOP = dict(temp=0.0, repeat_penalty=1.3, repeat_last_n=64)     # greedy, and a penalty that keeps the tiny model from repeating itself
PROMPT = [11, 200, 37, 4, 99]
N_CTX = 64


@pytest.fixture(scope="module")
def L():
    L = g.load()
    L.ggml_hip_init(0)
    return L


# ---------------------------------------------------------------------------------------------- 1. the sampler alone
V = 300
LONG = bytes(range(100, 230))
# the named cases' tokens, then ~50 tokens over a, b, c (lengths 0, 1, 31, 32, 33, 64, 65, 130 among them), then short fillers
NAMED = [b"xxHe", b"ll", b"o!yy", b"q", b"ab", LONG, b"abcd", b"x", b"abcdef", b"\0", b"\0\0", b"", b"cd"]
T_Q = 3


def sampler_vocab():
    rng = np.random.default_rng(7)
    v = NAMED + ref.abc_vocab(rng)
    return v + [bytes(rng.integers(97, 100, int(rng.integers(1, 4)), dtype=np.uint8)) for _ in range(V - len(v))]


# a case: operations of one row in order -- ("text", strings), ("ids", sequences, max_tokens), ("draw", token)
def case(strings, stream, ids=None, max_tokens=0):
    return [("text", strings)] + ([("ids", ids or [], max_tokens)] if ids is not None or max_tokens else []) + [("draw", t) for t in stream]


ABC0 = len(NAMED)       # first id of the a-b-c tokens: ABC0 + 5, + 6, + 7 have 64, 65 and 130 bytes
ROUNDS = [
    [case([b"Hello!"], [3, 0, 1, 2, 3]),                                   # a match spanning three tokens (cut 8: "Hello!yy")
     case([LONG[:5]], [4, 5, 4]),                                          # wholly inside a 130-byte token, at its start (cut 130)
     case([LONG[125:]], [4, 5, 4]),                                        # ... at its end (cut 5), in the token's third chunk of 64
     case([b"b" + LONG[:31]], [4, 5])],                                    # 32 bytes from the token before into the long one
    [case([b"zz", b"bcd", b"cd"], [7, 6]),                                 # two strings completing at the same byte: lowest k
     case([b"ef", b"bc"], [8]),                                            # a higher k completing earlier in the token: earliest j
     case([b"\0\0\0\0"], [9, 10, 11, 9]),                                  # longer than the drawn text: the fresh ring's zeros do not count; a token without bytes
     case([b"bcd"], [4, 12], ids=[[9], [4, 12]])],                         # id sequence and text on the same draw: id wins
    [case([b"bc"], [4, 12], max_tokens=2),                                 # text and budget on the same draw: text wins
     case([b"bc"], [12, 12], max_tokens=2),                                # ... the budget alone
     [("text", [b"bc"]), ("draw", 4), ("text", [b"bc"]), ("draw", 12), ("draw", 4), ("draw", 12)],                 # reset by set_stop_text
     [("text", [b"bc"]), ("draw", 4), ("ids", [[7]], 9), ("draw", 12), ("draw", 4), ("draw", 12)]],                # reset by set_stops
    [case([LONG[60:70], LONG[98:130]], [4, 5]),                            # across the first chunk's end; 32 bytes ending the token
     case([bytes([97, 98, 99])] * 16, [ABC0 + 5, ABC0 + 6, ABC0 + 7, ABC0 + 4]),                                   # 16 strings over the 64-, 65-, 130- and 33-byte tokens
     case([b"never"], [ABC0 + 7, ABC0 + 6, ABC0 + 5, ABC0 + 0, ABC0 + 1]),                                         # long tokens through the ring, nothing matches
     case([], [4, 12], max_tokens=2)],                                     # strings set, none given: the row is on, the budget ends it
]


def one_hot(tokens):
    x = np.zeros((len(tokens), V), np.float32)
    x[np.arange(len(tokens)), tokens] = 1.0
    return x


@pytest.fixture(scope="module")
def samplers(L):
    """s: the sampler under test with the vocabulary's bytes; plain: one that never hears of text stops. Both greedy without penalties"""
    vocab = sampler_vocab()
    pool, offs = ref.pool_of(vocab)
    s, plain = L.ggml_hip_sampler_create(5, V, 32), L.ggml_hip_sampler_create(5, V, 32)
    p = g.sampling(temp=0.0, repeat_penalty=1.0, repeat_last_n=0, seed=1)
    for r in range(5):
        assert L.ggml_hip_sampler_set_row(s, r, C.byref(p), None, 0) == 0 and L.ggml_hip_sampler_set_row(plain, r, C.byref(p), None, 0) == 0
    # refused while no vocabulary bytes are set, and nothing is made for it
    assert L.ggml_hip_sampler_set_stop_text(s, 0, C.byref(g.stop_text([b"a"]))) == 1
    assert L.ggml_hip_sampler_set_vocab_bytes(s, pool.ctypes.data, offs.ctypes.data) == 0
    yield L, s, plain, vocab
    L.ggml_hip_sampler_free(s)
    L.ggml_hip_sampler_free(plain)


def states(L, s, n=5):
    nd, rs, cut = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    assert L.ggml_hip_sampler_get_stops(s, nd.ctypes.data, rs.ctypes.data) == 0 and L.ggml_hip_sampler_get_stop_text(s, cut.ctypes.data) == 0
    return list(zip(rs.tolist(), nd.tolist(), cut.tolist()))


@pytest.mark.parametrize("rnd", range(len(ROUNDS)))
def test_sampler_named_cases_four_rows_a_launch(samplers, rnd):
    """rows 0..3 play four cases in one launch per draw, row 4 has no text stops and draws what the plain sampler's row 4 draws"""
    L, s, plain, vocab = samplers
    rng = np.random.default_rng(100 + rnd)
    ops = [list(c) for c in ROUNDS[rnd]]
    want = [ref.Restated() for _ in range(4)]
    for r in range(4):                                      # (whatever the round before left)
        assert L.ggml_hip_sampler_set_stops(s, r, None) == 0 and L.ggml_hip_sampler_set_stop_text(s, r, None) == 0
    lg, tk, tkp = g.DevBuf(5 * V * 4), g.DevBuf(5 * 4), g.DevBuf(5 * 4)
    last = [-1] * 4
    exp = [(RUNNING, 0, 0)] * 4
    try:
        while any(ops):
            toks = []
            for r in range(4):
                while ops[r] and ops[r][0][0] != "draw":
                    op = ops[r].pop(0)
                    if op[0] == "text":
                        assert L.ggml_hip_sampler_set_stop_text(s, r, C.byref(g.stop_text(op[1]))) == 0
                        want[r].set_text(op[1])
                    else:
                        assert L.ggml_hip_sampler_set_stops(s, r, C.byref(g.stops(op[1], max_tokens=op[2]))) == 0
                        want[r].set_ids(op[1], op[2])
                    exp[r] = (RUNNING, 0, 0)
                toks.append(ops[r].pop(0)[1] if ops[r] else T_Q)
            toks.append(int(rng.integers(0, V)))
            x = one_hot(toks)
            L.ggml_hip_memcpy_h2d(lg.ptr, x.ctypes.data, x.nbytes)
            L.ggml_hip_sampler_sample(s, lg.ptr, V, tk.ptr)
            L.ggml_hip_sampler_sample(plain, lg.ptr, V, tkp.ptr)
            got, gotp = tk.to_host(np.int32, (5,)).tolist(), tkp.to_host(np.int32, (5,)).tolist()
            assert gotp == toks and got[4] == gotp[4]
            for r in range(4):
                if want[r].reason == RUNNING:
                    exp[r] = want[r].draw(toks[r], vocab[toks[r]])
                    last[r] = toks[r]
                assert got[r] == last[r]                    # (an ended row is frozen: its token stays)
            assert states(L, s) == exp + [(RUNNING, 0, 0)], (rnd, toks)
        assert [e[0] != RUNNING for e in exp].count(True) >= 3 or rnd == 3
    finally:
        for b in (lg, tk, tkp):
            b.free()


def test_sampler_refusals_change_nothing(samplers):
    L, s, plain, vocab = samplers
    pool, offs = ref.pool_of(vocab)
    for r in range(5):
        assert L.ggml_hip_sampler_set_stops(s, r, None) == 0 and L.ggml_hip_sampler_set_stop_text(s, r, None) == 0
    assert L.ggml_hip_sampler_set_stop_text(s, 0, C.byref(g.stop_text([b"bcd", b"q"]))) == 0
    lg, tk = g.DevBuf(5 * V * 4), g.DevBuf(5 * 4)

    def draw(t):
        x = one_hot([t, T_Q, T_Q, T_Q, T_Q])
        L.ggml_hip_memcpy_h2d(lg.ptr, x.ctypes.data, x.nbytes)
        L.ggml_hip_sampler_sample(s, lg.ptr, V, tk.ptr)
        return states(L, s)[0]

    try:
        assert draw(4) == (RUNNING, 1, 0)                   # "ab"
        bad = [g.stop_text([b"x"]) for _ in range(4)]
        bad[0].n, bad[1].n, bad[2].len[0], bad[3].len[0] = 17, -1, 0, 33
        for b in bad:
            assert L.ggml_hip_sampler_set_stop_text(s, 0, C.byref(b)) == 1
        for row in (-1, 5):
            assert L.ggml_hip_sampler_set_stop_text(s, row, C.byref(g.stop_text([b"x"]))) == 1
        down = offs.copy()
        down[10] = down[9] - 1                              # offsets that do not ascend
        assert L.ggml_hip_sampler_set_vocab_bytes(s, pool.ctypes.data, down.ctypes.data) == 1
        big = offs.copy()
        big[V] = (16 << 20) + 1                             # a pool beyond 16 MB (refused before a byte of it is read)
        assert L.ggml_hip_sampler_set_vocab_bytes(s, pool.ctypes.data, big.ctypes.data) == 1
        assert states(L, s)[0] == (RUNNING, 1, 0)
        assert draw(12) == (TEXT0, 2, 3)                    # "ab" + "cd": the "ab" drawn before the refusals still counts
        # copy_row carries strings, ring and cut_bytes; a sampler without vocabulary bytes refuses a row that has strings
        assert L.ggml_hip_sampler_copy_row(s, 3, s, 0) == 0
        assert states(L, s)[3] == (TEXT0, 2, 3)
        assert L.ggml_hip_sampler_copy_row(plain, 0, s, 0) == 1
        assert L.ggml_hip_sampler_copy_row(s, 3, s, 1) == 0 and states(L, s)[3] == (RUNNING, 0, 0)
    finally:
        lg.free()
        tk.free()
        assert L.ggml_hip_sampler_set_stop_text(s, 0, None) == 0


# ---------------------------------------------------------------------------------------------- 2. the model loops
@pytest.fixture(scope="module")
def vocab512(L, tmp_path_factory):
    d = tmp_path_factory.mktemp("stop_text_vocab")
    ref.write_vocab_ggcc(str(d / "v512.ggcc"), ref.coded_vocab(HP["n_vocab"]))
    ref.write_vocab_ggcc(str(d / "v300.ggcc"), ref.coded_vocab(300))
    v, small = g.Vocab(str(d / "v512.ggcc")), g.Vocab(str(d / "v300.ggcc"))
    yield v, small
    v.free()
    small.free()


def start(m, seed=1234):
    """the prompt evaluated, the row seeded with the prompt as its window, every stop off, the first token drawn"""
    m.eval(PROMPT, 0, logits_all=False)
    m.set_sampling(g.sampling(seed=seed, **P_LOOP), PROMPT)
    m.set_stops(None)
    m.set_stop_text(None)
    return m.sample()


def straddle(pieces, lo=6, hi=8):
    """(a, the bytes from the middle of piece lo to the middle of piece hi) of the pieces' concatenation"""
    text = b"".join(pieces)
    a = sum(len(p) for p in pieces[:lo]) + len(pieces[lo]) // 2
    b = sum(len(p) for p in pieces[:hi]) + len(pieces[hi]) // 2
    assert all(len(p) >= 2 for p in (pieces[lo], pieces[hi])) and 1 <= b - a <= 32
    return a, text[a:b]


@pytest.fixture(scope="module")
def single(L, vocab512):
    """the model with its synthetic vocabulary, its first token, the unstopped 24 loop tokens and their bytes (computed once, never changed)"""
    weights = synth.make_model(ob.Oracle(), HP, ob.Q4_0, seed=77)
    m = g.FalconModel(weights, n_ctx=N_CTX, n_batch=8)
    vocab, small = vocab512
    # refusals before a vocabulary is there, and of one of the wrong size
    with pytest.raises(ValueError):
        m.set_stop_text(g.stop_text([b"x"]))
    with pytest.raises(ValueError):
        m.set_vocab(small)
    with pytest.raises(ValueError):
        m.set_stop_text(g.stop_text([b"x"]))
    assert m.stop_text_state() == 0 and m.stop_state() == (0, RUNNING)
    m.set_vocab(vocab)
    first = start(m)
    want = m.decode_sample(first, len(PROMPT), 24, use_graph=False).tolist()
    yield m, first, want, [vocab.token_bytes(t) for t in want], vocab
    m.free()


@pytest.mark.parametrize("use_graph", [False, True])
def test_single_stream_ends_inside_a_token_and_continues(single, use_graph):
    m, first, want, pieces, vocab = single
    n0 = len(PROMPT)
    a, stop = straddle(pieces)
    text = b"".join(pieces)
    assert text.find(stop) == a                             # its first occurrence is the one from step 6 to step 8
    cut = len(b"".join(pieces[:9])) - a
    assert start(m) == first
    assert m.decode_sample(first, n0, 24, use_graph=use_graph).tolist() == want      # (this path's unstopped run)
    m.set_stop_poll(4)
    try:
        c0 = g.graph_captures(m)
        assert start(m) == first
        m.set_stop_text(g.stop_text([stop, b"@never@"]))
        assert m.stop_state() == (0, RUNNING) and m.stop_text_state() == 0
        out = m.decode_sample(first, n0, 24, use_graph=use_graph).tolist()
        assert out[:9] == want[:9] and out[9:] == [-1] * 15
        assert m.stop_state() == (9, TEXT0) and m.stop_text_state() == cut
        assert b"".join(pieces[:9])[:-cut] == text[:a]      # the contract: the drawn tokens minus cut_bytes is the text before the stop
        assert 8 < m.loop_steps() <= (8 // 4 + 2) * 4, m.loop_steps()
        if use_graph:
            assert g.graph_captures(m) == c0 + 1            # text stops first set: one re-capture
        # the restated rule over the same stream
        r = ref.Restated()
        r.set_text([stop, b"@never@"])
        assert [r.draw(t, p) for t, p in zip(want[:9], pieces[:9])][-1] == (TEXT0, 9, cut)
        # changed strings: no re-capture; two calls: the ring carries the first call's bytes
        assert start(m) == first
        m.set_stop_text(g.stop_text([b"@never@", stop]))
        assert m.decode_sample(first, n0, 7, use_graph=use_graph).tolist() == want[:7] and m.stop_state() == (7, RUNNING)
        assert m.decode_sample(want[6], n0 + 7, 5, use_graph=use_graph).tolist() == want[7:9] + [-1] * 3
        assert m.stop_state() == (9, TEXT0 + 1) and m.stop_text_state() == cut
        if use_graph:
            assert g.graph_captures(m) == c0 + 1
        # the row continues from its end exactly as the unstopped run
        m.set_stop_text(None)
        assert m.stop_state() == (0, RUNNING) and m.stop_text_state() == 0
        assert m.decode_sample(want[8], n0 + 9, 6, use_graph=use_graph).tolist() == want[9:15]
        if use_graph:
            assert g.graph_captures(m) == c0 + 2            # ... and off again: one more
        # a budget on the same draw loses to the text; set_stops on a row with strings starts ring and cut_bytes afresh
        assert start(m) == first
        m.set_stop_text(g.stop_text([stop]))
        assert m.decode_sample(first, n0, 7, use_graph=use_graph).tolist() == want[:7]
        m.set_stops(g.stops(max_tokens=2))                  # (the bytes of steps 0..6 are gone: the text cannot complete at step 8)
        assert m.decode_sample(want[6], n0 + 7, 5, use_graph=use_graph).tolist() == want[7:9] + [-1] * 3
        assert m.stop_state() == (2, BUDGET) and m.stop_text_state() == 0
        assert start(m) == first
        m.set_stop_text(g.stop_text([stop]))
        m.set_stops(g.stops(max_tokens=9))
        assert m.decode_sample(first, n0, 24, use_graph=use_graph).tolist() == want[:9] + [-1] * 15
        assert m.stop_state() == (9, TEXT0) and m.stop_text_state() == cut
    finally:
        m.set_stop_poll(16)
        m.set_stops(None)
        m.set_stop_text(None)


FIRST5, POS5, STEPS5 = [7, 300, 42, 99, 150], [0, 5, 11, 3, 8], 24


def seed_rows(sc):
    for t in range(5):
        sc.set_sampling(t, g.sampling(seed=50 + t, **P_LOOP), [FIRST5[t]])
        sc.set_stops(t, None)
        sc.set_stop_text(t, None)


@pytest.fixture(scope="module")
def lockstep(single):
    m, vocab = single[0], single[4]
    sc = g.SeqContext(m, N_CTX, 5)
    seed_rows(sc)
    want = sc.decode_sample(FIRST5, POS5, STEPS5, use_graph=False)
    yield sc, want, [[vocab.token_bytes(int(t)) for t in want[:, s]] for s in range(5)]
    sc.free()


@pytest.mark.parametrize("use_graph", [False, True])
def test_lock_step_slots_end_on_their_own_strings(lockstep, use_graph):
    """slot 1: the text from step 6 to step 8; slot 0: a text inside its token of step 3; slot 2: strings that never match and a budget of
    10; slot 3: no strings, a budget of 12; slot 4: an id stop on its token of step 5 next to strings that never match"""
    sc, want, pieces = lockstep
    a1, stop1 = straddle(pieces[1])
    assert b"".join(pieces[1]).find(stop1) == a1
    stop0 = pieces[0][3][1:3]
    assert len(stop0) == 2
    k4 = next(k for k in range(2, 12) if int(want[k, 4]) not in want[:k, 4].tolist())
    exp, rows = [], []
    for s, (strings, ids, mx) in enumerate([([stop0], None, 0), ([b"@never@", stop1], None, 0), ([b"@never@"] * 16, [], 10), (None, [], 12),
                                            ([b"@never@"], [[int(want[k4, 4])]], 0)]):
        r = ref.Restated()
        if strings is not None:
            r.set_text(strings)
        if ids is not None:
            r.set_ids(ids, mx)
        rows.append((strings, ids, mx))
        e = None
        for t, p in zip(want[:, s].tolist(), pieces[s]):
            e = r.draw(t, p)
            if e[0] != RUNNING:
                break
        exp.append(e)
    assert exp[1] == (TEXT0 + 1, 9, len(b"".join(pieces[1][:9])) - a1) and exp[0][0] == TEXT0 and exp[0][1] <= 4
    assert exp[2][:2] == (BUDGET, 10) and exp[3][:2] == (BUDGET, 12) and exp[4][:2] == (0, k4 + 1)
    sc.set_stop_poll(4)
    try:
        seed_rows(sc)
        c0 = g.graph_captures(sc)
        if use_graph:
            sc.decode_sample(FIRST5, POS5, 1, use_graph=True)
            seed_rows(sc)
            c0 = g.graph_captures(sc)
        for s, (strings, ids, mx) in enumerate(rows):
            if ids is not None:
                sc.set_stops(s, g.stops(ids, max_tokens=mx))
            if strings is not None:
                sc.set_stop_text(s, g.stop_text(strings))
        out = sc.decode_sample(FIRST5, POS5, STEPS5, use_graph=use_graph)
        n, reason = sc.stop_state()
        cut = sc.stop_text_state()
        for s in range(5):
            assert (int(reason[s]), int(n[s]), int(cut[s])) == exp[s], s
            assert out[:exp[s][1], s].tolist() == want[:exp[s][1], s].tolist() and (out[exp[s][1]:, s] == -1).all(), s
        assert 11 < sc.loop_steps() <= (11 // 4 + 2) * 4, sc.loop_steps()      # (every slot has stops; the last ends at step 11)
        if use_graph:
            assert g.graph_captures(sc) == c0 + 1
        # slot 1 continues exactly as the unstopped run once its stops are cleared (the others stay ended)
        sc.set_stop_text(1, None)
        nxt = sc.decode_sample([int(want[exp[s][1] - 1, s]) for s in range(5)], [POS5[s] + exp[s][1] for s in range(5)], 4, use_graph=use_graph)
        assert nxt[:, 1].tolist() == want[9:13, 1].tolist()
        assert all((nxt[:, s] == -1).all() for s in (0, 2, 3, 4))
    finally:
        sc.set_stop_poll(16)
        seed_rows(sc)


def test_stop_text_moves_into_a_slot_with_the_sampler_row(single):
    """a text whose first bytes are drawn in the prompt's own context (falcon_hip_sample) and whose last bytes are drawn in the slot"""
    m, first, want, pieces, vocab = single
    fb = vocab.token_bytes(first)
    stop = fb[-2:] + pieces[0] + pieces[1][:1]
    r = ref.Restated()
    r.set_text([stop])
    assert r.draw(first, fb) == (RUNNING, 1, 0)
    exp = [r.draw(t, p) for t, p in zip(want[:2], pieces[:2])]
    assert exp[0][0] == RUNNING and exp[1] == (TEXT0, 3, len(stop) + len(pieces[1]) - 1)
    sc2 = g.SeqContext(m, N_CTX, 2)
    try:
        m.eval(PROMPT, 0, logits_all=False)
        m.set_sampling(g.sampling(seed=1234, **P_LOOP), PROMPT)
        m.set_stops(None)
        m.set_stop_text(g.stop_text([stop]))
        assert m.sample() == first and m.stop_state() == (1, RUNNING)
        assert g.copy_seq(sc2, 1, m, 0, len(PROMPT)) == 0 and g.copy_sampling(sc2, 1, m, 0) == 0
        out = sc2.decode_sample([0, first], [0, len(PROMPT)], 8, use_graph=True)
        assert out[:2, 1].tolist() == want[:2] and (out[2:, 1] == -1).all() and (out[:, 0] >= 0).all()
        n, reason = sc2.stop_state()
        assert (int(reason[1]), int(n[1]), int(sc2.stop_text_state()[1])) == exp[1]
        assert (int(reason[0]), int(n[0]), int(sc2.stop_text_state()[0])) == (RUNNING, 0, 0)
        # a row without stops copied over it turns its strings off
        assert g.copy_sampling(sc2, 1, sc2, 0) == 0
        n, reason = sc2.stop_state()
        assert (int(reason[1]), int(n[1]), int(sc2.stop_text_state()[1])) == (RUNNING, 0, 0)
    finally:
        sc2.free()
        m.set_stop_text(None)


def test_refusals_at_model_level_change_nothing(single, vocab512):
    m, first, want, pieces, vocab = single
    n0 = len(PROMPT)
    assert start(m) == first
    m.set_stop_text(g.stop_text([pieces[1] + pieces[2][:1]]))
    assert m.decode_sample(first, n0, 1).tolist() == want[:1]
    bad = [g.stop_text([b"x"]) for _ in range(4)]
    bad[0].n, bad[1].n, bad[2].len[0], bad[3].len[0] = 17, -1, 0, 33
    for b in bad:
        with pytest.raises(ValueError):
            m.set_stop_text(b)
    with pytest.raises(ValueError):
        g._set_stop_text(m.ctx, 1, g.stop_text([b"x"]))     # a plain context has one sequence
    with pytest.raises(ValueError):
        m.set_vocab(vocab512[1])                            # a vocabulary of another size than the model's n_vocab
    assert m.stop_state() == (1, RUNNING) and m.stop_text_state() == 0
    assert m.decode_sample(want[0], n0 + 1, 4).tolist() == want[1:3] + [-1] * 2      # the next draws are what they would have been
    assert m.stop_state() == (3, TEXT0) and m.stop_text_state() == len(pieces[1]) + len(pieces[2])
    # a context without lm_head refuses both entries
    weights = synth.make_model(ob.Oracle(), HP, ob.Q4_0, seed=77)
    front = g.FalconModel(weights, n_ctx=N_CTX, n_batch=8, layer_begin=0, layer_end=1)
    try:
        with pytest.raises(ValueError):
            front.set_vocab(vocab)
        with pytest.raises(ValueError):
            front.set_stop_text(g.stop_text([b"x"]))
        with pytest.raises(RuntimeError):
            front.stop_text_state()
    finally:
        front.free()
        m.set_stop_text(None)


# ---------------------------------------------------------------------------------------------- 3. the example, end to end
@pytest.fixture(scope="module")
def bpe_model(tmp_path_factory):
    """the tiny model with a real BPE vocabulary that tests/test_gpu_sample.py's example tests build"""
    import bpe_fixture
    import ggcc_writer
    vocab, merges = bpe_fixture.build(n_merges=308)
    hp = dict(synth.HP_TINY_MQA)
    hp["n_vocab"] = len(vocab)
    w = synth.make_model(ob.Oracle(), hp, ob.Q4_0, seed=321)
    path = str(tmp_path_factory.mktemp("bpe") / "tiny_bpe.ggcc")
    ggcc_writer.write_ggcc(path, w, vocab, merges)
    return path


def _example(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_prints_the_text_up_to_the_stop_text(L, bpe_model):
    """falcon_generate.py --stop-text T with the real tokenizer: T is cut from the unstopped output across a token boundary (so that --stop,
    comparing ids, could not find it) and the command prints exactly the unstopped text up to str.find(T); the batch example likewise"""
    gen, bat = _example("falcon_generate"), _example("falcon_batch_generate")
    prompt, n, seed = "The quick brown fox didn't jump", 14, 3
    samp = lambda s: g.sampling(seed=s, logit_bias={int(L.falcon_hip_token_eos()): float("-inf")})      # noqa: E731
    _, ids, raw = gen.generate(bpe_model, prompt, n, n_ctx=64, sampling=samp(seed), ignore_eos=True)
    vocab = g.Vocab(bpe_model)
    try:
        pieces = [vocab.token_bytes(int(t)) for t in ids]
    finally:
        vocab.free()
    assert b"".join(pieces) == raw and len(pieces) == n
    found = None
    for k in range(3, n - 1):                               # the last byte(s) of token k and the first of token k + 1, where that is new and printable
        if not pieces[k] or not pieces[k + 1]:
            continue
        at = len(b"".join(pieces[:k + 1])) - min(2, len(pieces[k]))
        t = raw[at:at + min(2, len(pieces[k])) + min(2, len(pieces[k + 1]))]
        if found is None and raw.find(t) == at and t.isascii() and t.decode().isprintable() and not t.startswith(b"-"):
            found = (at, t.decode())
    assert found is not None, pieces
    at, T = found
    text = raw.decode("utf-8", errors="replace")
    assert raw[:at].decode("utf-8", errors="replace") == text[:text.find(T)]
    res = gen.generate(bpe_model, prompt, n, n_ctx=64, sampling=samp(seed), ignore_eos=True, stop_text=[T])
    assert res[2] == raw[:at] and b"".join(pieces[:len(res[1])]).startswith(raw[:at + len(T)])
    got = bat.generate_batch(bpe_model, [prompt, "A"], n, n_seq=2, n_ctx=64, sampling=samp(0), seeds=[seed, 5], ignore_eos=True, stop_text=[T])
    assert got[0][2] == raw[:at]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "falcon_generate.py"), "--model", bpe_model, "--prompt", prompt, "-n", str(n),
                        "--n-ctx", "64", "--seed", str(seed), "--ignore-eos", "--stop-text=" + T], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == prompt + text[:text.find(T)] + "\n"

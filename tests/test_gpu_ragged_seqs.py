"""GPU: ragged lock-step steps -- every sequence of a lock-step context at its own position (falcon_hip_eval_seqs,
falcon_hip_decode_greedy_seqs) with prompts entering the slots by a prefill in an ordinary context and a KV slot copy
(falcon_hip_context_copy_seq). A row's logits depend on its own token, position and cache only: they equal the same row
of a uniform step of a context of the same size whose sequences are clones of it, and, where lock-step rows equal
contexts of their own (the column mat-vec range), that context's."""
import importlib.util
import os

import numpy as np
import pytest

import ggllm_cpp_amd as g
from oracle import binding as ob
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _init():
    g.init(0)


class order:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        g.load().ggml_hip_reference_order(self.mode)

    def __exit__(self, *a):
        g.load().ggml_hip_reference_order(0)


def _lengths(B, cap=45):
    return [1 + (4 * b) % cap for b in range(B)]                    # 1, 5, 9, 17, ... tokens


def _streams(hp, lengths, n_steps, seed=100):
    """per sequence: its prompt and the tokens it is fed afterwards"""
    return [(synth.tokens(n, hp["n_vocab"], seed=seed + b), synth.tokens(n_steps, hp["n_vocab"], seed=seed + 500 + b)) for b, n in enumerate(lengths)]


def _fill(m, ctxs, streams):
    """prefill sequence b's prompt in the model's own context and copy its cache into slot b of every context in ctxs"""
    for b, (p, _) in enumerate(streams):
        m.eval(p, 0, logits_all=False)
        for sc in ctxs:
            assert g.copy_seq(sc, b, m, 0, p.size) == 0


def _ragged(sc, streams, n_steps):
    """n_steps ragged eval_seqs steps: row b of step i = token i of sequence b's continuation at position len(prompt) + i"""
    out = []
    for i in range(n_steps):
        out.append(sc.eval([int(c[i]) for _, c in streams], [p.size + i for p, _ in streams]))
    return out


def _single(m, stream, n_steps):
    """the same sequence in the model's own context"""
    p, c = stream
    m.eval(p, 0, logits_all=False)
    return [m.eval(c[i:i + 1], p.size + i)[0] for i in range(n_steps)]


def _clones(m, B, n_ctx, stream, n_steps):
    """row 0 of a UNIFORM step (eval_stage) of a context of B clones of one sequence"""
    p, c = stream
    sc = g.SeqContext(m, n_ctx, B)
    m.eval(p, 0, logits_all=False)
    for j in range(B):
        assert g.copy_seq(sc, j, m, 0, p.size) == 0
    rows = [sc.eval([int(c[i])] * B, p.size + i)[0] for i in range(n_steps)]
    sc.free()
    return rows


@pytest.mark.parametrize("hp,t,B", [(synth.HP_TINY_MQA, ob.Q4_0, 4), (synth.HP_TINY_GQA, ob.Q5_1, 3), (synth.HP_TINY_GQA, ob.Q4_K, 12),
                                    (synth.HP_TINY_GQA, ob.Q6_K, 7)])
def test_ragged_rows_equal_contexts_of_their_own(oracle, hp, t, B):
    """the column mat-vec range (legacy B <= 4, k-quants at tiny widths B <= 12): every ragged row is the single context continuing that sequence, bit for bit"""
    w = synth.make_model(oracle, hp, t, seed=31)
    m = g.FalconModel(w, n_ctx=64, n_batch=48)
    streams = _streams(hp, _lengths(B), 4)
    sc = g.SeqContext(m, 64, B)
    _fill(m, [sc], streams)
    got = _ragged(sc, streams, 4)
    sc.free()
    for b in range(B):
        want = _single(m, streams[b], 4)
        for i in range(4):
            assert np.array_equal(got[i][b], want[i]), (b, i)
    m.free()


@pytest.mark.parametrize("t", [ob.Q4_0, ob.Q4_K])
@pytest.mark.parametrize("B", [7, 16, 40, 80])
def test_ragged_rows_equal_clones_in_every_lock_step_form(oracle, t, B):
    """the streaming small-batch form (7, 16), the two-branch form (40) and the tile GEMM (80): ragged row s = row 0 of a uniform step of B clones of s"""
    hp = synth.HP_TINY_GQA
    w = synth.make_model(oracle, hp, t, seed=32)
    m = g.FalconModel(w, n_ctx=64, n_batch=48)
    streams = _streams(hp, _lengths(B), 3, seed=200)
    sc = g.SeqContext(m, 64, B)
    _fill(m, [sc], streams)
    got = _ragged(sc, streams, 3)
    sc.free()
    for s in (0, B // 2 + 1, B - 1):
        want = _clones(m, B, 64, streams[s], 3)
        for i in range(3):
            assert np.array_equal(got[i][s], want[i]), (s, i)
    m.free()


@pytest.mark.parametrize("B", [3, 7, 40])
def test_equal_positions_are_the_uniform_step(oracle, B):
    """all positions equal: eval_seqs gives exactly eval_stage's bits"""
    hp = synth.HP_TINY_MQA
    w = synth.make_model(oracle, hp, ob.Q4_0, seed=33)
    m = g.FalconModel(w, n_ctx=32, n_batch=16)
    streams = _streams(hp, [9] * B, 3, seed=300)
    a, u = g.SeqContext(m, 32, B), g.SeqContext(m, 32, B)
    _fill(m, [a, u], streams)
    for i in range(3):
        tok = [int(c[i]) for _, c in streams]
        assert np.array_equal(a.eval(tok, [9 + i] * B), u.eval(tok, 9 + i)), i
    a.free(); u.free(); m.free()


@pytest.mark.parametrize("mode,hp,t", [(1, synth.HP_TINY_MQA, ob.Q4_0), (1, synth.HP_TINY_GQA, ob.Q4_K), (2, synth.HP_TINY_MQA, ob.Q4_0), (2, synth.HP_TINY_GQA, ob.Q5_1)])
def test_ragged_rows_in_the_reference_orders(oracle, mode, hp, t):
    """ggml_hip_reference_order(1) (one thread per output, f64 attention through k_rope_kv / k_attention) and (2) (the fast reference order): each
    ragged row of 5 sequences equals the oracle's order-0 evaluation of that sequence alone"""
    w = synth.make_model(oracle, hp, t, seed=34)
    B, n = 5, 3
    m = g.FalconModel(w, n_ctx=32, n_batch=24)
    streams = _streams(hp, _lengths(B, 21), n, seed=400)
    with order(mode):
        sc = g.SeqContext(m, 32, B)
        _fill(m, [sc], streams)
        got = _ragged(sc, streams, n)
        sc.free()
    m.free()
    oracle.lib.orc_set_sum_order(0)
    for b, (p, c) in enumerate(streams):
        mo = oracle.model(w, 32)
        mo.eval(p, 0)
        for i in range(n):
            want = mo.eval(c[i:i + 1], p.size + i)[0]
            assert np.array_equal(got[i][b], want), (b, i)


@pytest.mark.parametrize("B", [3, 40])
def test_device_loop_equals_the_host_loop(oracle, B):
    """decode_greedy_seqs with and without the hipGraph = eval_seqs + argmax per step; an eval_seqs at n_past + n_steps continues from there"""
    hp = synth.HP_TINY_GQA
    w = synth.make_model(oracle, hp, ob.Q4_0, seed=35)
    m = g.FalconModel(w, n_ctx=64, n_batch=48)
    streams = _streams(hp, _lengths(B), 1, seed=500)
    ctxs = [g.SeqContext(m, 64, B) for _ in range(3)]
    _fill(m, ctxs, streams)
    first = np.array([int(c[0]) for _, c in streams], np.int32)
    pos = np.array([p.size for p, _ in streams], np.int32)
    n = 6
    host, tok = [], first.copy()
    for s in range(n):
        tok = ctxs[0].eval(tok, pos + s).argmax(axis=1).astype(np.int32)      # (numpy: the first maximum)
        host.append(tok)
    host = np.stack(host)
    plain = ctxs[1].decode_greedy(first, pos, n, use_graph=False)
    graph = ctxs[2].decode_greedy(first, pos, n, use_graph=True)
    assert np.array_equal(plain, host) and np.array_equal(graph, host)
    nxt = [sc.eval(host[-1], pos + n) for sc in ctxs]
    assert np.array_equal(nxt[1], nxt[0]) and np.array_equal(nxt[2], nxt[0])
    # a second call on the captured graph, from other positions
    again = ctxs[2].decode_greedy(host[-1], pos + n, 2, use_graph=True)
    tok = host[-1]
    for s in range(2):
        tok = ctxs[0].eval(tok, pos + n + s).argmax(axis=1).astype(np.int32)
        assert np.array_equal(again[s], tok), s
    for sc in ctxs:
        sc.free()
    m.free()


def test_slot_copies(oracle):
    """a slot copied back into an ordinary context continues with the lock-step row's bits; a prefix forked into two slots gives two identical rows;
    refused copies (another model, another RoPE table, a sequence out of range, more rows than n_ctx) return 1 and leave the caches as they were"""
    hp = synth.HP_TINY_MQA
    w = synth.make_model(oracle, hp, ob.Q4_0, seed=36)
    m = g.FalconModel(w, n_ctx=32, n_batch=24)
    B = 4
    streams = _streams(hp, [3, 7, 11, 2], 4, seed=600)
    sc, ref = g.SeqContext(m, 32, B), g.SeqContext(m, 32, B)
    _fill(m, [sc, ref], streams)
    got = _ragged(sc, streams, 3)
    _ragged(ref, streams, 3)
    # slot 2 -> the model's own context, one more step there and in the slot
    p, c = streams[2]
    assert g.copy_seq(m, 0, sc, 2, p.size + 3) == 0
    alone = m.eval(c[3:4], p.size + 3)[0]
    assert np.array_equal(sc.eval([int(x[3]) for _, x in streams], [q.size + 3 for q, _ in streams])[2], alone)
    ref.eval([int(x[3]) for _, x in streams], [q.size + 3 for q, _ in streams])
    # refusals: nothing copied
    other = g.FalconModel(w, n_ctx=32, n_batch=24)
    other.eval(synth.tokens(20, hp["n_vocab"], seed=9), 0)
    rope = g.SeqContext(m, 32, B, rope_n_ctx=4096)
    m.eval(synth.tokens(20, hp["n_vocab"], seed=10), 0)
    assert g.copy_seq(sc, 0, other, 0, 8) == 1
    assert g.copy_seq(sc, 0, rope, 0, 8) == 1 and g.copy_seq(rope, 0, sc, 0, 8) == 1
    assert g.copy_seq(sc, B, m, 0, 8) == 1 and g.copy_seq(sc, -1, m, 0, 8) == 1 and g.copy_seq(sc, 0, m, 1, 8) == 1
    assert g.copy_seq(sc, 0, m, 0, 33) == 1 and g.copy_seq(sc, 0, m, 0, -1) == 1
    tok, pos = [int(x[0]) for _, x in streams], [q.size + 4 for q, _ in streams]
    assert np.array_equal(sc.eval(tok, pos), ref.eval(tok, pos))
    rope.free(); other.free(); sc.free(); ref.free()
    # fork: one prefix into two slots
    fk = g.SeqContext(m, 32, B)
    _fill(m, [fk], streams)
    p, c = streams[1]
    m.eval(p, 0, logits_all=False)
    assert g.copy_seq(fk, 3, m, 0, p.size) == 0
    lg = fk.eval([5, int(c[0]), 6, int(c[0])], [2, p.size, 1, p.size])
    assert np.array_equal(lg[1], lg[3])
    assert np.array_equal(lg[1], got[0][1])
    fk.free(); m.free()


def test_positions_out_of_range_are_refused(oracle):
    """a position < 0 or >= n_ctx: 1, nothing evaluated -- the next valid step's logits are those of a context that never saw the call"""
    hp = synth.HP_TINY_MQA
    w = synth.make_model(oracle, hp, ob.Q4_0, seed=37)
    m = g.FalconModel(w, n_ctx=16, n_batch=8)
    B = 3
    streams = _streams(hp, [2, 5, 7], 2, seed=700)
    sc, ref = g.SeqContext(m, 16, B), g.SeqContext(m, 16, B)
    _fill(m, [sc, ref], streams)
    L = g.load()
    tok = np.array([int(c[0]) for _, c in streams], np.int32)
    out = np.zeros((4, B), np.int32)
    for bad in ([-1, 5, 7], [2, 16, 7], [2, 5, 40]):
        pos = np.array(bad, np.int32)
        assert L.falcon_hip_eval_seqs(sc.ctx, tok.ctypes.data, pos.ctypes.data) == 1
    pos = np.array([2, 5, 13], np.int32)
    assert L.falcon_hip_decode_greedy_seqs(sc.ctx, tok.ctypes.data, pos.ctypes.data, 4, out.ctypes.data) == 1
    badtok = np.array([int(c[0]) for _, c in streams[:2]] + [hp["n_vocab"]], np.int32)
    assert L.falcon_hip_eval_seqs(sc.ctx, badtok.ctypes.data, np.array([2, 5, 7], np.int32).ctypes.data) == 2
    pos = [2, 5, 7]
    assert np.array_equal(sc.eval(tok, pos), ref.eval(tok, pos))
    sc.free(); ref.free(); m.free()


def test_ragged_at_falcon40b_width(oracle):
    """one 40B-shaped block (Q4_K, GQA 128/8, two norms) with spread positions: 2 sequences (the column kernels) = contexts of their own and clones,
    8 sequences (the k-quant small-batch forms) = clones"""
    hp = dict(n_vocab=512, n_embd=8192, n_head=128, n_head_kv=8, n_layer=1, n_ff=32768, two_norms=True)
    w = synth.make_model_fast(hp, ob.Q4_K, seed=38)
    m = g.FalconModel(w, n_ctx=32, n_batch=24)
    for B in (2, 8):
        streams = _streams(hp, [1 + (3 * b) % 22 for b in range(B)], 2, seed=800 + B)
        sc = g.SeqContext(m, 32, B)
        _fill(m, [sc], streams)
        got = _ragged(sc, streams, 2)
        sc.free()
        for s in ((0, 1) if B == 2 else (1, 7)):
            want = _clones(m, B, 32, streams[s], 2)
            for i in range(2):
                assert np.array_equal(got[i][s], want[i]), (B, s, i)
        if B == 2:
            for s in range(2):
                want = _single(m, streams[s], 2)
                for i in range(2):
                    assert np.array_equal(got[i][s], want[i]), (s, i)
    m.free()


def test_long_position_spread(oracle):
    """16 sequences at positions from 1 to 2000 of a 2048-token context: rows equal clones"""
    hp = synth.HP_TINY_GQA
    w = synth.make_model(oracle, hp, ob.Q4_0, seed=39)
    m = g.FalconModel(w, n_ctx=2048, n_batch=2000)
    B = 16
    lengths = [int(x) for x in np.linspace(1, 2000, B)]
    streams = _streams(hp, lengths, 2, seed=900)
    sc = g.SeqContext(m, 2048, B)
    _fill(m, [sc], streams)
    got = _ragged(sc, streams, 2)
    sc.free()
    for s in (0, 9, B - 1):
        want = _clones(m, B, 2048, streams[s], 2)
        for i in range(2):
            assert np.array_equal(got[i][s], want[i]), (s, i)
    m.free()


def test_batch_generate_example(oracle, tmp_path):
    """examples/falcon_batch_generate.py: 7 prompts of different lengths through 3 slots (refilled as prompts finish) -- each result is
    examples/falcon_generate.py's for that prompt"""
    import bpe_fixture
    import ggcc_writer
    vocab, merges = bpe_fixture.build(n_merges=308)
    hp = dict(synth.HP_TINY_MQA)
    hp["n_vocab"] = len(vocab)
    w = synth.make_model(oracle, hp, ob.Q4_0, seed=321)
    path = str(tmp_path / "tiny_bpe.ggcc")
    ggcc_writer.write_ggcc(path, w, vocab, merges)

    def load(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    gen, bat = load("falcon_generate"), load("falcon_batch_generate")
    prompts = ["The quick brown fox didn't jump", "A", "Once upon a time, in a land far away, there lived",
               "hello world", "What is 2 + 2?", "The rain in Spain stays mainly in the plain, they say", "x y z"]
    got = bat.generate_batch(path, prompts, 9, n_seq=3, n_ctx=64, chunk=4)
    assert len(got) == len(prompts)
    for p, (ids, out, text) in zip(prompts, got):
        want = gen.generate(path, p, 9, n_ctx=64)
        assert np.array_equal(ids, want[0]) and out.tolist() == want[1].tolist() and text == want[2], p


# ---- ragged rows against the ORACLE at long, boundary-straddling positions (the tests above compare GPU rows with GPU rows at positions below 64) ----
LONG_LENGTHS = [1, 127, 128, 129, 255, 256, 257, 385, 513, 1000, 1535, 2040]       # around every 128-row step of the decode attention, up to the context's end
CHUNK = 100                                                                         # prompt tokens per eval: what test_matrix_pipe_attention_ragged_prompts pins whole-model


def _long_ragged(oracle, hp, t, B, gpu_order, oracle_order):
    """B sequences prefilled to LONG_LENGTHS[:B] in the model's own context (CHUNK tokens per eval, every chunk's logits compared with the oracle's first: a
    prefill mismatch must not pass for a decode finding), slot-copied, then 4 ragged steps by eval_seqs and by decode_greedy_seqs without and with the graph:
    each row / token equals the oracle evaluating that sequence alone. Returns the list of complaints."""
    n_ctx, n = 2048, 4
    w = synth.make_model(oracle, hp, t, seed=36)
    lengths = LONG_LENGTHS[:B]
    streams = _streams(hp, lengths, n, seed=600)
    failures = []
    want_rows, want_greedy = [], []
    with order(gpu_order):
        m = g.FalconModel(w, n_ctx=n_ctx, n_batch=CHUNK)
        sc = g.SeqContext(m, n_ctx, B)
        try:
            for b, (p, c) in enumerate(streams):
                oracle.lib.orc_set_sum_order(oracle_order)
                try:
                    mo = oracle.model(w, n_ctx)
                    for a in range(0, p.size, CHUNK):
                        lo = mo.eval(p[a:a + CHUNK], a, 8)
                        lg = m.eval(p[a:a + CHUNK], a)
                        assert np.array_equal(lg, lo), "PREFILL of sequence %d, tokens %d..: not a decode finding" % (b, a)
                    assert g.copy_seq(sc, b, m, 0, p.size) == 0
                    want_rows.append([mo.eval(c[i:i + 1], p.size + i, 8)[0] for i in range(n)])
                    cur, toks = int(c[0]), []
                    for i in range(n):
                        cur = int(mo.eval(np.array([cur], np.int32), p.size + i, 8)[0].argmax())
                        toks.append(cur)
                    want_greedy.append(toks)
                finally:
                    oracle.lib.orc_set_sum_order(0)
            got = _ragged(sc, streams, n)
            for b in range(B):
                for i in range(n):
                    if not np.array_equal(got[i][b], want_rows[b][i]):
                        failures.append("eval_seqs: sequence %d (position %d) step %d differs from the oracle" % (b, lengths[b] + i, i))
            first = np.array([int(c[0]) for _, c in streams], np.int32)
            pos = np.array(lengths, np.int32)
            want = np.array(want_greedy, np.int32).T                                   # [n][B]
            for use_graph in (False, True):
                dev = sc.decode_greedy(first, pos, n, use_graph=use_graph)
                for s, b in zip(*np.nonzero(dev != want)):
                    failures.append("decode_greedy_seqs (graph %s): sequence %d (position %d) step %d: another token than the oracle's" % (use_graph, b, lengths[b] + s, s))
        finally:
            sc.free(); m.free()
    return failures


@pytest.mark.parametrize("hp,t,B", [(synth.HP_TINY_MQA, ob.Q4_0, 4), (synth.HP_TINY_GQA, ob.Q4_K, 12)])
def test_long_ragged_rows_equal_the_oracle(oracle, hp, t, B):
    """the column mat-vec range, where a ragged row's bits are a single context's: k_attn_decode_seqs with every row at another position between 1 and 2043
    (one key, the 128-row step boundaries, the end of a 2048 context) against the oracle in the backend's order (orc_set_sum_order(2), one column)"""
    failures = _long_ragged(oracle, hp, t, B, 0, 2)
    assert not failures, "\n".join(failures)


def test_long_ragged_rows_in_reference_order_2(oracle):
    """the same in the fast reference order against the oracle's order 0 (the f64 rule of test_gpu_decode_attention.py applies)"""
    failures = _long_ragged(oracle, synth.HP_TINY_MQA, ob.Q4_0, 4, 2, 0)
    assert not failures, "\n".join(failures)

"""GPU: scoring on the device. ggml_hip_score_rows (csrc/kernels_score.hip) against the host statement of the same header
(tests/host/score_harness.cpp::score_fq, itself pinned to the reference's lines with the host libm by tests/test_score_cpu.py):
the 64 bits of the sequential double sum and the 32 bits of the probability; falcon_hip_eval_score against falcon_hip_eval +
get_logits + score_fq; falcon_hip_perplexity against its own definition; examples/falcon_score.py end to end."""
import ctypes as C
import ctypes.util
import os
import sys

import numpy as np
import pytest

import ggllm_cpp_amd as g
import score_ref as sr
import synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.0


@pytest.fixture(scope="module")
def L():
    L = g.load()
    L.ggml_hip_init(0)
    return L


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return sr.build_harness(tmp_path_factory.mktemp("score"))


@pytest.fixture(scope="module")
def sets():
    return {"a": sr.set_a(), "b": sr.set_b(), "c": sr.set_c(), "d": sr.set_d(), "d1": sr.set_d(1)}


def device_score(L, rows, V, targets):
    """one launch over rows [R][stride]; the three outputs start as SENTINEL"""
    R, S = rows.shape
    lg, tg = g.DevBuf(host=rows), g.DevBuf(host=np.ascontiguousarray(targets, np.int32))
    pb, mb, sb = (g.DevBuf(host=np.full(R, SENTINEL, dt)) for dt in (np.float32, np.float32, np.float64))
    try:
        L.ggml_hip_score_rows(lg.ptr, S, R, V, tg.ptr, pb.ptr, mb.ptr, sb.ptr)
        L.ggml_hip_synchronize()
        return pb.to_host(np.float32, (R,)), mb.to_host(np.float32, (R,)), sb.to_host(np.float64, (R,))
    finally:
        for b in (lg, tg, pb, mb, sb):
            b.free()


def launch_case(base, R, seed, pad=0):
    """R rows cycling through the set (row 129 of a 130-row launch = row 0 again, same target), a quarter of the targets -1"""
    n, V = base.shape
    rows = np.full((R, V + pad), 1e30, np.float32)               # (what lies between the rows must not be read)
    rows[:, :V] = base[np.arange(R) % n]
    tg = sr.targets_for(rows[:, :V], seed)
    skip = np.random.default_rng(seed + 1).permutation(np.arange(1, R))[:R // 4]
    tg[skip] = -1
    if R == 130:
        rows[129], tg[129] = rows[0], tg[0]
    return rows, tg


def check_launch(L, H, rows, V, tg):
    want = sr.host_score(H.score_fq, rows, tg, V=V)
    got = device_score(L, rows, V, tg)
    on = tg >= 0
    assert on[0] and np.all(np.isfinite(want[0][on]))
    for a in got:
        assert np.all(a[~on] == SENTINEL), "a skipped row's slot was written"
    assert np.array_equal(got[2][on].view(np.uint64), want[2][on].view(np.uint64)), "sum bits"
    assert np.array_equal(got[0][on].view(np.uint32), want[0][on].view(np.uint32)), "prob bits"
    assert np.array_equal(got[1][on], want[1][on]), "max"
    return got


@pytest.mark.parametrize("R", [1, 65, 130])
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "d1"])
def test_kernel_matches_score_fq(L, H, sets, name, R):
    """sets (a)-(d) in launches of 1, 65 and 130 rows: the sum's 64 bits, the probability's 32, the maximum; skipped rows keep
    their sentinel; the same row at row 0 and at row 129 gives the same bits"""
    base = sets[name]
    rows, tg = launch_case(base, R, 100 + R)
    got = check_launch(L, H, rows, base.shape[1], tg)
    if R == 130:
        assert got[2][:1].view(np.uint64) == got[2][129:].view(np.uint64) and got[0][:1].view(np.uint32) == got[0][129:].view(np.uint32)


def test_kernel_row_stride(L, H, sets):
    """row_stride = V + 7 (rows no longer 16-byte aligned), the gaps filled with 1e30"""
    base = sets["d"]
    rows, tg = launch_case(base, 65, 7, pad=7)
    check_launch(L, H, rows, base.shape[1], tg)


def test_kernel_ignores_reference_order(L, H, sets):
    base = sets["b"]
    rows, tg = launch_case(base, 65, 9)
    L.ggml_hip_reference_order(2)
    try:
        check_launch(L, H, rows, base.shape[1], tg)
    finally:
        L.ggml_hip_reference_order(0)


# ---------------------------------------------------------------------------------------------- model level
MODELS = [("mqa_q4_0", synth.HP_TINY_MQA, ob.Q4_0), ("gqa_q5_1", synth.HP_TINY_GQA, ob.Q5_1)]


def _targets(rng, logits):
    """per row one of: -1, 0, V-1, the argmax, a random id -- every kind present in 8 rows"""
    N, V = logits.shape
    kinds = [np.full(N, -1), np.zeros(N, np.int64), np.full(N, V - 1), logits.argmax(axis=1), rng.integers(0, V, N)]
    return np.array([kinds[(r + 1) % 5][r] for r in range(N)], np.int32)


def _check_probs(H, got, logits, tg):
    want = sr.host_score(H.score_fq, logits, tg)[0]
    on = tg >= 0
    assert np.array_equal(got[on].view(np.uint32), want[on].view(np.uint32)) and np.all(np.isnan(got[~on])) and on.sum() >= 6


@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("name,hp,t", MODELS)
def test_eval_score_matches_eval_and_score_fq(L, H, oracle, name, hp, t, order):
    """falcon_hip_eval_score of 8 tokens at n_past 0 and of 8 more at 8: the probabilities score_fq gives over the rows
    falcon_hip_eval + get_logits return for the same calls; no logits afterwards; falcon_hip_sample draws what it draws after eval"""
    w = synth.make_model(oracle, hp, t, seed=4321)
    toks = synth.tokens(16, hp["n_vocab"], seed=5)
    rng = np.random.default_rng(3)
    L.ggml_hip_reference_order(order)
    try:
        m = g.FalconModel(w, n_ctx=64, n_batch=16)
        try:
            lg_a, lg_b = m.eval(toks[:8], 0), m.eval(toks[8:], 8)
            tok_eval = m.sample()
            assert tok_eval == int(lg_b[-1].argmax())                 # (rows start greedy)
            tg_a, tg_b = _targets(rng, lg_a), _targets(rng, lg_b)
            p_a = m.score(toks[:8], 0, tg_a)
            assert not L.falcon_hip_get_logits(m.ctx)
            p_b = m.score(toks[8:], 8, tg_b)
            assert not L.falcon_hip_get_logits(m.ctx)
            assert m.sample() == tok_eval
            _check_probs(H, p_a, lg_a, tg_a)
            _check_probs(H, p_b, lg_b, tg_b)
            assert np.array_equal(m.eval(toks[8:], 8), lg_b) and L.falcon_hip_get_logits(m.ctx)     # and back
        finally:
            m.free()
    finally:
        L.ggml_hip_reference_order(0)


def test_refusals(L, oracle):
    hp = synth.HP_TINY_MQA
    V = hp["n_vocab"]
    w = synth.make_model(oracle, hp, ob.Q4_0, seed=4321)
    toks = synth.tokens(8, V, seed=6)
    tg = np.array([3, -1, V - 1, 0, 17, -1, 200, 5], np.int32)
    m = g.FalconModel(w, n_ctx=32, n_batch=8)
    try:
        first = m.score(toks, 0, tg)
        bad = tg.copy()
        bad[4] = V
        out = np.full(8, SENTINEL, np.float32)
        assert L.falcon_hip_eval_score(m.ctx, toks.ctypes.data, 8, 0, bad.ctypes.data, out.ctypes.data) == 2
        assert np.all(out == SENTINEL)
        with pytest.raises(ValueError):
            m.score(toks, 0, bad)
        again = m.score(toks, 0, tg)
        assert np.array_equal(first.view(np.uint32), again.view(np.uint32))
        t9, g9, o9 = synth.tokens(9, V, seed=6), np.zeros(9, np.int32), np.zeros(9, np.float32)
        assert L.falcon_hip_eval_score(m.ctx, t9.ctypes.data, 9, 0, g9.ctypes.data, o9.ctypes.data) == 1      # as falcon_hip_eval: more than n_batch
    finally:
        m.free()
    stage = g.FalconModel(w, n_ctx=32, n_batch=8, layer_begin=0, layer_end=1)      # no lm_head
    try:
        out = np.full(8, SENTINEL, np.float32)
        assert L.falcon_hip_eval_score(stage.ctx, toks.ctypes.data, 8, 0, tg.ctypes.data, out.ctypes.data) == 1
        assert np.all(out == SENTINEL)
    finally:
        stage.free()


def _logf():
    """the host libm's logf: what -std::log(float) in falcon_hip_perplexity (and in the reference) calls"""
    f = C.CDLL(ctypes.util.find_library("m") or "libm.so.6").logf
    f.restype, f.argtypes = C.c_float, [C.c_float]
    return f


@pytest.mark.parametrize("name,hp,t", MODELS)
def test_perplexity_is_the_sum_over_score(L, H, oracle, golden, name, hp, t):
    """falcon_hip_perplexity(n_ctx 32, n_batch 8) == the sum, in position order, of -log over FalconModel.score calls made here
    == the same sum from falcon_hip_eval's logits through score_fq (as doubles, bit for bit)"""
    tokens = np.ascontiguousarray(golden["ggcc_models"][f"{name}_ppl_tokens"], np.int32)
    w = synth.make_model(oracle, hp, t, seed=4321)
    logf = _logf()
    n_ctx, n_batch = 32, 8
    m = g.FalconModel(w, n_ctx=64, n_batch=16)
    try:
        nll, count = m.perplexity(tokens, n_ctx, n_batch)
        nll_score = nll_eval = 0.0
        n = 0
        for c in range(tokens.size // n_ctx):
            chunk = tokens[c * n_ctx:(c + 1) * n_ctx]
            for j in range(0, n_ctx, n_batch):
                pos = np.arange(j, j + n_batch)
                tg = np.where((pos >= min(512, n_ctx // 2)) & (pos < n_ctx - 1), chunk[np.minimum(pos + 1, n_ctx - 1)], -1).astype(np.int32)
                p_dev = m.score(chunk[j:j + n_batch], j, tg)
                p_host = sr.host_score(H.score_fq, m.eval(chunk[j:j + n_batch], j), tg)[0]
                for r in np.flatnonzero(tg >= 0):
                    nll_score += -logf(float(p_dev[r]))
                    nll_eval += -logf(float(p_host[r]))
                    n += 1
        assert count == n == 45
        assert nll == nll_score == nll_eval and np.isfinite(nll) and nll > 0
    finally:
        m.free()


# ---------------------------------------------------------------------------------------------- the example, end to end
@pytest.fixture(scope="module")
def bpe_model(tmp_path_factory):
    """a tiny model with a real BPE vocabulary (tests/bpe_fixture.py), as tests/test_gpu_sample.py builds it"""
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


def test_falcon_score_example(L, H, bpe_model, monkeypatch, capsys):
    """examples/falcon_score.py on three candidates (two share their first token): the printed sums and counts are those of a
    host computation over the logits of the same sequence of evaluations (falcon_hip_eval + score_fq)"""
    ex = _example("falcon_score")
    prompt, cands = "The quick brown fox", [" jumps over the dog", " jumps high", " didn't jump"]
    ids, res = ex.score_candidates(bpe_model, prompt, cands, n_ctx=64)
    n = int(ids.size)
    cids = [r[0] for r in res]
    assert len({int(c[0]) for c in cids}) == 2 and all(c.size > 1 for c in cids)
    m = g.FalconModel.from_ggcc(bpe_model, n_ctx=64, n_batch=max(n, max(int(c.size) for c in cids)))
    try:
        def p_of(logits_row, t):
            return sr.host_score(H.score_fq, logits_row[None, :], [t])[0][0]
        first = {}
        for c in cids:
            t = int(c[0])
            if t not in first:
                first[t] = p_of(m.eval(ids, 0)[-1], t) if not first else p_of(m.eval(ids[-1:], n - 1)[-1], t)
        want = []
        for c in cids:
            lp = float(np.log(np.float64(first[int(c[0])])))
            lg = m.eval(c, n)
            for i in range(c.size - 1):
                lp += float(np.log(np.float64(p_of(lg[i], int(c[i + 1])))))
            want.append((lp, int(c.size)))
    finally:
        m.free()
    assert [(lp, cnt) for _, lp, cnt in res] == want
    assert all(np.isfinite(lp) and lp < 0 for lp, _ in want)
    monkeypatch.setattr(sys, "argv", ["falcon_score.py", "--model", bpe_model, "--prompt", prompt, "--n-ctx", "64"] + cands)
    ex.main()
    assert capsys.readouterr().out.splitlines() == [ex.format_line(c, lp, cnt) for c, (lp, cnt) in zip(cands, want)]

"""GPU: log-probabilities on the device. ggml_hip_logprob_rows (csrc/kernels_logprob.hip) against the host statement of the same
header (tests/host/logprob_harness.cpp, itself pinned to the scoring harness and a numpy yardstick by tests/test_logprob_cpu.py):
the sum's 64 bits, every probability's 32 bits, the ids; against ggml_hip_score_rows on the same device rows; then the records of
the sampled loops (falcon_hip_context_set_logprobs / falcon_hip_get_logprobs) against the harness on the logits of a host loop, and
the examples' --logprobs output."""
import os
import sys

import numpy as np
import pytest

import ggllm_cpp_amd as g
import logprob_ref as lr
import score_ref as sr
import synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.0
ID_SENTINEL = -77


@pytest.fixture(scope="module")
def L():
    L = g.load()
    L.ggml_hip_init(0)
    return L


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return lr.build_harness(tmp_path_factory.mktemp("logprob"))


def _bits(a):
    """floats as the unsigned integers of their bits (integers as they are)"""
    a = np.ascontiguousarray(a)
    return a.view({np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}.get(a.dtype, a.dtype))


def _same(xs, ys):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


def device_logprob(L, rows, V, chosen, n_top, expect_rc=0):
    """one launch over rows [R][stride]; every output starts as a sentinel. Returns prob, top_id, top_prob, max, sum"""
    R, S = rows.shape
    lg, ch = g.DevBuf(host=rows), g.DevBuf(host=np.ascontiguousarray(chosen, np.int32))
    nt = max(n_top, 1)
    pb, mb = (g.DevBuf(host=np.full(R, SENTINEL, np.float32)) for _ in range(2))
    sb = g.DevBuf(host=np.full(R, SENTINEL, np.float64))
    ib, tb = g.DevBuf(host=np.full((R, nt), ID_SENTINEL, np.int32)), g.DevBuf(host=np.full((R, nt), SENTINEL, np.float32))
    try:
        rc = g.logprob_rows(lg, S, R, V, ch, n_top, pb, ib, tb, mb, sb)
        L.ggml_hip_synchronize()
        assert rc == expect_rc
        return (pb.to_host(np.float32, (R,)), ib.to_host(np.int32, (R, nt))[:, :max(n_top, 0)], tb.to_host(np.float32, (R, nt))[:, :max(n_top, 0)],
                mb.to_host(np.float32, (R,)), sb.to_host(np.float64, (R,)))
    finally:
        for b in (lg, ch, pb, mb, sb, ib, tb):
            b.free()


def device_score(L, rows, V, targets):
    R, S = rows.shape
    lg, tg, pb = g.DevBuf(host=rows), g.DevBuf(host=np.ascontiguousarray(targets, np.int32)), g.DevBuf(host=np.full(R, SENTINEL, np.float32))
    try:
        L.ggml_hip_score_rows(lg.ptr, S, R, V, tg.ptr, pb.ptr, None, None)
        L.ggml_hip_synchronize()
        return pb.to_host(np.float32, (R,))
    finally:
        for b in (lg, tg, pb):
            b.free()


def launch_case(base, R, seed, pad=0):
    """R rows cycling through the set; chosen ids cycle through 0, V-1, the argmax, a random id, and every fifth row (not row 0) has -1;
    what lies between the rows (pad) is 1e30 and must not be read"""
    n, V = base.shape
    rows = np.full((R, V + pad), 1e30, np.float32)
    rows[:, :V] = base[np.arange(R) % n]
    ch = sr.targets_for(rows[:, :V], seed)
    ch[np.arange(R) % 5 == 4] = -1
    if R > n:
        rows[R - 1], ch[R - 1] = rows[0], ch[0]                  # (the same row at both ends of a launch)
    return rows, ch


def check_launch(L, H, rows, V, ch, n_top):
    want = lr.host_logprob(H, rows, ch, n_top, V=V)
    got = device_logprob(L, rows, V, ch, n_top)
    on = ch >= 0
    assert np.array_equal(_bits(got[4]), _bits(want[4])), "sum bits"
    assert np.array_equal(got[3], want[3]), "max"
    assert np.array_equal(_bits(got[0][on]), _bits(want[0][on])) and np.all(np.isfinite(want[0][on])), "prob bits"
    assert np.all(np.isnan(got[0][~on])), "a negative chosen id gives NaN"
    assert np.array_equal(got[1], want[1]), "top ids"
    assert np.array_equal(_bits(got[2]), _bits(want[2])), "top prob bits"
    return got


SETS = {"v333": (lambda: sr.set_b(), 0), "v4099": (lambda: sr.set_d(), 5), "v65024": (lambda: sr.set_a(), 0),
        "v33": (lambda: sr.set_d(33), 0), "v1": (lambda: sr.set_d(1), 0), "ties": (lambda: lr.tie_rows(), 0)}


WIDTH = {"v333": 333, "v4099": sr.V_ODD, "v65024": sr.V_MODEL, "v33": 33, "v1": 1, "ties": lr.V_TIES}


@pytest.mark.parametrize("name,n_top", [(name, n) for name in SETS for n in (0, 1, 5, 32) if n <= WIDTH[name]])
def test_kernel_matches_harness(L, H, name, n_top):
    """every bit of every output against fq_logprob_row; a 1-row launch and a 300-row launch (more rows than CUs, the first row again
    as the last) give that row the same record"""
    base = SETS[name][0]()
    pad = SETS[name][1]
    V = base.shape[1]
    assert V == WIDTH[name]
    launches = [base.shape[0]] if name == "v65024" else [1, 300]
    got = {}
    for R in launches:
        rows, ch = launch_case(base, R, 300 + n_top, pad)
        got[R] = check_launch(L, H, rows, V, ch, n_top)
    if 300 in got:
        assert _same([a[0] for a in got[1]], [a[0] for a in got[300]]) and _same([a[299] for a in got[300]], [a[0] for a in got[300]])


def test_kernel_tie_rule_and_minus_inf(L, H):
    """the tie set: the lowest ids holding the maximum (the yardstick with the wrong tie rule differs in every row); set d's -inf row at
    V = 33 with n_top 32 beyond its 28 finite entries: the -inf ids last, ascending, with probability 0"""
    rows = lr.tie_rows()
    got = check_launch(L, H, rows, rows.shape[1], np.zeros(rows.shape[0], np.int32), 32)
    for r, row in enumerate(rows):
        assert np.array_equal(got[1][r], np.flatnonzero(row == row.max())[:32])
        assert not np.array_equal(got[1][r], lr.top_ids(row, 32, ties_id_descending=True))
    rows = sr.set_d(33)[2:3]
    finite = int(np.isfinite(rows[0]).sum())
    got = check_launch(L, H, rows, 33, np.array([1], np.int32), 32)
    assert finite == 28 and np.array_equal(got[1][0], lr.top_ids(rows[0], 32))
    assert np.all(got[2][0, finite:] == 0) and np.all(np.diff(got[1][0, finite:]) > 0)
    z = lr.zero_row()[None, :]
    assert check_launch(L, H, z, z.shape[1], np.array([17], np.int32), 5)[1][0, :4].tolist() == [17, 40, 3, 9]


@pytest.mark.parametrize("name", ["v333", "v4099", "v65024"])
def test_kernel_equals_score_rows(L, H, name):
    """the chosen probability and each of 5 top probabilities are what ggml_hip_score_rows gives on the same device rows for those ids"""
    base = SETS[name][0]()
    rows, ch = launch_case(base, base.shape[0], 17, SETS[name][1])
    V = base.shape[1]
    got = device_logprob(L, rows, V, ch, 5)
    on = ch >= 0
    sc = device_score(L, rows, V, ch)
    assert np.array_equal(_bits(got[0][on]), _bits(sc[on])) and np.all(sc[~on] == SENTINEL)
    for j in range(5):
        assert np.array_equal(_bits(got[2][:, j]), _bits(device_score(L, rows, V, got[1][:, j]))), j


def test_kernel_ignores_reference_order(L, H):
    base = sr.set_b()
    rows, ch = launch_case(base, 64, 9)
    L.ggml_hip_reference_order(2)
    try:
        check_launch(L, H, rows, base.shape[1], ch, 5)
    finally:
        L.ggml_hip_reference_order(0)


@pytest.mark.parametrize("V,n_top", [(333, 33), (5, 6), (333, -1)])
def test_kernel_refusals(L, V, n_top):
    """n_top 33, n_top > V, n_top -1: 1 is returned and no output is touched"""
    rows = sr.set_b()[:2, :V].copy()
    R = rows.shape[0]
    lg, ch = g.DevBuf(host=rows), g.DevBuf(host=np.zeros(R, np.int32))
    pb, tb = g.DevBuf(host=np.full(R, SENTINEL, np.float32)), g.DevBuf(host=np.full((R, 40), SENTINEL, np.float32))
    ib = g.DevBuf(host=np.full((R, 40), ID_SENTINEL, np.int32))
    try:
        assert g.logprob_rows(lg, V, R, V, ch, n_top, pb, ib, tb) == 1
        L.ggml_hip_synchronize()
        assert np.all(pb.to_host(np.float32, (R,)) == SENTINEL) and np.all(tb.to_host(np.float32, (R, 40)) == SENTINEL)
        assert np.all(ib.to_host(np.int32, (R, 40)) == ID_SENTINEL)
        if n_top == 33:
            assert g.logprob_rows(lg, V, R, V, ch, 1, pb, None, None) == 1            # a missing required pointer
            assert g.logprob_rows(lg, V, R, V, ch, 0, pb, None, None) == 0            # top_* may be NULL at n_top 0
            L.ggml_hip_synchronize()
            assert np.all(np.isfinite(pb.to_host(np.float32, (R,)))) and np.all(pb.to_host(np.float32, (R,)) != SENTINEL)
    finally:
        for b in (lg, ch, pb, tb, ib):
            b.free()


# ---------------------------------------------------------------------------------------------- model level
HP = dict(n_vocab=512, n_embd=256, n_head=4, n_head_kv=1, n_layer=2, n_ff=1024, two_norms=False)      # tests/test_gpu_sample.py's
P_LOOP = dict(temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64)
PROMPT = [11, 200, 37, 4, 99]
N_TOP = 3


@pytest.fixture(scope="module")
def weights():
    return synth.make_model(ob.Oracle(), HP, ob.Q4_0, seed=77)


def _same_records(H, got, logits, chosen, n_top=N_TOP):
    """got: (prob [n], ids [n][n_top], probs [n][n_top]) == the harness on logits [n][V] with those chosen ids, bit for bit"""
    want = lr.host_logprob(H, np.asarray(logits, np.float32), chosen, n_top)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.all(np.isfinite(got[0])) and np.all(got[0] > 0), "chosen prob"
    assert np.array_equal(got[1], want[1]), "top ids"
    assert np.array_equal(_bits(got[2]), _bits(want[2])), "top probs"


def _run_single(m, p, use_graph, n_top, split):
    """prompt, sample(), 8 decode_sample steps (at once or as 2 x 4); returns the 9 tokens and, with n_top >= 0, the 9 records"""
    m.eval(PROMPT, 0, logits_all=False)
    m.set_sampling(p, PROMPT)
    m.set_logprobs(n_top)
    first = m.sample()
    recs = [m.logprobs()] if n_top >= 0 else []
    toks = [first]
    n0 = len(PROMPT)
    for a, k in ([(0, 8)] if not split else [(0, 4), (4, 4)]):
        toks += m.decode_sample(toks[-1], n0 + a, k, use_graph=use_graph).tolist()
        if n_top >= 0:
            recs.append(m.logprobs())
            assert recs[-1][0].shape == (k,) and recs[-1][1].shape == (k, n_top)
    return toks, tuple(np.concatenate([r[i] for r in recs]) for i in range(3)) if n_top >= 0 else None


@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("use_graph", [False, True])
def test_decode_sample_records_match_host_loop(L, H, weights, order, use_graph):
    """tokens do not move when logprobs are switched on; sample() records one step; the 9 records are the harness on the logits of the
    host loop eval_token + logits() over the same tokens; 8 steps at once == 2 x 4; switched off again the loop is the old one"""
    p = g.sampling(seed=1234, **P_LOOP)
    L.ggml_hip_reference_order(order)
    try:
        m = g.FalconModel(weights, n_ctx=64, n_batch=16)
        try:
            off, none = _run_single(m, p, use_graph, -1, False)
            assert none is None
            with pytest.raises(RuntimeError):
                m.logprobs()
            toks, rec = _run_single(m, p, use_graph, N_TOP, False)
            assert toks == off
            toks2, rec2 = _run_single(m, p, use_graph, N_TOP, True)
            assert toks2 == off and _same(rec, rec2)
            # the host loop over the same tokens
            m.set_logprobs(-1)
            logits = [m.eval(PROMPT, 0, logits_all=False)[-1]]
            for s in range(8):
                m.eval_token(toks[s], len(PROMPT) + s)
                logits.append(np.array(m.logits()).reshape(-1))
            _same_records(H, rec, np.stack(logits), np.array(toks, np.int32))
            assert _run_single(m, p, use_graph, -1, False)[0] == off            # off again: the old launches, the old tokens
            if order == 2:
                # what falcon_score.py would report for prompt + continuation (prompt and decode paths agree bit for bit in this order)
                seq = np.array(PROMPT + toks, np.int32)
                tg = np.full(seq.size - 1, -1, np.int32)
                tg[len(PROMPT) - 1:] = seq[len(PROMPT):]
                scored = m.score(seq[:-1], 0, tg)
                assert np.array_equal(_bits(scored[len(PROMPT) - 1:]), _bits(rec[0]))
        finally:
            m.free()
    finally:
        L.ggml_hip_reference_order(0)


@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("use_graph", [False, True])
def test_decode_sample_seqs_records_match_host_loop(L, H, weights, order, use_graph):
    """3 sequences at positions [0, 5, 11] with their own parameters and seeds, one greedy: tokens as with logprobs off; the records
    are the harness on the logits eval_seqs returns for the same steps; 6 steps at once == 2 x 3"""
    L.ggml_hip_reference_order(order)
    model = g.FalconModel(weights, n_ctx=64, n_batch=8)
    n_seq, steps = 3, 6
    ps = [g.sampling(seed=50 + t, **P_LOOP) for t in range(n_seq)]
    ps[2] = g.sampling(temp=0.0, repeat_penalty=1.1, seed=9)
    first, pos = [7, 300, 42], [0, 5, 11]
    try:
        sc, sc2 = g.SeqContext(model, 64, n_seq), g.SeqContext(model, 64, n_seq)
        try:
            def run(n_top, chunks):
                for t in range(n_seq):
                    sc2.set_sampling(t, ps[t], [first[t]])
                sc2.set_logprobs(n_top)
                tok, out, recs, at = list(first), [], [], 0
                for k in chunks:
                    o = sc2.decode_sample(tok, [pp + at for pp in pos], k, use_graph=use_graph)
                    out += o.tolist()
                    tok, at = o[-1].tolist(), at + k
                    if n_top >= 0:
                        recs.append(sc2.logprobs())
                        assert recs[-1][0].shape == (k, n_seq) and recs[-1][2].shape == (k, n_seq, n_top)
                return out, tuple(np.concatenate([r[i] for r in recs]) for i in range(3)) if n_top >= 0 else None
            off, _ = run(-1, [steps])
            got, rec = run(N_TOP, [steps])
            assert got == off
            got2, rec2 = run(N_TOP, [3, 3])
            assert got2 == off and _same(rec, rec2)
            assert run(-1, [3, 3])[0] == off
            tok = list(first)
            for s in range(steps):
                logits = sc.eval(tok, [pp + s for pp in pos])
                _same_records(H, tuple(r[s] for r in rec), logits, np.array(off[s], np.int32))
                tok = off[s]
            sc2.set_logprobs(0)                                                     # the chosen token only, and sample() on a lock-step context
            sc2.eval(first, pos)
            for t in range(n_seq):
                sc2.set_sampling(t, ps[t], [first[t]])
            drawn = sc2.sample()
            p0, i0, q0 = sc2.logprobs()
            assert drawn.tolist() == off[0] and p0.shape == (1, n_seq) and i0.shape == (1, n_seq, 0) and np.array_equal(_bits(p0[0]), _bits(rec[0][0]))
        finally:
            sc.free()
            sc2.free()
    finally:
        model.free()
        L.ggml_hip_reference_order(0)


def test_state(L, weights):
    """get_logprobs returns 1 while off and after decode_greedy; set_logprobs(33) (and -2) is refused and changes nothing"""
    m = g.FalconModel(weights, n_ctx=64, n_batch=8)
    try:
        pb, ib, tb = np.full(64, SENTINEL, np.float32), np.full(64 * 32, ID_SENTINEL, np.int32), np.full(64 * 32, SENTINEL, np.float32)
        get = lambda: L.falcon_hip_get_logprobs(m.ctx, pb.ctypes.data, ib.ctypes.data, tb.ctypes.data)
        m.eval(PROMPT, 0, logits_all=False)
        m.set_sampling(g.sampling(seed=5, **P_LOOP), PROMPT)
        first = m.sample()
        assert get() == 1 and np.all(pb == SENTINEL)
        assert L.falcon_hip_context_set_logprobs(m.ctx, 33) == 1 and L.falcon_hip_context_set_logprobs(m.ctx, -2) == 1
        with pytest.raises(ValueError):
            m.set_logprobs(33)
        assert get() == 1
        m.set_logprobs(2)
        assert get() == 1                                                           # on, but nothing recorded yet
        m.decode_sample(first, len(PROMPT), 3, use_graph=True)
        assert get() == 0 and np.all(pb[:3] > 0) and np.all(pb[3:] == SENTINEL) and np.all(ib[:6] >= 0) and np.all(ib[6:] == ID_SENTINEL)
        assert L.falcon_hip_context_set_logprobs(m.ctx, 33) == 1 and get() == 0     # a refused setting keeps the old one
        m.decode_greedy(first, len(PROMPT), 3, use_graph=True)
        assert get() == 1
        m.decode_sample(first, len(PROMPT), 2, use_graph=True)
        assert get() == 0
        m.set_logprobs(-1)
        assert get() == 1
    finally:
        m.free()


# ---------------------------------------------------------------------------------------------- the examples, end to end
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


def _main_lines(ex, argv, monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", argv)
    ex.main()
    return capsys.readouterr().out.splitlines()


def test_falcon_generate_logprobs(L, bpe_model, monkeypatch, capsys):
    """--logprobs 2: the first line is the output without the flag (greedy tokens from the sampled loop at temp 0); one line per token;
    the printed total is the sum of the recorded logs"""
    ex = _example("falcon_generate")
    argv = ["falcon_generate.py", "--model", bpe_model, "--prompt", "The quick brown fox", "-n", "7", "--n-ctx", "64"]
    plain = _main_lines(ex, argv, monkeypatch, capsys)
    lines = _main_lines(ex, argv + ["--logprobs", "2"], monkeypatch, capsys)
    assert len(plain) >= 1 and lines[:len(plain)] == plain
    ids, out, text, rec = ex.generate(bpe_model, "The quick brown fox", 7, n_ctx=64, logprobs=2)
    assert np.array_equal(out, ex.generate(bpe_model, "The quick brown fox", 7, n_ctx=64)[1]) and out.size > 0
    assert rec[0].shape == (out.size,) and rec[1].shape == (out.size, 2) and np.all(rec[1][:, 0] == out)      # (greedy: the chosen token leads)
    assert np.array_equal(_bits(rec[0]), _bits(np.ascontiguousarray(rec[2][:, 0])))
    assert len(lines) == len(plain) + out.size + 1
    assert lines[-1] == "total logprob: %.6f (%d tokens)" % (float(np.sum(np.log(rec[0].astype(np.float64)))), out.size)
    # with sampler flags: the same text as without --logprobs
    flags = ["-s", "7", "--temp", "0.8", "--ignore-eos"]
    assert _main_lines(ex, argv + flags + ["--logprobs", "0"], monkeypatch, capsys)[:len(plain)] == _main_lines(ex, argv + flags, monkeypatch, capsys)


def test_falcon_batch_generate_logprobs(L, bpe_model, tmp_path, monkeypatch, capsys):
    """3 prompts through 2 slots: the texts first, as without the flag, and falcon_generate.py's; then per prompt its records (greedy: the
    chosen token is the first alternative, with the same probability) and the total of their logs"""
    gen, bat = _example("falcon_generate"), _example("falcon_batch_generate")
    prompts = ["The quick brown fox didn't jump", "A", "hello world"]
    f = tmp_path / "prompts.txt"
    f.write_text("\n".join(prompts) + "\n", encoding="utf-8")
    argv = ["falcon_batch_generate.py", "--model", bpe_model, "--prompts", str(f), "--n-seq", "2", "-n", "6", "--n-ctx", "64"]
    plain = _main_lines(bat, argv, monkeypatch, capsys)
    lines = _main_lines(bat, argv + ["--logprobs", "2"], monkeypatch, capsys)
    assert len(plain) == 3 and lines[:3] == plain
    totals = [x for x in lines if x.startswith("total logprob: ")]
    res = bat.generate_batch(bpe_model, prompts, 6, n_seq=2, n_ctx=64, logprobs=2)
    for p, r, tot in zip(prompts, res, totals):
        want = gen.generate(bpe_model, p, 6, n_ctx=64)
        assert np.array_equal(r[1], want[1]) and r[3][0].shape == (r[1].size,) and np.array_equal(r[3][1][:, 0], r[1]), p      # (greedy: the chosen token leads)
        assert _same([r[3][0]], [r[3][2][:, 0]]) and np.all(r[3][0] > 0) and np.all(r[3][0] <= 1)
        assert tot == "total logprob: %.6f (%d tokens)" % (float(np.sum(np.log(r[3][0].astype(np.float64)))), r[1].size)
    assert len(totals) == 3

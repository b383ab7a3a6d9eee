"""GPU: guidance at model level (falcon_hip_context_set_guidance). The sampled lock-step loop with pairs against a host loop over the SAME
context -- eval per step, logits to the host, the harness mix (tests/host/guide_harness.cpp), the reference's sampling functions, the drawn
token fed to both rows of the pair -- with and without the captured step; re-capture, stops, refusals, generate_guided and the example."""
import importlib.util
import os
import sys

import numpy as np
import pytest

import ggllm_cpp_amd as g
import guide_ref as gr
import sample_ref
import synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = synth.HP_TINY_MQA
V, N_CTX, STEPS = HP["n_vocab"], 64, 24
P_LOOP = dict(temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64)


@pytest.fixture(scope="module")
def L():
    L = g.load()
    L.ggml_hip_init(0)
    return L


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return gr.build_harness(tmp_path_factory.mktemp("guide"))


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """four reference contexts: one generator each, for up to four rows that draw side by side"""
    if not os.path.exists(sample_ref.REF_SO):
        pytest.skip("oracle/_ref/libfalcon_ref.so is not built (make -C oracle ref_falcon)")
    path = sample_ref.tiny_ggcc(str(tmp_path_factory.mktemp("ggcc") / "tiny.ggcc"))
    rs = [sample_ref.RefSampler(path) for _ in range(4)]
    yield rs
    for r in rs:
        r.free()


@pytest.fixture(scope="module")
def model(L):
    m = g.FalconModel(synth.make_model(ob.Oracle(), HP, ob.Q4_0, seed=4321), n_ctx=N_CTX, n_batch=16)
    yield m
    m.free()


# (sequences, pairs (leader, guide, scale), first tokens, positions): one pair; two pairs at ragged positions and different scales, one guide below
# its leader and one above; two pairs and two unguided rows
CONFIGS = {
    "two": (2, [(0, 1, 1.5)], [7, 300], [3, 9]),
    "four": (4, [(0, 1, 1.5), (3, 2, -0.5)], [7, 300, 42, 5], [0, 5, 11, 2]),
    "six": (6, [(1, 4, 7.5), (5, 0, 1.5)], [7, 300, 42, 5, 99, 410], [0, 5, 11, 2, 8, 1]),
}


def params_for(B, pairs):
    """a parameter set per row; the rows that draw get the sampled chain with their own seeds, but one: greedy"""
    ps = [g.sampling(seed=50 + t, **P_LOOP) for t in range(B)]
    ps[pairs[-1][0]] = g.sampling(temp=0.0, repeat_penalty=1.1, repeat_last_n=64, seed=9)
    return ps


def set_rows(sc, ps, first):
    for t, p in enumerate(ps):
        sc.set_sampling(t, p, [first[t]])


def host_loop(sc, H, refs, ps, pairs, first, pos, steps):
    """the yardstick: [steps][B] tokens; a guide row's entry is its leader's"""
    B = sc.n_seq
    guides = {gd for _, gd, _ in pairs}
    drawing = [t for t in range(B) if t not in guides]
    assert len(drawing) <= len(refs)
    for i, t in enumerate(drawing):
        refs[i].seed(ps[t].seed)
    hist = {t: [first[t]] for t in drawing}
    tok, want = list(first), []
    for s in range(steps):
        lg = sc.eval(tok, [p + s for p in pos])
        rows = lg.copy()
        for ld, gd, scale in pairs:
            rows[ld] = gr.host_mix(H, lg, V, [ld], [gd], [scale])[0][0]
        nxt = [0] * B
        for i, t in enumerate(drawing):
            nxt[t] = refs[i].draw(rows[t], ps[t], g.sampling_window(hist[t], N_CTX, ps[t].repeat_last_n))
            hist[t].append(nxt[t])
        for ld, gd, _ in pairs:
            nxt[gd] = nxt[ld]
        want.append(nxt)
        tok = nxt
    return want


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_decode_sample_matches_host_loop(L, H, refs, model, name, use_graph):
    B, pairs, first, pos = CONFIGS[name]
    ps = params_for(B, pairs)
    sc = g.SeqContext(model, N_CTX, B)
    try:
        want = host_loop(sc, H, refs, ps, pairs, first, pos, STEPS)
        set_rows(sc, ps, first)
        for ld, gd, scale in pairs:
            sc.set_guidance(ld, gd, scale)
        gs, scl = sc.guidance()
        assert [(t, int(gs[t]), float(scl[t])) for t in range(B) if gs[t] >= 0] == sorted(pairs)
        got = sc.decode_sample(first, pos, STEPS, use_graph=use_graph)
        assert got.tolist() == want
        # the same run without guidance: other tokens for every leader (the mix is not dead), the same for the rows that have no guide
        for ld, _, _ in pairs:
            sc.set_guidance(ld, None)
        set_rows(sc, ps, first)
        plain = sc.decode_sample(first, pos, STEPS, use_graph=use_graph)
        guides = {gd for _, gd, _ in pairs}
        for ld, _, _ in pairs:
            assert np.any(plain[:, ld] != got[:, ld]), ld
        for t in range(B):
            if t not in guides and t not in {ld for ld, _, _ in pairs}:
                assert np.array_equal(plain[:, t], got[:, t]), t
        # in two calls: the pair goes on exactly where it was
        set_rows(sc, ps, first)
        for ld, gd, scale in pairs:
            sc.set_guidance(ld, gd, scale)
        a = sc.decode_sample(first, pos, 10, use_graph=use_graph)
        b = sc.decode_sample(a[-1], [p + 10 for p in pos], STEPS - 10, use_graph=use_graph)
        assert a.tolist() + b.tolist() == want
    finally:
        sc.free()


def test_sample_after_eval_honours_the_pairs(L, H, refs, model):
    """falcon_hip_sample after falcon_hip_eval_seqs: the leader's draw is from the mixed row, the guide's entry is the leader's"""
    B, pairs, first, pos = CONFIGS["four"]
    ps = params_for(B, pairs)
    sc = g.SeqContext(model, N_CTX, B)
    try:
        want = host_loop(sc, H, refs, ps, pairs, first, pos, 1)[0]
        set_rows(sc, ps, first)
        for ld, gd, scale in pairs:
            sc.set_guidance(ld, gd, scale)
        sc.eval(first, pos)
        assert sc.sample().tolist() == want
    finally:
        sc.free()


def test_recapture_only_at_first_pair_on_and_last_pair_off(L, model):
    """graph_captures moves when the first pair comes and the last goes, not when a scale or a pair changes; afterwards the context draws
    what a context that never had guidance draws"""
    B, first, pos = 4, [7, 300, 42, 5], [0, 5, 11, 2]
    ps = [g.sampling(seed=50 + t, **P_LOOP) for t in range(B)]
    sc, fresh = g.SeqContext(model, N_CTX, B), g.SeqContext(model, N_CTX, B)

    def run(c):
        set_rows(c, ps, first)
        return c.decode_sample(first, pos, 4, use_graph=True), g.graph_captures(c)
    try:
        _, c0 = run(sc)
        assert run(sc)[1] == c0
        sc.set_guidance(0, 1, 1.5)
        a, c1 = run(sc)
        assert c1 == c0 + 1
        sc.set_guidance(0, 1, 7.5)
        b, c2 = run(sc)
        assert c2 == c1 and np.array_equal(a[:, 0], a[:, 1]) and np.array_equal(b[:, 0], b[:, 1])
        sc.set_guidance(0, 2, 7.5)
        sc.set_guidance(3, 1, -0.5)
        c, c3 = run(sc)
        assert c3 == c1 and np.array_equal(c[:, 0], c[:, 2]) and np.array_equal(c[:, 3], c[:, 1])
        sc.set_guidance(0, None)
        assert run(sc)[1] == c1
        sc.set_guidance(3, None)
        d, c4 = run(sc)
        assert c4 == c1 + 1
        assert np.array_equal(d, run(fresh)[0])
    finally:
        sc.free()
        fresh.free()


@pytest.mark.parametrize("use_graph", [False, True])
def test_stops_on_every_leader_end_the_loop_and_the_pair_continues(L, model, use_graph):
    """two pairs, a budget on either leader: the loop ends early, the guides' columns are their leaders' (-1 behind the end included); with the stops
    cleared the next call continues both rows of each pair to the tokens of an unstopped run"""
    B, pairs, first, pos = CONFIGS["four"]
    ps = params_for(B, pairs)
    sc = g.SeqContext(model, N_CTX, B)
    try:
        sc.set_stop_poll(2)
        set_rows(sc, ps, first)
        for ld, gd, scale in pairs:
            sc.set_guidance(ld, gd, scale)
        want = sc.decode_sample(first, pos, STEPS, use_graph=use_graph)
        assert sc.loop_steps() == STEPS and np.all(want >= 0)
        set_rows(sc, ps, first)
        sc.set_stops(0, g.stops(max_tokens=6))
        sc.set_stops(3, g.stops(max_tokens=6))
        got = sc.decode_sample(first, pos, STEPS, use_graph=use_graph)
        assert sc.loop_steps() < STEPS
        assert np.array_equal(got[:6], want[:6]) and np.all(got[6:] == -1)
        assert np.array_equal(got[:, 1], got[:, 0]) and np.array_equal(got[:, 2], got[:, 3])
        n_drawn, reason = sc.stop_state()
        assert (n_drawn[0], n_drawn[3], reason[0], reason[3]) == (6, 6, g.STOP_BUDGET, g.STOP_BUDGET)
        # the stops cleared (generators and windows stay): both rows of either pair go on from the sixth token, exactly
        sc.set_stops(0, None)
        sc.set_stops(3, None)
        rest = sc.decode_sample(got[5], [p + 6 for p in pos], STEPS - 6, use_graph=use_graph)
        assert np.array_equal(rest, want[6:])
    finally:
        sc.free()


def test_refusals_leave_the_context_usable(L, model):
    """what set_guidance refuses at model level, and what is refused while a pair exists; after each the context draws what it drew before"""
    B, pairs, first, pos = CONFIGS["four"]
    ps = params_for(B, pairs)
    w = synth.make_model(ob.Oracle(), HP, ob.Q4_0, seed=4321)
    # a context of one sequence; contexts without an lm_head
    assert L.falcon_hip_context_set_guidance(model.ctx, 0, 1, 1.5) == 1 and L.falcon_hip_context_set_guidance(model.ctx, 0, -1, 1.5) == 1
    stage = g.FalconModel(w, n_ctx=N_CTX, n_batch=8, layer_begin=0, layer_end=1)
    try:
        ss = g.SeqContext(stage, N_CTX, 2)
        try:
            assert L.falcon_hip_context_set_guidance(ss.ctx, 0, 1, 1.5) == 1
            assert L.falcon_hip_context_get_guidance(ss.ctx, None, None) == 1
        finally:
            ss.free()
    finally:
        stage.free()
    sc = g.SeqContext(model, N_CTX, B)
    try:
        assert sc.guidance()[0].tolist() == [-1] * B            # (before the context ever sampled)
        sc.set_guidance(2, None)                                # off where nothing is on
        with pytest.raises(ValueError):
            sc.set_guidance(9, None)
        set_rows(sc, ps, first)
        for ld, gd, scale in pairs:
            sc.set_guidance(ld, gd, scale)
        want = sc.decode_sample(first, pos, 6, use_graph=True)

        def same():
            assert sc.guidance()[0].tolist() == [1, -1, -1, 2]
            set_rows(sc, ps, first)
            assert np.array_equal(sc.decode_sample(first, pos, 6, use_graph=True), want)
        for seq, gd, scale in ((0, 0, 1.5), (4, 1, 1.5), (0, 4, 1.5), (-1, 1, 1.5), (0, 3, 1.5), (0, 2, 1.5), (1, 0, 1.5), (2, 1, 1.5),
                               (0, 1, float("nan")), (0, 1, float("inf"))):
            with pytest.raises(ValueError):
                sc.set_guidance(seq, gd, scale)
        same()
        with pytest.raises(ValueError):
            sc.set_context_stop(True)
        for seq in (0, 1, 2, 3):
            assert L.falcon_hip_context_swap(sc.ctx, seq, 0, None, 0, 1) == 1
        same()
        for ld, _, _ in pairs:
            sc.set_guidance(ld, None)
        sc.set_context_stop(True)
        with pytest.raises(ValueError):
            sc.set_guidance(0, 1, 1.5)
        sc.set_context_stop(False)
        for ld, gd, scale in pairs:
            sc.set_guidance(ld, gd, scale)
        same()
    finally:
        sc.free()


# ---------------------------------------------------------------------------------------------- generate_guided and the example, end to end
@pytest.fixture(scope="module")
def bpe_model(tmp_path_factory):
    """a tiny model with a real BPE vocabulary (tests/bpe_fixture.py), as tests/test_gpu_sample.py builds it"""
    import bpe_fixture
    import ggcc_writer
    vocab, merges = bpe_fixture.build(n_merges=308)
    hp = dict(HP)
    hp["n_vocab"] = len(vocab)
    w = synth.make_model(ob.Oracle(), hp, ob.Q4_0, seed=321)
    path = str(tmp_path_factory.mktemp("bpe") / "tiny_bpe.ggcc")
    ggcc_writer.write_ggcc(path, w, vocab, merges)
    return path


def host_guided(m, H, ids, neg, n_predict, scale, draw):
    """generate_guided's definition on the host: the two prefills, then per step one lock-step eval of the pair, the harness mix and draw(mixed row, history)"""
    ids, neg = [int(t) for t in ids], [int(t) for t in neg]
    nv = m.hp["n_vocab"]
    sc = g.SeqContext(m, m.n_ctx, 2)
    try:
        for slot, toks in enumerate((ids, neg)):
            if len(toks) > 1:
                m.eval(toks[:-1], 0, logits_all=False)
                assert g.copy_seq(sc, slot, m, 0, len(toks) - 1) == 0
        tok, hist, out = [ids[-1], neg[-1]], list(ids), []
        for s in range(n_predict):
            lg = sc.eval(tok, [len(ids) - 1 + s, len(neg) - 1 + s])
            t = draw(gr.host_mix(H, lg, nv, [0], [1], [scale])[0][0], hist)
            out.append(t)
            hist.append(t)
            tok = [t, t]
        return out
    finally:
        sc.free()


@pytest.mark.parametrize("use_graph", [False, True])
def test_generate_guided_equals_host_replay(L, H, refs, model, use_graph):
    prompt, negative = [11, 200, 37, 4, 99], [3, 450, 8]
    p = g.sampling(seed=1234, **P_LOOP)
    refs[0].seed(p.seed)
    want = host_guided(model, H, prompt, negative, 12, 1.5, lambda y, hist: refs[0].draw(y, p, g.sampling_window(hist, N_CTX, p.repeat_last_n)))
    assert g.generate_guided(model, prompt, negative, 12, p, 1.5, use_graph=use_graph) == want
    # a one-token negative prompt (no prefill for slot 1), a budget that ends the pair early
    refs[0].seed(p.seed)
    want = host_guided(model, H, prompt, [5], 12, 7.5, lambda y, hist: refs[0].draw(y, p, g.sampling_window(hist, N_CTX, p.repeat_last_n)))
    end = {}
    assert g.generate_guided(model, prompt, [5], 12, p, 7.5, stops=g.stops(max_tokens=7), use_graph=use_graph, end=end) == want[:7]
    assert (end["n_drawn"], end["reason"]) == (7, g.STOP_BUDGET)


def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_falcon_generate_prints_the_guided_replay(L, H, bpe_model, monkeypatch, capsys):
    """examples/falcon_generate.py --cfg-negative-prompt ... --cfg-scale 1.5 --temp 0 prints the text of the host replay (greedy on the mixed row, up to
    end-of-text); --cfg-scale alone takes the begin-of-text token as the negative prompt; the flags it is not combined with are refused with a message"""
    ex = _example("falcon_generate")
    prompt, negative, n = "The quick brown fox", "A slow dog", 10
    eos, bos = int(L.falcon_hip_token_eos()), int(L.falcon_hip_token_bos())
    vocab = g.Vocab(bpe_model)
    m = g.FalconModel.from_ggcc(bpe_model, n_ctx=64, n_batch=16)
    try:
        texts = []
        for neg in (vocab.tokenize(negative), np.array([bos], np.int32)):
            out = host_guided(m, H, vocab.tokenize(prompt), neg, n, 1.5, lambda y, hist: int(np.argmax(y)))
            out = out[:out.index(eos)] if eos in out else out
            texts.append(prompt + vocab.detokenize(out).decode("utf-8", errors="replace") + "\n")
    finally:
        m.free()
        vocab.free()
    # (--temp 0 brings falcon_main's other defaults along: the replay applies no penalty, so its repeat penalty is turned off)
    base = ["falcon_generate.py", "--model", bpe_model, "--prompt", prompt, "-n", str(n), "--n-ctx", "64", "--temp", "0", "--repeat-penalty", "1"]
    monkeypatch.setattr(sys, "argv", base + ["--cfg-negative-prompt", negative, "--cfg-scale", "1.5"])
    ex.main()
    assert capsys.readouterr().out == texts[0]
    monkeypatch.setattr(sys, "argv", base + ["--cfg-scale", "1.5"])
    ex.main()
    assert capsys.readouterr().out == texts[1]
    for extra, word in ((["--draft", "4"], "--draft"), (["--context-swap"], "--context-swap"), (["--prompt-cache", "x.session"], "--prompt-cache")):
        monkeypatch.setattr(sys, "argv", base + ["--cfg-negative-prompt", negative] + extra)
        with pytest.raises(SystemExit) as e:
            ex.main()
        assert word in str(e.value) and "--cfg" in str(e.value)

"""GPU: generation past n_ctx as falcon_main does it (falcon_main.cpp:694-751). The reference's own runs on the tiny BPE model at -c 32
(tests/golden/ctx_swap.npz: the printed bytes and the ids of every reset block; written on a CPU by tests/gen_ctx_swap_golden.py) are
reproduced through the library in reference orders 1 and 2; the pieces -- the stop at the end of the cache inside the sampler's launch,
resume, the swap of a single stream and of a lock-step slot -- are checked against the cache's bytes, the stop states and runs of the
existing primitives."""

import os

import numpy as np
import pytest

import ctx_swap_ref as cr
import ggllm_cpp_amd as g
import session_ref as sr
import synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

RUNNING, BUDGET, CONTEXT, TEXT0 = g.STOP_RUNNING, g.STOP_BUDGET, g.STOP_CONTEXT, g.STOP_TEXT0
N_CTX = cr.N_CTX


@pytest.fixture(scope="module")
def env(oracle, golden, tmp_path_factory):
    """the tiny byte-level-BPE model as a GGCC file, its vocabulary, the golden"""
    import bpe_fixture
    import ggcc_writer
    L = g.load()
    L.ggml_hip_init(0)
    path = str(tmp_path_factory.mktemp("ctx_swap") / "tiny_bpe.ggcc")
    vocab, merges = bpe_fixture.build(n_merges=308)
    hp = dict(synth.HP_TINY_MQA)
    hp["n_vocab"] = len(vocab)
    ggcc_writer.write_ggcc(path, synth.make_model(oracle, hp, ob.Q4_0, seed=321), vocab, merges)
    z = golden["ctx_swap"]
    v = g.Vocab(path)
    yield dict(L=L, path=path, vocab=v, gold={k: z[k] for k in z.files}, eos=int(L.falcon_hip_token_eos()))
    v.free()


class order:
    """ggml_hip_reference_order(mode) for a block"""

    def __init__(self, L, mode):
        self.L, self.mode = L, mode

    def __enter__(self):
        self.L.ggml_hip_reference_order(self.mode)

    def __exit__(self, *a):
        self.L.ggml_hip_reference_order(0)


def case(env, name):
    """(prompt ids, n_system, n_predict, n_batch, keep, sampling parameters) of a golden case, the flags read as falcon_main reads them"""
    prompt, n_predict, n_batch, seed, keep, system, flags = cr.CASES[name]
    v = env["vocab"]
    sys_ids = v.tokenize(system, add_bos=False).tolist() if system else []
    ids = sys_ids + v.tokenize(prompt, add_bos=False).tolist()
    assert ids == env["gold"][name + ".prompt_ids"].tolist()
    base = dict(seed=seed, logit_bias={env["eos"]: float("-inf")})            # (--ignore-eos; the other defaults are falcon_main's)
    ext = {}
    for flag, val in zip(flags[::2], flags[1::2]):
        if flag == "--temp":
            base["temp"] = float(val)
        else:
            ext[{"--mirostat": "mirostat", "--tfs": "tfs_z", "--typical": "typical_p"}[flag]] = int(val) if flag == "--mirostat" else float(val)
    return ids, len(sys_ids), n_predict, n_batch, keep, (g.sampling_ext(**ext, **base) if ext else g.sampling(**base))


def blocks_of(gold, name):
    ids, out = gold[name + ".block_ids"].tolist(), []
    for n in gold[name + ".block_len"].tolist():
        out.append(ids[:n])
        ids = ids[n:]
    return out


def prefill(model, ids, n_batch, params):
    for i in range(0, len(ids), n_batch):
        model.eval(ids[i:i + n_batch], i, logits_all=False)
    (model.set_sampling_ext if isinstance(params, g.SamplingExt) else model.set_sampling)(params, ids)


def kv_rows(obj, hp, n_tok, seq=None):
    """K and V rows [0, n_tok) of a sequence, read back through copy_state"""
    blob = obj.copy_state(n_tok) if seq is None else obj.copy_state(seq, n_tok)
    s = sr.split_state(bytes(blob), hp["n_layer"], hp["n_head_kv"] * 64)
    assert s["n_tok"] == n_tok
    return s["k"].tobytes() + s["v"].tobytes()


# ---------------------------------------------------------------------------------------------- 1. the reference's runs
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", list(cr.CASES))
def test_golden_case(env, name, mode):
    """prompt bytes + detokenised tokens are the bytes falcon_main printed; the driver's swaps are its reset blocks"""
    ids, n_sys, n_predict, n_batch, keep, params = case(env, name)
    gold, v = env["gold"], env["vocab"]
    with order(env["L"], mode):
        m = g.FalconModel.from_ggcc(env["path"], n_ctx=N_CTX, n_batch=n_batch)
        try:
            out, swaps = g.generate_swap(m, ids, n_predict, params, n_keep=keep, n_system=n_sys, n_batch=n_batch)
            n_drawn, reason = m.stop_state()
        finally:
            m.free()
    want = blocks_of(gold, name)
    assert len(swaps) == len(want) >= 2
    assert [r for _, r in swaps] == [b[:-1] for b in want]
    assert [(nk, r + b[-1:]) for (nk, r), b in zip(swaps, want)] == cr.replay(ids, out, N_CTX, n_batch, keep, n_sys)
    assert out == gold[name + ".drawn"].tolist()
    assert v.detokenize(ids) + v.detokenize(out) == bytes(gold[name + ".stdout"])
    assert (n_drawn, reason) == (n_predict, BUDGET)


# ---------------------------------------------------------------------------------------------- 2. the row ends at the draw that fills its cache
def test_row_ends_at_the_filling_draw_and_kept_rows_stay(env):
    ids, n_sys, _, n_batch, _, params = case(env, "p_keep6")
    m = g.FalconModel.from_ggcc(env["path"], n_ctx=N_CTX, n_batch=n_batch)
    try:
        prefill(m, ids, n_batch, params)
        m.set_context_stop(True)
        first = m.sample()
        nk = 6
        before = kv_rows(m, m.hp, nk)
        out = m.decode_sample(first, len(ids), 40, use_graph=True).tolist()
        fill = N_CTX - len(ids)                             # steps that evaluate positions len(ids) .. n_ctx - 1: the last one's draw fills the cache
        assert all(t >= 0 for t in out[:fill]) and out[fill:] == [-1] * (40 - fill)
        assert m.stop_state() == (1 + fill, CONTEXT)        # (the first draw counted: the stops were on)
        assert kv_rows(m, m.hp, nk) == before
        frozen = kv_rows(m, m.hp, N_CTX)
        # riding on frozen: the same token at the same position, the same rows, nothing drawn
        assert m.decode_sample(out[fill - 2], N_CTX - 1, 5, use_graph=True).tolist() == [-1] * 5
        assert kv_rows(m, m.hp, N_CTX) == frozen and m.stop_state() == (1 + fill, CONTEXT)
        hist = cr.prompt_history(ids, n_batch) + [first] + out[:fill]
        a, r = g.swap_plan(N_CTX, len(ids), len(hist), n_keep=nk)
        assert (a, r) == (6, 10)
        m.context_swap(a, hist[len(hist) - 1 - r:len(hist) - 1], n_batch)
        assert m.stop_state() == (1 + fill, RUNNING)
        after = kv_rows(m, m.hp, N_CTX)
        assert kv_rows(m, m.hp, nk) == before
        assert after != frozen                              # (rows behind the kept ones were evaluated again)
        with pytest.raises(ValueError):
            m.resume()                                      # running: refused
        with pytest.raises(ValueError):
            m.context_swap(a, hist[:r], n_batch)            # ... and so is a second swap
    finally:
        m.free()


# ---------------------------------------------------------------------------------------------- 3. nothing is written past a slot
def test_frozen_row_writes_nothing_past_its_slot(env):
    """slot 1 has ended and its whole cache is read; slot 0 fills its cache and rides on frozen for 20 steps: slot 1's rows, the first of which
    lies right behind slot 0's last, keep their bytes"""
    ids, _, _, n_batch, _, params = case(env, "p25_keep0")
    m = g.FalconModel.from_ggcc(env["path"], n_ctx=N_CTX, n_batch=n_batch)
    sc = g.SeqContext(m, N_CTX, 2)
    try:
        prefill(m, ids, n_batch, params)
        first = m.sample()
        assert g.copy_seq(sc, 0, m, 0, len(ids)) == 0 and g.copy_sampling(sc, 0, m, 0) == 0
        sc.set_sampling(1, params, ids)
        sc.set_stops(1, g.stops(max_tokens=1))
        sc.set_context_stop(True)
        sc.set_stop_poll(64)                                # (no early end: the frozen steps are what is looked at)
        tok, pos = np.array([first, 7], np.int32), np.array([len(ids), 0], np.int32)
        out = sc.decode_sample(tok, pos, 2)
        assert out[0, 1] >= 0 and out[1, 1] == -1 and sc.stop_state()[1].tolist() == [RUNNING, BUDGET]
        other = kv_rows(sc, m.hp, N_CTX, seq=1)
        tok[0], pos[0] = out[1, 0], len(ids) + 2
        fill = N_CTX - int(pos[0])
        out = sc.decode_sample(tok, pos, fill + 20)
        assert sc.loop_steps() == fill + 20
        assert all(t >= 0 for t in out[:fill, 0]) and (out[fill:, 0] == -1).all() and (out[:, 1] == -1).all()
        assert sc.stop_state()[1].tolist() == [CONTEXT, BUDGET] and int(sc.stop_state()[0][0]) == 2 + fill      # (the draw in the prompt's own context came before the slot's stops)
        assert kv_rows(sc, m.hp, N_CTX, seq=1) == other
    finally:
        sc.free()
        m.free()


# ---------------------------------------------------------------------------------------------- 4. precedence on the filling draw
def test_other_rules_win_on_the_filling_draw(env):
    """the tokens are learnt from a first run; then an id sequence, the budget and a stop string that complete on the filling draw each end the
    row with their own reason, and such a row is neither resumed nor swapped"""
    ids, _, _, n_batch, _, params = case(env, "p_keep0")
    v = env["vocab"]
    m = g.FalconModel.from_ggcc(env["path"], n_ctx=N_CTX, n_batch=n_batch)
    try:
        m.set_vocab(v)

        def run(stops=None, text=None):
            prefill(m, ids, n_batch, params)
            m.set_stops(stops)
            m.set_stop_text(text)
            m.set_context_stop(True)
            first = m.sample()
            out = [first] + [t for t in m.decode_sample(first, len(ids), 40).tolist() if t >= 0]
            return out, m.stop_state()

        out, (n, reason) = run()
        assert reason == CONTEXT and n == len(out) == 1 + N_CTX - len(ids)
        never = next(t for t in range(m.hp["n_vocab"]) if t not in out)      # (a sequence that does not complete, ahead of the one that does)
        for stops, text, want in ((g.stops([out[-3:]]), None, 0), (g.stops(max_tokens=n), None, BUDGET),
                                  (None, g.stop_text([(v.detokenize(out[-3:]))[-32:]]), TEXT0), (g.stops([[never], out[-3:]], max_tokens=n), None, 1)):
            got, state = run(stops, text)
            assert got == out and state == (n, want), (want, state)
            with pytest.raises(ValueError):
                m.resume()
            with pytest.raises(ValueError):
                m.context_swap(0, out[:4], n_batch)
            assert m.stop_state() == (n, want)
    finally:
        m.free()


# ---------------------------------------------------------------------------------------------- 5. the stops' state crosses the swap
def first_end(drawn, seq=None, text=None, vocab=None):
    """draws until a stop sequence / stop string first completes in a stream (None: never)"""
    raw = b""
    for i, t in enumerate(drawn):
        if seq is not None and drawn[max(0, i + 1 - len(seq)):i + 1] == seq:
            return i + 1
        if text is not None:
            b = vocab.token_bytes(t)
            if text in raw[max(0, len(raw) - len(text) + 1):] + b:
                return i + 1
            raw += b
    return None


def test_stop_state_survives_the_swap(env):
    ids, n_sys, n_predict, n_batch, keep, params = case(env, "p_keep0")
    gold, v = env["gold"], env["vocab"]
    drawn = gold["p_keep0.drawn"].tolist()
    at = 1 + N_CTX - len(ids)                               # draws up to and including the one that fills the cache
    seq = drawn[at - 1:at + 1]                              # the last draw before the swap, the first one after it
    text = (v.token_bytes(drawn[at - 1]) + v.token_bytes(drawn[at]))[-32:]
    assert first_end(drawn, seq=seq) == at + 1 and first_end(drawn, text=text, vocab=v) == at + 1, "the fixture's stream repeats the pair earlier"
    with order(env["L"], 1):
        m = g.FalconModel.from_ggcc(env["path"], n_ctx=N_CTX, n_batch=n_batch)
        try:
            m.set_vocab(v)
            out, swaps = g.generate_swap(m, ids, n_predict, params, n_keep=keep, n_batch=n_batch, stops=g.stops([seq]))
            assert out == drawn[:at + 1] and len(swaps) == 1 and m.stop_state() == (at + 1, 0)
            m.set_stop_text(None)
            out, swaps = g.generate_swap(m, ids, n_predict, params, n_keep=keep, n_batch=n_batch, stops=g.stops(), stop_text=g.stop_text([text]))
            assert out == drawn[:at + 1] and len(swaps) == 1 and m.stop_state() == (at + 1, TEXT0)
            assert m.stop_text_state() == len(text)         # (the match ends with the token's last byte)
            m.set_stop_text(None)
            out, swaps = g.generate_swap(m, ids, 50, params, n_keep=keep, n_batch=n_batch)      # a budget across two swaps
            assert out == drawn[:50] and len(swaps) == 2 and m.stop_state() == (50, BUDGET)
        finally:
            m.free()


# ---------------------------------------------------------------------------------------------- 6. lock-step slots
SLOTS = ("p_keep0", "p25_keep0", "sys_mirostat2")           # prompts of 11, 25 and 19 tokens: three different steps at which a cache is full


def run_slots(env, m, sc, jobs, captures=None):
    """every job in a slot of its own, swapped in place whenever it ends with STOP_CONTEXT, until its budget; returns the drawn tokens per slot"""
    B = len(jobs)
    sc.set_context_stop(True)
    tok, pos, drawn = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    gen, hist, live = [], [], [True] * B
    for s, (ids, n_sys, n_predict, n_batch, keep, params) in enumerate(jobs):
        prefill(m, ids, n_batch, params)
        m.set_stops(g.stops(max_tokens=n_predict))
        first = m.sample()
        assert g.copy_seq(sc, s, m, 0, len(ids)) == 0 and g.copy_sampling(sc, s, m, 0) == 0
        tok[s], pos[s], drawn[s] = first, len(ids), 1
        gen.append([first])
        hist.append(cr.prompt_history(ids, n_batch) + [first])
    while any(live):
        out = sc.decode_sample(tok, pos, 2 * N_CTX, use_graph=True)
        n_drawn, reason = sc.stop_state()
        for s, (ids, n_sys, n_predict, n_batch, keep, params) in enumerate(jobs):
            if not live[s]:
                continue
            new = out[:int(n_drawn[s] - drawn[s]), s].tolist()
            assert new and min(new) >= 0
            gen[s] += new
            hist[s] += new
            drawn[s] = n_drawn[s]
            if reason[s] == CONTEXT:
                nk, nr = g.swap_plan(N_CTX, len(ids), len(hist[s]), n_keep=keep, n_system=n_sys)
                sc.context_swap(s, nk, hist[s][len(hist[s]) - 1 - nr:len(hist[s]) - 1], n_batch)
                tok[s], pos[s] = new[-1], nk + nr
                if captures is not None:
                    captures.append(g.graph_captures(sc))
            else:
                assert reason[s] == BUDGET
                live[s], tok[s], pos[s] = False, 0, 0       # (parked: an ended row rides on frozen wherever it is told to)
    return gen


def by_hand(m, job):
    """the same generation through the primitives that were there before: eval, sample, decode_sample within the cache"""
    ids, n_sys, n_predict, n_batch, keep, params = job
    prefill(m, ids, n_batch, params)
    m.set_stops(None)
    tok = m.sample()
    out, hist, pos = [tok], cr.prompt_history(ids, n_batch) + [tok], len(ids)
    while len(out) < n_predict:
        if pos == N_CTX:
            nk, nr = cr.plan(N_CTX, n_sys, keep, len(ids), len(hist))
            regen = hist[len(hist) - 1 - nr:len(hist) - 1]
            for i in range(0, nr, n_batch):
                m.eval(regen[i:i + n_batch], nk + i, logits_all=False)
            pos = nk + nr
        got = m.decode_sample(tok, pos, min(n_predict - len(out), N_CTX - pos), use_graph=True).tolist()
        out += got
        hist += got
        pos += len(got)
        tok = got[-1]
    return out


@pytest.mark.parametrize("mode", [2, 0])
def test_lock_step_slots_swap_in_place(env, mode):
    """three slots reach the end of their caches at different steps and are swapped in place while the others ride on. Reference order 2: every
    slot's tokens are the golden's for its prompt. Default order: they are what one stream gives through eval + decode_sample"""
    jobs = [case(env, n) for n in SLOTS]
    with order(env["L"], mode):
        m = g.FalconModel.from_ggcc(env["path"], n_ctx=N_CTX, n_batch=8)
        sc = g.SeqContext(m, N_CTX, len(jobs))
        try:
            caps = []
            gen = run_slots(env, m, sc, jobs, caps)
            want = [env["gold"][n + ".drawn"].tolist() for n in SLOTS] if mode == 2 else [by_hand(m, j) for j in jobs]
            assert len(caps) >= 6 and len(set(caps[1:])) == 1, caps       # no standing buffer moved: one captured step serves every later call
        finally:
            sc.free()
            m.free()
    for s, name in enumerate(SLOTS):
        assert gen[s] == want[s], name


# ---------------------------------------------------------------------------------------------- 7. the captured step survives the swaps
def test_capture_count_is_constant_from_the_second_swap(env):
    ids, n_sys, n_predict, n_batch, keep, params = case(env, "p_keep0")
    m = g.FalconModel.from_ggcc(env["path"], n_ctx=N_CTX, n_batch=n_batch)
    try:
        caps, swap = [], m.context_swap

        def counted(*a):
            swap(*a)
            caps.append(g.graph_captures(m))
        m.context_swap = counted
        out, swaps = g.generate_swap(m, ids, n_predict, params, n_keep=keep, n_batch=n_batch, use_graph=True)
        caps.append(g.graph_captures(m))
        assert len(swaps) == 4 and len(caps) == 5 and caps[0] >= 1 and len(set(caps[1:])) == 1, caps
    finally:
        m.free()


# ---------------------------------------------------------------------------------------------- 8. off: the refusal stays
def test_off_decode_past_n_ctx_is_still_refused(env):
    ids, _, _, n_batch, _, params = case(env, "p_keep0")
    m = g.FalconModel.from_ggcc(env["path"], n_ctx=N_CTX, n_batch=n_batch)
    sc = g.SeqContext(m, N_CTX, 2)
    try:
        sc.set_sampling(0, params, ids)
        sc.set_sampling(1, params, ids)
        with pytest.raises(RuntimeError, match=r"\(1\)"):
            sc.decode_sample([3, 4], [20, 0], 13)
        assert sc.decode_sample([3, 4], [20, 0], 12).shape == (12, 2)
        sc.set_context_stop(True)
        sc.set_context_stop(False)                          # on and off again: the refusal is back
        with pytest.raises(RuntimeError, match=r"\(1\)"):
            sc.decode_sample([3, 4], [20, 0], 13)
        assert sc.stop_state()[1].tolist() == [RUNNING, RUNNING]
    finally:
        sc.free()
        m.free()


# ---------------------------------------------------------------------------------------------- 9. the examples
def _example(name):
    import importlib.util
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "examples"))
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_examples_generate_past_the_context(env, monkeypatch, capfdbinary):
    """falcon_generate.py --context-swap prints the reference's bytes for its -n 80 run; falcon_batch_generate.py --context-swap gives two prompts
    through two slots, swapped in place, the reference's tokens; without the flag both refuse what they refused"""
    gen, bat = _example("falcon_generate"), _example("falcon_batch_generate")
    gold = env["gold"]
    params = g.sampling(temp=0.0, seed=1, logit_bias={env["eos"]: float("-inf")})
    with order(env["L"], 2):
        ids, out, raw = gen.generate(env["path"], cr.CLI_PROMPT, 80, n_ctx=N_CTX, sampling=params, ignore_eos=True, context_swap=True, n_batch=8)
        assert cr.CLI_PROMPT.encode() + raw == bytes(gold["p_keep0.stdout"]) and out.tolist() == gold["p_keep0.drawn"].tolist()
        res = bat.generate_batch(env["path"], [cr.CLI_PROMPT, cr.P25], 40, n_seq=2, n_ctx=N_CTX, sampling=params, ignore_eos=True, context_swap=True, n_batch=8)
        assert res[0][1].tolist() == gold["p_keep0.drawn"].tolist()[:40] and res[1][1].tolist() == gold["p25_keep0.drawn"].tolist()
        import sys
        monkeypatch.setattr(sys, "argv", ["falcon_generate.py", "--model", env["path"], "--context-swap", "-c", "32", "-b", "8", "-n", "80", "--temp", "0",
                                          "--ignore-eos", "-s", "1", "-p", cr.CLI_PROMPT])
        capfdbinary.readouterr()
        gen.main()                                           # the command line prints the reference's bytes (and a newline)
        assert capfdbinary.readouterr().out == bytes(gold["p_keep0.stdout"]) + b"\n"
    with pytest.raises(ValueError, match="exceed n_ctx"):
        gen.generate(env["path"], cr.CLI_PROMPT, 80, n_ctx=N_CTX, sampling=params, ignore_eos=True)
    with pytest.raises(ValueError, match="exceed n_ctx"):
        bat.generate_batch(env["path"], [cr.CLI_PROMPT], 80, n_seq=2, n_ctx=N_CTX, sampling=params, ignore_eos=True)

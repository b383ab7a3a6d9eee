"""GPU: the device sampler (csrc/kernels_sample.hip) against the reference's own sampling functions
(oracle/_ref/libfalcon_ref.so, tests/sample_ref.py) -- same tokens, same generator stream over consecutive draws -- and the
sampled decode loops (falcon_hip_decode_sample[_seqs]) against a host loop of evals, get_logits and the reference functions."""
import ctypes as C
import os

import numpy as np
import pytest

import ggllm_cpp_amd as g
import sample_ref
import synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    L = g.load()
    L.ggml_hip_init(0)
    return L


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    if not os.path.exists(sample_ref.REF_SO):
        pytest.skip("oracle/_ref/libfalcon_ref.so is not built (make -C oracle ref_falcon)")
    r = sample_ref.RefSampler(sample_ref.tiny_ggcc(str(tmp_path_factory.mktemp("ggcc") / "tiny.ggcc")))
    yield r
    r.free()


def device_draws(L, rows_per_row, params, windows, n_draws, n_ctx=64):
    """one sampler row per parameter set; draw d of row r samples rows_per_row[r][d % len]"""
    R, V = len(params), rows_per_row[0][0].size
    s = L.ggml_hip_sampler_create(R, V, n_ctx)
    assert s
    lg = L.ggml_hip_malloc(R * V * 4)
    tk = L.ggml_hip_malloc(R * 4 + 64)
    try:
        for r, (p, w) in enumerate(zip(params, windows)):
            h = np.ascontiguousarray(w, np.int32)
            assert L.ggml_hip_sampler_set_row(s, r, C.byref(p), h.ctypes.data if h.size else None, h.size) == 0
        out = np.zeros((n_draws, R), np.int32)
        for d in range(n_draws):
            x = np.ascontiguousarray(np.stack([rows_per_row[r][d % len(rows_per_row[r])] for r in range(R)]), np.float32)
            L.ggml_hip_memcpy_h2d(lg, x.ctypes.data, x.nbytes)
            L.ggml_hip_sampler_sample(s, lg, V, tk)
            L.ggml_hip_memcpy_d2h(out[d].ctypes.data, tk, R * 4)
            L.ggml_hip_synchronize()
        return out
    finally:
        L.ggml_hip_free(lg)
        L.ggml_hip_free(tk)
        L.ggml_hip_sampler_free(s)


CASES = [  # (top_k, top_p, temp, penalties, spread)
    (40, 0.95, 0.8, True, 3.0), (40, 1.0, 1.5, False, 3.0), (1024, 0.95, 0.8, True, 2.0), (1, 1.0, 0.8, False, 3.0),
    (5000, 0.95, 0.3, True, 3.0), (5000, 1.0, 1.5, False, 1.0), (0, 0.95, 0.8, True, 2.0), (0, 0.1, 1.5, False, 3.0),
    (0, 1.0, 0.8, False, 40.0), (40, 0.95, 0.0, True, 3.0), (0, 1.0, 0.0, False, 3.0), (40, 0.95, 0.8, False, 60.0),
]


@pytest.mark.parametrize("n_vocab", [65024, 333])
def test_kernel_matches_reference(L, ref, n_vocab):
    """ggml_hip_sampler_sample over 24 consecutive draws per row: both top-k forms (k <= 1024 in LDS, larger k and the whole
    vocabulary through the HBM sort), greedy, top_k 1 (no draw), wide rows whose softmax terms go denormal, penalties and a
    -inf bias -- the tokens and the generator stream of the reference's functions"""
    rng = np.random.default_rng(n_vocab + 1)
    n_draws = 24
    params, windows, rows = [], [], []
    for i, (top_k, top_p, temp, pen, spread) in enumerate(CASES):
        w = [int(t) for t in rng.integers(0, n_vocab, 64)] if pen else []
        params.append(g.sampling(temp=temp, top_k=top_k, top_p=top_p, repeat_penalty=1.1 if pen else 1.0, repeat_last_n=len(w),
                                 frequency_penalty=0.25 if pen else 0.0, presence_penalty=0.5 if pen else 0.0, seed=1000 + 17 * i,
                                 logit_bias={3: float("-inf"), 5: 2.5} if pen else None))
        windows.append(w)
        rows.append([sample_ref.tie_free_row(rng, n_vocab, spread) for _ in range(3)])
    got = device_draws(L, rows, params, windows, n_draws)
    for r, p in enumerate(params):
        want = sample_ref.run_ref(ref, rows[r], p, windows[r], n_draws)
        assert list(got[:, r]) == want, CASES[r]


def test_kernel_tie_rule_matches_host_restatement(L, tmp_path):
    """rows full of ties (small integers): value descending, id ascending, as the host restatement of fq_sample.h"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path / "libsample_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I",
                           os.path.join(root, "ggllm.cpp_amd", "csrc"), "-o", so, os.path.join(root, "tests", "host", "sample_harness.cpp")])
    H = C.CDLL(so)
    H.sample_mt_seed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    H.sample_chain.restype = C.c_int
    H.sample_chain.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                               C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(5)
    V, n_draws = 4000, 12
    cases = [(40, 0.95, 0.8), (2000, 0.95, 1.0), (0, 1.0, 0.8), (0, 0.95, 0.0)]
    params = [g.sampling(temp=t, top_k=k, top_p=tp, repeat_penalty=1.0, repeat_last_n=0, seed=7 + i) for i, (k, tp, t) in enumerate(cases)]
    rows = [[rng.integers(-3, 4, V).astype(np.float32) for _ in range(2)] for _ in cases]
    got = device_draws(L, rows, params, [[] for _ in cases], n_draws)
    for r, p in enumerate(params):
        mt, mti = (C.c_uint32 * 624)(), C.c_int()
        H.sample_mt_seed(mt, C.byref(mti), p.seed)
        want = []
        for d in range(n_draws):
            x = np.ascontiguousarray(rows[r][d % 2])
            want.append(H.sample_chain(x.ctypes.data, V, p.temp, p.top_k, p.top_p, 1.0, 0.0, 0.0, None, 0, 0, None, None, mt, C.byref(mti)))
        assert list(got[:, r]) == want, cases[r]


def test_refusals(L):
    s = L.ggml_hip_sampler_create(2, 100, 32)
    try:
        ok = g.sampling()
        assert L.ggml_hip_sampler_set_row(s, 0, C.byref(ok), None, 0) == 0
        for bad in (g.sampling(tfs_z=0.9), g.sampling(typical_p=0.5), g.sampling(mirostat=1), g.sampling(mirostat=2),
                    g.sampling(logit_bias={i: 1.0 for i in range(17)}), g.sampling(logit_bias={100: 1.0}), g.sampling(logit_bias={-1: 1.0})):
            assert L.ggml_hip_sampler_set_row(s, 0, C.byref(bad), None, 0) == 1
        h = np.array([5, 100], np.int32)
        assert L.ggml_hip_sampler_set_row(s, 0, C.byref(ok), h.ctypes.data, 2) == 1          # history id outside the vocabulary
        assert L.ggml_hip_sampler_set_row(s, 2, C.byref(ok), None, 0) == 1                  # row out of range
    finally:
        L.ggml_hip_sampler_free(s)


# ---------------------------------------------------------------------------------------------- the model-level loops
HP = dict(n_vocab=512, n_embd=256, n_head=4, n_head_kv=1, n_layer=2, n_ff=1024, two_norms=False)


@pytest.fixture(scope="module")
def weights():
    return synth.make_model(ob.Oracle(), HP, ob.Q4_0, seed=77)


P_LOOP = dict(temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64)


@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("use_graph", [False, True])
def test_decode_sample_matches_host_loop(L, ref, weights, order, use_graph):
    """prompt, falcon_hip_sample, then decode_sample (8 steps at once and as 2 x 4) against eval_token + get_logits + the
    reference functions with falcon_main's window"""
    prompt = [11, 200, 37, 4, 99]
    p = g.sampling(seed=1234, **P_LOOP)
    L.ggml_hip_reference_order(order)
    try:
        m = g.FalconModel(weights, n_ctx=64, n_batch=8)
        try:
            # host loop
            lg = m.eval(prompt, 0, logits_all=False)[-1]
            ref.seed(p.seed)
            hist = list(prompt)
            want = []
            for step in range(9):
                t = ref.draw(lg, p, g.sampling_window(hist, 64, p.repeat_last_n))
                want.append(t)
                hist.append(t)
                if step < 8:
                    m.eval_token(t, len(prompt) + step)
                    lg = m.logits()
            # device: 8 steps at once
            m.eval(prompt, 0, logits_all=False)
            m.set_sampling(p, prompt)
            first = m.sample()
            got = [first] + list(m.decode_sample(first, len(prompt), 8, use_graph=use_graph))
            assert got == want
            # 2 x 4
            m.eval(prompt, 0, logits_all=False)
            m.set_sampling(p, prompt)
            first = m.sample()
            a = list(m.decode_sample(first, len(prompt), 4, use_graph=use_graph))
            b = list(m.decode_sample(a[-1], len(prompt) + 4, 4, use_graph=use_graph))
            assert [first] + a + b == want
        finally:
            m.free()
    finally:
        L.ggml_hip_reference_order(0)


@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("use_graph", [False, True])
def test_decode_sample_seqs_matches_host_loop(L, ref, weights, order, use_graph):
    """3 sequences at their own positions (ragged) with their own parameters and seeds against eval_seqs + the reference
    functions: 6 steps at once and as 2 x 3"""
    L.ggml_hip_reference_order(order)
    model = g.FalconModel(weights, n_ctx=64, n_batch=8)
    n_seq, steps = 3, 6
    ps = [g.sampling(seed=50 + t, **P_LOOP) for t in range(n_seq)]
    ps[2] = g.sampling(temp=0.0, repeat_penalty=1.1, seed=9)
    first, pos = [7, 300, 42], [0, 5, 11]
    try:
        sc = g.SeqContext(model, 64, n_seq)
        try:
            tok, want, logits = list(first), [], []
            for s in range(steps):
                logits.append(sc.eval(tok, [pp + s for pp in pos]))
                # one reference context holds one generator: each sequence's draws are replayed from its seed
                nxt = []
                for t in range(n_seq):
                    ref.seed(ps[t].seed)
                    hh = [first[t]]
                    for s2 in range(s + 1):
                        x = ref.draw(logits[s2][t], ps[t], g.sampling_window(hh, 64, ps[t].repeat_last_n))
                        hh.append(x)
                    nxt.append(x)
                want.append(nxt)
                tok = nxt
            sc2 = g.SeqContext(model, 64, n_seq)
            try:
                for t in range(n_seq):
                    sc2.set_sampling(t, ps[t], [first[t]])
                got = sc2.decode_sample(first, pos, steps, use_graph=use_graph)
                assert got.tolist() == want
                for t in range(n_seq):
                    sc2.set_sampling(t, ps[t], [first[t]])
                a = sc2.decode_sample(first, pos, 3, use_graph=use_graph)
                b = sc2.decode_sample(a[-1], [pp + 3 for pp in pos], 3, use_graph=use_graph)
                assert a.tolist() + b.tolist() == want
            finally:
                sc2.free()
        finally:
            sc.free()
    finally:
        model.free()
        L.ggml_hip_reference_order(0)


def test_set_sampling_refuses_unsupported(L, weights):
    m = g.FalconModel(weights, n_ctx=32, n_batch=4)
    try:
        for bad in (g.sampling(tfs_z=0.95), g.sampling(typical_p=0.9), g.sampling(mirostat=2), g.sampling(logit_bias={512: 1.0})):
            with pytest.raises(ValueError):
                m.set_sampling(bad, [1, 2])
    finally:
        m.free()


# ---------------------------------------------------------------------------------------------- the examples, end to end
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def bpe_model(tmp_path_factory):
    """a tiny model with a real BPE vocabulary (tests/bpe_fixture.py): the one tests/test_gpu_dropin.py runs falcon_main on"""
    import bpe_fixture
    import ggcc_writer
    vocab, merges = bpe_fixture.build(n_merges=308)
    hp = dict(synth.HP_TINY_MQA)
    hp["n_vocab"] = len(vocab)
    w = synth.make_model(ob.Oracle(), hp, ob.Q4_0, seed=321)
    path = str(tmp_path_factory.mktemp("bpe") / "tiny_bpe.ggcc")
    ggcc_writer.write_ggcc(path, w, vocab, merges)
    return path


@pytest.mark.parametrize("temp", ["0.8", "0"])
def test_falcon_main_prints_what_falcon_generate_samples(L, bpe_model, temp):
    """the reference's own falcon_main (oracle/_ref/falcon_main_hip: its argument parser, tokenizer, context seeding, window and
    sampler chain on the host; falcon_eval on the device in reference order 2, whose logits are the reference's) prints the
    same bytes as examples/falcon_generate.py with the same flags and seed -- and evaluates the prompt tokens the example does"""
    import re
    import subprocess
    exe = os.path.join(ROOT, "oracle", "_ref", "falcon_main_hip")
    if not os.path.exists(exe):
        pytest.skip("falcon_main_hip was not built (make -C oracle ref_falcon_hip)")
    prompt, n = "The quick brown fox didn't jump", 12
    flags = ["-s", "7", "--temp", temp, "--top-k", "40", "--top-p", "0.95", "--repeat-penalty", "1.1", "--ignore-eos"]
    r = subprocess.run([exe, "-m", bpe_model, "-p", prompt, "-n", str(n), "-t", "2", "-c", "64", "-b", "8", "--verbose-prompt"] + flags,
                       capture_output=True, env=dict(os.environ, GGML_HIP_REFERENCE_ORDER="2"), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    err = r.stderr.decode("utf-8", errors="replace")
    m = re.search(r"number of tokens in prompt = (\d+)\n", err)
    assert m, err[-3000:]
    cli_ids = [int(x) for x in re.findall(r"^ *(\d+) -> '", err[m.end():], re.M)[:int(m.group(1))]]
    gen = _example("falcon_generate")
    a = gen.argparse.ArgumentParser()
    gen.add_sampling_args(a)
    p = gen.sampling_from_args(a.parse_args(flags))
    L.ggml_hip_reference_order(2)
    try:
        ids, out, text = gen.generate(bpe_model, prompt, n, n_ctx=64, sampling=p)
    finally:
        L.ggml_hip_reference_order(0)
    assert ids.tolist() == cli_ids
    assert len(out) == n
    assert r.stdout == prompt.encode() + text


def test_batch_generate_samples_what_falcon_generate_samples(L, bpe_model):
    """examples/falcon_batch_generate.py with the sampler: 7 prompts of different lengths, each with its own seed, through 3 slots
    refilled as prompts finish -- every prompt's continuation is falcon_generate.py's for that prompt and seed"""
    gen, bat = _example("falcon_generate"), _example("falcon_batch_generate")
    prompts = ["The quick brown fox didn't jump", "A", "Once upon a time, in a land far away, there lived",
               "hello world", "What is 2 + 2?", "The rain in Spain stays mainly in the plain, they say", "x y z"]
    seeds = [3 + 11 * i for i in range(len(prompts))]
    got = bat.generate_batch(bpe_model, prompts, 9, n_seq=3, n_ctx=64, chunk=4, sampling=g.sampling(seed=0), seeds=seeds)
    assert len(got) == len(prompts)
    for p, s, (ids, out, text) in zip(prompts, seeds, got):
        want = gen.generate(bpe_model, p, 9, n_ctx=64, sampling=g.sampling(seed=s))
        assert np.array_equal(ids, want[0]) and out.tolist() == want[1].tolist() and text == want[2], p


def test_copy_sampling_refuses_bad_rows(L, weights):
    m = g.FalconModel(weights, n_ctx=32, n_batch=4)
    try:
        sc = g.SeqContext(m, 32, 2)
        try:
            m.set_sampling(g.sampling(seed=1), [1, 2])
            assert g.copy_sampling(sc, 1, m, 0) == 0
            assert g.copy_sampling(sc, 2, m, 0) == 1
            assert g.copy_sampling(m, 0, sc, -1) == 1
        finally:
            sc.free()
    finally:
        m.free()

"""GPU: tail-free, typical and mirostat 1 / 2 in the device sampler (csrc/kernels_sample.hip's EXT instantiation, entered through
ggml_hip_sampler_set_row_ext) against the host restatement of the same header (tests/host/sample_chain_harness.cpp, which
tests/test_sample_chain_cpu.py pins to the reference's functions), and the sampled decode loops with those branches against a
host loop of evals, logits and the reference's own functions."""
import ctypes as C
import os

import numpy as np
import pytest

import ggllm_cpp_amd as g
import sample_chain_ref as scr
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
def H(tmp_path_factory):
    return scr.build_harness(tmp_path_factory.mktemp("sample_chain"))


class DeviceRows:
    """a sampler of len(params) rows set through set_row_ext; draw() samples one logits row per sampler row"""

    def __init__(self, L, n_vocab, params, windows, n_ctx=64):
        self.L, self.R, self.V = L, len(params), n_vocab
        self.s = L.ggml_hip_sampler_create(self.R, n_vocab, n_ctx)
        assert self.s
        self.lg = L.ggml_hip_malloc(self.R * n_vocab * 4)
        self.tk = L.ggml_hip_malloc(self.R * 4 + 64)
        for r, (p, w) in enumerate(zip(params, windows)):
            assert self.set(r, p, w) == 0

    def set(self, r, p, w=()):
        h = np.ascontiguousarray(w, np.int32)
        return self.L.ggml_hip_sampler_set_row_ext(self.s, r, C.byref(p), h.ctypes.data if h.size else None, h.size)

    def draw(self, rows):
        L = self.L
        x = np.ascontiguousarray(np.stack(rows), np.float32)
        out = np.zeros(self.R, np.int32)
        L.ggml_hip_memcpy_h2d(self.lg, x.ctypes.data, x.nbytes)
        L.ggml_hip_sampler_sample(self.s, self.lg, self.V, self.tk)
        L.ggml_hip_memcpy_d2h(out.ctypes.data, self.tk, self.R * 4)
        L.ggml_hip_synchronize()
        return out

    def mu(self):
        mu = np.zeros(self.R, np.float32)
        assert self.L.ggml_hip_sampler_get_mu(self.s, mu.ctypes.data) == 0
        return mu

    def free(self):
        self.L.ggml_hip_free(self.lg)
        self.L.ggml_hip_free(self.tk)
        self.L.ggml_hip_sampler_free(self.s)


def _bits(x):
    return np.float32(x).view(np.uint32).item()


def _four(n_vocab, rng):
    """default, tail-free with typical, mirostat 1, mirostat 2 -- different parameters, windows and seeds in one launch"""
    w = [int(t) for t in rng.integers(0, n_vocab, 64)]
    params = [g.sampling_ext(temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64, seed=21),
              g.sampling_ext(tfs_z=0.95, typical_p=0.9, temp=0.9, top_k=200, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64, frequency_penalty=0.2, seed=22,
                             logit_bias={5: 2.5}),
              g.sampling_ext(mirostat=1, mirostat_tau=5.0, mirostat_eta=0.1, temp=0.8, repeat_penalty=1.0, repeat_last_n=0, seed=23),
              g.sampling_ext(mirostat=2, mirostat_tau=3.0, mirostat_eta=0.5, temp=1.5, repeat_penalty=1.1, repeat_last_n=64, presence_penalty=0.5, seed=24)]
    windows = [w, w[::-1], [], w]
    return params, windows


@pytest.mark.parametrize("n_vocab", [300, 4000])
def test_kernel_matches_host_restatement(L, H, n_vocab):
    """12 draws of 4 rows in one launch -- the default chain beside tail-free + typical (the LDS form, typical's second sort),
    mirostat 1 and mirostat 2 (the HBM sort): the host restatement's tokens, and its mu bit for bit after the last draw"""
    rng = np.random.default_rng(n_vocab + 3)
    params, windows = _four(n_vocab, rng)
    rows = [[sample_ref.tie_free_row(rng, n_vocab, s) for _ in range(3)] for s in (3.0, 2.0, 3.0, 4.0)]
    dev = DeviceRows(L, n_vocab, params, windows)
    try:
        got = np.stack([dev.draw([rows[r][d % 3] for r in range(4)]) for d in range(12)])
        mu = dev.mu()
    finally:
        dev.free()
    for r, p in enumerate(params):
        h = scr.HostChain(H, p, n_vocab)
        want, mus = h.run(rows[r], windows[r], 12)
        assert h.ambiguous.value == 0, r
        assert list(got[:, r]) == want, r
        assert _bits(mu[r]) == mus[-1], r


def test_kernel_mirostat2_whole_vocabulary(L, H):
    """n_vocab 65024 (Falcon's): 4 draws of mirostat 2 over the HBM sort of the whole row"""
    n_vocab = 65024
    rng = np.random.default_rng(11)
    p = g.sampling_ext(mirostat=2, mirostat_tau=5.0, mirostat_eta=0.1, temp=0.8, repeat_penalty=1.1, repeat_last_n=64, seed=31)
    w = [int(t) for t in rng.integers(0, n_vocab, 64)]
    rows = [sample_ref.tie_free_row(rng, n_vocab, 3.0) for _ in range(2)]
    dev = DeviceRows(L, n_vocab, [p], [w])
    try:
        got = [int(dev.draw([rows[d % 2]])[0]) for d in range(4)]
        mu = dev.mu()
    finally:
        dev.free()
    h = scr.HostChain(H, p, n_vocab)
    want, mus = h.run(rows, w, 4)
    assert h.ambiguous.value == 0
    assert got == want and _bits(mu[0]) == mus[-1]


def test_refusals_change_nothing(L, H):
    """what set_row_ext refuses, and after each refusal the row's next draw and its mu are what they would have been"""
    n_vocab = 300
    rng = np.random.default_rng(2)
    ok = g.sampling_ext(mirostat=2, mirostat_tau=4.0, mirostat_eta=0.3, temp=0.8, repeat_penalty=1.0, repeat_last_n=0, seed=5)
    rows = [sample_ref.tie_free_row(rng, n_vocab, 3.0) for _ in range(3)]
    nan, inf = float("nan"), float("inf")
    bad = [g.sampling_ext(mirostat=3), g.sampling_ext(mirostat=-1), g.sampling_ext(tfs_z=0.9, top_k=0), g.sampling_ext(typical_p=0.9, top_k=1025),
           g.sampling_ext(typical_p=0.9, top_k=-5), g.sampling_ext(mirostat=1, mirostat_tau=nan), g.sampling_ext(mirostat=2, mirostat_eta=inf),
           g.sampling_ext(mirostat_tau=-inf), g.sampling_ext(tfs_z=0.9, logit_bias={n_vocab: 1.0}), g.sampling_ext(mirostat=1, logit_bias={i: 1.0 for i in range(17)})]
    h = scr.HostChain(H, ok, n_vocab)
    want, mus = h.run(rows, [], len(bad) + 1)
    dev = DeviceRows(L, n_vocab, [ok], [[]])
    try:
        assert _bits(dev.mu()[0]) == _bits(8.0)             # 2 tau
        for i, b in enumerate(bad):
            assert dev.set(0, b) == 1, i
            assert int(dev.draw([rows[i % 3]])[0]) == want[i] and _bits(dev.mu()[0]) == mus[i], i
        hist = np.array([5, n_vocab], np.int32)
        assert L.ggml_hip_sampler_set_row_ext(dev.s, 0, C.byref(ok), hist.ctypes.data, 2) == 1         # history id outside the vocabulary
        assert L.ggml_hip_sampler_set_row_ext(dev.s, 1, C.byref(ok), None, 0) == 1                     # row out of range
        assert int(dev.draw([rows[len(bad) % 3]])[0]) == want[len(bad)] and _bits(dev.mu()[0]) == mus[len(bad)]
        # accepted: the limit does not bind where mirostat or greedy ignores the stages; the old entry keeps refusing them
        for fine in (g.sampling_ext(tfs_z=0.9, typical_p=0.9, top_k=1024), g.sampling_ext(tfs_z=0.9, top_k=0, mirostat=2), g.sampling_ext(typical_p=0.5, top_k=0, temp=0.0)):
            assert dev.set(0, fine) == 0
        assert L.ggml_hip_sampler_set_row(dev.s, 0, C.byref(g.sampling(tfs_z=0.9)), None, 0) == 1
        assert L.ggml_hip_sampler_set_row(dev.s, 0, C.byref(g.sampling()), None, 0) == 0
        assert _bits(dev.mu()[0]) == 0                      # set_row: no mirostat, mu 0
    finally:
        dev.free()


def test_copy_row_continues_the_stream(L, H):
    """ggml_hip_sampler_copy_row carries the stages' parameters and mu: after 3 draws a copy in another sampler draws what the source draws"""
    n_vocab = 300
    rng = np.random.default_rng(4)
    ps = [g.sampling_ext(mirostat=1, mirostat_tau=4.0, mirostat_eta=0.5, temp=0.8, repeat_penalty=1.1, repeat_last_n=16, seed=8),
          g.sampling_ext(tfs_z=0.9, typical_p=0.8, temp=0.8, top_k=100, repeat_penalty=1.1, repeat_last_n=16, seed=9)]
    rows = [sample_ref.tie_free_row(rng, n_vocab, 3.0) for _ in range(3)]
    a = DeviceRows(L, n_vocab, ps, [[1, 2, 3], [4, 5]])
    b = DeviceRows(L, n_vocab, [g.sampling_ext(), g.sampling_ext()], [[], []])
    try:
        for d in range(3):
            a.draw([rows[d], rows[d]])
        assert L.ggml_hip_sampler_copy_row(b.s, 1, a.s, 0) == 0 and L.ggml_hip_sampler_copy_row(b.s, 0, a.s, 1) == 0
        assert _bits(b.mu()[1]) == _bits(a.mu()[0])
        for d in range(6):
            x, y = a.draw([rows[d % 3], rows[d % 3]]), b.draw([rows[d % 3], rows[d % 3]])
            assert (x[0], x[1]) == (y[1], y[0]), d
        assert _bits(b.mu()[1]) == _bits(a.mu()[0]) != _bits(8.0)
    finally:
        a.free()
        b.free()


# ---------------------------------------------------------------------------------------------- the model-level loops
HP = dict(synth.HP_TINY_MQA)


@pytest.fixture(scope="module")
def weights():
    return synth.make_model(ob.Oracle(), HP, ob.Q4_0, seed=78)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    if not os.path.exists(sample_ref.REF_SO):
        pytest.skip("oracle/_ref/libfalcon_ref.so is not built (make -C oracle ref_falcon)")
    r = scr.RefChain(scr.ggcc_with_vocab(str(tmp_path_factory.mktemp("ggcc") / "v512.ggcc"), HP["n_vocab"]))       # (mirostat 1's N)
    yield r
    r.free()


LOOP = {"typical": dict(typical_p=0.9, temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64),
        "mirostat2": dict(mirostat=2, mirostat_tau=3.0, mirostat_eta=0.5, temp=0.8, repeat_penalty=1.1, repeat_last_n=64)}


@pytest.mark.parametrize("mode", sorted(LOOP))
@pytest.mark.parametrize("use_graph", [False, True])
def test_decode_sample_matches_host_loop(L, ref, weights, mode, use_graph):
    """prompt, falcon_hip_sample, then decode_sample (8 steps at once and as 2 x 4) against eval_token + logits + the reference's
    functions with falcon_main's window and mu; the second half of 2 x 4 replays the first half's captured step"""
    prompt = [11, 200, 37, 4, 99]
    p = g.sampling_ext(seed=4321, **LOOP[mode])
    m = g.FalconModel(weights, n_ctx=64, n_batch=8)
    try:
        lg = m.eval(prompt, 0, logits_all=False)[-1]
        ref.start(p)
        hist, want = list(prompt), []
        for step in range(9):
            t = ref.draw_ext(lg, p, g.sampling_window(hist, 64, p.base.repeat_last_n))
            want.append(t)
            hist.append(t)
            if step < 8:
                m.eval_token(t, len(prompt) + step)
                lg = m.logits()
        want_mu = _bits(ref.mu.value)
        m.eval(prompt, 0, logits_all=False)
        m.set_sampling_ext(p, prompt)
        first = m.sample()
        got = [first] + list(m.decode_sample(first, len(prompt), 8, use_graph=use_graph))
        assert got == want
        if p.base.mirostat:
            assert _bits(m.mirostat_mu()) == want_mu
        m.eval(prompt, 0, logits_all=False)
        m.set_sampling_ext(p, prompt)
        first = m.sample()
        a = list(m.decode_sample(first, len(prompt), 4, use_graph=use_graph))
        caps = g.graph_captures(m)
        b = list(m.decode_sample(a[-1], len(prompt) + 4, 4, use_graph=use_graph))
        assert [first] + a + b == want
        assert g.graph_captures(m) == caps
    finally:
        m.free()


@pytest.mark.parametrize("use_graph", [False, True])
def test_decode_sample_seqs_matches_host_loop(L, ref, weights, use_graph):
    """3 ragged sequences in one lock-step loop -- default chain, tail-free, mirostat 1 -- against eval_seqs + the reference's functions"""
    model = g.FalconModel(weights, n_ctx=64, n_batch=8)
    n_seq, steps = 3, 6
    ps = [g.sampling_ext(seed=60, temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64),
          g.sampling_ext(seed=61, tfs_z=0.9, temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64),
          g.sampling_ext(seed=62, mirostat=1, mirostat_tau=4.0, mirostat_eta=0.3, temp=0.8, repeat_penalty=1.1, repeat_last_n=64)]
    first, pos = [7, 300, 42], [0, 5, 11]
    try:
        sc = g.SeqContext(model, 64, n_seq)
        try:
            tok, want, logits, mu = list(first), [], [], 0
            for s in range(steps):
                logits.append(sc.eval(tok, [pp + s for pp in pos]))
                nxt = []
                for t in range(n_seq):                      # one reference context holds one generator: each sequence is replayed from its seed
                    ref.start(ps[t])
                    hh = [first[t]]
                    for s2 in range(s + 1):
                        x = ref.draw_ext(logits[s2][t], ps[t], g.sampling_window(hh, 64, ps[t].base.repeat_last_n))
                        hh.append(x)
                    nxt.append(x)
                    mu = _bits(ref.mu.value)                # (the last sequence's: the mirostat one)
                want.append(nxt)
                tok = nxt
            sc2 = g.SeqContext(model, 64, n_seq)
            try:
                for t in range(n_seq):
                    sc2.set_sampling_ext(t, ps[t], [first[t]])
                got = sc2.decode_sample(first, pos, steps, use_graph=use_graph)
                assert got.tolist() == want
                assert _bits(sc2.mirostat_mu()[2]) == mu
            finally:
                sc2.free()
        finally:
            sc.free()
    finally:
        model.free()


def test_stops_freeze_mu_and_copy_sampling_carries_it(L, weights):
    """a mirostat row that ends by budget keeps the mu of its last draw however many steps the loop goes on, and
    falcon_hip_context_copy_sampling hands the stages and mu to a lock-step slot"""
    prompt = [3, 141, 59]
    p = g.sampling_ext(seed=77, mirostat=2, mirostat_tau=3.0, mirostat_eta=0.5, temp=0.8, repeat_penalty=1.1, repeat_last_n=64)
    m = g.FalconModel(weights, n_ctx=64, n_batch=8)
    try:
        m.eval(prompt, 0, logits_all=False)
        m.set_sampling_ext(p, prompt)
        assert _bits(m.mirostat_mu()) == _bits(6.0)
        first = m.sample()
        free_run = list(m.decode_sample(first, len(prompt), 3))
        mu3 = _bits(m.mirostat_mu())
        m.eval(prompt, 0, logits_all=False)
        m.set_sampling_ext(p, prompt)
        assert m.sample() == first
        m.set_stops(g.stops(max_tokens=3))
        out = list(m.decode_sample(first, len(prompt), 7))
        assert out[:3] == free_run and out[3:] == [-1] * 4
        assert m.stop_state() == (3, g.STOP_BUDGET)
        assert _bits(m.mirostat_mu()) == mu3 != _bits(6.0)
        sc = g.SeqContext(m, 64, 2)
        try:
            assert g.copy_sampling(sc, 1, m, 0) == 0
            assert _bits(sc.mirostat_mu()[1]) == mu3 and _bits(sc.mirostat_mu()[0]) == 0
        finally:
            sc.free()
    finally:
        m.free()


def test_set_sampling_ext_refuses(L, weights):
    m = g.FalconModel(weights, n_ctx=32, n_batch=4)
    try:
        for bad in (g.sampling_ext(mirostat=3), g.sampling_ext(tfs_z=0.95, top_k=0), g.sampling_ext(typical_p=0.9, top_k=2000),
                    g.sampling_ext(mirostat=2, mirostat_tau=float("nan")), g.sampling_ext(mirostat=1, logit_bias={512: 1.0})):
            with pytest.raises(ValueError):
                m.set_sampling_ext(bad, [1, 2])
        m.set_sampling_ext(g.sampling_ext(mirostat=1), [1, 2])
        assert _bits(m.mirostat_mu()) == _bits(10.0)
    finally:
        m.free()


# ---------------------------------------------------------------------------------------------- the examples, end to end
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bpe_model(tmp_path_factory):
    """a tiny model with a real BPE vocabulary (tests/bpe_fixture.py), as tests/test_gpu_sample.py's"""
    import bpe_fixture
    import ggcc_writer
    vocab, merges = bpe_fixture.build(n_merges=308)
    hp = dict(synth.HP_TINY_MQA)
    hp["n_vocab"] = len(vocab)
    w = synth.make_model(ob.Oracle(), hp, ob.Q4_0, seed=321)
    path = str(tmp_path_factory.mktemp("bpe") / "tiny_bpe.ggcc")
    ggcc_writer.write_ggcc(path, w, vocab, merges)
    return path


@pytest.mark.parametrize("extra", [["--mirostat", "2", "--mirostat-ent", "3", "--mirostat-lr", "0.5"], ["--mirostat", "1"], ["--typical", "0.9", "--tfs", "0.95"]],
                         ids=["mirostat2", "mirostat1", "typical"])
def test_falcon_main_prints_what_falcon_generate_samples(L, bpe_model, extra):
    """the reference's own falcon_main (oracle/_ref/falcon_main_hip: its parser, window, static mu and sampling branches on the host,
    falcon_eval on the device in reference order 2) prints the bytes examples/falcon_generate.py generates with the same flags"""
    import importlib.util
    import subprocess
    exe = os.path.join(ROOT, "oracle", "_ref", "falcon_main_hip")
    if not os.path.exists(exe):
        pytest.skip("falcon_main_hip was not built (make -C oracle ref_falcon_hip)")
    prompt, n = "The quick brown fox didn't jump", 12
    flags = ["-s", "7", "--temp", "0.8", "--top-k", "40", "--top-p", "0.95", "--repeat-penalty", "1.1", "--ignore-eos"] + extra
    r = subprocess.run([exe, "-m", bpe_model, "-p", prompt, "-n", str(n), "-t", "2", "-c", "64", "-b", "8"] + flags,
                       capture_output=True, env=dict(os.environ, GGML_HIP_REFERENCE_ORDER="2"), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    spec = importlib.util.spec_from_file_location("falcon_generate", os.path.join(ROOT, "examples", "falcon_generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    a = gen.argparse.ArgumentParser()
    gen.add_sampling_args(a)
    p = gen.sampling_from_args(a.parse_args(flags))
    assert isinstance(p, g.SamplingExt)
    L.ggml_hip_reference_order(2)
    try:
        ids, out, text = gen.generate(bpe_model, prompt, n, n_ctx=64, sampling=p)
    finally:
        L.ggml_hip_reference_order(0)
    assert len(out) == n
    assert r.stdout == prompt.encode() + text

"""GPU: F16 Falcon files through the model-level entries (csrc/kernels_f16.hip under csrc/falcon_model.hip and csrc/falcon_stage.hip): all-F16 files as falcon_convert.py
writes them (MQA; GQA with two norms) and a Q4_0 file whose lm_head stayed F16 (falcon_quantize --leave-output-tensor from an F16 source).

Against the reference: under ggml_hip_reference_order(1) and (2) the logits equal, bit for bit, those of the real libfalcon.cpp (scalar build) on the same
files -- tests/golden/f16_models.npz (scripts/gen_f16_golden.py), and a live run of oracle/_ref/libfalcon_ref.so where it is built. Under order 0 the
entries are checked against each other."""
import ctypes as C
import hashlib
import importlib.util
import os

import numpy as np
import pytest

import ggllm_cpp_amd as g
import ggcc_writer
import sample_ref
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, N_PROMPT, N_EXT, N_DECODE = 1357, 9, 3, 12
MODELS = {"mqa_f16": (synth.HP_TINY_MQA, None), "gqa_f16": (synth.HP_TINY_GQA, None), "mqa_q4_0_f16head": (synth.HP_TINY_MQA, 2)}


@pytest.fixture(scope="module")
def L():
    g.init(0)
    lib = g.load()
    yield lib
    lib.ggml_hip_reference_order(0)


@pytest.fixture(scope="module")
def files(L, tmp_path_factory):
    """name -> path of the GGCC file (the quantized one is made by falcon_hip_model_quantize, whose files are the reference's byte for byte)"""
    td = tmp_path_factory.mktemp("f16_models")
    out = {}
    for name, (hp, ftype) in MODELS.items():
        src = str(td / (name + "_src.ggcc"))
        ggcc_writer.write_ggcc(src, synth.make_model_float(hp, seed=SEED, f16=True))
        if ftype is None:
            out[name] = src
        else:
            out[name] = str(td / (name + ".ggcc"))
            g.quantize_model(src, out[name], ftype, quantize_output_tensor=False)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_device(path, tokens):
    """prompt with logits_all, extension at n_past > 0, 12 single-token steps"""
    m = g.FalconModel.from_ggcc(path, n_ctx=64, n_batch=16)
    try:
        pre = m.eval(tokens[:N_PROMPT], 0)
        ext = m.eval(tokens[N_PROMPT:N_PROMPT + N_EXT], N_PROMPT)
        p0 = N_PROMPT + N_EXT
        dec = np.concatenate([m.eval(tokens[i:i + 1], i) for i in range(p0, p0 + N_DECODE)])
        return pre, ext, dec
    finally:
        m.free()


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", list(MODELS))
def test_logits_equal_the_reference(L, golden, files, name, order):
    gg = golden["f16_models"]
    sha = np.frombuffer(hashlib.sha256(open(files[name], "rb").read()).digest(), np.uint8)
    assert np.array_equal(sha, gg[f"{name}_sha256"]), "not the file the reference evaluated"
    tokens = gg[f"{name}_tokens"]
    L.ggml_hip_reference_order(order)
    try:
        pre, ext, dec = run_device(files[name], tokens)
    finally:
        L.ggml_hip_reference_order(0)
    for what, got in (("prefill", pre), ("ext", ext), ("decode", dec)):
        want = gg[f"{name}_{what}_logits"]
        assert got.shape == want.shape
        assert np.array_equal(bits(got), bits(want)), f"{what}: {int((bits(got) != bits(want)).sum())} of {want.size} logits differ, max |d| {np.abs(got - want).max():.3e}"


@pytest.mark.skipif(not os.path.exists(sample_ref.REF_SO), reason="oracle/_ref/libfalcon_ref.so is not built")
def test_logits_equal_a_live_reference_run(L, files):
    R = C.CDLL(sample_ref.REF_SO)
    R.reff_load.restype = C.c_void_p; R.reff_load.argtypes = [C.c_char_p, C.c_int, C.c_int]
    R.reff_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    R.reff_free.argtypes = [C.c_void_p]
    name = "gqa_f16"
    hp = MODELS[name][0]
    tokens = synth.tokens(14, hp["n_vocab"], seed=4242)                       # (other tokens than the fixture's)
    ctx = R.reff_load(os.fsencode(files[name]), 64, 16)
    assert ctx
    try:
        want = []
        for lo, hi in ((0, 7), (7, 12), (12, 13), (13, 14)):
            lg = np.zeros((hi - lo, hp["n_vocab"]), np.float32)
            assert R.reff_eval(ctx, tokens[lo:hi].ctypes.data, hi - lo, lo, 2, lg.ctypes.data) == 0
            want.append(lg)
    finally:
        R.reff_free(ctx)
    L.ggml_hip_reference_order(2)
    try:
        m = g.FalconModel.from_ggcc(files[name], n_ctx=64, n_batch=16)
        try:
            got = [m.eval(tokens[lo:hi], lo) for lo, hi in ((0, 7), (7, 12), (12, 13), (13, 14))]
        finally:
            m.free()
    finally:
        L.ggml_hip_reference_order(0)
    for a, b in zip(got, want):
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name", list(MODELS))
def test_weight_bytes_count_two_per_f16_weight(L, files, name):
    hp, ftype = MODELS[name]
    E, FF, V, QKV = hp["n_embd"], hp["n_ff"], hp["n_vocab"], (hp["n_head"] + 2 * hp["n_head_kv"]) * 64
    per_block = E * QKV + E * E + 2 * E * FF
    m = g.FalconModel.from_ggcc(files[name], n_ctx=16, n_batch=4)
    try:
        if ftype is None:
            assert m.weight_bytes() == 2 * (hp["n_layer"] * per_block + V * E)
        else:
            assert m.weight_bytes() == hp["n_layer"] * per_block // 32 * 18 + 2 * V * E
    finally:
        m.free()


@pytest.mark.parametrize("name", list(MODELS))
def test_order0_graph_decode_equals_plain_launches_and_eval_token(L, files, name):
    hp = MODELS[name][0]
    tokens = synth.tokens(6, hp["n_vocab"], seed=31)
    m = g.FalconModel.from_ggcc(files[name], n_ctx=64, n_batch=8)
    try:
        first = int(m.eval(tokens, 0, logits_all=False)[-1].argmax())
        plain = m.decode_greedy(first, tokens.size, 10, use_graph=False)
        m.eval(tokens, 0, logits_all=False)
        graph = m.decode_greedy(first, tokens.size, 10, use_graph=True)
        assert plain.tolist() == graph.tolist()
        # the same tokens from eval_token + argmax on the host; its logits are those of falcon_hip_eval at the same position
        m.eval(tokens, 0, logits_all=False)
        tok, want, rows = first, [], []
        for s in range(10):
            m.eval_token(tok, tokens.size + s)
            rows.append(m.logits())
            tok = int(rows[-1].argmax())
            want.append(tok)
        assert plain.tolist() == want
        m.eval(tokens, 0, logits_all=False)
        tok = first
        for s in range(3):
            lg = m.eval([tok], tokens.size + s)[0]
            assert np.array_equal(bits(lg), bits(rows[s]))
            tok = want[s]
    finally:
        m.free()


@pytest.mark.parametrize("name", ["gqa_f16", "mqa_q4_0_f16head"])
@pytest.mark.parametrize("n_seq", [3, 6])
def test_order0_lockstep_row_equals_the_sequence_alone(L, files, name, n_seq):
    """ragged lock-step steps (falcon_hip_eval_seqs) of 3 (the few-column mat-mul forms) and 6 (the 8-column form) sequences, their slots filled by
    falcon_hip_context_copy_seq: every row's logits are those of the sequence evaluated alone.
    The F16 mat-mul has one order for every N, so for the all-F16 file that holds at any number of sequences. The QUANTIZED blocks of the Q4_0 file have it in the
    default order only while the column mat-vec kernels serve the pass (legacy formats: up to 4 sequences; from 5 on the small-batch mat-mul sums a row in K-split
    partial sums -- tests/test_gpu_ragged_seqs.py states the same rule for every quantized model): there, at 6 sequences, the row is compared with row 0 of a
    lock-step context of 6 CLONES of that sequence, i.e. with the sequence alone in the same launch form."""
    hp, ftype = MODELS[name]
    V = hp["n_vocab"]
    clones = ftype is not None and n_seq > 4
    model = g.FalconModel.from_ggcc(files[name], n_ctx=64, n_batch=8)
    try:
        prompts = [synth.tokens(2 + (3 * t) % 5, V, seed=60 + t) for t in range(n_seq)]
        steps = 3
        sc = g.SeqContext(model, 64, n_seq)
        try:
            # every prompt is evaluated in the model's own context, enters its slot by copy_seq, and goes on alone there
            alone, tok0 = [], []
            for t, p in enumerate(prompts):
                lg = model.eval(p, 0, logits_all=False)[-1]
                assert g.copy_seq(sc, t, model, 0, p.size) == 0
                nxt, rows = int(lg.argmax()), []
                tok0.append(nxt)
                if clones:
                    cl = g.SeqContext(model, 64, n_seq)
                    try:
                        for j in range(n_seq):
                            assert g.copy_seq(cl, j, model, 0, p.size) == 0
                        for s in range(steps):
                            rows.append(cl.eval([nxt] * n_seq, [int(p.size) + s] * n_seq)[0])
                            nxt = int(rows[-1].argmax())
                    finally:
                        cl.free()
                else:
                    for s in range(steps):
                        rows.append(model.eval([nxt], p.size + s)[0])
                        nxt = int(rows[-1].argmax())
                alone.append(rows)
            tok = list(tok0)
            pos = [int(p.size) for p in prompts]
            for s in range(steps):
                lg = sc.eval(tok, [pp + s for pp in pos])
                for t in range(n_seq):
                    assert np.array_equal(bits(lg[t]), bits(alone[t][s])), (s, t)
                tok = [int(lg[t].argmax()) for t in range(n_seq)]
            # the device loop over the same slots
            for use_graph in (False, True):
                got = sc.decode_greedy(tok0, pos, steps, use_graph=use_graph)
                want = [[int(alone[t][s].argmax()) for t in range(n_seq)] for s in range(steps)]
                assert got.tolist() == want
        finally:
            sc.free()
    finally:
        model.free()


@pytest.mark.skipif(not os.path.exists(sample_ref.REF_SO), reason="oracle/_ref/libfalcon_ref.so is not built")
@pytest.mark.parametrize("use_graph", [False, True])
def test_decode_sample_seqs_matches_host_loop(L, files, tmp_path, use_graph):
    """as tests/test_gpu_sample.py: 3 ragged sequences with their own parameters and seeds against eval_seqs + the reference's sampler functions"""
    ref = sample_ref.RefSampler(sample_ref.tiny_ggcc(str(tmp_path / "tiny.ggcc")))
    name = "mqa_f16"
    model = g.FalconModel.from_ggcc(files[name], n_ctx=64, n_batch=8)
    n_seq, steps = 3, 6
    P = dict(temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64)
    ps = [g.sampling(seed=50 + t, **P) for t in range(n_seq)]
    ps[2] = g.sampling(temp=0.0, repeat_penalty=1.1, seed=9)
    first, pos = [7, 300, 42], [0, 5, 11]
    try:
        sc = g.SeqContext(model, 64, n_seq)
        sc2 = g.SeqContext(model, 64, n_seq)
        try:
            tok, want, logits = list(first), [], []
            for s in range(steps):
                logits.append(sc.eval(tok, [pp + s for pp in pos]))
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
            for t in range(n_seq):
                sc2.set_sampling(t, ps[t], [first[t]])
            got = sc2.decode_sample(first, pos, steps, use_graph=use_graph)
            assert got.tolist() == want
        finally:
            sc.free()
            sc2.free()
    finally:
        model.free()
        ref.free()


def test_decode_sample_matches_sample_after_eval_token(L, files):
    """falcon_hip_decode_sample (plain and captured) draws what falcon_hip_sample draws from eval_token's rows"""
    name = "mqa_q4_0_f16head"
    prompt = [11, 200, 37, 4, 99]
    p = g.sampling(seed=1234, temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64)
    m = g.FalconModel.from_ggcc(files[name], n_ctx=64, n_batch=8)
    try:
        m.eval(prompt, 0, logits_all=False)
        m.set_sampling(p, prompt)
        want = [m.sample()]
        for s in range(6):
            m.eval_token(want[-1], len(prompt) + s)
            m.logits()
            want.append(m.sample())
        for use_graph in (False, True):
            m.eval(prompt, 0, logits_all=False)
            m.set_sampling(p, prompt)
            first = m.sample()
            assert [first] + m.decode_sample(first, len(prompt), 6, use_graph=use_graph).tolist() == want
    finally:
        m.free()


def test_perplexity_equals_the_reference_loop(L, golden, files):
    gg = golden["f16_models"]
    name = "mqa_f16"
    m = g.FalconModel.from_ggcc(files[name], n_ctx=64, n_batch=16)
    try:
        L.ggml_hip_reference_order(1)
        nll, count = m.perplexity(gg[f"{name}_ppl_tokens"], n_ctx=32, n_batch=8)
    finally:
        L.ggml_hip_reference_order(0)
        m.free()
    assert count == int(gg[f"{name}_ppl_count"]) == 45
    assert abs(nll - float(gg[f"{name}_ppl_nll"])) <= 1e-9 * abs(nll)


def test_falcon_generate_example_runs_on_an_f16_file(L, tmp_path):
    import bpe_fixture
    vocab, merges = bpe_fixture.build(n_merges=308)
    hp = dict(synth.HP_TINY_MQA)
    hp["n_vocab"] = len(vocab)
    path = str(tmp_path / "tiny_bpe_f16.ggcc")
    ggcc_writer.write_ggcc(path, synth.make_model_float(hp, seed=321, f16=True), vocab, merges)
    spec = importlib.util.spec_from_file_location("falcon_generate", os.path.join(ROOT, "examples", "falcon_generate.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    prompt = "The quick brown fox didn't jump"
    ids, out, text = ex.generate(path, prompt, 6, n_ctx=64)
    m = g.FalconModel.from_ggcc(path, n_ctx=64, n_batch=16)
    try:
        exp = [int(m.eval(ids, 0, logits_all=False)[-1].argmax())]
        for i in range(5):
            exp.append(int(m.eval(exp[-1:], ids.size + i)[-1].argmax()))
    finally:
        m.free()
    eos = g.load().falcon_hip_token_eos()
    if eos in exp:
        exp = exp[:exp.index(eos)]
    assert out.tolist() == exp
    v = g.Vocab(path)
    try:
        assert v.detokenize(out) == text
    finally:
        v.free()

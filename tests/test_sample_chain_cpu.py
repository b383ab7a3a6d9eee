"""CPU: the restatement of tail-free, typical and mirostat 1 / 2 the device compiles (ggllm.cpp_amd/csrc/fq_sample_chain.h) is
host-compiled with g++ (tests/host/sample_chain_harness.cpp) and checked bit for bit: its logf and log2f against the host
libm's on every non-negative float, its expf on the positive arguments typical opens, its powf on the slices and the random
pairs the chain can produce, and the whole chain -- tokens, generator stream and mirostat's mu after every draw -- against the
reference's own functions (oracle/_ref/libfalcon_ref.so, skipped when that build is absent)."""
import ctypes as C
import itertools
import math
import os
import struct

import numpy as np
import pytest

import ggllm_cpp_amd as g
import sample_chain_ref as scr
import sample_ref

THREADS = max(1, min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return scr.build_harness(tmp_path_factory.mktemp("sample_chain"))


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _float(b):
    return struct.unpack("<f", struct.pack("<I", b))[0]


SPECIAL_RANGES = [(0x7f800001, 0x7f800010), (0x7fbffff0, 0x7fc00010), (0x7ffffff0, 0x7fffffff),      # NaNs, signalling and quiet
                  (0x80000000, 0x80000010), (0x807ffff0, 0x80800010), (0xbf7ffff8, 0xbf800008),      # -0, negative subnormals and normals
                  (0xff7ffff0, 0xff800010), (0xffc00000, 0xffc00010), (0xfffffff0, 0xffffffff)]      # -max, -inf, negative NaNs


@pytest.mark.parametrize("fn", [0, 1], ids=["logf", "log2f"])
def test_log_equals_libm_on_every_non_negative_float(harness, fn):
    """+0, every subnormal, every normal, +inf (about 2.1 G inputs), and NaN / negative inputs (a NaN result is a NaN: its sign
    and payload are not compared)"""
    first = C.c_uint32()
    for lo, hi in [(0, 0x7f800000)] + SPECIAL_RANGES:
        bad = harness.chain_fn_mismatches(fn, lo, hi, THREADS, C.byref(first))
        assert bad == 0, f"{bad} inputs in [{lo:#x}, {hi:#x}] differ from libm, the first at {_float(first.value)!r} ({first.value:#x})"


def test_expf_equals_libm_on_the_positive_arguments_typical_opens(harness):
    """after typical data[0] is not the maximum, so the softmaxes behind it call expf(logit - data[0].logit) with positive
    arguments: every f32 in [+0, 104]"""
    first = C.c_uint32()
    bad = harness.chain_fn_mismatches(2, 0, _bits(104.0), THREADS, C.byref(first))
    assert bad == 0, f"{bad} inputs differ from libm expf, the first at {_float(first.value)!r}"


@pytest.mark.parametrize("x,lim", [(2.0, 64.0), (7.0, 4.0), (300.0, 4.0), (512.0, 4.0), (4000.0, 4.0), (65024.0, 4.0)])
def test_powf_equals_libm_on_the_chain_slices(harness, x, lim):
    """powf(2, mu) for every f32 mu in [-64, 64]; powf(N, y) for every f32 y in [-4, 4]"""
    first = C.c_uint32()
    for lo, hi in ((0, _bits(lim)), (0x80000000, _bits(-lim))):
        bad = harness.chain_powf_mismatches(x, lo, hi, THREADS, C.byref(first))
        assert bad == 0, f"{bad} exponents differ from libm powf({x}, y), the first at y = {_float(first.value)!r}"


def test_powf_equals_libm_on_random_pairs(harness):
    """2^30 pseudo-random (x > 0, y): x over [2^-48, 2^48) -- wider than epsilon_hat 2^mu / (1 - N^-epsilon_hat) gets for the
    mu a generation reaches -- y of either sign over [2^-12, 2^7)"""
    first = C.c_uint64()
    bad = harness.chain_powf_random_mismatches(20240611, 1 << 30, THREADS, C.byref(first))
    x, y = C.c_float(), C.c_float()
    harness.chain_powf_pair(20240611, first.value if bad else 0, C.byref(x), C.byref(y))
    assert bad == 0, f"{bad} pairs differ from libm powf, the first ({x.value!r}, {y.value!r})"


def test_powf_special_cases(harness):
    """what the chain can reach when s_hat degenerates: x NaN, negative, 0 or inf, y NaN, 0 or inf, overflow and underflow"""
    nan, inf = float("nan"), float("inf")
    xs = [nan, -nan, -inf, -3.5, -2.0, -1.0, -0.5, -1e-40, -0.0, 0.0, 1e-45, 1e-40, 0.5, 1.0, 1.5, 2.0, 7.0, 65024.0, 3e38, inf, _float(0x7f800001)]
    ys = [nan, -inf, -1e30, -150.0, -149.5, -127.0, -3.0, -2.0, -1.0, -0.5, -1e-45, -0.0, 0.0, 1e-45, 0.5, 1.0, 2.0, 3.0, 127.0, 128.0, 1e30, inf, _float(0x7fa00000)]
    for x, y in itertools.product(xs, ys):
        assert harness.chain_powf_same(x, y), (x, y)
    for x, want in ((nan, -2 ** 31), (inf, -2 ** 31), (-inf, -2 ** 31), (2147483648.0, -2 ** 31), (-2147483648.0, -2 ** 31), (2147483520.0, 2147483520),
                    (3.99, 3), (-3.99, -3), (0.0, 0)):
        assert harness.chain_f2i(x) == want, x


# ------------------------------------------------------------------------------------------------ the chain
VOCABS = [7, 300, 4000, 65024]


@pytest.fixture(scope="module", params=VOCABS)
def ref(request, tmp_path_factory):
    """one reference context per row length (ref.rows_vocab): mirostat 1 reads N from the context (ref.n_vocab), so its n_vocab
    is the row length -- but for 7, which the reference's loader does not survive (it looks its special tokens up by id):
    those rows are sampled with the 300-token context's N, and the restatement is handed the same N"""
    if not os.path.exists(sample_ref.REF_SO):
        pytest.skip("oracle/_ref/libfalcon_ref.so is not built (make -C oracle ref_falcon)")
    n = max(request.param, 300)
    r = scr.RefChain(scr.ggcc_with_vocab(str(tmp_path_factory.mktemp("ggcc") / ("v%d.ggcc" % n)), n))
    r.rows_vocab = request.param
    yield r
    r.free()


def _rows(rng, n_vocab):
    """spreads at which the kept candidates' probabilities stay normal numbers (the contract); 2 rows at 65024. From 4000 tokens
    on no flat rows: typical at top_k 1000 then keeps several hundred candidates whose f32 scores, folded around the entropy,
    collide on most rows -- outside the contract"""
    spreads = [2.0, 6.0] if n_vocab > 10000 else [2.0, 6.0, 3.0, 4.0, 5.0, 2.5] if n_vocab > 1000 else [1.0, 3.0, 6.0, 0.5, 2.0, 4.0]
    return [sample_ref.tie_free_row(rng, n_vocab, spread=s) for s in spreads]


def _check(harness, ref, rows, p, window, n_draws, what):
    want, want_mu = scr.run_ref(ref, rows, p, window, n_draws)
    h = scr.HostChain(harness, p, ref.n_vocab)
    got, got_mu = h.run(rows, window, n_draws)
    assert h.ambiguous.value == 0, ("the rows leave the contract (a tie or a non-normal probability)", what)
    assert got == want, what
    if p.base.mirostat:
        assert got_mu == want_mu, what


# rows drawn from these seeds stay inside the contract at every point of the grids below (asserted for every case, never
# skipped): typical's f32 scores of several hundred kept candidates collide on an occasional row, which another seed avoids
ROW_SEED = {7: 107, 300: 400, 4000: 4101, 65024: 65125}
MIROSTAT_SEED = {7: 207, 300: 500, 4000: 4200, 65024: 65226}      # (dividing by temp can tie two of several thousand kept logits)
STAGES = [(0.5, 1.0), (0.9, 1.0), (0.95, 1.0), (1.0, 0.5), (1.0, 0.9), (1.0, 0.95), (0.95, 0.9), (0.5, 0.5), (0.9, 0.95)]      # (tfs_z, typical_p)


def test_tail_free_and_typical_match_reference(harness, ref):
    """tail-free and typical, each alone and together, over top_k 1 / 2 / 3 (tail-free's early return and its smallest live
    case) / 40 / 1000, with and without top-p and penalties: the same tokens from one generator over consecutive draws.
    With typical on, the survivors reach top-p and the final softmax in score order (data[0] is not the maximum)."""
    n_vocab = ref.rows_vocab
    rng = np.random.default_rng(ROW_SEED[n_vocab])
    rows = _rows(rng, n_vocab)
    n_draws = 6 if n_vocab > 10000 else 24
    for (tfs_z, typ), top_k, top_p, (temp, pen) in itertools.product(STAGES, [1, 2, 3, 40, 1000], [1.0, 0.95], [(0.8, False), (1.5, True)]):
        window = [int(t) for t in rng.integers(0, n_vocab, 64)] if pen else []
        p = g.sampling_ext(tfs_z=tfs_z, typical_p=typ, temp=temp, top_k=top_k, top_p=top_p, repeat_penalty=1.1 if pen else 1.0, repeat_last_n=len(window),
                           frequency_penalty=0.3 if pen else 0.0, presence_penalty=0.2 if pen else 0.0, seed=int(rng.integers(0, 2 ** 31)),
                           logit_bias={n_vocab - 1: 1.5} if pen else None)
        _check(harness, ref, rows, p, window, n_draws, (n_vocab, tfs_z, typ, top_k, top_p, temp, pen))


def test_typical_reorders_the_candidates(harness):
    """the consequence the expf domain test covers: with typical on, the first survivor need not be the most probable token --
    top-p and the final softmax then subtract a logit that is not the maximum (the grid above compares such draws with the reference)"""
    rng = np.random.default_rng(7)
    row = sample_ref.tie_free_row(rng, 4000, spread=1.0)
    p1 = g.sampling_ext(typical_p=0.001, temp=1.0, top_k=1000, top_p=1.0, repeat_penalty=1.0, repeat_last_n=0, seed=3)      # keeps only the most typical token
    h = scr.HostChain(harness, p1)
    assert h.draw(row, []) != int(np.argmax(row)) and h.ambiguous.value == 0


@pytest.mark.parametrize("version", [1, 2])
def test_mirostat_matches_reference(harness, ref, version):
    """24 consecutive draws per (tau, eta, temp), with and without penalties: the same tokens, and after every draw the same mu
    bit for bit, so the truncation length follows the reference's. The default chain's stages are set too: mirostat ignores them."""
    n_vocab = ref.rows_vocab
    rng = np.random.default_rng(MIROSTAT_SEED[n_vocab] + version)
    # (65024: rows on which mu hovers instead of running away -- once mirostat keeps tens of thousands of candidates, dividing
    # by temp ties two of them on any row, which is outside the contract)
    rows = [sample_ref.tie_free_row(rng, n_vocab, spread=s) for s in (3.0, 4.0)] if n_vocab > 10000 else _rows(rng, n_vocab)
    for tau, eta, temp, pen in itertools.product([3.0, 5.0], [0.1, 0.5], [0.8, 1.5], [False, True]):
        window = [int(t) for t in rng.integers(0, n_vocab, 64)] if pen else []
        p = g.sampling_ext(mirostat=version, mirostat_tau=tau, mirostat_eta=eta, temp=temp, top_k=40, top_p=0.95, tfs_z=0.9, typical_p=0.9,
                           repeat_penalty=1.1 if pen else 1.0, repeat_last_n=len(window), frequency_penalty=0.3 if pen else 0.0,
                           presence_penalty=0.2 if pen else 0.0, seed=int(rng.integers(0, 2 ** 31)), logit_bias={n_vocab - 1: -2.0} if pen else None)
        _check(harness, ref, rows, p, window, 24, (n_vocab, version, tau, eta, temp, pen))


def test_mirostat_mu_moves(harness, ref):
    """the grid above is not vacuous: mu leaves 2 tau and the number of kept candidates changes between draws"""
    n_vocab = ref.rows_vocab
    rng = np.random.default_rng(5)
    rows = _rows(rng, n_vocab)
    p = g.sampling_ext(mirostat=2, mirostat_tau=3.0, mirostat_eta=0.5, temp=0.8, repeat_penalty=1.0, repeat_last_n=0, seed=9)
    _, mus = scr.HostChain(harness, p, ref.n_vocab).run(rows, [], 24)
    assert len(set(mus)) > (2 if n_vocab == 7 else 12)
    assert mus[0] != np.float32(6.0).view(np.uint32).item() or n_vocab == 7


def test_greedy_ignores_the_new_stages(harness, ref):
    p = g.sampling_ext(mirostat=2, tfs_z=0.5, typical_p=0.5, temp=0.0, repeat_penalty=1.0, repeat_last_n=0, seed=1)
    rng = np.random.default_rng(6)
    rows = _rows(rng, ref.rows_vocab)
    _check(harness, ref, rows, p, [], 4, "greedy")
    assert not math.isnan(scr.HostChain(harness, p, ref.n_vocab).mu.value)


def test_example_flags_choose_the_ext_path():
    """examples/falcon_generate.py: falcon_main's --tfs / --typical / --mirostat / --mirostat-lr / --mirostat-ent give a SamplingExt
    (set through set_sampling_ext) with falcon_main's defaults for the rest; without any of them the old path and structure stay"""
    import argparse
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("falcon_generate", os.path.join(root, "examples", "falcon_generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ap = argparse.ArgumentParser()
    gen.add_sampling_args(ap)
    p = gen.sampling_from_args(ap.parse_args(["--mirostat", "2", "--mirostat-ent", "3", "--mirostat-lr", "0.5", "-s", "5"]))
    assert isinstance(p, g.SamplingExt) and (p.base.mirostat, p.mirostat_tau, p.mirostat_eta, p.base.seed, p.base.top_k) == (2, 3.0, 0.5, 5, 40)
    p = gen.sampling_from_args(ap.parse_args(["--tfs", "0.5", "--typical", "0.25", "--top-k", "100", "-s", "6"]))
    assert isinstance(p, g.SamplingExt) and (p.base.tfs_z, p.base.typical_p, p.base.mirostat, p.mirostat_tau, p.base.top_k) == (0.5, 0.25, 0, 5.0, 100)
    gen.set_seed(p, -1)
    assert p.base.seed == 2 ** 32 - 1
    p = gen.sampling_from_args(ap.parse_args(["--temp", "0.7", "-s", "5"]))
    assert isinstance(p, g.Sampling)
    assert gen.sampling_from_args(ap.parse_args([])) is None

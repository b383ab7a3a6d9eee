"""CPU: embeddings. (1) The expectation the GPU tests use -- oracle.layer_norm with ln_f over the oracle's last hidden plane -- is what the REAL
reference returned from falcon_get_embeddings (tests/golden/embedding.npz, tests/gen_embedding_golden.py), bit for bit. (2) The pooling arithmetic
of csrc/fq_embed.h as tests/embed_ref.py states it, pinned on hand-made rows whose chain order matters, and the operator cases' inputs checked for
order-free normalisation. (3) The embedding section of the session file (csrc/fq_session.h) through tests/host/embed_session_harness.cpp: the
reference's file with the row parses, re-composes to its own bytes and is refused by a context that expects another size; also as a stand-alone
program under the host sanitizers."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import embed_ref as er
from embed_ref import MODELS, bits, golden_model, oracle_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ggllm.cpp_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "host", "embed_session_harness.cpp")
E_TRUNCATED, E_EMBEDDING = 4, 7


# ------------------------------------------------------------------------------------------------ (1) oracle vs golden
@pytest.mark.parametrize("name", sorted(MODELS))
def test_oracle_layer_norm_of_last_plane_is_the_reference_embedding(oracle, golden, name):
    g = golden["embedding"]
    hp, w = golden_model(oracle, name)
    tokens, n_prompt = g[name + "_tokens"], int(g["n_prompt"])
    emb = g[name + "_emb"]
    assert emb.shape == (tokens.size - n_prompt, hp["n_embd"])
    pieces = [n_prompt] + [1] * (tokens.size - n_prompt)
    rows = oracle_rows(oracle, w, tokens, pieces, int(g["n_ctx"]))
    ends = np.cumsum(pieces) - 1                       # the last position of every eval
    assert np.array_equal(bits(rows[ends[:-1]]), bits(emb))
    assert np.array_equal(bits(rows[ends[-1]]), bits(g[name + "_next_emb"]))


def test_golden_model_files_are_the_seeded_models(oracle, golden, tmp_path):
    import ggcc_writer
    import lora_ref
    for name in MODELS:
        path = str(tmp_path / (name + ".ggcc"))
        ggcc_writer.write_ggcc(path, golden_model(oracle, name)[1])
        assert lora_ref.sha256_file(path) == str(golden["embedding"][name + "_model_sha256"])


# ------------------------------------------------------------------------------------------------ (2) the pooling reference
def test_chain_order_is_row_order():
    col = er.ORDER_COLUMN
    assert col.dtype == np.float32 and col.tolist() == [2.0 ** 60, 1.0, -2.0 ** 60]
    rows = np.stack([col, col[[0, 2, 1]], col[[1, 0, 2]]], axis=1)          # the same three values, three orders
    acc, n = er.accumulate(rows)
    assert n == 3 and acc.tolist() == [0.0, 1.0, 0.0]                       # (2^60 + 1 is not an f64: the 1 survives only when it comes last)
    assert er.mean(acc, n).tolist() == [0.0, np.float32(1.0 / 3.0), 0.0]


def test_chain_carries_across_calls():
    rng = np.random.default_rng(5)
    rows = (rng.standard_normal((70, 96)) * 10.0 ** rng.integers(-6, 6, (70, 96))).astype(np.float32)
    one = er.accumulate(rows)
    acc, n = None, 0
    for a, b in ((0, 1), (1, 65), (65, 70)):
        acc, n = er.accumulate(rows[a:b], acc, n)
    assert n == one[1] == 70 and np.array_equal(acc.view(np.uint64), one[0].view(np.uint64))
    want = np.zeros(96, np.float64)
    for r in rows:                                                          # the definition, one add at a time
        want = want + r.astype(np.float64)
    assert np.array_equal(acc.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(bits(er.pooled(rows, False, [1, 64, 5])), bits((want / 70.0).astype(np.float32)))


def test_unit_vector_definition():
    m = np.array([3.0, 0.0, -4.0], np.float32)
    assert er.sum_squares(m) == 25.0 and er.unit(m).tolist() == [np.float32(0.6), 0.0, np.float32(-0.8)]
    rng = np.random.default_rng(6)
    m = rng.standard_normal(4544).astype(np.float32)
    part = [0.0] * er.THREADS
    for i, v in enumerate(m.astype(np.float64)):                            # thread t chains the columns t, t + 256, ...
        part[i % er.THREADS] = part[i % er.THREADS] + v * v
    s = 0.0
    for p in part:
        s = s + p
    assert er.sum_squares(m) == s
    assert np.array_equal(bits(er.unit(m)), bits((m.astype(np.float64) / np.sqrt(np.float64(s))).astype(np.float32)))


def test_operator_cases_are_order_free():
    """every case of tests/test_gpu_embed.py: its seed (the first that passes, searched here) gives a unit vector whose f32 values are the same for s
    summed in index order, reversed, pairwise and in the kernel's order; and the order-sensitive column sits where the test says"""
    assert len(er.CASE_SHAPES) == 16
    for n_embd, n_rows in er.CASE_SHAPES:
        seed = er.case_seed(n_embd, n_rows)
        assert seed - (1000 * n_embd + n_rows) < 50, (n_embd, n_rows)
        x = er.case_rows(n_embd, n_rows, seed)
        m = er.mean(*er.accumulate(x))
        assert er.order_free(m) and er.sum_squares(m) > 0
        assert sum(er.case_splits(n_rows)) == n_rows and er.case_splits(n_rows)[0] == 1
        if n_rows >= 3:
            for col in {0, 63, 64, n_embd - 1} & set(range(n_embd)):
                assert m[col] == 0.0
            moved = x[[0, n_rows - 1] + list(range(1, n_rows - 1))]          # 2^60, -2^60, then the 1: another chain, another mean
            assert er.mean(*er.accumulate(moved))[0] == np.float32(1.0 / n_rows)


# ------------------------------------------------------------------------------------------------ (3) the session file's embedding section
@pytest.fixture(scope="module")
def H(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("embed_session") / "libembed_session_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, "-o", out, HARNESS])
    L = C.CDLL(out)
    vp = C.c_void_p
    L.es_parse.restype, L.es_parse.argtypes = C.c_int, [vp, C.c_long, vp, C.c_long, vp]
    L.es_state_bytes.restype, L.es_state_bytes.argtypes = C.c_long, [vp, C.c_long, C.c_int, C.c_long]
    L.es_recompose.restype, L.es_recompose.argtypes = C.c_long, [vp, C.c_long, vp, C.c_long, vp]
    return L


def _dims(b):
    hp = struct.unpack_from("<9i", bytes(b[:48]), 8)                       # n_vocab, n_ctx, n_embd, n_head, n_head_kv, n_layer, ...
    return np.array([hp[1], hp[5], hp[4] * 64], np.int32), hp[2]


def _parse(H, b, dims, expect):
    b = np.ascontiguousarray(b, np.uint8)
    info = np.full(12, -77, np.int64)
    rc = H.es_parse(b.ctypes.data, b.size, dims.ctypes.data, expect, info.ctypes.data)
    assert rc == 0 or (info == -77).all()
    return rc, info


@pytest.mark.parametrize("name", sorted(MODELS))
def test_golden_session_with_the_row_round_trips(H, golden, name):
    g = golden["embedding"]
    b = np.ascontiguousarray(g[name + "_file"])
    dims, E = _dims(b)
    rc, info = _parse(H, b, dims, E)
    assert rc == 0
    n_tok, blob, cap, size, lg_off, emb_size, emb_off, kv_ntok, k_off, v_off, n_bytes, _ = (int(x) for x in info)
    assert (n_tok, kv_ntok, emb_size) == (12, 12, E) and blob + n_bytes == b.size
    assert emb_off == lg_off + 4 * cap + 8 and k_off == emb_off + 4 * E + 8 + 4
    assert n_bytes == H.es_state_bytes(dims.ctypes.data, cap, kv_ntok, E) == H.es_state_bytes(dims.ctypes.data, cap, kv_ntok, 0) + 4 * E
    # the row in the file is the embedding the reference returned after its last eval
    row = np.frombuffer(bytes(b), np.float32, E, emb_off)
    assert np.array_equal(bits(row), bits(g[name + "_emb"][-1]))
    again = np.full(b.size, 0xEE, np.uint8)
    assert H.es_recompose(b.ctypes.data, b.size, dims.ctypes.data, E, again.ctypes.data) == b.size
    assert again.tobytes() == b.tobytes()


def test_embedding_size_is_refused_in_both_directions(H, golden):
    g = golden["embedding"]
    b = np.ascontiguousarray(g["gqa_q5_1_file"])
    dims, E = _dims(b)
    assert _parse(H, b, dims, E)[0] == 0
    for expect in (0, E - 1, E + 1, 4):
        assert _parse(H, b, dims, expect)[0] == E_EMBEDDING
    plain = np.ascontiguousarray(golden["session"]["gqa_q5_1_file"])      # a file of the reference without the row
    pdims, pE = _dims(plain)
    assert _parse(H, plain, pdims, 0)[0] == 0
    for expect in (pE, pE - 1, 1):
        assert _parse(H, plain, pdims, expect)[0] == E_EMBEDDING
    # the size field itself rewritten to n_embd - 1: refused at n_embd, and at n_embd - 1 the sections behind no longer fit
    _, info = _parse(H, b, dims, E)
    emb_off = int(info[6])
    c = b.copy()
    c[emb_off - 8:emb_off] = np.frombuffer(struct.pack("<Q", E - 1), np.uint8)
    assert _parse(H, c, dims, E)[0] == E_EMBEDDING
    assert _parse(H, c, dims, E - 1)[0] != 0


def test_every_truncation_inside_the_section_is_truncated(H, golden):
    g = golden["embedding"]
    for name in ("mqa_q4_0", "gqa_q4_k"):
        b = np.ascontiguousarray(g[name + "_file"])
        dims, E = _dims(b)
        _, info = _parse(H, b, dims, E)
        emb_off = int(info[6])
        for n in range(emb_off - 8, emb_off + 4 * E):
            assert _parse(H, b[:n], dims, E)[0] == E_TRUNCATED, n


def test_section_under_the_host_sanitizers(golden, tmp_path):
    """the same harness as a stand-alone program (-DES_MAIN) built with -fsanitize=address,undefined and run as its own process over the golden files: every
    parse from an exact-size heap buffer. Where the compiler lacks the sanitizer runtimes the same program is built and run without them."""
    exe = str(tmp_path / "embed_session_main")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DES_MAIN", "-I", CSRC, "-o", exe, HARNESS]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    g = golden["embedding"]
    for name in sorted(MODELS):
        b = np.ascontiguousarray(g[name + "_file"])
        path = str(tmp_path / (name + ".session"))
        b.tofile(path)
        (n_ctx, n_layer, row), E = _dims(b)
        r = subprocess.run([exe, path, str(n_ctx), str(n_layer), str(row), str(E)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr

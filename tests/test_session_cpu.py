"""CPU: the session-file format the library writes and parses (ggllm.cpp_amd/csrc/fq_session.h), host-compiled with g++ (tests/host/session_harness.cpp)
and checked against golden files the reference itself wrote (tests/golden/session.npz, scripts/gen_session_golden.py), against the numpy restatement
of the layout (tests/session_ref.py) and, for the generator text, against libstdc++'s own std::mt19937 in a small program compiled here."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import session_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ggllm.cpp_amd", "csrc")
MODELS = ("mqa_q4_0", "gqa_q5_1")
OK, E_MAGIC, E_HPARAMS, E_CAPACITY, E_TRUNCATED, E_NTOK, E_KV_SIZE, E_EMBEDDING, E_RNG, E_LOGITS = range(10)


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("session") / "libsession_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, "-o", out,
                           os.path.join(ROOT, "tests", "host", "session_harness.cpp")])
    L = C.CDLL(out)
    vp = C.c_void_p
    L.ss_rng_format.restype, L.ss_rng_format.argtypes = C.c_long, [vp, C.c_int, vp]
    L.ss_rng_parse.restype, L.ss_rng_parse.argtypes = C.c_int, [vp, C.c_long, vp, vp]
    L.ss_mt_after.restype, L.ss_mt_after.argtypes = None, [C.c_uint32, C.c_int, vp, vp]
    L.ss_parse.restype, L.ss_parse.argtypes = C.c_int, [vp, C.c_long, vp, C.c_long, vp, vp, vp, vp]
    L.ss_file_bytes.restype, L.ss_file_bytes.argtypes = C.c_long, [C.c_long, vp, C.c_long, C.c_int]
    L.ss_write.restype = C.c_long
    L.ss_write.argtypes = [vp, vp, vp, C.c_long, vp, vp, C.c_int, C.c_long, vp, C.c_long, C.c_int, vp, vp]
    return L


def _file(golden, name):
    return np.ascontiguousarray(golden["session"][name + "_file"])


def _hp(b):
    return np.array(struct.unpack_from("<9i", bytes(b[:48]), 8), np.int32)


def _dims(hp, n_ctx=None):
    d = dict(zip(sr.HP_FIELDS, hp.tolist()))
    return np.array([d["n_ctx"] if n_ctx is None else n_ctx, d["n_layer"], d["n_head_kv"] * 64], np.int32)


SENTINEL = 0x5A5A5A5A


def parse(H, b, hp, capacity, dims):
    """(code, info, mt, hp_out); the outputs are pre-filled with a sentinel so that a refusal that touched them shows"""
    b = np.ascontiguousarray(b, np.uint8)
    info, mt, hp_out = np.full(11, SENTINEL, np.int64), np.full(sr.MT_N, SENTINEL, np.uint32), np.full(9, SENTINEL, np.int32)
    rc = H.ss_parse(b.ctypes.data, b.size, hp.ctypes.data, capacity, dims.ctypes.data, info.ctypes.data, mt.ctypes.data, hp_out.ctypes.data)
    return rc, info, mt, hp_out


def write(H, hp, tokens, dims, mt, pos, logits_cap, logits, kv_ntok, k_bytes, v_bytes):
    tokens, logits = np.ascontiguousarray(tokens, np.int32), np.ascontiguousarray(logits, np.float32)
    mt = np.ascontiguousarray(mt, np.uint32)
    n = H.ss_file_bytes(tokens.size, dims.ctypes.data, logits_cap, kv_ntok)
    out = np.full(n, 0xEE, np.uint8)
    k, v = np.frombuffer(k_bytes, np.uint8), np.frombuffer(v_bytes, np.uint8)
    got = H.ss_write(out.ctypes.data, hp.ctypes.data, tokens.ctypes.data, tokens.size, dims.ctypes.data, mt.ctypes.data, pos, logits_cap,
                     logits.ctypes.data, logits.size, kv_ntok, k.ctypes.data if k.size else None, v.ctypes.data if v.size else None)
    assert got == n
    return out


def test_overhead_constant_is_the_golden_files(H, golden):
    """kv_size of both golden files = 4 * overhead + 12 * ne: the constant named in the header is the reference build's"""
    assert H.ss_overhead() == sr.TENSOR_OVERHEAD
    for name in MODELS:
        b = _file(golden, name)
        _, _, st, _ = sr.split_file(b)
        hp = _hp(b)
        n_ctx, n_layer, row = _dims(hp).tolist()
        assert st["kv_size"] == sr.kv_size(n_layer, row, n_ctx) == 4 * H.ss_overhead() + 12 * row * n_layer * n_ctx


@pytest.mark.parametrize("name", MODELS)
def test_golden_round_trip(H, golden, name):
    """parse a file the reference wrote into sections, write them again: the same bytes; the sections are those of the numpy restatement"""
    b = _file(golden, name)
    hp, dims = _hp(b), _dims(_hp(b))
    rc, info, mt, hp_out = parse(H, b, hp, 64, dims)
    assert rc == OK and np.array_equal(hp_out, hp)
    n_tok, tok_off, blob, cap, size, lg_off, kv_ntok, k_off, v_off, n_bytes, pos = (int(x) for x in info)
    ref_hp, ref_tok, st, ref_off = sr.split_file(b)
    assert (n_tok, blob, cap, size, kv_ntok, pos) == (ref_tok.size, ref_off, st["logits_cap"], st["logits"].size, st["n_tok"], st["pos"])
    assert blob + n_bytes == b.size and np.array_equal(mt, st["mt"])
    assert n_tok == 12 and kv_ntok == 12 and np.array_equal(ref_tok, golden["session"][name + "_tokens"][:12])
    kvb = int(dims[1]) * kv_ntok * int(dims[2]) * 4
    assert v_off == k_off + kvb and v_off + kvb == b.size
    raw = bytes(b)
    tokens = np.frombuffer(raw, np.int32, n_tok, tok_off)
    logits = np.frombuffer(raw, np.float32, size, lg_off)
    again = write(H, hp, tokens, dims, mt, pos, cap, logits, kv_ntok, raw[k_off:k_off + kvb], raw[v_off:v_off + kvb])
    assert again.tobytes() == raw
    # ... and the numpy restatement builds the same file from its own sections
    state = sr.build_state(st["mt"], st["pos"], st["logits_cap"], st["logits"], int(dims[1]), int(dims[2]), int(dims[0]), st["k"], st["v"])
    assert sr.build_file(ref_hp, ref_tok, state) == raw


@pytest.mark.parametrize("name", MODELS)
def test_generator_text_round_trip(H, golden, name):
    """the golden generator text -> 624 words and a position -> text: identical; it is std::mt19937(1), untouched (the reference drew nothing)"""
    _, _, st, _ = sr.split_file(_file(golden, name))
    text = np.frombuffer(st["rng_text"], np.uint8).copy()
    mt, pos = np.zeros(sr.MT_N, np.uint32), C.c_int(-1)
    assert H.ss_rng_parse(text.ctypes.data, text.size, mt.ctypes.data, C.byref(pos)) == OK
    out = np.zeros(sr.RNG_BYTES, np.uint8)
    n = H.ss_rng_format(mt.ctypes.data, pos.value, out.ctypes.data)
    assert out[:n].tobytes() == st["rng_text"] == sr.rng_text(mt, pos.value)
    seeded, p = sr.mt_seeded(1)
    assert pos.value == p == 624 and np.array_equal(mt, seeded)


_MT_PROGRAM = r"""
#include <iostream>
#include <random>
#include <cstdlib>
int main(int argc, char ** argv) {
    std::mt19937 rng(std::atoi(argv[1]));
    for (int i = 0, n = std::atoi(argv[2]); i < n; ++i) (void) rng();
    std::cout << rng;
    return 0;
}
"""


def test_generator_after_draws_formats_as_libstdcxx_streams_it(H, tmp_path):
    """the device sampler's generator (csrc/fq_sample.h, what a sampler row holds) after 0, 1, 623, 624 and 625 draws formats to the text
    std::mt19937 streams after as many: the position convention (624 = twist before the next draw) is libstdc++'s, on both sides of a twist"""
    src, exe = str(tmp_path / "mt.cpp"), str(tmp_path / "mt")
    open(src, "w").write(_MT_PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, src])
    for seed in (1, 7):
        for n in (0, 1, 623, 624, 625):
            want = subprocess.run([exe, str(seed), str(n)], capture_output=True, check=True).stdout
            mt, pos = np.zeros(sr.MT_N, np.uint32), C.c_int(-1)
            H.ss_mt_after(seed, n, mt.ctypes.data, C.byref(pos))
            out = np.zeros(sr.RNG_BYTES, np.uint8)
            k = H.ss_rng_format(mt.ctypes.data, pos.value, out.ctypes.data)
            assert out[:k].tobytes() == want, (seed, n)
            back, p = np.zeros(sr.MT_N, np.uint32), C.c_int(-1)
            assert H.ss_rng_parse(out.ctypes.data, k, back.ctypes.data, C.byref(p)) == OK
            assert np.array_equal(back, mt) and p.value == pos.value


def _refused(H, b, hp, capacity, dims, code):
    rc, info, mt, hp_out = parse(H, b, hp, capacity, dims)
    assert rc == code, (rc, code)
    assert (info == SENTINEL).all() and (mt == SENTINEL).all() and (hp_out == SENTINEL).all()      # nothing touched


def test_every_refusal_has_its_code_and_touches_nothing(H, golden):
    b = _file(golden, "gqa_q5_1")
    hp, dims = _hp(b), _dims(_hp(b))
    rc, info, _, _ = parse(H, b, hp, 64, dims)
    assert rc == OK
    blob, lg_off, cap, k_off = int(info[2]), int(info[5]), int(info[3]), int(info[7])
    emb_off = lg_off + 4 * cap

    def patched(off, fmt, value):
        c = b.copy()
        c[off:off + struct.calcsize(fmt)] = np.frombuffer(struct.pack(fmt, value), np.uint8)
        return c

    _refused(H, patched(0, "<I", 0x67676D6C), hp, 64, dims, E_MAGIC)                 # another magic
    _refused(H, patched(4, "<I", 2), hp, 64, dims, E_MAGIC)                          # another version
    other = hp.copy(); other[5] += 1                                                 # the caller's model has one layer more
    _refused(H, b, other, 64, dims, E_HPARAMS)
    other = hp.copy(); other[8] = 3                                                  # ... or another ftype: any byte of the record
    _refused(H, b, other, 64, dims, E_HPARAMS)
    _refused(H, b, hp, 11, dims, E_CAPACITY)                                         # 12 tokens, room for 11
    assert parse(H, b, hp, 12, dims)[0] == OK
    for n in (0, 7, 8, 20, 43, 44, 47, 48 + 4 * 11, blob, blob + 7, blob + 8 + 100, lg_off - 1, lg_off + 4 * cap, emb_off + 8 + 11, k_off, b.size - 1):
        _refused(H, b[:n], hp, 64, dims, E_TRUNCATED)                                # every section cut short
    _refused(H, patched(44, "<I", 1 << 30), hp, 1 << 31, dims, E_TRUNCATED)           # a token count beyond the file
    _refused(H, patched(lg_off - 16, "<Q", 1 << 62), hp, 64, dims, E_TRUNCATED)       # a logits capacity beyond the file (and beyond size_t when scaled)
    _refused(H, patched(k_off - 4, "<i", -1), hp, 64, dims, E_NTOK)
    _refused(H, patched(k_off - 4, "<i", int(dims[0]) + 1), hp, 64, dims, E_NTOK)
    _refused(H, b, hp, 64, _dims(hp, n_ctx=8), E_NTOK)                               # 12 rows into a context of 8
    _refused(H, patched(k_off - 4, "<i", 13), hp, 64, dims, E_TRUNCATED)              # one row more than the file holds
    _refused(H, patched(k_off - 12, "<Q", sr.kv_size(2, 128, 32) + 4), hp, 64, dims, E_KV_SIZE)
    _refused(H, b, hp, 64, _dims(hp, n_ctx=64), E_KV_SIZE)                           # the same model at another n_ctx
    _refused(H, patched(emb_off, "<Q", 4), hp, 64, dims, E_EMBEDDING)
    _refused(H, patched(lg_off - 8, "<Q", cap + 1), hp, 64, dims, E_LOGITS)
    n_text = struct.unpack_from("<Q", bytes(b[blob:blob + 8]))[0]
    _refused(H, patched(blob, "<Q", sr.RNG_BYTES + 1), hp, 64, dims, E_RNG)           # a text longer than its buffer
    _refused(H, patched(blob, "<Q", n_text - 4), hp, 64, dims, E_RNG)                 # the position cut off: 624 numbers
    _refused(H, patched(blob, "<Q", 0), hp, 64, dims, E_RNG)
    _refused(H, patched(blob + 8 + n_text - 3, "<B", ord("7")), hp, 64, dims, E_RNG)  # position 724
    _refused(H, patched(blob + 8 + 3, "<B", ord("x")), hp, 64, dims, E_RNG)           # not a number
    _refused(H, patched(blob + 8 + 1, "<B", ord("9")), hp, 64, dims, E_RNG)           # first word 19812433254... > 32 bits


def test_empty_cache_writes_and_parses(H):
    """kv_ntok 0: no K or V bytes; a logits row and a drawn-from generator survive the trip"""
    hp = np.array([512, 32, 256, 4, 1, 2, 7, 0, 2], np.int32)
    dims = _dims(hp)
    mt, pos = np.zeros(sr.MT_N, np.uint32), C.c_int(0)
    H.ss_mt_after(7, 5, mt.ctypes.data, C.byref(pos))
    logits = np.random.default_rng(3).standard_normal(512).astype(np.float32)
    b = write(H, hp, [], dims, mt, pos.value, 512, logits, 0, b"", b"")
    empty = np.zeros((2, 0, 64), np.float32)
    assert b.tobytes() == sr.build_file(hp, [], sr.build_state(mt, pos.value, 512, logits, 2, 64, 32, empty, empty))
    rc, info, mt2, _ = parse(H, b, hp, 0, dims)
    assert rc == OK and info[0] == 0 and info[6] == 0 and info[7] == info[8] == b.size and info[10] == pos.value == 5
    assert np.array_equal(mt2, mt)


def test_parser_under_the_host_sanitizers(golden, tmp_path):
    """the header plus a stand-alone main (tests/host/session_parse_main.cpp) that parses a golden file, three truncations of it and one with kv_ntok =
    n_ctx + 1 from exact-size heap buffers, built with -fsanitize=address,undefined and run as its own process (a host program: nothing sanitized is
    loaded into Python). Where the compiler lacks the sanitizer runtimes the same program is built and run without them."""
    exe, src = str(tmp_path / "session_parse_main"), os.path.join(ROOT, "tests", "host", "session_parse_main.cpp")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, src]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    for name in MODELS:
        b = _file(golden, name)
        path = str(tmp_path / (name + ".session"))
        b.tofile(path)
        n_ctx, n_layer, row = _dims(_hp(b)).tolist()
        r = subprocess.run([exe, path, str(n_ctx), str(n_layer), str(row)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr

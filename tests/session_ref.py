"""The reference's session file and state blob (libfalcon.cpp:4185-4564), restated in numpy for the tests: sections to bytes and back, the V
transpose, the generator text. Independent of csrc/fq_session.h, which tests/test_session_cpu.py checks against this and against golden files the
reference itself wrote (tests/golden/session.npz)."""
import struct

import numpy as np

MAGIC, VERSION, RNG_BYTES, MT_N = 0x6767736E, 1, 65536, 624
TENSOR_OVERHEAD = 416          # ggml_tensor_overhead() of the reference's build, from the golden files' kv_size
HP_FIELDS = ("n_vocab", "n_ctx", "n_embd", "n_head", "n_head_kv", "n_layer", "n_falcon_type", "n_bpe_merges", "ftype")


def kv_size(n_layer, row, n_ctx):
    """MEM_REQ_KV_SELF (libfalcon.cpp:162-175), f32, the build without FALCON_NO_KV_UPGRADE"""
    return 4 * TENSOR_OVERHEAD + 3 * 4 * row * n_layer * n_ctx


def mt_seeded(seed):
    """std::mt19937(seed): (624 words, position 624)"""
    st = np.random.RandomState(seed).get_state()
    assert st[0] == "MT19937" and st[2] == MT_N
    return st[1].astype(np.uint32), MT_N


def rng_text(mt, pos):
    """what libstdc++ streams for the engine: the words, then the position, decimal, one space between"""
    return (" ".join(str(int(w)) for w in mt) + " " + str(int(pos))).encode()


def rng_parse(text):
    w = [int(x) for x in text.split()]
    assert len(w) == MT_N + 1 and 0 <= w[-1] <= MT_N
    return np.array(w[:-1], np.uint32), w[-1]


def v_to_file(v):
    """cache order [layer][pos][row] -> file order [layer][row][pos]"""
    return np.ascontiguousarray(np.transpose(v, (0, 2, 1)))


def staging(k_cache, v_cache, n_tok, first_row=0):
    """what ggml_hip_kv_pack writes for caches [layer][rows][row]: K rows as they lie, then V transposed (float32, flat)"""
    k = np.ascontiguousarray(k_cache[:, first_row:first_row + n_tok])
    v = v_to_file(v_cache[:, first_row:first_row + n_tok])
    return np.concatenate([k.ravel(), v.ravel()]).astype(np.float32)


def build_state(mt, pos, logits_cap, logits, n_layer, row, n_ctx, k, v):
    """k, v: float32 [n_layer][n_tok][row] in cache order"""
    text = rng_text(mt, pos)
    lg = np.ascontiguousarray(logits, np.float32).ravel()
    n_tok = k.shape[1]
    assert k.shape == v.shape == (n_layer, n_tok, row) and lg.size <= logits_cap
    out = [struct.pack("<Q", len(text)), text + b"\0" * (RNG_BYTES - len(text)), struct.pack("<QQ", logits_cap, lg.size),
           lg.tobytes() + b"\0" * (4 * (logits_cap - lg.size)), struct.pack("<Q", 0), struct.pack("<Qi", kv_size(n_layer, row, n_ctx), n_tok),
           np.ascontiguousarray(k, np.float32).tobytes(), v_to_file(np.asarray(v, np.float32)).tobytes()]
    return b"".join(out)


def build_file(hp, tokens, state):
    """hp: the nine int32 in HP_FIELDS order"""
    tok = np.ascontiguousarray(tokens, np.int32)
    return struct.pack("<II9iI", MAGIC, VERSION, *[int(x) for x in hp], tok.size) + tok.tobytes() + state


def split_state(b, n_layer, row):
    """a state blob's sections; K and V come back in cache order [n_layer][n_tok][row]"""
    pos = 0
    n_text, = struct.unpack_from("<Q", b, pos); pos += 8
    text = bytes(b[pos:pos + n_text]); pos += RNG_BYTES
    cap, size = struct.unpack_from("<QQ", b, pos); pos += 16
    logits = np.frombuffer(b, np.float32, size, pos).copy(); pos += 4 * cap
    emb, = struct.unpack_from("<Q", b, pos); pos += 8
    kvs, n_tok = struct.unpack_from("<Qi", b, pos); pos += 12
    n = n_layer * n_tok * row
    k = np.frombuffer(b, np.float32, n, pos).reshape(n_layer, n_tok, row).copy(); pos += 4 * n
    v = np.transpose(np.frombuffer(b, np.float32, n, pos).reshape(n_layer, row, n_tok), (0, 2, 1)).copy(); pos += 4 * n
    mt, p = rng_parse(text)
    return dict(mt=mt, pos=p, rng_text=text, logits_cap=cap, logits=logits, embedding=emb, kv_size=kvs, n_tok=n_tok, k=k, v=v, n_bytes=pos)


def split_file(b):
    """(hp tuple, tokens, state section dict, offset of the blob)"""
    b = bytes(b)
    head = struct.unpack_from("<II9iI", b, 0)
    assert head[0] == MAGIC and head[1] == VERSION
    hp, n = head[2:11], head[11]
    tokens = np.frombuffer(b, np.int32, n, 48).copy()
    off = 48 + 4 * n
    d = dict(zip(HP_FIELDS, hp))
    st = split_state(b[off:], d["n_layer"], d["n_head_kv"] * (d["n_embd"] // d["n_head"]))
    assert off + st["n_bytes"] == len(b)
    return hp, tokens, st, off

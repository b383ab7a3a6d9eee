"""LoRA adapters for the tests (a helper, not a test): a writer for the reference's 'ggla' file, adapters drawn from a seed, the
COMPOSED EXPECTATION -- what llama_apply_lora_from_file_internal (libfalcon.cpp:3927-4170) makes of a matrix in the reference's scalar
build, restated with numpy and the reference's own (de)quantizers -- and the corpus of damaged files with the code each must give.

  per element [m][k]:  s (f64) = 0; for i in 0..r-1: s += f64(f32(A[k][i] * B[m][i]));  ba = f32(s)
                       scaling = f32(alpha) / f32(r);  if scaling != 1: ba = f32(ba * scaling)
  quantized W          W = quantize_row(dequantize_row(W) + ba)            F16 W   W = f16(f32(W) + ba)
  base file            F16 base: t = f16(f32(base) + ba), W = quantize_row(f32(t));   F32 base: W = quantize_row(base + ba)
  F16 loraA            A widened, B rounded to f16 and widened (ggml's f16 mat-mul), then as above

tests/gen_lora_golden.py proves this file against the real reference: a model composed here and loaded by
the reference gives the logits of the reference's own merge, bit for bit (tests/golden/lora.npz)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from oracle import binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGIC, VERSION = 0x67676C61, 1
F32, F16 = 0, 1
LEAVES = {"qkv": "self_attention.query_key_value.weight", "wo": "self_attention.dense.weight", "up": "mlp.dense_h_to_4h.weight",
          "down": "mlp.dense_4h_to_h.weight"}


# ------------------------------------------------------------------------------------------------ names <-> the weights dict of synth.make_model
def tensor_name(key):
    """key: 'tok_emb', 'lm_head' or (layer, 'qkv' | 'wo' | 'up' | 'down')"""
    if key == "tok_emb":
        return "transformer.word_embeddings.weight"
    if key == "lm_head":
        return "lm_head.weight"
    return "transformer.h.%d.%s" % (key[0], LEAVES[key[1]])


def matrix_keys(hp):
    return ["tok_emb", "lm_head"] + [(i, k) for i in range(hp["n_layer"]) for k in ("qkv", "wo", "up", "down")]


def shape_of(hp, key):
    """(K, M) of the matrix"""
    E, FF, V = hp["n_embd"], hp["n_ff"], hp["n_vocab"]
    if key in ("tok_emb", "lm_head"):
        return E, V
    return {"qkv": (E, (hp["n_head"] + 2 * hp["n_head_kv"]) * 64), "wo": (E, E), "up": (E, FF), "down": (FF, E)}[key[1]]


def get_matrix(weights, key):
    return weights[key] if isinstance(key, str) else weights["layers"][key[0]][key[1]]


def set_matrix(weights, key, value):
    if isinstance(key, str):
        weights[key] = value
    else:
        weights["layers"][key[0]][key[1]] = value


def copy_weights(weights):
    out = dict(weights)
    out["layers"] = [dict(lw) if lw is not None else None for lw in weights["layers"]]
    return out


# ------------------------------------------------------------------------------------------------ the file
def record(name, arr):
    """one tensor record without its alignment padding: (head + name, data); arr [ne1][ne0] f32 or f16"""
    arr = np.ascontiguousarray(arr)
    ftype = {np.dtype(np.float32): F32, np.dtype(np.float16): F16}[arr.dtype]
    nb = name.encode()
    return struct.pack("<5i", 2, len(nb), ftype, arr.shape[1], arr.shape[0]) + nb, arr.tobytes()


def write_ggla(path, r, alpha, records, magic=MAGIC, version=VERSION):
    """records: [(name, array [ne1][ne0])] in file order. Returns the offsets where each record begins (and the file's end)."""
    out = bytearray(struct.pack("<IIii", magic, version, r, alpha))
    marks = []
    for name, arr in records:
        marks.append(len(out))
        head, data = record(name, arr)
        out += head
        out += b"\0" * (-len(out) & 31)
        out += data
    marks.append(len(out))
    with open(path, "wb") as f:
        f.write(bytes(out))
    return marks


def draw_adapter(hp, keys, r, seed, a_f16=False, std=0.05):
    """{key: (A [K][r], B [M][r])}: N(0, std^2) as f32 (A as f16 when a_f16), one generator per target in the order given"""
    out = {}
    for n, key in enumerate(keys):
        K, M = shape_of(hp, key)
        rng = np.random.default_rng(seed + 1000 * n)
        A = (rng.standard_normal((K, r)) * std).astype(np.float32)
        B = (rng.standard_normal((M, r)) * std).astype(np.float32)
        out[key] = (A.astype(np.float16) if a_f16 else A, B)
    return out


def adapter_records(pairs, b_first=False):
    """pairs: [(key, A, B)] in application order -> records; b_first: loraB before loraA"""
    recs = []
    for key, A, B in pairs:
        n = tensor_name(key)
        two = [(n + ".loraA", A), (n + ".loraB", B)]
        recs += two[::-1] if b_first else two
    return recs


# ------------------------------------------------------------------------------------------------ the reference's (de)quantizers
_Q = {}


def _host_wquant():
    """ggllm.cpp_amd/csrc/fq_wquant.h compiled for the host (tests/host/wquant_harness.cpp): byte-pinned against the reference's quantizers by
    tests/test_wquant_cpu.py; used where oracle/_ref is absent"""
    if "host" not in _Q:
        src = os.path.join(ROOT, "tests", "host", "wquant_harness.cpp")
        out = os.path.join(ROOT, "tests", "host", "libwquant_host.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "ggllm.cpp_amd", "csrc"), "-o", out, src])
        L = C.CDLL(out)
        L.wquant_rows.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _Q["host"] = L
    return _Q["host"]


def _ref():
    if "ref" not in _Q:
        _Q["ref"] = ob.Ref(scalar=True) if ob.Ref.available(scalar=True) else None
    return _Q["ref"]


def have_reference():
    return _ref() is not None


def quantize(t, x):
    """[rows][K] f32 -> [rows][row_bytes]: quantize_row_q*_reference, a row at a time"""
    x = np.ascontiguousarray(x, np.float32)
    rows, K = x.shape
    if _ref() is not None:
        return _ref().quantize(t, x).reshape(rows, ob.row_bytes(t, K))
    out = np.zeros((rows, ob.row_bytes(t, K)), np.uint8)
    assert _host_wquant().wquant_rows(t, x.ctypes.data, x.size, out.ctypes.data, None) == 0
    return out


def dequantize(t, blocks, K):
    blocks = np.ascontiguousarray(blocks, np.uint8)
    rows = blocks.size // ob.row_bytes(t, K)
    if _ref() is not None:
        return _ref().dequantize(t, blocks, rows * K).reshape(rows, K)
    if "orc" not in _Q:
        _Q["orc"] = ob.Oracle()
    return _Q["orc"].dequantize(t, blocks, rows * K).reshape(rows, K)


# ------------------------------------------------------------------------------------------------ the composed expectation
def low_rank(A, B, r_header, alpha):
    """ba [M][K] f32 of steps 1 and 2"""
    if A.dtype == np.float16:
        A, B = A.astype(np.float32), B.astype(np.float16).astype(np.float32)
    assert A.dtype == np.float32 and B.dtype == np.float32 and A.shape[1] == B.shape[1]
    s = np.zeros((B.shape[0], A.shape[0]), np.float64)
    for i in range(A.shape[1]):
        s += np.multiply.outer(B[:, i], A[:, i]).astype(np.float64)      # (f32 x f32 -> f32: one rounding; the f64 sum in index order)
    ba = s.astype(np.float32)
    scaling = np.float32(alpha) / np.float32(r_header)
    return ba * scaling if scaling != np.float32(1.0) else ba


def merged(wtype, W, K, A, B, r_header, alpha, base=None):
    """the patched matrix: W ggml bytes [M][row_bytes] (wtype quantized) or f16 [M][K] (wtype F16); base: None, or the base file's f16 / f32 [M][K]"""
    ba = low_rank(A, B, r_header, alpha)
    if wtype == F16:
        assert base is None, "F16 destination with a base file: not pinned, refused by the library"
        return (np.ascontiguousarray(W).view(np.float16).reshape(-1, K).astype(np.float32) + ba).astype(np.float16)
    if base is None:
        y = dequantize(wtype, W, K) + ba
    elif base.dtype == np.float16:
        y = (base.astype(np.float32) + ba).astype(np.float16).astype(np.float32)
    else:
        y = base.astype(np.float32) + ba
    return quantize(wtype, y)


def compose(weights, pairs, r_header, alpha, base_weights=None):
    """a copy of the weights dict with every (key, A, B) of pairs merged in order; base_weights: the float model of the base file"""
    out = copy_weights(weights)
    hp, wt = weights["hparams"], weights["wtype"]
    for key, A, B in pairs:
        K, _ = shape_of(hp, key)
        base = None if base_weights is None else np.asarray(get_matrix(base_weights, key))
        set_matrix(out, key, merged(wt, get_matrix(out, key), K, A, B, r_header, alpha, base))
    return out


# ------------------------------------------------------------------------------------------------ damaged files
E_IO, E_MAGIC, E_VERSION, E_RANK, E_TRUNCATED, E_NOT_LORA, E_UNKNOWN, E_NDIMS, E_FTYPE, E_SHAPE, E_INNER, E_UNPAIRED, E_TYPE_PAIR = range(1, 14)
E_BASE_OPEN, E_BASE_TENSOR, E_BASE_F16_DST = 34, 35, 36


def damaged_corpus(dirname, hp):
    """[(label, path, expected code)] -- 0: a file that is good. Two small targets, r = 3."""
    keys = [(0, "wo"), (1, "qkv")]
    ad = draw_adapter(hp, keys, 3, seed=99)
    good = adapter_records([(k,) + ad[k] for k in keys])
    (nA0, A0), (nB0, B0), (nA1, A1), (nB1, B1) = good
    out = []

    def add(label, code, recs, r=3, alpha=6, raw=None, **kw):
        path = os.path.join(dirname, "lora_%s.bin" % label)
        marks = write_ggla(path, r, alpha, recs, **kw)
        if raw is not None:
            with open(path, "rb") as f:
                whole = f.read()
            with open(path, "wb") as f:
                f.write(raw(whole, marks))
        out.append((label, path, code))
        return marks

    marks = add("good", 0, good)
    add("magic", E_MAGIC, good, magic=0x67676D6C)
    add("version", E_VERSION, good, version=2)
    add("r_zero", E_RANK, good, r=0)
    add("r_negative", E_RANK, good, r=-3)
    add("no_suffix", E_NOT_LORA, [("transformer.h.0.self_attention.dense.weight", A0), (nB0, B0)])
    add("suffix_c", E_NOT_LORA, [(nA0[:-1] + "C", A0), (nB0, B0)])
    add("unknown_name", E_UNKNOWN, [("transformer.h.0.self_attention.nothing.weight.loraA", A0), (nB0, B0)])
    add("norm_name", E_UNKNOWN, [("transformer.h.0.input_layernorm.weight.loraA", A0), (nB0, B0)])
    add("layer_out_of_range", E_UNKNOWN, [("transformer.h.%d.self_attention.dense.weight.loraA" % hp["n_layer"], A0), (nB0, B0)])
    add("ndims_1", E_NDIMS, good, raw=lambda b, m: b[:m[1]] + struct.pack("<i", 1) + b[m[1] + 4:])
    add("ndims_3", E_NDIMS, good, raw=lambda b, m: b[:m[0]] + struct.pack("<i", 3) + b[m[0] + 4:])
    add("ftype_2", E_FTYPE, good, raw=lambda b, m: b[:m[0] + 8] + struct.pack("<i", 2) + b[m[0] + 12:])
    add("wrong_k", E_SHAPE, [(nA0, A0[:-1]), (nB0, B0)] + good[2:])
    add("wrong_m", E_SHAPE, [(nA0, A0), (nB0, B0[:-1])] + good[2:])
    add("other_models_matrix", E_SHAPE, [(nA0, A1), (nB0, B1)])
    add("second_pair_wrong_m", E_SHAPE, good[:2] + [(nA1, A1), (nB1, B1[:-1])])      # (the reference would leave the first matrix patched)
    add("inner_differs", E_INNER, [(nA0, A0), (nB0, B0[:, :2])])
    add("only_a", E_UNPAIRED, [(nA0, A0)])
    add("only_b_after_pair", E_UNPAIRED, good[:2] + [(nB1, B1)])
    add("a_twice", E_UNPAIRED, [(nA0, A0), (nA0, A0), (nB0, B0)])
    add("interleaved", E_UNPAIRED, [(nA0, A0), (nA1, A1), (nB0, B0), (nB1, B1)])
    add("b_f16", E_TYPE_PAIR, [(nA0, A0), (nB0, B0.astype(np.float16))])
    add("both_f16", E_TYPE_PAIR, [(nA0, A0.astype(np.float16)), (nB0, B0.astype(np.float16))])
    add("name_len_huge", E_TRUNCATED, good, raw=lambda b, m: b[:m[0] + 4] + struct.pack("<i", 1 << 20) + b[m[0] + 8:])
    add("name_len_negative", E_TRUNCATED, good, raw=lambda b, m: b[:m[0] + 4] + struct.pack("<i", -1) + b[m[0] + 8:])
    add("ne_huge", E_TRUNCATED, good, raw=lambda b, m: b[:m[2] + 16] + struct.pack("<i", 0x7FFFFFFF) + b[m[2] + 20:])
    # truncation: inside the header, at every record boundary, inside a record's head, its name and its data
    whole = open(out[0][1], "rb").read()
    cuts = [(2, E_TRUNCATED), (6, E_TRUNCATED), (12, E_TRUNCATED), (marks[0], 0), (marks[1], E_UNPAIRED), (marks[2], 0), (marks[3], E_UNPAIRED)]
    for k in range(4):
        cuts += [(marks[k] + 7, E_TRUNCATED), (marks[k] + 19, E_TRUNCATED), (marks[k] + 30, E_TRUNCATED), ((marks[k] + marks[k + 1]) // 2, E_TRUNCATED), (marks[k + 1] - 1, E_TRUNCATED)]
    for n, code in cuts:
        path = os.path.join(dirname, "lora_cut_%d.bin" % n)
        with open(path, "wb") as f:
            f.write(whole[:n])
        out.append(("cut_%d" % n, path, code))
    out.append(("missing_file", os.path.join(dirname, "lora_is_not_there.bin"), E_IO))
    return out


# ------------------------------------------------------------------------------------------------ the real reference (only where oracle/_ref was built)
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libfalcon_ref.so")


class _Params(C.Structure):
    """falcon_context_params of the reference's build (LLAMA_MAX_DEVICES == 1)"""
    _fields_ = [(n, C.c_int) for n in ("n_ctx", "n_batch", "n_gpu_layers", "i_gpu_start", "i_gpu_last", "main_gpu")] + [("tensor_split", C.c_float * 1), ("seed", C.c_int)] + \
               [(n, C.c_bool) for n in ("f16_kv", "logits_all", "vocab_only", "use_mmap", "use_mlock", "embedding")] + [("progress_callback", C.c_void_p), ("progress_callback_user_data", C.c_void_p)]


class Reference:
    """the reference's library through its own exported symbols; the model is loaded WITHOUT mmap, so that the merge may write into it"""

    def __init__(self):
        L = self.L = C.CDLL(REF_SO)
        L.falcon_context_default_params.restype = _Params
        L.falcon_init_from_file.restype = C.c_void_p
        L.falcon_init_from_file.argtypes = [C.c_char_p, _Params]
        L.llama_apply_lora_from_file.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int]
        L.reff_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.reff_free.argtypes = [C.c_void_p]
        L.falcon_init_backend()

    def logits(self, model_path, n_vocab, tokens, n_prompt, adapter=None, base=None, n_ctx=32):
        """[len(tokens)][n_vocab]: a prompt of n_prompt tokens, then single-token steps; the adapter merged first"""
        p = self.L.falcon_context_default_params()
        p.n_ctx, p.n_batch, p.n_gpu_layers, p.seed = n_ctx, 16, 0, 1
        p.f16_kv, p.logits_all, p.use_mmap = False, True, False
        ctx = self.L.falcon_init_from_file(os.fsencode(model_path), p)
        assert ctx, model_path
        try:
            if adapter is not None:
                rc = self.L.llama_apply_lora_from_file(ctx, os.fsencode(adapter), os.fsencode(base) if base else None, 1)
                assert rc == 0, "the reference refused %s" % adapter
            tok = np.ascontiguousarray(tokens, np.int32)
            out = np.zeros((tok.size, n_vocab), np.float32)
            assert self.L.reff_eval(ctx, tok.ctypes.data, n_prompt, 0, 1, out.ctypes.data) == 0
            for i in range(n_prompt, tok.size):
                assert self.L.reff_eval(ctx, tok[i:].ctypes.data, 1, i, 1, out[i:].ctypes.data) == 0
            return out
        finally:
            self.L.reff_free(ctx)


# ------------------------------------------------------------------------------------------------ the recorded cases (tests/golden/lora.npz)
# name: (hparams, matrix type, r, alpha, targets, F16 loraA, loraB first, first target again at the end, base file: None | "f16" | "f32")
CASES = {
    "q4_0":          ("mqa", ob.Q4_0, 8, 16, [(0, "qkv"), (1, "up"), (1, "down"), "lm_head"], False, False, False, None),
    "q4_1":          ("mqa", ob.Q4_1, 1, 16, [(0, "wo"), (1, "qkv")], False, False, False, None),
    "q5_0":          ("gqa", ob.Q5_0, 3, 16, [(0, "down"), "tok_emb"], False, True, False, None),
    "q5_1":          ("gqa", ob.Q5_1, 40, 16, [(0, "qkv"), (1, "wo")], False, False, False, None),
    "q8_0":          ("mqa", ob.Q8_0, 16, 16, [(0, "up"), "lm_head"], False, False, False, None),          # scaling exactly 1: no multiply
    "q2_k":          ("gqa", ob.Q2_K, 3, 16, [(1, "qkv"), (1, "down")], False, False, False, None),
    "q3_k":          ("mqa", ob.Q3_K, 5, 16, [(0, "wo"), (1, "up")], True, False, False, None),
    "q4_k":          ("gqa", ob.Q4_K, 8, 32, [(0, "qkv"), "lm_head"], False, False, True, None),
    "q5_k":          ("mqa", ob.Q5_K, 5, 16, ["tok_emb", (1, "down")], False, False, False, None),
    "q6_k":          ("gqa", ob.Q6_K, 8, 16, [(0, "up"), (1, "wo")], False, False, False, None),
    "f16":           ("mqa", F16, 8, 16, [(0, "qkv"), (1, "down"), "lm_head"], False, False, False, None),
    "base_f16_q4_0": ("mqa", ob.Q4_0, 8, 16, [(0, "qkv"), (1, "up")], False, False, False, "f16"),
    "base_f16_q4_k": ("gqa", ob.Q4_K, 5, 16, [(0, "wo"), "lm_head"], False, False, False, "f16"),
    "base_f32_q5_1": ("mqa", ob.Q5_1, 3, 16, [(1, "down"), (0, "qkv")], False, False, False, "f32"),
}
MODEL_SEED, TOKEN_SEED, N_TOKENS, N_PROMPT = 4321, 77, 12, 9


def build_case(oracle, name, dirname=None):
    """everything of a recorded case from its seeds: dict(hp, wtype, weights, r, alpha, pairs [(key, A, B)], keys, base_weights, tokens) and -- with dirname --
    the files: model, adapter, base (or None)"""
    import ggcc_writer
    import synth
    which, wt, r, alpha, keys, a_f16, b_first, twice, base = CASES[name]
    hp = synth.HP_TINY_MQA if which == "mqa" else synth.HP_TINY_GQA
    weights = synth.make_model_float(hp, seed=MODEL_SEED, f16=True) if wt == F16 else synth.make_model(oracle, hp, wt, seed=MODEL_SEED)
    seed = 1 + sorted(CASES).index(name)
    ad = draw_adapter(hp, keys, r, seed=seed, a_f16=a_f16)
    pairs = [(k,) + ad[k] for k in keys]
    if twice:
        again = draw_adapter(hp, keys[:1], r, seed=seed + 500, a_f16=a_f16)
        pairs.append((keys[0],) + again[keys[0]])
    base_weights = None if base is None else synth.make_model_float(hp, seed=MODEL_SEED + 1, f16=base == "f16")
    c = dict(name=name, hp=hp, wtype=wt, weights=weights, r=r, alpha=alpha, pairs=pairs, keys=keys, base_weights=base_weights,
             tokens=synth.tokens(N_TOKENS, hp["n_vocab"], seed=TOKEN_SEED), model=None, adapter=None, base=None)
    if dirname is not None:
        c["model"], c["adapter"] = os.path.join(dirname, name + "_model.bin"), os.path.join(dirname, name + "_adapter.bin")
        ggcc_writer.write_ggcc(c["model"], weights)
        write_ggla(c["adapter"], r, alpha, adapter_records(pairs, b_first=b_first))
        if base_weights is not None:
            c["base"] = os.path.join(dirname, name + "_base.bin")
            ggcc_writer.write_ggcc(c["base"], base_weights)
    return c


def compose_case(c):
    return compose(c["weights"], c["pairs"], c["r"], c["alpha"], c["base_weights"])


def sha256_file(path):
    import hashlib
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def sha256_bytes(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

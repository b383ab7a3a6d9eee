"""Writes tests/golden/f16_models.npz: the REAL reference's logits (falcon_eval of libfalcon.cpp, scalar build: oracle/_ref/libfalcon_ref.so,
`make -C oracle ref_falcon`) on tiny F16 Falcon files written by tests/ggcc_writer.py -- an MQA model, a GQA model with two norms, and the MQA model
quantized to Q4_0 by the reference's falcon_model_quantize with the output tensor left F16. Host only; tests/test_gpu_f16_model.py reads the fixture.

    python scripts/gen_f16_golden.py
"""
import ctypes as C
import hashlib
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ggcc_writer  # noqa: E402
import synth  # noqa: E402

SEED, TOKEN_SEED, PPL_SEED = 1357, 78, 98
N_PROMPT, N_EXT, N_DECODE = 9, 3, 12
MODELS = (("mqa_f16", synth.HP_TINY_MQA, None), ("gqa_f16", synth.HP_TINY_GQA, None), ("mqa_q4_0_f16head", synth.HP_TINY_MQA, 2))


def ref_lib():
    so = os.path.join(ROOT, "oracle", "_ref", "libfalcon_ref.so")
    if not os.path.exists(so):
        return None
    L = C.CDLL(so)
    L.reff_load.restype = C.c_void_p; L.reff_load.argtypes = [C.c_char_p, C.c_int, C.c_int]
    L.reff_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.reff_free.argtypes = [C.c_void_p]
    L.reff_token_nll.restype = C.c_double; L.reff_token_nll.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.reff_quantize.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    return L


def write_source(path, hp):
    ggcc_writer.write_ggcc(path, synth.make_model_float(hp, seed=SEED, f16=True))


def run_reference(L, path, hp, tokens, ppl_stream=None):
    """the reference's logits for: a 9-token prompt (every row), 3 more tokens in one call, 12 single-token steps; optionally the perplexity loop
    (falcon_perplexity.cpp:28-124: chunks of n_ctx 32 in batches of 8) driven by hand over falcon_eval"""
    V = hp["n_vocab"]
    ctx = L.reff_load(os.fsencode(path), 64, 16)
    assert ctx, path
    out = {}

    def ev(tok, n_past):
        lg = np.zeros((len(tok), V), np.float32)
        assert L.reff_eval(ctx, np.ascontiguousarray(tok, np.int32).ctypes.data, len(tok), n_past, 1, lg.ctypes.data) == 0
        return lg
    out["prefill_logits"] = ev(tokens[:N_PROMPT], 0)
    out["ext_logits"] = ev(tokens[N_PROMPT:N_PROMPT + N_EXT], N_PROMPT)
    p0 = N_PROMPT + N_EXT
    out["decode_logits"] = np.concatenate([ev(tokens[i:i + 1], i) for i in range(p0, p0 + N_DECODE)])
    if ppl_stream is not None:
        n_ctx, n_batch = 32, 8
        nll, count = 0.0, 0
        for i in range(len(ppl_stream) // n_ctx):
            start = i * n_ctx
            lgs = np.concatenate([ev(ppl_stream[start + j * n_batch:start + (j + 1) * n_batch], j * n_batch) for j in range(n_ctx // n_batch)])
            for j in range(min(512, n_ctx // 2), n_ctx - 1):
                nll += L.reff_token_nll(lgs[j].ctypes.data, V, int(ppl_stream[start + j + 1]))
                count += 1
        out["ppl_nll"], out["ppl_count"] = np.float64(nll), np.int64(count)
    L.reff_free(ctx)
    return out


def sha(path):
    return np.frombuffer(hashlib.sha256(open(path, "rb").read()).digest(), np.uint8)


def main():
    L = ref_lib()
    if L is None:
        sys.exit("oracle/_ref/libfalcon_ref.so is not built (make -C oracle ref_falcon)")
    d = {}
    with tempfile.TemporaryDirectory() as td:
        for name, hp, ftype in MODELS:
            src = os.path.join(td, name + "_src.ggcc")
            write_source(src, hp)
            path = src
            if ftype is not None:                                  # falcon_quantize --leave-output-tensor
                path = os.path.join(td, name + ".ggcc")
                assert L.reff_quantize(os.fsencode(src), os.fsencode(path), ftype, 0, 0) == 0
            tokens = synth.tokens(N_PROMPT + N_EXT + N_DECODE, hp["n_vocab"], seed=TOKEN_SEED)
            stream = synth.tokens(3 * 32 + 5, hp["n_vocab"], seed=PPL_SEED) if name == "mqa_f16" else None
            d[f"{name}_sha256"] = sha(path)
            d[f"{name}_tokens"] = tokens
            if stream is not None:
                d[f"{name}_ppl_tokens"] = stream
            for k, v in run_reference(L, path, hp, tokens, stream).items():
                d[f"{name}_{k}"] = v
    out = os.path.join(ROOT, "tests", "golden", "f16_models.npz")
    np.savez_compressed(out, **d)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()

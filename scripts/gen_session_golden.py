"""Writes tests/golden/session.npz: session files of the REAL reference (llama_save_session_file of libfalcon.cpp, scalar build:
oracle/_ref/libfalcon_ref.so, `make -C oracle ref_falcon`) for the two tiny GGCC models the drop-in tests write (HP_TINY_MQA Q4_0 and HP_TINY_GQA
Q5_1, synth.make_model(..., seed=4321), the token lists of tests/golden/ggcc_models.npz). Per model: 9 tokens evaluated in one call, 3 single-token
steps, the session saved with those 12 tokens (context: n_ctx 32, seed 1, logits_all, f32 KV), then the logits of the next step. Host only; the
reference runs in a child process (its ggml_init owns process-wide state). tests/test_session_cpu.py and tests/test_gpu_session.py read the fixture.

    python scripts/gen_session_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

N_CTX, N_BATCH, N_PROMPT, N_STEPS = 32, 16, 9, 3
MODELS = (("mqa_q4_0", "HP_TINY_MQA", "Q4_0"), ("gqa_q5_1", "HP_TINY_GQA", "Q5_1"))

# argv: libfalcon_ref.so, model, n_vocab, n_ctx, n_batch, tokens.npy, session path, out.npz [, session to load instead of evaluating]
CHILD = r"""
import ctypes as C, sys, numpy as np
so, path, nv, n_ctx, n_batch, out = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[8]
toks = np.ascontiguousarray(np.load(sys.argv[6]), np.int32)
L = C.CDLL(so)
L.reff_load.restype = C.c_void_p; L.reff_load.argtypes = [C.c_char_p, C.c_int, C.c_int]
L.reff_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
L.reff_free.argtypes = [C.c_void_p]
L.llama_save_session_file.restype = C.c_bool; L.llama_save_session_file.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]
L.llama_load_session_file.restype = C.c_bool; L.llama_load_session_file.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_void_p]
L.llama_get_state_size.restype = C.c_size_t; L.llama_get_state_size.argtypes = [C.c_void_p]
ctx = L.reff_load(path.encode(), n_ctx, n_batch)
assert ctx
def ev(t, n_past):
    lg = np.zeros((len(t), nv), np.float32)
    assert L.reff_eval(ctx, t.ctypes.data, len(t), n_past, 1, lg.ctypes.data) == 0
    return lg
res = {}
if len(sys.argv) > 9:
    got, n = np.zeros(n_ctx, np.int32), C.c_size_t(0)
    res["loaded"] = np.int64(bool(L.llama_load_session_file(ctx, sys.argv[9].encode(), got.ctypes.data, n_ctx, C.byref(n))))
    res["tokens"] = got[:n.value]
    n_tok = int(n.value)
else:
    n_tok = 12
    ev(toks[:9], 0)
    for i in range(9, n_tok):
        ev(toks[i:i + 1], i)
    assert L.llama_save_session_file(ctx, sys.argv[7].encode(), toks.ctypes.data, n_tok)
res["state_size"] = np.int64(L.llama_get_state_size(ctx))
res["next_logits"] = ev(toks[n_tok:n_tok + 1], n_tok)[0]
np.savez(out, **res)
L.reff_free(ctx)
"""


def ref_so():
    return os.path.join(ROOT, "oracle", "_ref", "libfalcon_ref.so")


def run_child(td, model_path, n_vocab, tokens, session_path, load=None):
    """the child above; returns its result arrays"""
    script, toks, out = os.path.join(td, "child.py"), os.path.join(td, "toks.npy"), os.path.join(td, "out.npz")
    open(script, "w").write(CHILD)
    np.save(toks, np.ascontiguousarray(tokens, np.int32))
    cmd = [sys.executable, script, ref_so(), model_path, str(n_vocab), str(N_CTX), str(N_BATCH), toks, session_path, out]
    r = subprocess.run(cmd + ([load] if load else []), capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-3000:])
    return dict(np.load(out))


def main():
    if not os.path.exists(ref_so()):
        sys.exit("oracle/_ref/libfalcon_ref.so is not built (make -C oracle ref_falcon)")
    import ggcc_writer
    import synth
    from oracle import binding as ob
    ob.build_oracle()
    oracle = ob.Oracle()
    gg = np.load(os.path.join(ROOT, "tests", "golden", "ggcc_models.npz"))
    d = {}
    with tempfile.TemporaryDirectory() as td:
        for name, hp_name, t_name in MODELS:
            hp, t = getattr(synth, hp_name), getattr(ob, t_name)
            path, sess = os.path.join(td, name + ".ggcc"), os.path.join(td, name + ".session")
            ggcc_writer.write_ggcc(path, synth.make_model(oracle, hp, t, seed=4321))
            # (the fixture's 12 tokens, and one more for the step behind the session)
            tokens = np.concatenate([gg[f"{name}_tokens"].astype(np.int32)[:N_PROMPT + N_STEPS], synth.tokens(1, hp["n_vocab"], seed=13)])
            assert tokens.size == N_PROMPT + N_STEPS + 1
            res = run_child(td, path, hp["n_vocab"], tokens, sess)
            d[f"{name}_file"] = np.frombuffer(open(sess, "rb").read(), np.uint8)
            d[f"{name}_tokens"] = tokens
            d[f"{name}_next_logits"] = res["next_logits"]
            d[f"{name}_state_size"] = res["state_size"]
            # the reference loads what it wrote and continues with the same bits
            back = run_child(td, path, hp["n_vocab"], tokens, sess, load=sess)
            assert back["loaded"] == 1 and np.array_equal(back["tokens"], tokens[:N_PROMPT + N_STEPS])
            assert np.array_equal(back["next_logits"], res["next_logits"])
    d["n_ctx"] = np.int64(N_CTX)
    out = os.path.join(ROOT, "tests", "golden", "session.npz")
    np.savez_compressed(out, **d)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()

"""Writes tests/golden/embedding.npz: what the REAL reference (oracle/_ref/libfalcon_ref.so, `make -C oracle ref_falcon`, scalar build) keeps in
ctx->embedding for a context made with params.embedding (libfalcon.cpp:2409-2435, 2551-2557), read through falcon_get_embeddings, and one session
file per model that carries the row (libfalcon.cpp:4203-4267). Three tiny models from their seeds (synth.make_model(..., seed=4321)): HP_TINY_MQA
Q4_0, HP_TINY_GQA Q5_1, HP_TINY_GQA Q4_K. Per model: 9 tokens in one eval, then 3 single-token steps (n_ctx 32, n_batch 16, seed 1, logits_all,
f32 KV); the embedding after each of the 4 evals, the session saved after the last, the logits and the embedding of one more step, the tokens and
the model file's sha256. The reference keeps the last row only, so the rows of every position that the pooled vectors need come from the oracle,
which tests/test_embed_cpu.py pins on the recorded ones. The child asserts first that falcon_context_default_params() read through lora_ref's ctypes
mirror shows the defaults of libfalcon.cpp:1387-1405: that pins the mirror's layout, `embedding` included. Host only; the reference runs in a child
process (its ggml_init owns process-wide state).

    python tests/gen_embedding_golden.py
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
MODELS = (("mqa_q4_0", "HP_TINY_MQA", "Q4_0"), ("gqa_q5_1", "HP_TINY_GQA", "Q5_1"), ("gqa_q4_k", "HP_TINY_GQA", "Q4_K"))
MODEL_SEED, TOKEN_SEED = 4321, 2024

# argv: repository root, model, n_vocab, n_embd, tokens.npy, session path, out.npz
CHILD = r"""
import ctypes as C, os, sys, numpy as np
root, path, nv, ne, out = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[7]
sys.path[:0] = [root, os.path.join(root, "tests")]
import lora_ref
toks = np.ascontiguousarray(np.load(sys.argv[5]), np.int32)
R = lora_ref.Reference()
L = R.L
# the mirror's layout, pinned on the defaults of libfalcon.cpp:1387-1405
p = L.falcon_context_default_params()
got = (p.n_ctx, p.n_batch, p.n_gpu_layers, p.i_gpu_start, p.i_gpu_last, p.main_gpu, p.tensor_split[0], p.seed, p.f16_kv, p.logits_all, p.vocab_only,
       p.use_mmap, p.use_mlock, p.embedding, p.progress_callback, p.progress_callback_user_data)
assert got == (512, 512, 0, -1, -1, 0, 0.0, -1, False, False, False, True, False, False, None, None), got
p.n_ctx, p.n_batch, p.n_gpu_layers, p.seed = int(sys.argv[8]), int(sys.argv[9]), 0, 1
p.f16_kv, p.logits_all, p.use_mmap, p.embedding = False, True, True, True
L.falcon_get_embeddings.restype = C.POINTER(C.c_float); L.falcon_get_embeddings.argtypes = [C.c_void_p]
L.llama_save_session_file.restype = C.c_bool; L.llama_save_session_file.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]
ctx = L.falcon_init_from_file(os.fsencode(path), p)
assert ctx
def ev(t, n_past):
    lg = np.zeros((len(t), nv), np.float32)
    assert L.reff_eval(ctx, t.ctypes.data, len(t), n_past, 1, lg.ctypes.data) == 0
    return lg, np.ctypeslib.as_array(L.falcon_get_embeddings(ctx), (ne,)).copy()
n_prompt, n_tok = int(sys.argv[10]), toks.size - 1
rows = [ev(toks[:n_prompt], 0)[1]]
for i in range(n_prompt, n_tok):
    rows.append(ev(toks[i:i + 1], i)[1])
assert L.llama_save_session_file(ctx, os.fsencode(sys.argv[6]), toks.ctypes.data, n_tok)
lg, row = ev(toks[n_tok:n_tok + 1], n_tok)
np.savez(out, emb=np.stack(rows), next_logits=lg[0], next_emb=row)
L.reff_free(ctx)
"""


def ref_so():
    return os.path.join(ROOT, "oracle", "_ref", "libfalcon_ref.so")


def main():
    if not os.path.exists(ref_so()):
        sys.exit("oracle/_ref/libfalcon_ref.so is not built (make -C oracle ref_falcon)")
    import ggcc_writer
    import lora_ref
    import synth
    from oracle import binding as ob
    ob.build_oracle()
    oracle = ob.Oracle()
    d = {}
    with tempfile.TemporaryDirectory() as td:
        script = os.path.join(td, "child.py")
        open(script, "w").write(CHILD)
        for name, hp_name, t_name in MODELS:
            hp, t = getattr(synth, hp_name), getattr(ob, t_name)
            path, sess, toks, out = (os.path.join(td, name + e) for e in (".ggcc", ".session", "_toks.npy", "_out.npz"))
            ggcc_writer.write_ggcc(path, synth.make_model(oracle, hp, t, seed=MODEL_SEED))
            tokens = synth.tokens(N_PROMPT + N_STEPS + 1, hp["n_vocab"], seed=TOKEN_SEED).astype(np.int32)
            np.save(toks, tokens)
            r = subprocess.run([sys.executable, script, ROOT, path, str(hp["n_vocab"]), str(hp["n_embd"]), toks, sess, out, str(N_CTX), str(N_BATCH), str(N_PROMPT)],
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-3000:])
            res = np.load(out)
            assert res["emb"].shape == (1 + N_STEPS, hp["n_embd"]) and np.abs(res["emb"]).max() > 0
            d[f"{name}_emb"] = res["emb"]
            d[f"{name}_next_emb"] = res["next_emb"]
            d[f"{name}_next_logits"] = res["next_logits"]
            d[f"{name}_tokens"] = tokens
            d[f"{name}_model_sha256"] = np.array(lora_ref.sha256_file(path))
            d[f"{name}_file"] = np.frombuffer(open(sess, "rb").read(), np.uint8)
    d["n_ctx"], d["n_batch"], d["n_prompt"] = np.int64(N_CTX), np.int64(N_BATCH), np.int64(N_PROMPT)
    out = os.path.join(ROOT, "tests", "golden", "embedding.npz")
    np.savez_compressed(out, **d)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()

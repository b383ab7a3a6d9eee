"""measurement aid (GPU): what scoring costs on a Falcon-7B-shaped synthetic Q4_0 model, before and after the soft-max moved to the device.

    python scripts/gpu_score.py [--out profiles/score_7b.json] [--lib PARENT/ggllm.cpp_amd/libggml_hip.so] [--layers L] [--rounds R]

  (i)   seconds per chunk of falcon_hip_perplexity at n_ctx 2048 / n_batch 512 over 3 chunks (the second and third are reported; the
        first carries the one-time allocations) with this tree's library;
  (ii)  the same call against another build of the library (--lib: the parent commit's, built from a git worktree of it), same box, the
        two alternating A/B/A/B, every measurement in a fresh process; both sides go through the same few ctypes calls of this file
        (model_create / set_tensor / context_create / perplexity), so the harness is the same code for both;
  (iii) ggml_hip_score_rows alone for 512 rows of 65 024 next to the launch before it in the stream (the lm_head mat-mul of the same
        batch), from a `rocprofv3 --kernel-trace --stats` run of its own over falcon_hip_eval_score of 512 tokens (2 blocks: the
        lm_head and the scoring launch do not depend on the depth).
The blocks of the synthetic model share their host arrays (every block has its own copy in HBM)."""
import argparse
import ctypes as C
import glob
import json
import os
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ggllm_cpp_amd as g  # noqa: E402
from ggllm_cpp_amd import synth  # noqa: E402

N_CTX, N_BATCH, CHUNKS = 2048, 512, 3


def q4_model(n_layer, seed=1234):
    one = synth.make_model_fast(dict(synth.HP_7B, n_layer=1), g.Q4_0, seed=seed)
    one["hparams"] = dict(synth.HP_7B, n_layer=n_layer)
    one["layers"] = one["layers"] * n_layer
    return one


def child_ppl(lib_path, n_layer):
    """one process, one library: seconds of falcon_hip_perplexity per chunk"""
    L = C.CDLL(lib_path)
    vp = C.c_void_p
    L.falcon_hip_model_create.restype, L.falcon_hip_model_create.argtypes = vp, [vp]
    L.falcon_hip_model_set_tensor.restype, L.falcon_hip_model_set_tensor.argtypes = C.c_int, [vp, C.c_char_p, C.c_int, vp, C.c_int64, C.c_int64]
    L.falcon_hip_context_create.restype, L.falcon_hip_context_create.argtypes = vp, [vp, C.c_int, C.c_int, C.c_int]
    L.falcon_hip_perplexity.restype, L.falcon_hip_perplexity.argtypes = C.c_int, [vp, vp, C.c_int64, C.c_int, C.c_int, vp]
    L.falcon_hip_context_free.argtypes = [vp]
    L.falcon_hip_model_free.argtypes = [vp]
    L.ggml_hip_init.argtypes = [C.c_int]
    L.ggml_hip_init(0)
    w = q4_model(n_layer)
    hp, wt = w["hparams"], w["wtype"]
    E, H, HKV, FF, V = hp["n_embd"], hp["n_head"], hp["n_head_kv"], hp["n_ff"], hp["n_vocab"]
    chp = g.HParams(V, E, H, HKV, n_layer, FF, 0, 0, n_layer)
    m = L.falcon_hip_model_create(C.byref(chp))

    def put(name, t, arr, ne0, ne1):
        arr = np.ascontiguousarray(arr)
        assert L.falcon_hip_model_set_tensor(m, name.encode(), t, arr.ctypes.data, ne0, ne1) == 0, name

    put("transformer.word_embeddings.weight", wt, w["tok_emb"], E, V)
    put("lm_head.weight", wt, w["lm_head"], E, V)
    put("transformer.ln_f.weight", g.F32, w["out_norm_w"], E, 1)
    put("transformer.ln_f.bias", g.F32, w["out_norm_b"], E, 1)
    for i, lw in enumerate(w["layers"]):
        p = "transformer.h.%d." % i
        put(p + "self_attention.query_key_value.weight", wt, lw["qkv"], E, (H + 2 * HKV) * 64)
        put(p + "self_attention.dense.weight", wt, lw["wo"], E, E)
        put(p + "mlp.dense_h_to_4h.weight", wt, lw["up"], E, FF)
        put(p + "mlp.dense_4h_to_h.weight", wt, lw["down"], FF, E)
        for k, leaf in g.TENSOR_NAMES_7B.items():
            put(p + leaf, g.F32, lw[k], E, 1)
    ctx = L.falcon_hip_context_create(m, N_CTX, N_BATCH, 0)
    toks = synth.tokens(N_CTX * CHUNKS, V, seed=9)
    secs, nlls, count = [], [], 0
    for c in range(CHUNKS):                                  # (chunks are independent: each starts from an empty context)
        nll = C.c_double(0.0)
        chunk = np.ascontiguousarray(toks[c * N_CTX:(c + 1) * N_CTX])
        t0 = time.perf_counter()
        count = L.falcon_hip_perplexity(ctx, chunk.ctypes.data, chunk.size, N_CTX, N_BATCH, C.byref(nll))
        secs.append(time.perf_counter() - t0)
        nlls.append(nll.value.hex())
    L.falcon_hip_context_free(ctx)
    L.falcon_hip_model_free(m)
    print("RESULT " + json.dumps(dict(lib=lib_path, seconds_per_chunk=secs, scored_per_chunk=count, nll_hex=nlls)))


def child_kernel():
    """the process rocprofv3 traces: falcon_hip_eval_score of 512 tokens, every row scored"""
    g.init(0)
    m = g.FalconModel(q4_model(2), n_ctx=N_BATCH, n_batch=N_BATCH)
    toks = synth.tokens(N_BATCH, synth.HP_7B["n_vocab"], seed=9)
    tg = synth.tokens(N_BATCH, synth.HP_7B["n_vocab"], seed=10)
    for _ in range(4):
        p = m.score(toks, 0, tg)
    m.free()
    print("probs", float(p.min()), float(p.max()))


def run_child(args, timeout, prefix=()):
    r = subprocess.run(list(prefix) + [sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.exit("child %s failed (%d):\n%s" % (args, r.returncode, (r.stdout + r.stderr)[-3000:]))       # nothing more is started on the device
    return r.stdout


def trace_summary(db):
    """per k_score_rows dispatch of the trace: its duration and the dispatch before it in the stream"""
    cur = sqlite3.connect(db).cursor()
    rows = list(cur.execute("select name, start, end, grid_x, workgroup_x from kernels order by start"))
    score, before = [], []
    for i, r in enumerate(rows):
        if "k_score_rows" in r[0] and i > 0:
            score.append((r[2] - r[1]) / 1e3)
            before.append((rows[i - 1][0][:120], (rows[i - 1][2] - rows[i - 1][1]) / 1e3, rows[i - 1][3]))
    return dict(score_rows_us=score, score_rows_grid_threads=rows and [r[3] for r in rows if "k_score_rows" in r[0]][:1],
                launch_before_us=[b[1] for b in before], launch_before_name=sorted({b[0] for b in before}), launch_before_grid_threads=sorted({b[2] for b in before}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_7b.json"))
    ap.add_argument("--lib", default=None, help="another build of libggml_hip.so to compare with (the parent commit's)")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=2, help="A/B rounds")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child == "ppl":
        return child_ppl(a.lib or g.LIB_PATH, a.layers)
    if a.child == "kernel":
        return child_kernel()

    res = dict(model="Falcon-7B shape, %d blocks, Q4_0, synthetic" % a.layers, n_ctx=N_CTX, n_batch=N_BATCH, chunks=CHUNKS, runs=[])
    order = ([("this", g.LIB_PATH)] + ([("parent", os.path.abspath(a.lib))] if a.lib else [])) * a.rounds
    for tag, lib in order:
        out = run_child(["--child", "ppl", "--lib", lib, "--layers", str(a.layers)], 600)
        line = [x for x in out.splitlines() if x.startswith("RESULT ")][-1]
        res["runs"].append(dict(json.loads(line[7:]), build=tag))
        print(tag, res["runs"][-1]["seconds_per_chunk"], flush=True)
    for tag in ("this", "parent"):
        xs = [s for r in res["runs"] if r["build"] == tag for s in r["seconds_per_chunk"][1:]]
        if xs:
            res[tag + "_seconds_per_chunk"] = dict(median=float(np.median(xs)), min=min(xs), max=max(xs), samples=xs)
    if a.lib:
        res["same_nll_bits"] = len({tuple(r["nll_hex"]) for r in res["runs"]}) == 1
        res["speedup"] = res["parent_seconds_per_chunk"]["median"] / res["this_seconds_per_chunk"]["median"]
    if not a.no_trace:
        with tempfile.TemporaryDirectory() as d:
            run_child(["--child", "kernel"], 600, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "trace", "--"])
            dbs = glob.glob(os.path.join(d, "**", "*results.db"), recursive=True)
            if not dbs:
                sys.exit("rocprofv3 left no result database")
            res["trace"] = trace_summary(dbs[0])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

"""measurement aid (GPU): what classifier-free guidance costs the sampled decode loops on Falcon-7B Q4_0 (synthetic weights), n_ctx 2048,
through the graph (one replay per step).

    python scripts/gpu_guide.py [--out profiles/guide_7b.json] [--lib PARENT/ggllm.cpp_amd/libggml_hip.so] [--steps S] [--reps R]

  parent   (--lib: another build of libggml_hip.so, the parent commit's) ms per step of falcon_hip_decode_sample_seqs on a two-sequence
           lock-step context with no pair set: that library beside TWO workers of this tree's library, the three taking turns
           (parent, this_a, this_b, parent, ...), every sample a fresh process through the same few ctypes calls of this file. The
           difference between this_a and this_b is the run's own A/A spread;
  loops    in one process, the settings taking turns, R samples each, every sample a warmed call of S steps: the single-stream sampled
           step (falcon_hip_decode_sample), the two-sequence sampled step with no pair, and the same step with one pair (scale 1.5);
  kernel   ggml_hip_guide_rows alone at n_vocab 65 024 for 1, 2 and 8 pairs next to a device-to-device copy of the same two rows per
           pair: microseconds per launch between two device events around 20 back-to-back launches, the median of 5."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ggllm_cpp_amd as g  # noqa: E402
from ggllm_cpp_amd import synth  # noqa: E402

N_CTX = 2048
FIRST, POS = [11, 23], [64, 80]


def stats(v):
    return {"samples": v, "median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def timed(f, steps):
    f()
    t0 = time.perf_counter()
    f()                                                   # (ends in a stream synchronise: the tokens come back)
    return (time.perf_counter() - t0) / steps * 1e3


def measure_loops(model, hp, S, R):
    hist = [int(t) for t in synth.tokens(64, hp["n_vocab"], seed=3)]
    model.set_sampling(g.sampling(seed=7), hist)
    sc = g.SeqContext(model, N_CTX, 2)
    for t in range(2):
        sc.set_sampling(t, g.sampling(seed=100 + t), hist)
    runs = {"single": [], "two_no_pair": [], "two_one_pair": [], "two_no_pair_again": []}
    for _ in range(R):
        runs["single"].append(timed(lambda: model.decode_sample(FIRST[0], POS[0], S, use_graph=True), S))
        runs["two_no_pair"].append(timed(lambda: sc.decode_sample(FIRST, POS, S, use_graph=True), S))
        sc.set_guidance(0, 1, 1.5)
        runs["two_one_pair"].append(timed(lambda: sc.decode_sample(FIRST, POS, S, use_graph=True), S))
        sc.set_guidance(0, None)
        runs["two_no_pair_again"].append(timed(lambda: sc.decode_sample(FIRST, POS, S, use_graph=True), S))
    sc.free()
    res = {"ms_per_step": {k: stats(v) for k, v in runs.items()}}
    med = {k: res["ms_per_step"][k]["median"] for k in runs}
    res["pair_over_no_pair_us"] = (med["two_one_pair"] - med["two_no_pair"]) * 1e3
    res["no_pair_a_a_us"] = (med["two_no_pair_again"] - med["two_no_pair"]) * 1e3
    res["guided_over_single_us"] = (med["two_one_pair"] - med["single"]) * 1e3
    res["guided_over_single_ratio"] = med["two_one_pair"] / med["single"]
    return res


def measure_kernel(L, V, pairs_list, launches=20, reps=5):
    out = {}
    rng = np.random.default_rng(65024)
    for P in pairs_list:
        lg = g.DevBuf(host=(rng.standard_normal((2 * P, V)) * 8.0).astype(np.float32))
        ld, gd = g.DevBuf(host=np.arange(0, 2 * P, 2, dtype=np.int32)), g.DevBuf(host=np.arange(1, 2 * P, 2, dtype=np.int32))
        sc, mx, cp = g.DevBuf(host=np.full(P, 1.5, np.float32)), g.DevBuf(nbytes=P * V * 4), g.DevBuf(nbytes=2 * P * V * 4)
        e0, e1 = L.ggml_hip_event_create(), L.ggml_hip_event_create()

        def us(f):
            v = []
            for _ in range(reps + 1):
                L.ggml_hip_event_record(e0)
                for _ in range(launches):
                    f()
                L.ggml_hip_event_record(e1)
                v.append(L.ggml_hip_event_elapsed_ms(e0, e1) / launches * 1e3)
            return stats(v[1:])                           # (the first round warms up)
        out["pairs_%d_us_per_launch" % P] = {"guide_rows": us(lambda: g.guide_rows(lg, V, V, P, ld, gd, sc, mx, V)),
                                             "copy_d2d_same_rows": us(lambda: L.ggml_hip_memcpy_d2d(cp.ptr, lg.ptr, 2 * P * V * 4))}
        for e in (e0, e1):
            L.ggml_hip_event_destroy(e)
        for b in (lg, ld, gd, sc, mx, cp):
            b.free()
    return out


def child_seqs(lib_path, S, R):
    """one process, one library, plain ctypes: ms per step of falcon_hip_decode_sample_seqs on two sequences, no pair (default chain, hipGraph)"""
    L = C.CDLL(lib_path)
    vp = C.c_void_p
    L.falcon_hip_model_create.restype, L.falcon_hip_model_create.argtypes = vp, [vp]
    L.falcon_hip_model_set_tensor.restype, L.falcon_hip_model_set_tensor.argtypes = C.c_int, [vp, C.c_char_p, C.c_int, vp, C.c_int64, C.c_int64]
    L.falcon_hip_context_create_seqs.restype, L.falcon_hip_context_create_seqs.argtypes = vp, [vp, C.c_int, C.c_int, C.c_int]
    L.falcon_hip_context_set_sampling.restype, L.falcon_hip_context_set_sampling.argtypes = C.c_int, [vp, C.c_int, C.POINTER(g.Sampling), vp, C.c_int]
    L.falcon_hip_decode_sample_seqs.restype, L.falcon_hip_decode_sample_seqs.argtypes = C.c_int, [vp, vp, vp, C.c_int, vp]
    L.falcon_hip_context_use_graph.argtypes = [vp, C.c_int]
    L.falcon_hip_context_free.argtypes = [vp]
    L.falcon_hip_model_free.argtypes = [vp]
    L.ggml_hip_init.argtypes = [C.c_int]
    L.ggml_hip_init(0)
    hp = dict(synth.HP_7B)
    w = synth.make_model_fast(hp, g.Q4_0, seed=1234)
    wt = w["wtype"]
    E, H, HKV, FF, V, NL = hp["n_embd"], hp["n_head"], hp["n_head_kv"], hp["n_ff"], hp["n_vocab"], hp["n_layer"]
    chp = g.HParams(V, E, H, HKV, NL, FF, 0, 0, NL)
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
    ctx = L.falcon_hip_context_create_seqs(m, N_CTX, 2, 0)
    hist = np.ascontiguousarray(synth.tokens(64, V, seed=3), np.int32)
    for t in range(2):
        par = g.sampling(seed=100 + t)
        assert L.falcon_hip_context_set_sampling(ctx, t, C.byref(par), hist.ctypes.data, hist.size) == 0
    L.falcon_hip_context_use_graph(ctx, 1)
    first, pos = np.array(FIRST, np.int32), np.array(POS, np.int32)
    out = np.zeros((S, 2), np.int32)
    ms = []
    for r in range(R + 1):
        t0 = time.perf_counter()
        assert L.falcon_hip_decode_sample_seqs(ctx, first.ctypes.data, pos.ctypes.data, S, out.ctypes.data) == 0
        ms.append((time.perf_counter() - t0) / S * 1e3)
    L.falcon_hip_context_free(ctx)
    L.falcon_hip_model_free(m)
    # (each call continues the rows' generators: every build makes the same calls, so the last call's tokens are the ones they must agree on)
    print("RESULT " + json.dumps(dict(lib=lib_path, ms_per_step=ms[1:], tokens=out.tolist())))


def run_child(args, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.exit("child %s failed (%d):\n%s" % (args, r.returncode, (r.stdout + r.stderr)[-3000:]))       # nothing more is started on the device
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guide_7b.json"))
    ap.add_argument("--lib", default=None, help="another build of libggml_hip.so to compare with (the parent commit's)")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=1, help="rounds of parent / this_a / this_b processes")
    ap.add_argument("--kernel-only", action="store_true", help="the kernel section alone, printed and not written")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child == "seqs":
        return child_seqs(a.lib or g.LIB_PATH, a.steps, a.reps)

    res = {"model": "falcon-7b q4_0 (synthetic)", "n_ctx": N_CTX, "steps": a.steps, "reps": a.reps}
    if a.lib:                                             # (first: fresh processes, before this one holds the model)
        runs = []
        for tag, lib in [("parent", os.path.abspath(a.lib)), ("this_a", g.LIB_PATH), ("this_b", g.LIB_PATH)] * a.rounds:
            out = run_child(["--child", "seqs", "--lib", lib, "--steps", str(a.steps), "--reps", str(a.reps)], 600)
            runs.append(dict(json.loads([x for x in out.splitlines() if x.startswith("RESULT ")][-1][7:]), build=tag))
            print(tag, runs[-1]["ms_per_step"], flush=True)
        par = {"same_tokens": len({json.dumps(r["tokens"]) for r in runs}) == 1}
        for tag in ("parent", "this_a", "this_b"):
            par[tag + "_ms_per_step"] = stats([x for r in runs if r["build"] == tag for x in r["ms_per_step"]])
        med = {tag: par[tag + "_ms_per_step"]["median"] for tag in ("parent", "this_a", "this_b")}
        par["this_a_over_parent"] = med["this_a"] / med["parent"]
        par["this_b_over_parent"] = med["this_b"] / med["parent"]
        par["this_b_over_this_a"] = med["this_b"] / med["this_a"]
        res["two_seq_no_pair_against_parent"] = par
    g.init(0)
    L = g.load()
    hp = dict(synth.HP_7B)
    res["kernel"] = measure_kernel(L, hp["n_vocab"], [1, 2, 8])
    print(json.dumps(res["kernel"]), flush=True)
    if a.kernel_only:
        return
    w = synth.make_model_fast(hp, g.Q4_0, seed=1234)
    model = g.FalconModel(w, n_ctx=N_CTX, n_batch=1)
    del w
    res.update(measure_loops(model, hp, a.steps, a.reps))
    model.free()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

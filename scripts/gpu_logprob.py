"""measurement aid (GPU): what log-probabilities cost the sampled decode loops on Falcon-7B Q4_0 (synthetic weights), n_ctx 2048.

    python scripts/gpu_logprob.py [--out profiles/logprob_7b.json] [--lib PARENT/ggllm.cpp_amd/libggml_hip.so] [--steps S] [--reps R]

  single   ms per token of falcon_hip_decode_sample (hipGraph, one replay per step, the default chain) with logprobs off, 0, 5 and 32;
  seqs     ms per pass of falcon_hip_decode_sample_seqs with 16 and with 256 sequences (positions spread over [0, 512)), same settings;
           the settings are interleaved off / 0 / 5 / 32 / off / ... in one process, R rounds, each sample a warmed call of S steps;
           "off" is measured twice per round (off, off2): the spread between the two is the run's own A/A spread;
  kernel   ggml_hip_logprob_rows alone (n_top 0, 5, 32) next to ggml_hip_score_rows on the same 1, 16 and 256 rows of 65 024 logits:
           microseconds per launch between two device events around 20 back-to-back launches, the median of 5;
  parent   (--lib: another build of libggml_hip.so, the parent commit's) ms per token of falcon_hip_decode_sample with this tree's
           library (logprobs off) and with that one, alternating A/B/A/B, every measurement in a fresh process through the same few
           ctypes calls of this file, so the harness is the same code for both."""
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
SETTINGS = (("off", -1), ("lp0", 0), ("lp5", 5), ("lp32", 32), ("off2", -1))


def stats(v):
    return {"samples": v, "median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def timed(f, steps):
    f()
    t0 = time.perf_counter()
    f()                                                   # (ends in a stream synchronise: the tokens come back)
    return (time.perf_counter() - t0) / steps * 1e3


def measure_loops(model, hp, S, R, batches):
    hist = [int(t) for t in synth.tokens(64, hp["n_vocab"], seed=3)]
    res = {}
    model.set_sampling(g.sampling(seed=7), hist)
    single = {k: [] for k, _ in SETTINGS}
    for _ in range(R):
        for k, n in SETTINGS:
            model.set_logprobs(n)
            single[k].append(timed(lambda: model.decode_sample(11, 64, S, use_graph=True), S))
    model.set_logprobs(-1)
    res["single_ms_per_token"] = {k: stats(v) for k, v in single.items()}
    for B in batches:
        sc = g.SeqContext(model, N_CTX, B)
        tok = synth.tokens(B, hp["n_vocab"], seed=42)
        pos = np.linspace(0, 512 - S - 1, B).astype(np.int32)
        for t in range(B):
            sc.set_sampling(t, g.sampling(seed=100 + t), hist)
        seqs = {k: [] for k, _ in SETTINGS}
        for _ in range(R):
            for k, n in SETTINGS:
                sc.set_logprobs(n)
                seqs[k].append(timed(lambda: sc.decode_sample(tok, pos, S, use_graph=True), S))
        sc.free()
        res["seqs_%d_ms_per_pass" % B] = {k: stats(v) for k, v in seqs.items()}
    for key, v in list(res.items()):
        off = v["off"]["median"]
        res[key + "_added_us"] = {k: (v[k]["median"] - off) * 1e3 for k in ("lp0", "lp5", "lp32", "off2")}
    return res


def measure_kernel(L, V, rows_list, launches=20, reps=5):
    out = {}
    rng = np.random.default_rng(65024)
    for R in rows_list:
        lg = g.DevBuf(host=(rng.standard_normal((R, V)) * 8.0).astype(np.float32))
        ch = g.DevBuf(host=rng.integers(0, V, R).astype(np.int32))
        pb, ib, tb = g.DevBuf(nbytes=R * 4), g.DevBuf(nbytes=R * 32 * 4), g.DevBuf(nbytes=R * 32 * 4)
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
        r = {"score_rows": us(lambda: L.ggml_hip_score_rows(lg.ptr, V, R, V, ch.ptr, pb.ptr, None, None))}
        for n in (0, 5, 32):
            r["logprob_rows_top%d" % n] = us(lambda: g.logprob_rows(lg, V, R, V, ch, n, pb, ib, tb))
        out["rows_%d_us_per_launch" % R] = r
        for e in (e0, e1):
            L.ggml_hip_event_destroy(e)
        for b in (lg, ch, pb, ib, tb):
            b.free()
    return out


def child_decode(lib_path, S, R):
    """one process, one library, plain ctypes: ms per token of falcon_hip_decode_sample (default chain, hipGraph)"""
    L = C.CDLL(lib_path)
    vp = C.c_void_p
    L.falcon_hip_model_create.restype, L.falcon_hip_model_create.argtypes = vp, [vp]
    L.falcon_hip_model_set_tensor.restype, L.falcon_hip_model_set_tensor.argtypes = C.c_int, [vp, C.c_char_p, C.c_int, vp, C.c_int64, C.c_int64]
    L.falcon_hip_context_create.restype, L.falcon_hip_context_create.argtypes = vp, [vp, C.c_int, C.c_int, C.c_int]
    L.falcon_hip_context_set_sampling.restype, L.falcon_hip_context_set_sampling.argtypes = C.c_int, [vp, C.c_int, C.POINTER(g.Sampling), vp, C.c_int]
    L.falcon_hip_decode_sample.restype, L.falcon_hip_decode_sample.argtypes = C.c_int, [vp, C.c_int32, C.c_int, C.c_int, vp]
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
    ctx = L.falcon_hip_context_create(m, N_CTX, 1, 0)
    hist = np.ascontiguousarray(synth.tokens(64, V, seed=3), np.int32)
    par = g.sampling(seed=7)
    assert L.falcon_hip_context_set_sampling(ctx, 0, C.byref(par), hist.ctypes.data, hist.size) == 0
    L.falcon_hip_context_use_graph(ctx, 1)
    out = np.zeros(S, np.int32)
    ms = []
    for r in range(R + 1):
        t0 = time.perf_counter()
        assert L.falcon_hip_decode_sample(ctx, 11, 64, S, out.ctypes.data) == 0
        ms.append((time.perf_counter() - t0) / S * 1e3)
    L.falcon_hip_context_free(ctx)
    L.falcon_hip_model_free(m)
    print("RESULT " + json.dumps(dict(lib=lib_path, ms_per_token=ms[1:], tokens=out.tolist())))


def run_child(args, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.exit("child %s failed (%d):\n%s" % (args, r.returncode, (r.stdout + r.stderr)[-3000:]))       # nothing more is started on the device
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logprob_7b.json"))
    ap.add_argument("--lib", default=None, help="another build of libggml_hip.so to compare with (the parent commit's)")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="A/B rounds of the parent comparison")
    ap.add_argument("--batches", default="16,256")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child == "decode":
        return child_decode(a.lib or g.LIB_PATH, a.steps, a.reps)

    res = {"model": "falcon-7b q4_0 (synthetic)", "n_ctx": N_CTX, "steps": a.steps, "reps": a.reps}
    if a.lib:                                             # (first: fresh processes, before this one holds the model)
        runs = []
        for tag, lib in [("this", g.LIB_PATH), ("parent", os.path.abspath(a.lib))] * a.rounds:
            out = run_child(["--child", "decode", "--lib", lib, "--steps", str(a.steps), "--reps", str(a.reps)], 600)
            runs.append(dict(json.loads([x for x in out.splitlines() if x.startswith("RESULT ")][-1][7:]), build=tag))
            print(tag, runs[-1]["ms_per_token"], flush=True)
        par = {"same_tokens": len({tuple(r["tokens"]) for r in runs}) == 1}
        for tag in ("this", "parent"):
            par[tag + "_ms_per_token"] = stats([x for r in runs if r["build"] == tag for x in r["ms_per_token"]])
            par[tag + "_per_process_median"] = [float(np.median(r["ms_per_token"])) for r in runs if r["build"] == tag]
        par["this_over_parent"] = par["this_ms_per_token"]["median"] / par["parent_ms_per_token"]["median"]
        res["off_against_parent"] = par
    g.init(0)
    L = g.load()
    hp = dict(synth.HP_7B)
    res["kernel"] = measure_kernel(L, hp["n_vocab"], [1, 16, 256])
    print(json.dumps(res["kernel"]), flush=True)
    w = synth.make_model_fast(hp, g.Q4_0, seed=1234)
    model = g.FalconModel(w, n_ctx=N_CTX, n_batch=1)
    del w
    res.update(measure_loops(model, hp, a.steps, a.reps, [int(b) for b in a.batches.split(",") if b]))
    model.free()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

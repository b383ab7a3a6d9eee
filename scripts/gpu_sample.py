"""measurement aid (GPU): sampled decode (falcon_main's default chain on the device) against greedy decode on Falcon-7B Q4_0
(synthetic weights), n_ctx 2048.

    python scripts/gpu_sample.py [--out FILE.json] [--steps S] [--reps R] [--batch B]

  single        ms per token of falcon_hip_decode_greedy and falcon_hip_decode_sample (hipGraph, one replay per step) with the
                default chain (top_k 40, top_p 0.95, temp 0.8, repeat_penalty 1.1 over 64 tokens), and with top_k <= 0 (the whole
                vocabulary through the HBM sort) at top_p 0.95
  seqs          ms per pass of falcon_hip_decode_greedy_seqs and falcon_hip_decode_sample_seqs with B sequences (positions
                spread over [0, 512))
  host          for comparison: B rows per step through the reference's own functions on the host, driven from Python (tests/sample_ref.py:
                a numpy candidate array and one ctypes call per function per row, so the figure includes that Python cost; the
                rows' copy to the host is excluded), when oracle/_ref/libfalcon_ref.so is present
Modes are interleaved, R rounds each; medians are reported beside every sample."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ggllm_cpp_amd as g  # noqa: E402
from ggllm_cpp_amd import synth  # noqa: E402

N_CTX = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()
    g.init(0)
    L = g.load()
    hp = dict(synth.HP_7B)
    w = synth.make_model_fast(hp, g.Q4_0, seed=1234)
    model = g.FalconModel(w, n_ctx=N_CTX, n_batch=1)
    del w
    S, R, B = a.steps, a.reps, a.batch
    default = g.sampling(seed=7)
    whole = g.sampling(top_k=0, seed=7)
    hist = [int(t) for t in synth.tokens(64, hp["n_vocab"], seed=3)]

    def t_single(mode):
        if mode == "greedy":
            f = lambda: model.decode_greedy(11, 64, S, use_graph=True)  # noqa: E731
        else:
            model.set_sampling(default if mode == "sample" else whole, hist)
            f = lambda: model.decode_sample(11, 64, S, use_graph=True)  # noqa: E731
        f()
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) / S * 1e3

    single = {m: [] for m in ("greedy", "sample", "sample_whole_vocab")}
    for _ in range(R):
        for m in single:
            single[m].append(t_single(m))
    res = {"model": "falcon-7b q4_0 (synthetic)", "n_ctx": N_CTX, "steps": S, "reps": R,
           "single_ms": {m: {"samples": v, "median": float(np.median(v))} for m, v in single.items()}}
    res["single_tok_s"] = {m: 1e3 / res["single_ms"][m]["median"] for m in single}
    res["single_sample_over_greedy_tok_s"] = res["single_tok_s"]["sample"] / res["single_tok_s"]["greedy"]

    sc = g.SeqContext(model, N_CTX, B)
    tok = synth.tokens(B, hp["n_vocab"], seed=42)
    pos = np.linspace(0, 512 - S - 1, B).astype(np.int32)
    for t in range(B):
        sc.set_sampling(t, g.sampling(seed=100 + t), hist)

    def t_seqs(mode):
        f = (lambda: sc.decode_greedy(tok, pos, S, use_graph=True)) if mode == "greedy" else (lambda: sc.decode_sample(tok, pos, S, use_graph=True))
        f()
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) / S * 1e3

    seqs = {m: [] for m in ("greedy", "sample")}
    for _ in range(R):
        for m in seqs:
            seqs[m].append(t_seqs(m))
    res["seqs"] = {"batch": B, "ms_per_pass": {m: {"samples": v, "median": float(np.median(v))} for m, v in seqs.items()}}
    res["seqs"]["sample_over_greedy_pass"] = res["seqs"]["ms_per_pass"]["sample"]["median"] / res["seqs"]["ms_per_pass"]["greedy"]["median"]

    import sample_ref
    if os.path.exists(sample_ref.REF_SO):
        lg = sc.eval(tok, pos)
        ref = sample_ref.RefSampler(sample_ref.tiny_ggcc(os.path.join(os.environ.get("TMPDIR", "/tmp"), "gpu_sample_tiny.ggcc")))
        ref.seed(7)
        win = g.sampling_window(hist, N_CTX, 64)
        t0 = time.perf_counter()
        for t in range(B):
            ref.draw(lg[t], default, win)
        res["host_reference_ms_per_step"] = {"rows": B, "ms": (time.perf_counter() - t0) * 1e3}
        ref.free()
    sc.free()
    model.free()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""measurement aid (GPU): ragged lock-step decode against uniform lock-step passes on Falcon-7B Q4_0 (synthetic weights), n_ctx 2048.

    python scripts/gpu_ragged_seqs.py [--out FILE.json] [--steps S] [--reps R]

Per-pass milliseconds for B sequences per pass and a position range P:
  ragged        falcon_hip_decode_greedy_seqs (hipGraph) with the B positions spread evenly over [0, P - S)
  max / mean    the same call with every position at the ragged batch's largest / mean position (uniform passes)
  pipe_max / pipe_mean   the uniform passes through the existing Pipeline world-1 path (falcon_hip_pipeline_run)
A ragged pass does a subset of the uniform-at-max pass's work (each row reads only its own keys). The modes are interleaved,
R rounds of each (A/B/A/B); the median per mode is reported beside every sample."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ggllm_cpp_amd as g  # noqa: E402
from ggllm_cpp_amd import synth  # noqa: E402

N_CTX = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="16,64,256")
    ap.add_argument("--ranges", default="512,2048")
    a = ap.parse_args()
    g.init(0)
    L = g.load()
    hp = dict(synth.HP_7B)
    w = synth.make_model_fast(hp, g.Q4_0, seed=1234)
    model = g.FalconModel(w, n_ctx=16, n_batch=1)
    del w
    S = a.steps
    rows = []
    for B in [int(x) for x in a.batches.split(",")]:
        sc = g.SeqContext(model, N_CTX, B)
        pipe = g.Pipeline(model, 0, 1, 1, B, N_CTX)
        tok = synth.tokens(B, hp["n_vocab"], seed=42)
        pipe.set_tokens(tok)

        def seqs(pos):
            sc.decode_greedy(tok, pos, S, use_graph=True)              # warm-up (and capture) at the same positions
            t0 = time.perf_counter()
            sc.decode_greedy(tok, pos, S, use_graph=True)
            return (time.perf_counter() - t0) / S * 1e3

        def piped(p0):
            pipe.run(S, p0)
            L.ggml_hip_synchronize()
            t0 = time.perf_counter()
            pipe.run(S, p0)
            L.ggml_hip_synchronize()
            return (time.perf_counter() - t0) / S * 1e3

        for P in [int(x) for x in a.ranges.split(",")]:
            ragged = np.array([(t * (P - S)) // B for t in range(B)], np.int32)        # evenly over [0, P - S)
            mx, mean = int(ragged.max()), int(round(float(ragged.mean())))
            modes = {"ragged": lambda: seqs(ragged), "max": lambda: seqs(np.full(B, mx, np.int32)), "mean": lambda: seqs(np.full(B, mean, np.int32)),
                     "pipe_max": lambda: piped(mx), "pipe_mean": lambda: piped(mean)}
            samples = {k: [] for k in modes}
            for _ in range(a.reps):
                for k, f in modes.items():
                    samples[k].append(round(f(), 4))
            med = {k: float(np.median(v)) for k, v in samples.items()}
            row = dict(B=B, P=P, steps=S, positions=dict(min=int(ragged.min()), max=mx, mean=mean), ms_per_pass=med, samples_ms=samples,
                       ragged_over_max=round(med["ragged"] / med["max"], 4), ragged_over_mean=round(med["ragged"] / med["mean"], 4),
                       seqs_over_pipe_at_max=round(med["max"] / med["pipe_max"], 4), seqs_over_pipe_at_mean=round(med["mean"] / med["pipe_mean"], 4))
            rows.append(row)
            print(json.dumps(row), flush=True)
        pipe.free()
        sc.free()
    model.free()
    res = dict(workload="Falcon-7B Q4_0 (synth.make_model_fast seed 1234), n_ctx %d, %d greedy steps per timed call, median of %d interleaved rounds" % (N_CTX, S, a.reps),
               rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

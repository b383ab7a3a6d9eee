"""measurement aid (GPU): falcon_hip_decode_sample on Falcon-7B Q4_0 (synthetic weights, n_ctx 2048) through the graph with each
of falcon_main's sampling branches, and the default chain against another build of the library (the parent commit's).

    python scripts/gpu_sample_chain.py [--out FILE.json] [--steps S] [--reps R] [--parent-tree DIR]

  default        top_k 40, top_p 0.95, temp 0.8, repeat_penalty 1.1 over 64 tokens (set through set_sampling: the kernel's
                 default instantiation)
  tfs_typical    the same with tfs_z 0.95 and typical_p 0.9 at top_k 40 (set_sampling_ext: the EXT instantiation, LDS form)
  whole_vocab    top_k 0, top_p 0.95: the whole-row HBM sort the default chain already pays there -- what mirostat's cost stands beside
  mirostat1 / 2  tau 5, eta 0.1 (the HBM sort, then the scalar tail of csrc/fq_sample_chain.h)
Every series runs in a worker process of its own holding its own copy of the model; the coordinator asks the workers for one
sample at a time, in turn, so the series are interleaved. Two workers of THIS tree measure the default chain (A and A': their
medians' difference is the run's A/A spread); with --parent-tree DIR (a checkout of the parent commit with its library built) a
third measures the default chain of that build. Medians are reported beside every sample."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CTX = 2048
MODES = ("default", "tfs_typical", "whole_vocab", "mirostat1", "mirostat2")


def worker(steps):
    """reads mode names from stdin, answers each with ms per token of one timed decode_sample call (after an untimed one)"""
    sys.path.insert(0, os.environ["GPU_SAMPLE_CHAIN_TREE"])
    import ggllm_cpp_amd as g
    from ggllm_cpp_amd import synth
    g.init(0)
    hp = dict(synth.HP_7B)
    w = synth.make_model_fast(hp, g.Q4_0, seed=1234)
    model = g.FalconModel(w, n_ctx=N_CTX, n_batch=1)
    del w
    hist = [int(t) for t in synth.tokens(64, hp["n_vocab"], seed=3)]

    def setup(mode):
        if mode == "default":
            model.set_sampling(g.sampling(seed=7), hist)
        elif mode == "whole_vocab":
            model.set_sampling(g.sampling(top_k=0, seed=7), hist)
        elif mode == "tfs_typical":
            model.set_sampling_ext(g.sampling_ext(tfs_z=0.95, typical_p=0.9, seed=7), hist)
        else:
            model.set_sampling_ext(g.sampling_ext(mirostat=int(mode[-1]), mirostat_tau=5.0, mirostat_eta=0.1, seed=7), hist)

    print("ready", flush=True)
    for line in sys.stdin:
        mode = line.strip()
        if not mode:
            break
        setup(mode)
        model.decode_sample(11, 64, steps, use_graph=True)
        setup(mode)
        t0 = time.perf_counter()
        model.decode_sample(11, 64, steps, use_graph=True)
        print("ms %.6f" % ((time.perf_counter() - t0) / steps * 1e3), flush=True)
    model.free()


class Worker:
    def __init__(self, tree, steps):
        env = dict(os.environ, GPU_SAMPLE_CHAIN_TREE=tree)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(steps)], env=env, stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True)

    def wait_ready(self):
        line = self.p.stdout.readline().strip()
        while line and line != "ready":                     # (the library's own start-up lines)
            line = self.p.stdout.readline().strip()
        if line != "ready":
            raise RuntimeError("a worker ended before it was ready")

    def ask(self, mode):
        self.p.stdin.write(mode + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        while line and not line.startswith("ms "):          # (anything else the library says)
            line = self.p.stdout.readline()
        if not line:
            raise RuntimeError("a worker ended in mode " + mode)
        return float(line[3:])

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=120)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.steps)
    import numpy as np
    series = [("A", ROOT, MODES), ("A2", ROOT, ("default",))]
    if a.parent_tree:
        series.append(("parent", os.path.abspath(a.parent_tree), ("default",)))
    workers = {name: Worker(tree, a.steps) for name, tree, _ in series}
    try:
        for wk in workers.values():
            wk.wait_ready()
        samples = {(name, m): [] for name, _, modes in series for m in modes}
        for _ in range(a.reps):
            for name, _, modes in series:
                for m in modes:
                    samples[(name, m)].append(workers[name].ask(m))
    finally:
        for wk in workers.values():
            wk.close()
    med = {k: float(np.median(v)) for k, v in samples.items()}
    res = {"model": "falcon-7b q4_0 (synthetic)", "n_ctx": N_CTX, "steps": a.steps, "reps": a.reps,
           "ms_per_token": {"%s/%s" % k: {"samples": v, "median": med[k]} for k, v in samples.items()},
           "default_aa_spread_ms": abs(med[("A", "default")] - med[("A2", "default")])}
    if a.parent_tree:
        res["default_minus_parent_ms"] = min(med[("A", "default")], med[("A2", "default")]) - med[("parent", "default")]
        res["default_worst_minus_parent_ms"] = max(med[("A", "default")], med[("A2", "default")]) - med[("parent", "default")]
    for m in MODES[1:]:
        res["%s_minus_default_ms" % m] = med[("A", m)] - med[("A", "default")]
    res["mirostat_minus_whole_vocab_ms"] = {m: med[("A", m)] - med[("A", "whole_vocab")] for m in ("mirostat1", "mirostat2")}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""measurement aid (GPU): what stops cost the sampled decode loop, and what the early exit saves, on Falcon-7B Q4_0 (synthetic
weights), n_ctx 2048, single stream, hipGraph (one replay per step), the default sampler chain.

    python scripts/gpu_stop.py [--out profiles/stop_7b.json] [--steps 128] [--reps 5]

One process on the device. Every step below runs under its own time limit: alarm(2) with SIGALRM left at its default action, so a
step that runs past its limit -- also one that never returns from a blocking call into the library, where no Python-level handler
would ever run -- is killed by the signal together with the whole process (the shell sees status 142). A step that fails raises,
which ends the run as well: nothing more is started on the device after a failure or a time-out.

  off       ms per step with stops never set: the parent's loop -- what every other figure is compared with;
  seqs16    ms per step with 16 stop sequences of 8 tokens that never match (the sampler's tail at its most expensive; the loop polls);
  poll      ms per step with a budget that is never reached at poll intervals 4, 16 and 64, interleaved A/B/A/B with "off";
  budget32  wall time of one 512-step call that ends by budget at step 32 (poll 16), next to 32 and 512 steps with stops off."""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ggllm_cpp_amd as g  # noqa: E402
from ggllm_cpp_amd import synth  # noqa: E402

N_CTX = 2048


def stats(v):
    return {"samples": v, "median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def step(name, seconds, f):
    """f() under its own time limit. SIGALRM keeps its default action: the kernel ends the process when the limit passes, whether or
    not the interpreter gets to run (a Python handler would wait for the blocking library call to return, which a hung step never does)"""
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    print("step %s (limit %d s)" % (name, seconds), flush=True)      # (the last such line names the step a time-out killed)
    signal.alarm(seconds)
    try:
        r = f()
    finally:
        signal.alarm(0)
    print(name, json.dumps(r), flush=True)
    return r


def run(a):
    S, R = a.steps, a.reps
    g.init(0)
    hp = dict(synth.HP_7B)
    box = {}

    def load():
        box["m"] = g.FalconModel(synth.make_model_fast(hp, g.Q4_0, seed=1234), n_ctx=N_CTX, n_batch=1)
        return "ok"
    step("load", 600, load)
    m = box["m"]
    hist = [int(t) for t in synth.tokens(64, hp["n_vocab"], seed=3)]
    m.set_sampling(g.sampling(seed=7), hist)

    def ms_per_step(n=S):
        m.decode_sample(11, 64, n, use_graph=True)          # (warm: a changed setting re-captures here)
        t0 = time.perf_counter()
        m.decode_sample(11, 64, n, use_graph=True)          # (ends in a stream synchronise: the tokens come back)
        return (time.perf_counter() - t0) / n * 1e3

    def configure(kind, poll=16):
        m.set_stop_poll(poll)
        if kind == "off":
            m.set_stops(None)
        elif kind == "seqs16":
            m.set_stops(g.stops([[100 + k] * 8 for k in range(16)]))
        else:
            m.set_stops(g.stops(max_tokens=1 << 30))

    def ab(settings):
        v = {k: [] for k, _, _ in settings}
        for _ in range(R):
            for k, kind, poll in settings:
                configure(kind, poll)
                v[k].append(ms_per_step())
                if kind != "off":
                    assert m.stop_state()[1] == g.STOP_RUNNING and m.loop_steps() == S, (k, m.stop_state(), m.loop_steps())
        return {k: stats(x) for k, x in v.items()}

    res = {"model": "falcon-7b q4_0 (synthetic)", "n_ctx": N_CTX, "steps": S, "reps": R}
    res["ms_per_step"] = step("seqs16", 300, lambda: ab([("off", "off", 16), ("seqs16", "seqs16", 16), ("off2", "off", 16)]))
    res["ms_per_step_poll"] = step("poll", 300, lambda: ab([("off", "off", 16), ("poll4", "budget", 4), ("poll16", "budget", 16), ("poll64", "budget", 64), ("off2", "off", 16)]))

    def budget():
        out = {}
        for name, n, budget_at in (("off_32_steps", 32, 0), ("off_512_steps", 512, 0), ("budget32_of_512", 512, 32)):
            v = []
            for _ in range(R + 1):
                m.set_stop_poll(16)
                m.set_stops(g.stops(max_tokens=budget_at) if budget_at else None)
                t0 = time.perf_counter()
                m.decode_sample(11, 64, n, use_graph=True)
                v.append((time.perf_counter() - t0) * 1e3)
            out[name + "_ms"] = stats(v[1:])                # (the first call captures)
            out[name + "_loop_steps"] = m.loop_steps()
        return out
    res["wall"] = step("budget32", 300, budget)
    m.set_stops(None)
    m.free()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stop_7b.json"))
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    run(ap.parse_args())

"""measurement aid (GPU): what the context stop costs the sampled decode loop, and what a context swap costs, on Falcon-7B Q4_0 (synthetic
weights), n_ctx 2048, single stream, hipGraph (one replay per step), the default sampler chain.

    python scripts/gpu_ctx_swap.py --parent-root ../parent-checkout [--out profiles/ctx_swap_7b.json] [--steps 128] [--reps 7]

--parent-root is a checkout of the parent commit with its library built (make -C ggllm.cpp_amd/csrc); without it only this build is
measured and the file says so. The driver (this process, which never touches the device) starts three workers -- the parent commit's
package and library, and this build's twice (A/A) -- each with the model loaded, and asks them for one sample at a time in turn, so
every figure is a median of samples interleaved with everyone else's:

  off        ms per step with the context stop never set (all three workers);
  on         ms per step with it on and never firing: 128 steps from position 64 (this build only);
  swap       ms per falcon_hip_context_swap at keep 0: the planner's tail of n_ctx / 2 tokens evaluated again in batches of 512 (this build only);
  eval       ms for falcon_hip_eval of the same tokens in the same batches, the swap's floor (this build only);
  swap_slot  ms per swap of one slot of a 16-slot lock-step context: the same evaluation in the context's own plain context plus the
             row copies in and out (this build only).

Nothing is judged: if "on" costs more than the run's A/A spread over "off" the file says so. A sequence is brought to the end of its
cache for a swap sample by one step at position n_ctx - 1 (what the cache holds does not matter to the time).

A worker runs every sample under its own time limit: alarm with SIGALRM left at its default action, so a sample that runs past its
limit ends the worker; the driver sees its pipe close, ends the other workers and exits non-zero: nothing more is started on the device
after a failure or a time-out."""
import argparse
import json
import os
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CTX, N_BATCH, N_SLOTS = 2048, 512, 16
SETTINGS = ("off", "on", "swap", "eval", "swap_slot")
PARENT_HAS = ("off",)


def worker(root, steps):
    """one build on the device: reads a setting per line, answers with one sample in ms"""
    sys.path.insert(0, root)
    import time
    import numpy as np
    import ggllm_cpp_amd as g
    from ggllm_cpp_amd import synth
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(600)
    g.init(0)
    hp = dict(synth.HP_7B)
    m = g.FalconModel(synth.make_model_fast(hp, g.Q4_0, seed=1234), n_ctx=N_CTX, n_batch=N_BATCH)
    hist = [int(t) for t in synth.tokens(64, hp["n_vocab"], seed=3)]
    m.set_sampling(g.sampling(seed=7), hist)
    new = hasattr(m, "context_swap")
    sc = None
    if new:
        nk, nr = g.swap_plan(N_CTX, 64, 3 * N_CTX)
        regen = [int(t) for t in synth.tokens(nr, hp["n_vocab"], seed=5)]
    signal.alarm(0)
    print("ready", flush=True)
    for line in sys.stdin:
        kind = line.strip()
        if kind == "quit":
            break
        signal.alarm(180)
        if kind in ("off", "on"):
            if new:
                m.set_context_stop(kind == "on")
            m.decode_sample(11, 64, steps, use_graph=True)      # (warm: a changed setting re-captures here)
            t0 = time.perf_counter()
            m.decode_sample(11, 64, steps, use_graph=True)      # (ends in a stream synchronise: the tokens come back)
            ms = (time.perf_counter() - t0) / steps * 1e3
            if kind == "on":
                assert m.stop_state()[1] == g.STOP_RUNNING and m.loop_steps() == steps
        elif kind == "eval":
            t0 = time.perf_counter()
            for i in range(0, nr, N_BATCH):
                m.eval(regen[i:i + N_BATCH], nk + i, logits_all=False)
            ms = (time.perf_counter() - t0) * 1e3
        elif kind == "swap":
            m.set_context_stop(True)
            m.decode_sample(11, N_CTX - 1, 1, use_graph=True)
            assert m.stop_state()[1] == g.STOP_CONTEXT
            t0 = time.perf_counter()
            m.context_swap(nk, regen, N_BATCH)
            ms = (time.perf_counter() - t0) * 1e3
        else:
            rounds = 1
            if sc is None:
                sc = g.SeqContext(m, N_CTX, N_SLOTS)
                for s in range(N_SLOTS):
                    sc.set_sampling(s, g.sampling(seed=7 + s), hist)
                sc.set_context_stop(True)
                rounds = 2                                       # (the context's first swap makes its plain context: not timed)
            pos = np.zeros(N_SLOTS, np.int32)
            pos[0] = N_CTX - 1
            for _ in range(rounds):
                for s in range(1, N_SLOTS):
                    sc.set_stops(s, g.stops(max_tokens=1))       # (the other slots draw one token and stay frozen)
                sc.decode_sample(np.full(N_SLOTS, 11, np.int32), pos, 1, use_graph=True)
                assert sc.stop_state()[1][0] == g.STOP_CONTEXT
                t0 = time.perf_counter()
                sc.context_swap(0, nk, regen, N_BATCH)
                ms = (time.perf_counter() - t0) * 1e3
        signal.alarm(0)
        print("ms %.6f" % ms, flush=True)
    if sc is not None:
        sc.free()
    m.free()


def stats(v):
    s = sorted(v)
    return {"samples": v, "median": (s[len(s) // 2] + s[(len(s) - 1) // 2]) / 2, "min": s[0], "max": s[-1]}


def run(a):
    roots = {"new_a": ROOT, "new_b": ROOT}
    if a.parent_root:
        roots["parent"] = os.path.abspath(a.parent_root)
    procs = {}
    try:
        for name, root in roots.items():                    # one after the other: three 7B models are made on the host first
            env = dict(os.environ)
            env.pop("GGLLM_HIP_LIB", None)                  # (each root loads its own library)
            p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root, "--steps", str(a.steps)], stdin=subprocess.PIPE,
                                 stdout=subprocess.PIPE, text=True, env=env)
            procs[name] = p
            if p.stdout.readline().strip() != "ready":
                raise RuntimeError("worker %s did not come up" % name)
            print("worker %s ready" % name, flush=True)

        def sample(name, kind):
            p = procs[name]
            p.stdin.write(kind + "\n")
            p.stdin.flush()
            ans = p.stdout.readline().split()
            if len(ans) != 2 or ans[0] != "ms":
                raise RuntimeError("worker %s ended at %s (status %s)" % (name, kind, p.poll()))
            return float(ans[1])

        v = {name: {k: [] for k in SETTINGS if name != "parent" or k in PARENT_HAS} for name in procs}
        order = list(procs)
        for rep in range(a.reps):
            for kind in SETTINGS:
                for name in order:
                    if kind in v[name]:
                        v[name][kind].append(sample(name, kind))
            order = order[1:] + order[:1]                   # (no worker is always the first behind a change of setting)
            print("rep %d done" % rep, flush=True)
    finally:
        for p in procs.values():
            try:
                p.stdin.write("quit\n")
                p.stdin.flush()
                p.wait(timeout=60)
            except Exception:
                p.kill()
    med = {name: {k: stats(x) for k, x in d.items()} for name, d in v.items()}
    spread = max(abs(med["new_a"][k]["median"] - med["new_b"][k]["median"]) for k in ("off", "on"))
    on_cost = {n: (med[n]["on"]["median"] - med[n]["off"]["median"]) * 1e3 for n in ("new_a", "new_b")}
    res = {"model": "falcon-7b q4_0 (synthetic)", "n_ctx": N_CTX, "n_batch": N_BATCH, "steps": a.steps, "reps": a.reps, "lock_step_slots": N_SLOTS,
           "regenerated_tokens": N_CTX // 2, "ms": med, "aa_spread_us_per_step": spread * 1e3, "on_minus_off_us_per_step": on_cost,
           "on_costs_more_than_the_spread": bool(min(on_cost.values()) > spread * 1e3),
           "swap_minus_eval_ms": {n: med[n]["swap"]["median"] - med[n]["eval"]["median"] for n in ("new_a", "new_b")},
           "swap_slot_minus_eval_ms": {n: med[n]["swap_slot"]["median"] - med[n]["eval"]["median"] for n in ("new_a", "new_b")},
           "parent_measured": "parent" in med}
    if "parent" in med:
        res["off_new_minus_parent_us_per_step"] = {n: (med[n]["off"]["median"] - med["parent"]["off"]["median"]) * 1e3 for n in ("new_a", "new_b")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: x for k, x in res.items() if k != "ms"}, indent=1))
    print({n: {k: round(x["median"], 4) for k, x in d.items()} for n, d in med.items()})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctx_swap_7b.json"))
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.steps)
    else:
        run(a)

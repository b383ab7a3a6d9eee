"""measurement aid (GPU): what a grammar costs the sampled decode loop, next to the parent commit, and what making one costs, on
Falcon-7B Q4_0 (synthetic weights), n_ctx 2048, single stream, hipGraph (one replay per step), the default sampler chain.

    python scripts/gpu_grammar.py --parent-root ../parent-checkout [--out profiles/grammar_7b.json] [--steps 128] [--reps 7]

--parent-root is a checkout of the parent commit with its library built (make -C ggllm.cpp_amd/csrc); without it only this build is
measured and the file says so. The driver (this process, which never touches the device) starts three workers -- the parent commit's
package and library, and this build's twice (A/A) -- each with the model loaded, and asks them for one sample at a time in turn, so
every figure is a median of samples interleaved with everyone else's:

  off       ms per step with no grammar ever set;
  g64       a 64-state automaton on the row     (this build only);
  g4096     a 4096-state automaton on the row   (this build only).

The automata are chains "at least n - 2 bytes of [a-z ]": every state allows every token of the synthetic vocabulary, so the draws are
those of "off" and the difference is the mask's reads and the advance alone; the row walks ~5 states per step, so the 4096-state
index is read at a new row every step. Acceptance: this build's "off" lies within the run's A/A spread (the largest difference
between the two same-build workers' medians over the settings) of the parent's "off". The cost with a grammar on is recorded, not judged.

Worker new_a also times falcon_hip_grammar_create at 64, 1024 and 4096 states (best of 3, wall clock around the call: uploads, the one
launch, the download of the counts), written beside the bytes the launch must at least read and write.

A worker runs every sample under its own time limit: alarm with SIGALRM left at its default action, so a sample that runs past its
limit ends the worker; the driver sees its pipe close, ends the other workers and exits non-zero: nothing more is started on the
device after a failure or a time-out."""
import argparse
import json
import os
import signal
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CTX = 2048
SETTINGS = ("off", "g64", "g4096")
CREATE_STATES = (64, 1024, 4096)


def chain(g, n_states):
    """state 0 dead, 1 .. n - 1 a chain over [a-z ], the last one looping and accepting"""
    import numpy as np
    t = np.zeros((n_states, 256), np.uint16)
    for s in range(1, n_states):
        t[s, 97:123] = min(s + 1, n_states - 1)
        t[s, 32] = min(s + 1, n_states - 1)
    acc = np.zeros(n_states, np.uint8)
    acc[n_states - 1] = 1
    return g.dfa(t, acc, 1)


def worker(root, steps, time_create):
    """one build on the device: reads a setting per line, answers with one sample of ms per step"""
    sys.path.insert(0, root)
    import time
    import ggllm_cpp_amd as g
    from ggllm_cpp_amd import synth
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(600)
    g.init(0)
    hp = dict(synth.HP_7B)
    m = g.FalconModel(synth.make_model_fast(hp, g.Q4_0, seed=1234), n_ctx=N_CTX, n_batch=1)
    hist = [int(t) for t in synth.tokens(64, hp["n_vocab"], seed=3)]
    m.set_sampling(g.sampling(seed=7), hist)
    has_grammar = hasattr(m, "set_grammar")
    grammars, create = {}, {}
    if has_grammar:
        # a vocabulary of n_vocab tokens of 3..8 lower-case bytes, every 500th a run of 40..130 blanks (Falcon's has such whitespace tokens)
        pool_bytes = 0
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "vocab.ggcc")
            with open(path, "wb") as f:
                f.write(struct.pack("<II", 0x67676363, 10) + struct.pack("<8I", hp["n_vocab"], 0, 0, 0, 0, 7, 0, 0))
                for t in range(hp["n_vocab"]):
                    w = b" " * (40 + t % 91) if t % 500 == 499 else bytes(97 + (t * 31 + i * 7) % 26 for i in range(3 + t % 6))
                    pool_bytes += len(w)
                    f.write(struct.pack("<I", len(w)) + w + struct.pack("<f", 0.0))
                f.write(struct.pack("<I", 0))
            vocab = g.Vocab(path)
        m.set_vocab(vocab)
        grammars = {"g64": m.grammar(chain(g, 64)), "g4096": m.grammar(chain(g, 4096))}
        if time_create:
            n_words = (hp["n_vocab"] + 63) // 64
            for n in CREATE_STATES:
                d, best = chain(g, n), None
                for _ in range(3):
                    t0 = time.perf_counter()
                    gr = m.grammar(d)
                    dt = (time.perf_counter() - t0) * 1e3
                    gr.free()
                    best = dt if best is None or dt < best else best
                floor = n * n_words * 8 + n * 512 + n + pool_bytes + (hp["n_vocab"] + 1) * 4
                create[str(n)] = {"ms": best, "min_bytes": floor, "index_bytes": n * n_words * 8, "walks": n * hp["n_vocab"]}
    signal.alarm(0)
    print("ready " + json.dumps(create), flush=True)
    for line in sys.stdin:
        kind = line.strip()
        if kind == "quit":
            break
        signal.alarm(120)
        if has_grammar:
            m.set_grammar(grammars.get(kind))               # (from the start state)
        m.decode_sample(11, 64, steps, use_graph=True)      # (warm: a changed setting re-captures here)
        if has_grammar:
            m.set_grammar(grammars.get(kind))
        t0 = time.perf_counter()
        m.decode_sample(11, 64, steps, use_graph=True)      # (ends in a stream synchronise: the tokens come back)
        ms = (time.perf_counter() - t0) / steps * 1e3
        if kind != "off":
            assert m.grammar_state > 1, (kind, m.grammar_state)
        signal.alarm(0)
        print("ms %.6f" % ms, flush=True)
    if has_grammar:
        m.set_grammar(None)
    m.free()


def stats(v):
    s = sorted(v)
    return {"samples": v, "median": (s[len(s) // 2] + s[(len(s) - 1) // 2]) / 2, "min": s[0], "max": s[-1]}


def run(a):
    roots = {"new_a": ROOT, "new_b": ROOT}
    if a.parent_root:
        roots["parent"] = os.path.abspath(a.parent_root)
    procs, create = {}, {}
    try:
        for name, root in roots.items():                    # one after the other: three 7B models are made on the host first
            env = dict(os.environ)
            env.pop("GGLLM_HIP_LIB", None)                  # (each root loads its own library)
            p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root, "--steps", str(a.steps)] + (["--time-create"] if name == "new_a" else []),
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
            procs[name] = p
            first = p.stdout.readline().strip()
            if not first.startswith("ready"):
                raise RuntimeError("worker %s did not come up" % name)
            if name == "new_a":
                create = json.loads(first[5:])
            print("worker %s ready" % name, flush=True)

        def sample(name, kind):
            p = procs[name]
            p.stdin.write(kind + "\n")
            p.stdin.flush()
            ans = p.stdout.readline().split()
            if len(ans) != 2 or ans[0] != "ms":
                raise RuntimeError("worker %s ended at %s (status %s)" % (name, kind, p.poll()))
            return float(ans[1])

        v = {name: {k: [] for k in SETTINGS if name != "parent" or k == "off"} for name in procs}
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
    us = lambda name, k: (med[name][k]["median"] - med[name]["off"]["median"]) * 1e3      # noqa: E731
    spread = max(abs(med["new_a"][k]["median"] - med["new_b"][k]["median"]) for k in SETTINGS)
    res = {"model": "falcon-7b q4_0 (synthetic)", "n_ctx": N_CTX, "steps": a.steps, "reps": a.reps, "ms_per_step": med,
           "aa_spread_us": spread * 1e3,
           "cost_us_per_step": {name: {k: us(name, k) for k in med[name] if k != "off"} for name in med},
           "grammar_create": create, "parent_measured": "parent" in med}
    if "parent" in med:
        d = min(abs(med[n]["off"]["median"] - med["parent"]["off"]["median"]) for n in ("new_a", "new_b"))
        res["off_new_minus_parent_us"] = {n: (med[n]["off"]["median"] - med["parent"]["off"]["median"]) * 1e3 for n in ("new_a", "new_b")}
        res["off_within_aa_spread"] = bool(d <= spread)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: x for k, x in res.items() if k != "ms_per_step"}, indent=1))
    print({n: {k: round(x["median"], 4) for k, x in d.items()} for n, d in med.items()})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grammar_7b.json"))
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--time-create", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.steps, a.time_create)
    else:
        run(a)

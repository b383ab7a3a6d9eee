"""measurement aid (GPU): what stop strings cost the sampled decode loop, next to the id stops and next to the parent commit, on
Falcon-7B Q4_0 (synthetic weights), n_ctx 2048, single stream, hipGraph (one replay per step), the default sampler chain.

    python scripts/gpu_stop_text.py --parent-root ../parent-checkout [--out profiles/stop_text_7b.json] [--steps 128] [--reps 7]

--parent-root is a checkout of the parent commit with its library built (make -C ggllm.cpp_amd/csrc); without it only this build is
measured and the file says so. The driver (this process, which never touches the device) starts three workers -- the parent commit's
package and library, and this build's twice (A/A) -- each with the model loaded, and asks them for one sample at a time in turn, so
every figure is a median of samples interleaved with everyone else's:

  off       ms per step with stops never set;
  ids16     16 stop sequences of 8 token ids that never match (the parent's own case, profiles/stop_7b.json);
  text1     1 stop string of 32 bytes that never matches   (this build only);
  text16    16 of them                                      (this build only).

The strings are lower-case letters, like the synthetic vocabulary's tokens, with one '#' four bytes before their end: a lane's
backward comparison passes its first bytes now and then before it fails, as a real stop word's does; it is not the cheapest case.
Acceptance: this build's "off" lies within the run's A/A spread (the largest difference between the two same-build workers' medians
over the four settings) of the parent's "off". The cost with strings on is recorded, not judged.

A worker runs every sample under its own time limit: alarm(2) with SIGALRM left at its default action, so a sample that runs past
its limit -- also one that never returns from the library -- ends the worker; the driver sees its pipe close, ends the other workers
and exits non-zero: nothing more is started on the device after a failure or a time-out."""
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
SETTINGS = ("off", "ids16", "text1", "text16")


def never_matching(k):
    s = bytes(97 + (7 * k + 3 * i) % 26 for i in range(32))
    return s[:28] + b"#" + s[29:]


def worker(root, steps):
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
    has_text = hasattr(m, "set_stop_text")
    if has_text:
        # a vocabulary of n_vocab tokens of 3..8 lower-case bytes, every 500th a run of 40..130 blanks (Falcon's has such whitespace tokens)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "vocab.ggcc")
            with open(path, "wb") as f:
                f.write(struct.pack("<II", 0x67676363, 10) + struct.pack("<8I", hp["n_vocab"], 0, 0, 0, 0, 7, 0, 0))
                for t in range(hp["n_vocab"]):
                    w = b" " * (40 + t % 91) if t % 500 == 499 else bytes(97 + (t * 31 + i * 7) % 26 for i in range(3 + t % 6))
                    f.write(struct.pack("<I", len(w)) + w + struct.pack("<f", 0.0))
                f.write(struct.pack("<I", 0))
            vocab = g.Vocab(path)
        m.set_vocab(vocab)
    signal.alarm(0)
    print("ready", flush=True)
    for line in sys.stdin:
        kind = line.strip()
        if kind == "quit":
            break
        signal.alarm(120)
        m.set_stops(g.stops([[100 + k] * 8 for k in range(16)]) if kind == "ids16" else None)
        if has_text:
            m.set_stop_text(g.stop_text([never_matching(k) for k in range(16 if kind == "text16" else 1)]) if kind.startswith("text") else None)
        m.decode_sample(11, 64, steps, use_graph=True)      # (warm: a changed setting re-captures here)
        t0 = time.perf_counter()
        m.decode_sample(11, 64, steps, use_graph=True)      # (ends in a stream synchronise: the tokens come back)
        ms = (time.perf_counter() - t0) / steps * 1e3
        if kind != "off":
            assert m.stop_state()[1] == g.STOP_RUNNING and m.loop_steps() == steps, (kind, m.stop_state(), m.loop_steps())
        signal.alarm(0)
        print("ms %.6f" % ms, flush=True)
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

        v = {name: {k: [] for k in SETTINGS if name != "parent" or not k.startswith("text")} for name in procs}
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
           "parent_measured": "parent" in med}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stop_text_7b.json"))
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.steps)
    else:
        run(a)

"""measurement aid (GPU): what keeping the embedding costs, next to the parent commit, on Falcon-7B Q4_0 (synthetic weights), n_ctx 2048,
n_batch 512, single stream.

    python scripts/gpu_embed.py --parent-root ../parent-checkout [--out profiles/embed_7b.json] [--steps 64] [--reps 7]

--parent-root is a checkout of the parent commit with its library built (make -C ggllm.cpp_amd/csrc); without it only this build is
measured and the file says so. The driver (this process, which never touches the device) starts three workers -- the parent commit's
package and library, and this build's twice (A/A) -- each with the model loaded, and asks them for one sample at a time in turn, so
every figure is a median of samples interleaved with everyone else's. A sample is one call of

  eval128 / eval512   falcon_hip_eval of 128 / 512 tokens at n_past 0, last row's logits                      (ms per call)
  step                falcon_hip_eval_token, `steps` single-token steps through the captured graph from
                      n_past 128, the last one's logits fetched                                                (ms per step)
  embed128 / embed512 falcon_hip_embed of the same tokens                                  (this build, modes 1 and 3 only)

in mode 0 (every worker), mode 1 and mode 3 (this build). (a) mode 0 of this build against the parent: the launches are the same, so
the expectation is a difference inside the A/A spread of the two same-build workers (the largest difference between their medians over
the mode-0 settings), which is recorded with the numbers; (b) modes 1 and 3 against mode 0: the row write, the norm launch on the
step, the accumulate launch; (c) falcon_hip_embed against falcon_hip_eval in the same mode: the head left out. (d) worker new_a also
times ggml_hip_embed_pool_accum alone on 512 x 4544 and 512 x 8192 rows next to a device-to-device copy of the same rows (events
around 20 calls each, best of 5).

A worker runs every sample under its own time limit: alarm with SIGALRM left at its default action, so a sample that runs past its
limit ends the worker; the driver sees its pipe close, ends the other workers and exits non-zero: nothing more is started on the
device after a failure or a time-out."""
import argparse
import json
import os
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CTX, N_BATCH = 2048, 512
CALLS = ("eval128", "eval512", "step")
EMBED_CALLS = ("embed128", "embed512")
ACCUM_SHAPES = ((512, 4544), (512, 8192))


def time_accum(g):
    """(d): {rows x n_embd: {accum_us, copy_us, bytes}}"""
    import numpy as np
    L = g.load()
    out = {}
    for n, E in ACCUM_SHAPES:
        x = g.DevBuf(host=np.random.default_rng(1).standard_normal((n, E)).astype(np.float32))
        y = g.DevBuf(n * E * 4)
        acc, cnt = g.DevBuf(host=np.zeros(E, np.float64)), g.DevBuf(host=np.zeros(1, np.int64))

        def us(fn, calls=20):
            fn()
            best = None
            for _ in range(5):
                e0, e1 = L.ggml_hip_event_create(), L.ggml_hip_event_create()
                L.ggml_hip_event_record(e0)
                for _ in range(calls):
                    fn()
                L.ggml_hip_event_record(e1)
                L.ggml_hip_synchronize()
                dt = L.ggml_hip_event_elapsed_ms(e0, e1) / calls * 1e3
                L.ggml_hip_event_destroy(e0); L.ggml_hip_event_destroy(e1)
                best = dt if best is None or dt < best else best
            return best
        out["%dx%d" % (n, E)] = {"accum_us": us(lambda: L.ggml_hip_embed_pool_accum(x.ptr, n, E, acc.ptr, cnt.ptr)),
                                 "copy_us": us(lambda: L.ggml_hip_memcpy_d2d(y.ptr, x.ptr, n * E * 4)), "bytes": n * E * 4}
        for b in (x, y, acc, cnt):
            b.free()
    return out


def worker(root, steps, time_ops):
    """one build on the device: reads "<mode> <call>" per line, answers with one sample in ms"""
    sys.path.insert(0, root)
    import time
    import ggllm_cpp_amd as g
    from ggllm_cpp_amd import synth
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(900)
    g.init(0)
    hp = dict(synth.HP_7B)
    m = g.FalconModel(synth.make_model_fast(hp, g.Q4_0, seed=1234), n_ctx=N_CTX, n_batch=N_BATCH)
    toks = synth.tokens(512, hp["n_vocab"], seed=3)
    has = hasattr(m, "set_embedding")
    ops = time_accum(g) if (time_ops and has) else {}
    signal.alarm(0)
    print("ready " + json.dumps(ops), flush=True)
    for line in sys.stdin:
        if line.strip() == "quit":
            break
        mode, call = line.split()
        mode = int(mode)
        signal.alarm(180)
        if has:
            m.set_embedding(last=bool(mode & 1), pool=bool(mode & 2))
            m.pool_reset()

        def once():
            if call == "step":
                for i in range(steps):
                    m.eval_token(int(toks[i]), 128 + i)
                m.logits()
                return steps
            n = int(call[-3:])
            if call.startswith("embed"):
                m.embed_tokens(toks[:n], 0)
            else:
                m.eval(toks[:n], 0, logits_all=False)
            return 1
        if call == "step":
            m.eval(toks[:128], 0, logits_all=False)
        once()                                              # (warm: a changed mode captures its step here)
        t0 = time.perf_counter()
        k = once()                                          # (ends in a stream synchronise)
        ms = (time.perf_counter() - t0) / k * 1e3
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
    procs, ops = {}, {}
    settings = [(0, c) for c in CALLS] + [(mode, c) for mode in (1, 3) for c in CALLS + EMBED_CALLS]
    try:
        for name, root in roots.items():                    # one after the other: three 7B models are made on the host first
            env = dict(os.environ)
            env.pop("GGLLM_HIP_LIB", None)                  # (each root loads its own library)
            p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root, "--steps", str(a.steps)] + (["--time-ops"] if name == "new_a" else []),
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
            procs[name] = p
            first = p.stdout.readline().strip()
            if not first.startswith("ready"):
                raise RuntimeError("worker %s did not come up" % name)
            if name == "new_a":
                ops = json.loads(first[5:])
            print("worker %s ready" % name, flush=True)

        def sample(name, mode, call):
            p = procs[name]
            p.stdin.write("%d %s\n" % (mode, call))
            p.stdin.flush()
            ans = p.stdout.readline().split()
            if len(ans) != 2 or ans[0] != "ms":
                raise RuntimeError("worker %s ended at mode %d %s (status %s)" % (name, mode, call, p.poll()))
            return float(ans[1])

        key = lambda mode, call: "mode%d_%s" % (mode, call)      # noqa: E731
        v = {name: {key(mo, c): [] for mo, c in settings if name != "parent" or mo == 0} for name in procs}
        order = list(procs)
        for rep in range(a.reps):
            for mo, c in settings:
                for name in order:
                    if key(mo, c) in v[name]:
                        v[name][key(mo, c)].append(sample(name, mo, c))
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
    md = lambda name, k: med[name][k]["median"]              # noqa: E731
    off = [key(0, c) for c in CALLS]
    spread = {k: abs(md("new_a", k) - md("new_b", k)) * 1e3 for k in off}
    res = {"model": "falcon-7b q4_0 (synthetic)", "n_ctx": N_CTX, "n_batch": N_BATCH, "steps": a.steps, "reps": a.reps, "unit": "ms per call (step: ms per step)",
           "ms": med, "aa_spread_us": spread, "parent_measured": "parent" in med,
           "mode_cost_us": {name: {key(mo, c): (md(name, key(mo, c)) - md(name, key(0, c))) * 1e3 for mo in (1, 3) for c in CALLS} for name in ("new_a", "new_b")},
           "embed_minus_eval_us": {name: {key(mo, "embed%d" % n): (md(name, key(mo, "embed%d" % n)) - md(name, key(mo, "eval%d" % n))) * 1e3 for mo in (1, 3) for n in (128, 512)}
                                   for name in ("new_a", "new_b")},
           "pool_accum_alone": ops}
    if "parent" in med:
        res["mode0_new_minus_parent_us"] = {n: {k: (md(n, k) - md("parent", k)) * 1e3 for k in off} for n in ("new_a", "new_b")}
        res["mode0_within_aa_spread"] = {k: bool(min(abs(md(n, k) - md("parent", k)) for n in ("new_a", "new_b")) * 1e3 <= spread[k]) for k in off}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: x for k, x in res.items() if k != "ms"}, indent=1))
    print({n: {k: round(x["median"], 4) for k, x in d.items()} for n, d in med.items()})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "embed_7b.json"))
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--time-ops", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.steps, a.time_ops)
    else:
        run(a)

"""measurement aid (GPU): what draft-and-verify decode costs and gains on Falcon-7B Q4_0 (synthetic weights), n_ctx 2048, single stream,
hipGraph (one replay per pass), the default sampler chain.

    python scripts/gpu_spec.py --parent-root ../parent-checkout [--out profiles/spec_7b.json] [--steps 128] [--reps 7]

--parent-root is a checkout of the parent commit with its library built (make -C ggllm.cpp_amd/csrc); without it only this build is
measured and the file says so. The driver (this process, which never touches the device) starts three workers -- the parent commit's
package and library, and this build's twice (A/A) -- each with the model loaded, and asks them for one sample at a time in turn, so
every figure is a median of samples interleaved with everyone else's (the set-up of scripts/gpu_ctx_swap.py):

  off         ms per step of falcon_hip_decode_sample with spec off (all three workers);
  miss:K      ms per pass of falcon_hip_decode_spec, K = 1, 3, 7, 15, with a guess that is wrong everywhere: every pass draws one token --
              the price of a miss, against `off` (this build only);
  hit:K       ms per pass with a guess that is right everywhere: every pass draws K + 1 tokens, 32 such passes; the K + 1 sampler rows
              run one after the other in the pass's last launch (this build only). The loop polls the device after every pass here and
              still launches up to two passes past the end, which draw nothing: they are in the elapsed time and in the divisor;
  plain:rep, lookup:rep     tokens per second of the plain loop and of prompt lookup at K = 3 (n-grams 1..3), greedy, 128 tokens behind a
              prompt that is the model's own greedy output fed back (256 tokens: a text that repeats itself), with the draws per pass;
  plain:rand, lookup:rand   the same, sampled, behind a prompt of 256 random ids, where nothing matches.

From miss and hit the file derives, per K, the break-even draws per pass: the a with  miss + (hit - miss) * (a - 1) / K = a * off, a
pass's cost taken as linear in the rows the sampler runs; below it the feature loses against the plain loop. Nothing is judged.

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
N_CTX, N_BATCH = 2048, 512
KS = (1, 3, 7, 15)
SETTINGS = ("off",) + tuple("miss:%d" % k for k in KS) + tuple("hit:%d" % k for k in KS) + ("plain:rep", "lookup:rep", "plain:rand", "lookup:rand")
PARENT_HAS = ("off",)
HIT_PASSES, LOOKUP_K, LOOKUP_TOKENS, PROMPT_TOKENS = 32, 3, 128, 256


def worker(root, steps):
    """one build on the device: reads a setting per line, answers with one sample: ms and a second figure (draws per pass; 0 where there is none)"""
    sys.path.insert(0, root)
    import time
    import ggllm_cpp_amd as g
    from ggllm_cpp_amd import synth
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(600)
    g.init(0)
    hp = dict(synth.HP_7B)
    V = hp["n_vocab"]
    m = g.FalconModel(synth.make_model_fast(hp, g.Q4_0, seed=1234), n_ctx=N_CTX, n_batch=N_BATCH)
    hist = [int(t) for t in synth.tokens(64, V, seed=3)]
    P = g.sampling(seed=7)
    m.set_sampling(P, hist)
    truth, prompts = {}, {}
    signal.alarm(0)
    print("ready", flush=True)

    def spec_run(K, guess, n):
        m.eval(hist, 0, logits_all=False)                   # (the rows in front of position 64: the same for every run, whatever was evaluated in between)
        m.set_sampling(P, hist)
        m.set_spec(K, g.SPEC_GIVEN)
        m.set_spec_guess(guess)
        t0 = time.perf_counter()
        out = m.decode_spec(11, 64, n, use_graph=True)
        dt = time.perf_counter() - t0
        return out.tolist(), dt

    def prompt_of(kind):
        """(prompt, sampler): the model's own greedy output fed back, or random ids under the default chain"""
        if kind not in prompts:
            if kind == "rand":
                prompts[kind] = ([int(t) for t in synth.tokens(PROMPT_TOKENS, V, seed=11)], g.sampling(seed=9))
            else:
                greedy = g.sampling(temp=0.0, repeat_penalty=1.0, repeat_last_n=0, seed=1)
                m.set_spec(0)
                m.eval(hist, 0, logits_all=False)
                m.set_sampling(greedy, hist)
                first = m.sample()
                prompts[kind] = ([first] + m.decode_sample(first, len(hist), PROMPT_TOKENS - 1, use_graph=True).tolist(), greedy)
        return prompts[kind]

    for line in sys.stdin:
        kind = line.strip()
        if kind == "quit":
            break
        signal.alarm(300)
        second = 0.0
        if kind == "off":
            if hasattr(m, "set_spec"):
                m.set_spec(0)
            m.decode_sample(11, 64, steps, use_graph=True)      # (warm: a changed setting re-captures here)
            t0 = time.perf_counter()
            m.decode_sample(11, 64, steps, use_graph=True)      # (ends in a stream synchronise: the tokens come back)
            ms = (time.perf_counter() - t0) / steps * 1e3
        elif kind.startswith(("miss:", "hit:")):
            K = int(kind.split(":")[1])
            n = steps if kind.startswith("miss") else HIT_PASSES * (K + 1)
            if (K, n) not in truth:                             # what this pass shape draws, found once: a run without drafts, then a fixed point
                m.set_stop_poll(16)
                t, _ = spec_run(K, [], n)
                for _ in range(8):
                    t2, _ = spec_run(K, t, n)
                    if t2 == t:
                        break
                    t = t2
                truth[(K, n)] = t
            t = truth[(K, n)]
            if kind.startswith("miss"):
                m.set_stop_poll(16)                             # (n passes, every one draws: the loop never looks)
                guess = [(x + 1) % V for x in t]
            else:
                m.set_stop_poll(1)
                guess = t
            spec_run(K, guess, n)                               # (warm: a changed K re-captures here)
            out, dt = spec_run(K, guess, n)
            passes, draws, _ = m.spec_stats()
            assert draws == n and len(out) == n and passes <= m.loop_steps() <= passes + 2, (draws, passes, m.loop_steps())
            if kind.startswith("miss"):
                assert passes == n, passes                      # (hit: the second figure says how many of the K + 1 rows the passes kept)
            ms = dt / m.loop_steps() * 1e3
            second = draws / passes
            m.set_stop_poll(16)
        else:
            how, what = kind.split(":")
            prompt, p = prompt_of(what)
            m.set_spec(0)
            for timed in (False, True):                         # (the first round warms: captures)
                m.eval(prompt, 0, logits_all=False)
                m.set_sampling(p, prompt)
                first = m.sample()
                if how == "lookup":
                    m.set_spec(LOOKUP_K, g.SPEC_LOOKUP, ngram=(1, 3), history=prompt + [first])
                    m.set_stop_poll(4)
                    t0 = time.perf_counter()
                    out = m.decode_spec(first, len(prompt), LOOKUP_TOKENS, use_graph=True)
                    dt = time.perf_counter() - t0
                    passes, draws, _ = m.spec_stats()
                    second = draws / passes
                    m.set_stop_poll(16)
                else:
                    t0 = time.perf_counter()
                    out = m.decode_sample(first, len(prompt), LOOKUP_TOKENS, use_graph=True)
                    dt = time.perf_counter() - t0
                    second = 1.0
                assert len(out) == LOOKUP_TOKENS
            ms = dt * 1e3                                       # (for LOOKUP_TOKENS tokens)
        signal.alarm(0)
        print("ms %.6f %.6f" % (ms, second), flush=True)
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
            if len(ans) != 3 or ans[0] != "ms":
                raise RuntimeError("worker %s ended at %s (status %s)" % (name, kind, p.poll()))
            return float(ans[1]), float(ans[2])

        v = {name: {k: [] for k in SETTINGS if name != "parent" or k in PARENT_HAS} for name in procs}
        per_pass = {name: {} for name in procs}
        order = list(procs)
        for rep in range(a.reps):
            for kind in SETTINGS:
                for name in order:
                    if kind in v[name]:
                        ms, second = sample(name, kind)
                        v[name][kind].append(ms)
                        per_pass[name][kind] = second
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
    new = ("new_a", "new_b")
    spread = abs(med["new_a"]["off"]["median"] - med["new_b"]["off"]["median"])
    res = {"model": "falcon-7b q4_0 (synthetic)", "n_ctx": N_CTX, "n_batch": N_BATCH, "steps": a.steps, "reps": a.reps, "hit_passes": HIT_PASSES,
           "lookup": {"K": LOOKUP_K, "ngram": [1, 3], "tokens": LOOKUP_TOKENS, "prompt_tokens": PROMPT_TOKENS},
           "ms": med, "draws_per_pass": per_pass, "aa_spread_us_per_step": spread * 1e3, "parent_measured": "parent" in med}
    if "parent" in med:
        d = {n: (med[n]["off"]["median"] - med["parent"]["off"]["median"]) * 1e3 for n in new}
        res["off_new_minus_parent_us_per_step"] = d
        res["off_differs_from_parent_by_more_than_the_spread"] = bool(min(abs(x) for x in d.values()) > spread * 1e3)
    be = {}
    for n in new:
        off = med[n]["off"]["median"]
        be[n] = {}
        for K in KS:
            miss, hit = med[n]["miss:%d" % K]["median"], med[n]["hit:%d" % K]["median"]
            slope = (hit - miss) / K                        # per further row the sampler runs
            # miss + slope * (a - 1) = a * off
            be[n][str(K)] = (miss - slope) / (off - slope) if off > slope else None
    res["break_even_draws_per_pass"] = be
    res["tokens_per_s"] = {n: {k: LOOKUP_TOKENS / (med[n][k]["median"] * 1e-3) for k in SETTINGS if ":re" in k or ":ra" in k} for n in new}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: x for k, x in res.items() if k != "ms"}, indent=1))
    print({n: {k: round(x["median"], 4) for k, x in d.items()} for n, d in med.items()})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_7b.json"))
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.steps)
    else:
        run(a)

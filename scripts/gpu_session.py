"""measurement aid (GPU): what saving and loading a session costs on Falcon-7B Q4_0 (synthetic weights), n_ctx 2048, next to the work a loaded
session replaces and to the plain streaming copy of the same bytes. Sessions of 128, 512 and 2048 tokens, the median of 7 runs each.

    python scripts/gpu_session.py [--out profiles/session_7b.json] [--reps 7]

One process on the device. Every step runs under its own time limit: alarm(2) with SIGALRM left at its default action, so a step that runs past
its limit is killed by the signal together with the whole process (status 142); a step that fails raises, which ends the run as well: nothing
more is started on the device after a failure or a time-out.

  (a) end to end, wall time: falcon_hip_eval of the prompt (twice, interleaved: the second series is the A/A spread of the run), save_session and
      load_session with the file on local disk, copy_state / set_state to and from host memory. ratio_* = the call / the eval it replaces.
  (b) the kernels alone, device time between two events around 20 launches: k_session_pack and k_session_unpack through ggml_hip_kv_pack /
      ggml_hip_kv_unpack on the context-shaped caches (32 layers, pitch 2048 rows, 64 floats per row), k_copy_seq_kv (falcon_hip_context_copy_seq
      between two contexts) moving the same rows -- the plain copy of the same bytes; pack is timed twice for the A/A spread."""
import argparse
import json
import os
import signal
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ggllm_cpp_amd as g  # noqa: E402
from ggllm_cpp_amd import synth  # noqa: E402

N_CTX, SIZES, LAUNCHES = 2048, (128, 512, 2048), 20


def stats(v):
    return {"samples": [round(float(x), 4) for x in v], "median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def step(name, seconds, f):
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    print("step %s (limit %d s)" % (name, seconds), flush=True)      # (the last such line names the step a time-out killed)
    signal.alarm(seconds)
    try:
        r = f()
    finally:
        signal.alarm(0)
    print(name, json.dumps(r), flush=True)
    return r


def wall_ms(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


class Ctx:
    """a second context of the model, as copy_seq takes it"""

    def __init__(self, ctx):
        self.ctx = ctx


def run(a):
    R = a.reps
    L = g.load()
    g.init(0)
    hp = dict(synth.HP_7B)
    box = {}

    def load():
        box["m"] = g.FalconModel(synth.make_model_fast(hp, g.Q4_0, seed=1234), n_ctx=N_CTX, n_batch=N_CTX)
        return "ok"
    step("load", 900, load)
    m = box["m"]
    other = Ctx(m.new_context(N_CTX, 1))
    res = {"model": "falcon-7b q4_0 (synthetic)", "n_ctx": N_CTX, "reps": R, "end_to_end_ms": {}, "kernels_us": {}}
    tmp = tempfile.mkdtemp(prefix="session_")
    path = os.path.join(tmp, "s.session")

    def end_to_end(n):
        tok = synth.tokens(n, hp["n_vocab"], seed=5)
        v = {k: [] for k in ("eval", "eval_again", "save_file", "load_file", "copy_state", "set_state")}
        m.eval(tok, 0, logits_all=False)                                  # (warm)
        for _ in range(R):
            v["eval"].append(wall_ms(lambda: m.eval(tok, 0, logits_all=False)))
            v["save_file"].append(wall_ms(lambda: m.save_session(path, tok)))
            v["load_file"].append(wall_ms(lambda: m.load_session(path)))
            v["eval_again"].append(wall_ms(lambda: m.eval(tok, 0, logits_all=False)))
            blob = []
            v["copy_state"].append(wall_ms(lambda: blob.append(m.copy_state(n))))
            v["set_state"].append(wall_ms(lambda: m.set_state(blob[0])))
        out = {k: stats(x) for k, x in v.items()}
        out["file_bytes"] = os.path.getsize(path)
        ev = out["eval"]["median"]
        for k in ("save_file", "load_file", "copy_state", "set_state"):
            out["ratio_" + k] = out[k]["median"] / ev
        out["aa_spread_eval"] = abs(out["eval_again"]["median"] - ev) / ev
        return out

    def kernels(n):
        nl, hkv = hp["n_layer"], hp["n_head_kv"]
        rows = nl * N_CTX * hkv * 64
        kb, vb = g.DevBuf(host=np.arange(rows, dtype=np.float32)), g.DevBuf(host=np.arange(rows, dtype=np.float32) + 0.5)
        sb = g.DevBuf(2 * nl * n * hkv * 64 * 4)
        e0, e1 = L.ggml_hip_event_create(), L.ggml_hip_event_create()

        def timed(f):
            f()                                                           # (warm)
            L.ggml_hip_synchronize()
            L.ggml_hip_event_record(e0)
            for _ in range(LAUNCHES):
                f()
            L.ggml_hip_event_record(e1)
            L.ggml_hip_synchronize()
            return L.ggml_hip_event_elapsed_ms(e0, e1) / LAUNCHES * 1e3
        v = {k: [] for k in ("pack", "unpack", "copy_seq", "pack_again")}
        for _ in range(R):
            v["pack"].append(timed(lambda: g.kv_pack(kb, vb, sb, nl, hkv, n, N_CTX, 0)))
            v["unpack"].append(timed(lambda: g.kv_unpack(kb, vb, sb, nl, hkv, n, N_CTX, 0)))
            v["copy_seq"].append(timed(lambda: g.copy_seq(other, 0, m, 0, n)))
            v["pack_again"].append(timed(lambda: g.kv_pack(kb, vb, sb, nl, hkv, n, N_CTX, 0)))
        for b in (kb, vb, sb):
            b.free()
        for e in (e0, e1):
            L.ggml_hip_event_destroy(e)
        out = {k: stats(x) for k, x in v.items()}
        cp = out["copy_seq"]["median"]
        out["bytes_moved_each_way"] = 2 * nl * n * hkv * 64 * 4
        out["ratio_pack"], out["ratio_unpack"] = out["pack"]["median"] / cp, out["unpack"]["median"] / cp
        out["aa_spread_pack"] = abs(out["pack_again"]["median"] - out["pack"]["median"]) / out["pack"]["median"]
        return out

    for n in SIZES:
        res["end_to_end_ms"][str(n)] = step("end_to_end_%d" % n, 300, lambda: end_to_end(n))
    for n in SIZES:
        res["kernels_us"][str(n)] = step("kernels_%d" % n, 120, lambda: kernels(n))
    L.falcon_hip_context_free(other.ctx)
    m.free()
    os.remove(path)
    os.rmdir(tmp)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_7b.json"))
    ap.add_argument("--reps", type=int, default=7)
    run(ap.parse_args())

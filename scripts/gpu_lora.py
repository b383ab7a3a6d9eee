"""measurement aid (GPU): what falcon_hip_model_apply_lora costs on Falcon-7B Q4_0 (synthetic weights): an adapter of r = 16 on all four matrices of every
block (128 pairs, N(0, 0.05^2) values, F32), applied twice to the same model -- the first call also loads the kernels' code objects, the second is the merge
itself. Wall time of the whole call: reading and checking the file, uploads, dequantize -> low-rank add -> quantize -> re-tile per chunk, the two device waits.

    python scripts/gpu_lora.py [--out profiles/lora_7b.json]

One process on the device. Every step runs under its own time limit: alarm(2) with SIGALRM left at its default action, so a step that runs past its limit is
killed by the signal together with the whole process (status 142); a step that fails raises, which ends the run as well."""
import argparse
import json
import os
import signal
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ggllm_cpp_amd as g  # noqa: E402
from ggllm_cpp_amd import synth  # noqa: E402

R, ALPHA = 16, 32
LEAVES = ("self_attention.query_key_value.weight", "self_attention.dense.weight", "mlp.dense_h_to_4h.weight", "mlp.dense_4h_to_h.weight")


def step(name, seconds, f):
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    print("step %s (limit %d s)" % (name, seconds), flush=True)
    signal.alarm(seconds)
    try:
        r = f()
    finally:
        signal.alarm(0)
    print(name, json.dumps(r), flush=True)
    return r


def write_adapter(path, hp):
    E, FF, QKV = hp["n_embd"], hp["n_ff"], (hp["n_head"] + 2 * hp["n_head_kv"]) * 64
    shapes = ((E, QKV), (E, E), (E, FF), (FF, E))
    rng = np.random.default_rng(7)
    pairs = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<IIii", 0x67676C61, 1, R, ALPHA))
        for il in range(hp["n_layer"]):
            for leaf, (K, M) in zip(LEAVES, shapes):
                for half, rows in (("A", K), ("B", M)):
                    nb = ("transformer.h.%d.%s.lora%s" % (il, leaf, half)).encode()
                    f.write(struct.pack("<5i", 2, len(nb), 0, R, rows))
                    f.write(nb)
                    f.write(b"\0" * (-f.tell() & 31))
                    f.write((rng.standard_normal((rows, R)) * 0.05).astype(np.float32).tobytes())
                pairs += 1
    return pairs


def run(a):
    g.init(0)
    hp = dict(synth.HP_7B)
    box = {}

    def load():
        box["m"] = g.FalconModel(synth.make_model_fast(hp, g.Q4_0, seed=1234), n_ctx=64, n_batch=8)
        return "ok"
    step("load", 900, load)
    m = box["m"]
    tmp = tempfile.mkdtemp(prefix="lora_")
    path = os.path.join(tmp, "adapter.bin")
    pairs = step("write_adapter", 300, lambda: write_adapter(path, hp))
    res = {"model": "falcon-7b q4_0 (synthetic)", "r": R, "alpha": ALPHA, "pairs": pairs, "adapter_bytes": os.path.getsize(path),
           "weight_bytes": int(m.weight_bytes()), "apply_ms": []}

    def apply():
        t0 = time.perf_counter()
        m.apply_lora(path)
        return (time.perf_counter() - t0) * 1e3
    tok = synth.tokens(4, hp["n_vocab"], seed=5)
    before = m.eval(tok, 0, logits_all=False)
    for i in range(2):
        res["apply_ms"].append(round(step("apply_%d" % i, 600, apply), 2))
    after = m.eval(tok, 0, logits_all=False)
    res["logits_moved"] = bool(np.isfinite(after).all() and not np.array_equal(before, after))
    m.free()
    os.remove(path)
    os.rmdir(tmp)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_7b.json"))
    run(ap.parse_args())

"""measurement aid (GPU): Falcon-7B with F16 weights (synthetic, 2 bytes per weight in HBM) through the exact F16 mat-mul (csrc/kernels_f16.hip), and -- in the
same run, as a floor -- Falcon-7B Q8_0 in ggml_hip_reference_order(1), the one-thread-per-output parity instrument.

    python scripts/gpu_f16.py [--out profiles/f16_7b.json] [--steps S] [--reps R] [--layers L]

  decode      ms per token of falcon_hip_decode_greedy through the captured graph (one replay per step), n_ctx 2048, at position 64
  lockstep    ms per pass of falcon_hip_decode_greedy_seqs with 16 and with 64 sequences
  prompt      ms of falcon_hip_eval of a 128-token prompt
  floor       ms per token of the Q8_0 model in reference order 1 (plain launches)
Every F16 entry carries its share of the F16 roofline: (2 bytes x weights streamed per step) / 8 TB/s divided by the measured time.
The blocks of the synthetic models share their host arrays (every block has its own copy in HBM: the traffic is the real model's)."""
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
HBM_BYTES_PER_S = 8e12


def f16_model(hp, seed=1234):
    E, H, HKV, FF, V = hp["n_embd"], hp["n_head"], hp["n_head_kv"], hp["n_ff"], hp["n_vocab"]
    rng = np.random.default_rng(seed)

    def mat(rows, k):
        return (rng.standard_normal((rows, k), dtype=np.float32) * np.float32(0.02)).astype(np.float16)

    def ln():
        return ((1.0 + 0.02 * rng.standard_normal(E)).astype(np.float32), (0.02 * rng.standard_normal(E)).astype(np.float32))
    lw = dict(qkv=mat((H + 2 * HKV) * 64, E), wo=mat(E, E), up=mat(FF, E), down=mat(E, FF))
    lw["ln_w"], lw["ln_b"] = ln()
    if hp.get("two_norms"):
        lw["ln2_w"], lw["ln2_b"] = ln()
    m = dict(hparams=dict(hp), wtype=g.F16, layers=[lw] * hp["n_layer"])
    m["tok_emb"] = mat(V, E)
    m["lm_head"] = m["tok_emb"]
    m["out_norm_w"], m["out_norm_b"] = ln()
    return m


def q8_model(hp, seed=1234):
    one = synth.make_model_fast(dict(hp, n_layer=1), g.Q8_0, seed=seed)
    one["hparams"] = dict(hp)
    one["layers"] = one["layers"] * hp["n_layer"]
    return one


def median(xs):
    return float(np.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_7b.json"))
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    a = ap.parse_args()
    g.init(0)
    L = g.load()
    hp = dict(synth.HP_7B, n_layer=a.layers)
    S, R = a.steps, a.reps
    res = dict(model="Falcon-7B shape, %d blocks, synthetic" % a.layers, n_ctx=N_CTX, steps=S, reps=R)

    def timed(f, per):
        f()
        xs = []
        for _ in range(R):
            t0 = time.perf_counter()
            f()
            xs.append((time.perf_counter() - t0) / per * 1e3)
        return xs

    model = g.FalconModel(f16_model(hp), n_ctx=N_CTX, n_batch=128)
    wbytes = model.weight_bytes()
    roof_ms = wbytes / HBM_BYTES_PER_S * 1e3
    res["f16_weight_bytes"] = int(wbytes)
    res["f16_roofline_ms_per_step"] = roof_ms

    def entry(xs, tokens_per_step=1):
        ms = median(xs)
        return dict(ms=ms, samples_ms=xs, tok_per_s=tokens_per_step * 1e3 / ms, roofline_share=roof_ms / ms)

    res["f16_decode"] = entry(timed(lambda: model.decode_greedy(11, 64, S, use_graph=True), S))
    prompt = synth.tokens(128, hp["n_vocab"], seed=3)
    res["f16_prompt_128"] = entry(timed(lambda: model.eval(prompt, 0, logits_all=False), 1), 128)
    for B in (16, 64):
        sc = g.SeqContext(model, N_CTX, B)
        first = synth.tokens(B, hp["n_vocab"], seed=5)
        pos = [(37 * t) % 512 for t in range(B)]
        res["f16_lockstep_%d" % B] = entry(timed(lambda: sc.decode_greedy(first, pos, 4, use_graph=True), 4), B)
        sc.free()
    model.free()

    q8 = g.FalconModel(q8_model(hp), n_ctx=N_CTX, n_batch=1)
    L.ggml_hip_reference_order(1)
    try:
        xs = timed(lambda: q8.decode_greedy(11, 64, 4, use_graph=False), 4)
    finally:
        L.ggml_hip_reference_order(0)
    q8.free()
    res["q8_0_reference_order_1_decode"] = dict(ms=median(xs), samples_ms=xs, tok_per_s=1e3 / median(xs))
    res["f16_decode_not_slower_than_floor"] = bool(res["f16_decode"]["ms"] <= res["q8_0_reference_order_1_decode"]["ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    if not res["f16_decode_not_slower_than_floor"]:
        sys.exit("F16 decode is slower than the one-thread-per-output instrument: the lanes are not streaming")


if __name__ == "__main__":
    main()

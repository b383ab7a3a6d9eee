#!/usr/bin/env python3
"""which kernels run (GPU): one pass over every launch form of the model paths, for a kernel trace that two commits can be compared by --
    rocprofv3 --kernel-trace --stats -- python scripts/gpu_launch_lists.py [7b|40b ...] [q4_0|q5_1|q4_k|q2_k ...]
The per-kernel call counts of the stats file are the launch lists' fingerprint: the template arguments in the kernel names carry the tile cfg and the K split
(k_gemm_q<TYPE, S, TT, RB>, k_gemm_skinny<TYPE, S>, ..). Public Python API only, so that the script runs unchanged on an older commit.
Synthetic two-block models of the 7B-like (4608 / 18432) and the 40B (8192 / 32768) widths; per model: prompts of 1 .. 384 tokens, lock-step contexts of 2 .. 64
sequences, a greedy and a sampled decode loop, draft-and-verify passes, the fused modes, and for the legacy formats the reference orders.
LAUNCH_LISTS_GRAPH=1 adds the same steps through the captured graphs -- not under the tracer: stream capture under rocprofv3's kernel trace has crashed it
(scripts/gpu_prof.sh), and a replayed graph holds the launches the plain step makes."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ggllm_cpp_amd as g
from ggllm_cpp_amd import synth

SHAPES = {"7b": dict(n_vocab=512, n_embd=4608, n_head=72, n_head_kv=2, n_layer=2, n_ff=18432, two_norms=True),
          "40b": dict(n_vocab=512, n_embd=8192, n_head=128, n_head_kv=8, n_layer=2, n_ff=32768, two_norms=True)}
TYPES = {"q4_0": g.Q4_0, "q5_1": g.Q5_1, "q4_k": g.Q4_K, "q2_k": g.Q2_K}
PROMPTS = [1, 4, 5, 16, 17, 32, 33, 128, 288, 384]
SEQS = [2, 3, 4, 8, 16, 32, 33, 64]
N_CTX = 512
GRAPH = os.environ.get("LAUNCH_LISTS_GRAPH", "0") != "0"
if not GRAPH:
    os.environ["FALCON_HIP_STAGE_GRAPH"] = "0"          # (the stage steps as plain launches too)

args = [a.lower() for a in sys.argv[1:]]
shapes = [s for s in SHAPES if s in args] or list(SHAPES)
types = [t for t in TYPES if t in args] or list(TYPES)

g.init(0)
L = g.load()
for shape in shapes:
    hp = SHAPES[shape]
    toks = synth.tokens(max(PROMPTS), hp["n_vocab"], seed=42)
    for tname in types:
        legacy = tname in ("q4_0", "q5_1")
        m = g.FalconModel(synth.make_model_fast(hp, TYPES[tname], seed=7), n_ctx=N_CTX, n_batch=max(PROMPTS))
        for N in PROMPTS:
            m.eval(toks[:N], 0, logits_all=False)
        for B in SEQS:
            sc = g.SeqContext(m, 64, B)
            sc.eval(toks[:B], 0)
            sc.decode_greedy(toks[:B], [1] * B, 1, use_graph=GRAPH)
            sc.free()
        m.eval(toks[:16], 0, logits_all=False)
        m.decode_greedy(int(toks[16]), 16, 4, use_graph=False)
        if GRAPH:
            m.decode_greedy(int(toks[16]), 16, 4, use_graph=True)
        m.set_sampling(g.sampling(seed=1234), toks[:16].tolist())
        m.decode_sample(int(toks[16]), 16, 4, use_graph=False)
        if GRAPH:
            m.decode_sample(int(toks[16]), 16, 4, use_graph=True)
        for K in (1, 3, 7):
            m.eval(toks[:16], 0, logits_all=False)
            m.set_sampling(g.sampling(seed=1234), toks[:16].tolist())
            m.set_spec(K, g.SPEC_GIVEN)
            m.set_spec_guess([1] * 16)
            m.decode_spec(int(toks[16]), 16, 8)
        m.set_spec(0)
        for mode in (0, 1, 2, 3, 5):
            m.set_fused(mode)
            m.eval(toks[16:17], 16, logits_all=False)
            if GRAPH:
                m.eval_token(int(toks[17]), 17)
        m.set_fused(2)
        if legacy:
            for order in (1, 2):
                L.ggml_hip_reference_order(order)
                try:
                    for N in (1, 2, 5, 17, 128, 288):
                        m.eval(toks[:N], 0, logits_all=False)
                    m.eval(toks[17:18], 17, logits_all=False)
                    sc = g.SeqContext(m, 64, 4)
                    sc.eval(toks[:4], 0)
                    sc.free()
                finally:
                    L.ggml_hip_reference_order(0)
        assert m.sync_error() == 0
        m.free()
        print("%s %s: done" % (shape, tname), flush=True)

"""one prompt-attention launch under the process's FQ_ATTN_* switches (read once per process, so a case is a process):
    python scripts/gpu_attn_plan_case.py H HKV N n_past out.npz
prints the plan the default form takes (csrc/fq_attn_forms.h, through ggml_hip_debug_attention_plan) and saves the outputs of the default order (form 0 and
form 32) and of reference order 1 for tests/test_gpu_block_ops.py::test_attention_switches_reach_their_plans, which owns the inputs (attn_case_inputs) and the bounds"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ggllm_cpp_amd as g


def attn_case_inputs(H, HKV, N, n_past, D=64):
    rng = np.random.default_rng(H * 1000 + N + n_past)
    return (rng.standard_normal((N, H + 2 * HKV, D)).astype(np.float32), rng.standard_normal((n_past + N, HKV, D)).astype(np.float32),
            rng.standard_normal((n_past + N, HKV, D)).astype(np.float32))


def main():
    H, HKV, N, n_past = (int(a) for a in sys.argv[1:5])
    D = 64
    g.init(0)
    L = g.load()
    qkv, kc, vc = attn_case_inputs(H, HKV, N, n_past)
    qb, kb, vb, ob_ = g.DevBuf(host=qkv), g.DevBuf(host=kc), g.DevBuf(host=vc), g.DevBuf(N * H * D * 4)
    plan = (C.c_longlong * 16)()
    L.ggml_hip_debug_attention_plan(N, H, HKV, D, n_past, plan)
    print("plan family %d R %d lds %d scratch %d" % (plan[0], plan[1], plan[12], plan[14]), flush=True)

    def run():
        L.ggml_hip_memset(ob_.ptr, 0xFF, N * H * D * 4)
        L.ggml_hip_attention(qb.ptr, N, H, HKV, D, n_past, kb.ptr, vb.ptr, ob_.ptr)
        return ob_.to_host(np.float32, (N, H * D))

    got = run()
    L.ggml_hip_debug_attention_form(32)
    got32 = run()
    L.ggml_hip_debug_attention_form(0)
    L.ggml_hip_reference_order(1)
    got64 = run()
    L.ggml_hip_reference_order(0)
    np.savez(sys.argv[5], got=got, got32=got32, got64=got64, plan=np.array(list(plan), np.int64))


if __name__ == "__main__":
    main()

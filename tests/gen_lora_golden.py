"""Writes tests/golden/lora.npz from the REAL reference (oracle/_ref/libfalcon_ref.so, built by `make -C oracle ref_falcon ref_scalar`): CPU only,
and only where the reference's sources were there to build it.  python tests/gen_lora_golden.py

Per case of lora_ref.CASES: the synthetic model, the adapter and (where the case has one) the base model file are written from their seeds; the
reference loads the model without mmap, merges the adapter with its own llama_apply_lora_from_file and evaluates a 9-token prompt and three single-token
steps. The file records those logits, the tokens, the sha256 of the input files and of every composed target matrix.
It asserts, case by case, that a model file COMPOSED by tests/lora_ref.py (numpy + the reference's quantizers) and loaded by the reference plainly gives
the same logits bit for bit: the fixture proves the helper the GPU tests compare bytes against."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ggcc_writer  # noqa: E402
import lora_ref as lr  # noqa: E402
from oracle import binding as ob  # noqa: E402


def one_case(name, out_path):
    """a process of its own per case: the reference's library keeps ggml contexts across loads and runs out of them after a dozen models"""
    ob.build_oracle()
    oracle = ob.Oracle()
    ref = lr.Reference()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        c = lr.build_case(oracle, name, d)
        V, tok = c["hp"]["n_vocab"], c["tokens"]
        merged = ref.logits(c["model"], V, tok, lr.N_PROMPT, adapter=c["adapter"], base=c["base"])
        plain = ref.logits(c["model"], V, tok, lr.N_PROMPT)
        composed = lr.compose_case(c)
        path = os.path.join(d, name + "_composed.bin")
        ggcc_writer.write_ggcc(path, composed)
        direct = ref.logits(path, V, tok, lr.N_PROMPT)
        assert np.isfinite(merged).all() and not np.array_equal(merged, plain), name
        assert np.array_equal(merged.view(np.uint32), direct.view(np.uint32)), "%s: the composed expectation is not the reference's merge" % name
        changed = []
        for key in dict.fromkeys(k for k, _, _ in c["pairs"]):
            a, b = np.asarray(lr.get_matrix(c["weights"], key)).view(np.uint8), np.asarray(lr.get_matrix(composed, key)).view(np.uint8)
            changed.append(float(np.mean(a != b)))
            out["%s.sha.%s" % (name, lr.tensor_name(key))] = np.array(lr.sha256_bytes(lr.get_matrix(composed, key)))
        assert min(changed) > 0.5, "%s: an adapter that leaves %s of a target's bytes alone proves little" % (name, 1 - min(changed))
        out[name + ".logits"] = merged
        out[name + ".tokens"] = tok
        out[name + ".model_sha256"] = np.array(lr.sha256_file(c["model"]))
        out[name + ".adapter_sha256"] = np.array(lr.sha256_file(c["adapter"]))
        if c["base"]:
            out[name + ".base_sha256"] = np.array(lr.sha256_file(c["base"]))
        print("%-14s ok: %d pairs, bytes changed per target %s" % (name, len(c["pairs"]), " ".join("%.2f" % x for x in changed)), flush=True)
    np.savez(out_path, **out)


def main():
    assert os.path.exists(lr.REF_SO) and lr.have_reference(), "the reference's build (oracle/_ref) is needed"
    if len(sys.argv) == 4 and sys.argv[1] == "--case":
        return one_case(sys.argv[2], sys.argv[3])
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name in lr.CASES:
            part = os.path.join(d, name + ".npz")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--case", name, part], stderr=subprocess.DEVNULL)
            with np.load(part) as z:
                out.update({k: z[k] for k in z.files})
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "lora.npz"), **out)


if __name__ == "__main__":
    main()

"""CPU: the LoRA adapter reader (ggllm.cpp_amd/csrc/fq_lora.h) and the helper the GPU tests compare against (tests/lora_ref.py).
  * the reader's codes on a corpus of damaged files (lora_ref.damaged_corpus), through a stand-alone host program (tests/host/lora_parse_main.cpp, built with
    -fsanitize=address,undefined where the compiler has the runtimes) and through the library's host-only falcon_hip_lora_scan;
  * the composed expectation against the real reference (llama_apply_lora_from_file of oracle/_ref/libfalcon_ref.so), where that was built."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ggllm_cpp_amd as g
import lora_ref as lr
import synth
from oracle import binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = synth.HP_TINY_MQA
REF_SO = lr.REF_SO


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return lr.damaged_corpus(str(tmp_path_factory.mktemp("lora_corpus")), HP)


def test_corpus_covers_every_reader_code(corpus):
    assert {c for _, _, c in corpus} == set(range(0, 14))
    assert sum(1 for label, _, _ in corpus if label.startswith("cut_")) >= 20


def test_reader_codes_standalone_program(corpus, tmp_path):
    """every file of the corpus from an exact-size heap buffer, in a process of its own (nothing sanitized is loaded into python)"""
    exe, src = str(tmp_path / "lora_parse_main"), os.path.join(ROOT, "tests", "host", "lora_parse_main.cpp")
    base = ["g++", "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "ggllm.cpp_amd", "csrc"), "-o", exe, src]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(base)                                    # (a compiler without the sanitizer runtimes: the codes are still checked)
    args = [str(HP[k]) for k in ("n_vocab", "n_embd", "n_head", "n_head_kv", "n_layer", "n_ff")]
    for _, path, code in corpus:
        args += [path, str(code)]
    res = subprocess.run([exe] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def test_lora_scan_codes(corpus):
    g.build()
    for label, path, code in corpus:
        if code == 0:
            r, alpha, n = g.lora_scan(path, HP)
            assert (r, alpha) == (3, 6) and n == {"good": 2, "cut_16": 0}.get(label, 1), label
        else:
            with pytest.raises(g.LoraError) as e:
                g.lora_scan(path, HP)
            assert e.value.code == code, label


def test_lora_scan_good_files(tmp_path):
    """either half first, a name twice, F16 loraA, every kind of target, r from 1 to 40; and the same file against another model's hparams"""
    g.build()
    keys = [(0, "qkv"), (0, "wo"), (1, "up"), (1, "down"), "lm_head", "tok_emb"]
    for r, a_f16, b_first in ((1, False, False), (5, True, False), (40, False, True)):
        ad = lr.draw_adapter(HP, keys, r, seed=5, a_f16=a_f16)
        pairs = [(k,) + ad[k] for k in keys] + [(keys[0],) + ad[keys[0]]]
        path = str(tmp_path / ("ok_%d.bin" % r))
        lr.write_ggla(path, r, 16, lr.adapter_records(pairs, b_first=b_first))
        assert g.lora_scan(path, HP) == (r, 16, 7)
        with pytest.raises(g.LoraError) as e:
            g.lora_scan(path, synth.HP_TINY_GQA)
        assert e.value.code == lr.E_SHAPE


def test_low_rank_is_the_sequential_f64_chain():
    """the vectorised helper against the definition, element by element, on values whose f32 products round"""
    rng = np.random.default_rng(3)
    A = (rng.standard_normal((7, 5)) * 0.05).astype(np.float32)
    B = (rng.standard_normal((4, 5)) * 0.05).astype(np.float32)
    for alpha, r_header in ((10, 5), (5, 5)):
        ba = lr.low_rank(A, B, r_header, alpha)
        for m in range(4):
            for k in range(7):
                s = 0.0
                for i in range(5):
                    s += float(np.float32(A[k, i] * B[m, i]))
                v = np.float32(s)
                if alpha != r_header:
                    v = np.float32(v * (np.float32(alpha) / np.float32(r_header)))
                assert ba[m, k] == v
    A16 = A.astype(np.float16)
    assert np.array_equal(lr.low_rank(A16, B, 5, 5), lr.low_rank(A16.astype(np.float32), B.astype(np.float16).astype(np.float32), 5, 5))


# ------------------------------------------------------------------------------------------------ against the real reference
@pytest.mark.skipif(not (os.path.exists(REF_SO) and ob.Ref.available(scalar=True)), reason="oracle/_ref (the reference's own build) is absent")
def test_composed_expectation_is_the_references_merge(tmp_path, oracle):
    """one fresh case beyond the recorded ones (tests/gen_lora_golden.py asserts the same for each of those): the reference's logits after its own merge
    equal its logits on a model file composed by lora_ref"""
    import ggcc_writer
    hp, wt = HP, ob.Q5_0
    w = synth.make_model(oracle, hp, wt, seed=4321)
    keys = [(0, "up"), (1, "wo"), "lm_head"]
    ad = lr.draw_adapter(hp, keys, 6, seed=11)
    pairs = [(k,) + ad[k] for k in keys]
    model, patched, adapter = str(tmp_path / "m.bin"), str(tmp_path / "p.bin"), str(tmp_path / "a.bin")
    ggcc_writer.write_ggcc(model, w)
    lr.write_ggla(adapter, 6, 16, lr.adapter_records(pairs))
    composed = lr.compose(w, pairs, 6, 16)
    ggcc_writer.write_ggcc(patched, composed)
    changed = np.mean(np.asarray(composed["lm_head"]) != np.asarray(w["lm_head"]))
    assert changed > 0.5, "the adapter must move the weights (%.2f of the bytes changed)" % changed
    ref = lr.Reference()
    tok = synth.tokens(12, hp["n_vocab"], seed=77)
    merged = ref.logits(model, hp["n_vocab"], tok, 9, adapter=adapter)
    plain = ref.logits(model, hp["n_vocab"], tok, 9)
    direct = ref.logits(patched, hp["n_vocab"], tok, 9)
    assert not np.array_equal(merged, plain)
    assert np.array_equal(merged.view(np.uint32), direct.view(np.uint32))

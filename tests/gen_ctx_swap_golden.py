"""Writes tests/golden/ctx_swap.npz from the REAL reference: CPU only, and only where the reference's sources were there to build it.
    python tests/gen_ctx_swap_golden.py

The reference's falcon_main is built in a temporary directory from its unchanged sources and the scalar objects of `make -C oracle ref_falcon`
(as gen_cli in oracle/gen_golden.py builds it; nothing of it is kept) and run on the tiny byte-level-BPE model with -c 32, so that every case of
ctx_swap_ref.CASES runs out of context at least twice. Stored per case: the bytes falcon_main printed, and from --verbose-prompt's stderr the
token ids of every `#CONTEXT_RESET_START: embd.size(): N ... #RESET_END` block -- the regenerated tokens and the waiting one -- with N, flat
with the block lengths beside them. N comes from the header: a token's text may itself hold '(', ')' and digits, so the entries are taken
from the back -- the last `(id) `, then that token's own bytes -- and must use the body up exactly.

The generator also asserts, case by case, that the planner restated in ctx_swap_ref.py reproduces every block from the case's own token
stream (the tokens of stdout behind the prompt)."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ctx_swap_ref as cr  # noqa: E402
import ggllm_cpp_amd as g  # noqa: E402
from oracle import binding as ob  # noqa: E402
from oracle import gen_golden as gg  # noqa: E402

REF = "/root/reference"


def build_main(td):
    obj = os.path.join(ROOT, "oracle", "_ref", "obj")
    sc = "-march=x86-64 -mno-sse3 -mno-ssse3 -mno-avx -mno-avx2 -mno-fma -mno-f16c".split()
    subprocess.check_call("sh %s/scripts/build-info.sh > build-info.h 2>/dev/null" % REF, shell=True, cwd=td)
    objs = [os.path.join(obj, f) for f in ("libfalcon.o", "cmpnct_unicode.o", "ggml.o", "k_quants.o")]
    exe = os.path.join(td, "falcon_main")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-pthread", *sc, "-DGGML_USE_K_QUANTS", "-I" + REF, "-I" + REF + "/examples", "-I" + td,
                           os.path.join(REF, "examples/falcon/falcon_main.cpp"), os.path.join(REF, "examples/falcon_common.cpp"), *objs, "-lm", "-o", exe],
                          stderr=subprocess.DEVNULL)
    return exe


def reset_blocks(stderr, vocab):
    """[[ids]] of every reset block of falcon_main's stderr"""
    blocks = []
    for m in re.finditer(rb"#CONTEXT_RESET_START: embd\.size\(\): (\d+)\n(.*?) #RESET_END\n", stderr, re.S):
        n, body = int(m.group(1)), m.group(2)
        ids = []
        for _ in range(n):                                   # from the back: "...text(id) " -- the id is the entry's last parenthesis, its text the token's own bytes
            e = re.search(rb"\((\d+)\) $", body, re.S)
            assert e, body
            ids.append(int(e.group(1)))
            text = vocab.token_bytes(ids[-1])
            assert body[:e.start()].endswith(text), (body, text)
            body = body[:e.start() - len(text)]
        assert body == b"" and len(ids) == n, (n, body)
        blocks.append(ids[::-1])
    return blocks


def drawn_stream(vocab, text, prompt_ids, n_predict, n_batch, keep, n_system, blocks):
    """The ids falcon_main drew, which it never prints: THE split of the printed bytes into n_predict tokens that agrees with the reset blocks. Where
    the swaps fall depends on counts alone, so a replay over placeholders says which draws each block names; the rest follows from the bytes if
    exactly one split fits -- asserted."""
    marks = [-1 - i for i in range(n_predict)]
    known = {}
    for (_, want), got in zip(cr.replay(prompt_ids, marks, cr.N_CTX, n_batch, keep, n_system), blocks):
        assert len(want) == len(got)
        for m, t in zip(want, got):
            if m < 0:
                known[-1 - m] = t
            else:
                assert m == t                                # (a prompt-batch-last token pulled in by the clamp)
    by_first = {}
    for t in range(vocab.n_vocab):
        b = vocab.token_bytes(t)
        if b:
            by_first.setdefault(b[0], []).append((t, b))
    ways = {}

    def count(i, pos):                                       # splits of text[pos:] into draws i .., capped at 2
        if i == n_predict:
            return 1 if pos == len(text) else 0
        if pos >= len(text):
            return 0
        if (i, pos) not in ways:
            n = 0
            for t, b in by_first.get(text[pos], ()):
                if known.get(i, t) == t and text.startswith(b, pos):
                    n = min(2, n + count(i + 1, pos + len(b)))
            ways[(i, pos)] = n
        return ways[(i, pos)]

    assert count(0, 0) == 1, "%d splits of the text fit the blocks" % count(0, 0)
    out, pos = [], 0
    for i in range(n_predict):
        for t, b in by_first[text[pos]]:
            if known.get(i, t) == t and text.startswith(b, pos) and count(i + 1, pos + len(b)) == 1:
                out.append(t)
                pos += len(b)
                break
    return out


def main():
    assert os.path.isdir(REF) and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "obj", "libfalcon.o")), "the reference's build (make -C oracle ref_falcon) is needed"
    ob.build_oracle()
    O = ob.Oracle()
    d = {}
    with tempfile.TemporaryDirectory() as td:
        exe = build_main(td)
        path = os.path.join(td, "tiny_bpe.ggcc")
        gg.cli_model(O, path)
        vocab = g.Vocab(path)
        for name, (prompt, n_predict, n_batch, seed, keep, system, flags) in cr.CASES.items():
            r = subprocess.run([exe, "-m", path, "--verbose-prompt", *cr.main_args(name)], capture_output=True)
            assert r.returncode == 0, r.stderr[-2000:]
            blocks = reset_blocks(r.stderr, vocab)
            assert len(blocks) >= 2, (name, len(blocks))
            sys_ids = vocab.tokenize(system, add_bos=False).tolist() if system else []
            ids = sys_ids + vocab.tokenize(prompt, add_bos=False).tolist()
            head = vocab.detokenize(ids)
            assert r.stdout.startswith(head), (name, r.stdout[:80], head)
            drawn = drawn_stream(vocab, r.stdout[len(head):], ids, n_predict, n_batch, keep, len(sys_ids), blocks)
            assert [b for _, b in cr.replay(ids, drawn, cr.N_CTX, n_batch, keep, len(sys_ids))] == blocks, name
            d[name + ".drawn"] = np.array(drawn, np.int32)
            d[name + ".stdout"] = np.frombuffer(r.stdout, np.uint8)
            d[name + ".prompt_ids"] = np.array(ids, np.int32)
            d[name + ".n_system"] = np.array(len(sys_ids), np.int32)
            d[name + ".block_len"] = np.array([len(b) for b in blocks], np.int32)
            d[name + ".block_ids"] = np.array([t for b in blocks for t in b], np.int32)
            print("%-16s prompt %2d, blocks %s" % (name, len(ids), [len(b) for b in blocks]), flush=True)
            print("    %r" % r.stdout)
        vocab.free()
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ctx_swap.npz"), **d)


if __name__ == "__main__":
    main()

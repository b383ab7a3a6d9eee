"""The stop rule of csrc/fq_stop.h + csrc/fq_stop_text.h restated in a few lines of Python (bytes.find over the growing text), and
the synthetic vocabularies the stop-text tests draw from. Shared by tests/test_stop_text_cpu.py and tests/test_gpu_stop_text.py."""
import struct

import numpy as np

RUNNING, BUDGET, TEXT0 = -1, -2, 16


class Restated:
    """one row: id sequences and a budget (set_ids), stop strings (set_text); draw(token, its bytes) -> (reason, n_drawn, cut_bytes)"""

    def __init__(self):
        self.seqs, self.max_tokens, self.strings = [], 0, []
        self.fresh()

    def fresh(self):
        self.ids, self.text, self.reason, self.cut = [], b"", RUNNING, 0

    def set_ids(self, seqs, max_tokens=0):
        self.seqs, self.max_tokens = [list(q) for q in seqs], max_tokens
        self.fresh()

    def set_text(self, strings):
        self.strings = [bytes(s) for s in strings]
        self.fresh()

    def draw(self, token, b):
        assert self.reason == RUNNING                      # (a row that has ended is not drawn for)
        before = len(self.text)
        self.ids.append(token)
        self.text += b
        n = len(self.ids)
        for k, q in enumerate(self.seqs):                   # fq_stop.h: the lowest id sequence that the drawn tokens end with ...
            if len(q) <= n and self.ids[n - len(q):] == q:
                self.reason = k
                break
        else:
            if self.max_tokens > 0 and n == self.max_tokens:          # ... else the budget
                self.reason = BUDGET
            # fq_stop_text.h: the string that completes first inside the new token (find from the first place that ends in it), the lowest k of those
            ends = [(at + len(s), k) for k, s in enumerate(self.strings) for at in [self.text.find(s, max(0, before - len(s) + 1))] if at >= 0]
            if ends:
                end, k = min(ends)
                self.reason, self.cut = TEXT0 + k, len(self.text) - (end - len(self.strings[k]))
        return self.reason, n, self.cut


def abc_vocab(rng, n=50):
    """about 50 tokens over a three-letter alphabet, so that matches and overlaps are frequent; the lengths include 0, 1, 31, 32, 33, 64, 65
    and 130, the rest are short"""
    lens = [0, 1, 31, 32, 33, 64, 65, 130] + [int(x) for x in rng.integers(1, 5, n - 8)]
    return [bytes(rng.integers(97, 100, l, dtype=np.uint8)) for l in lens]


def pool_of(vocab):
    """(pool uint8, offsets int32 [n + 1]) of a list of byte strings: what ggml_hip_sampler_set_vocab_bytes takes"""
    offs = np.zeros(len(vocab) + 1, np.int32)
    offs[1:] = np.cumsum([len(b) for b in vocab])
    pool = np.frombuffer(b"".join(vocab) or b"\0", np.uint8).copy()
    return pool, offs


def coded_vocab(n):
    """n tokens with bytes of their own: token t reads 'Xyz' + some dots, X a capital and yz small letters that spell t, so a text cut from
    the middle of one token to the middle of the next but one holds a whole token and can be found nowhere else unless that token recurs.
    Ids 0..11 (the tokenizer's special tokens) read '<t>'"""
    out = []
    for t in range(n):
        out.append(("<%d>" % t).encode() if t < 12 else bytes([65 + t % 26, 97 + (t // 26) % 26, 97 + t // 676]) + b"." * (1 + t % 3))
    return out


def write_vocab_ggcc(path, vocab):
    """a GGCC v10 file that holds a vocabulary and nothing behind it: all falcon_hip_vocab_load_ggcc reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<II", 0x67676363, 10))
        f.write(struct.pack("<8I", len(vocab), 0, 0, 0, 0, 7, 0, 0))
        for w in vocab:
            f.write(struct.pack("<I", len(w)) + w + struct.pack("<f", 0.0))
        f.write(struct.pack("<I", 0))

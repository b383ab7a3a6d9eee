#!/usr/bin/env python3
"""How likely is each continuation? Multiple-choice scoring on one MI355X without a logit leaving the device.

    python examples/falcon_score.py --model falcon-7b-q4_0.ggcc --prompt "The capital of France is" " Paris" " London" " a city"

For every candidate continuation it prints the summed log-probability of its tokens given the prompt (natural log, the
reference's soft-max: falcon_perplexity.cpp:12-27) and the token count. Steps: the prompt is evaluated ONCE
(falcon_hip_eval_score, the target on its last row = a candidate's first token; one more eval_score of the last prompt
token per further distinct first token), then each candidate is evaluated at n_past = len(prompt) over the same cache
prefix -- the KV cache is append-only, so evaluating at a position again overwrites what an earlier candidate left there.
Per call n_tokens probabilities cross the bus instead of n_tokens x n_vocab logits."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ggllm_cpp_amd as g  # noqa: E402


def score_candidates(model_path, prompt, candidates, n_ctx=2048, device=0, add_bos=False):
    """returns (prompt ids, [(candidate ids, summed log-probability, token count)]); the sum is a float64 that takes
    log(float64(prob)) token by token, in order"""
    g.init(device)
    vocab = g.Vocab(model_path)
    try:
        ids = vocab.tokenize(prompt, add_bos=add_bos)
        cands = [vocab.tokenize(c, add_bos=False) for c in candidates]
    finally:
        vocab.free()
    if ids.size == 0 or any(c.size == 0 for c in cands):
        raise ValueError("empty prompt or candidate")
    n = int(ids.size)
    if n + max(int(c.size) for c in cands) > n_ctx:
        raise ValueError("prompt + candidate exceed n_ctx")
    model = g.FalconModel.from_ggcc(model_path, n_ctx=n_ctx, n_batch=max(n, max(int(c.size) for c in cands)))
    try:
        first_prob = {}
        for c in cands:
            t = int(c[0])
            if t in first_prob:
                continue
            if not first_prob:                                   # the whole prompt, once
                tg = np.full(n, -1, np.int32)
                tg[-1] = t
                first_prob[t] = model.score(ids, 0, tg)[-1]
            else:                                                # its last token again, for another target
                first_prob[t] = model.score(ids[-1:], n - 1, [t])[0]
        out = []
        for c in cands:
            lp = float(np.log(np.float64(first_prob[int(c[0])])))
            if c.size > 1:
                tg = np.append(c[1:], -1).astype(np.int32)       # row i of the candidate predicts its token i + 1
                for p in model.score(c, n, tg)[:-1]:
                    lp += float(np.log(np.float64(p)))
            out.append((c, lp, int(c.size)))
        return ids, out
    finally:
        model.free()


def format_line(text, logprob, count):
    return "%12.6f  %3d tokens  %r" % (logprob, count, text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True)
    ap.add_argument("--prompt", required=True)
    ap.add_argument("candidates", nargs="+", help="continuations to score (mind the leading space of a word)")
    ap.add_argument("--n-ctx", type=int, default=2048)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    _, res = score_candidates(a.model, a.prompt, a.candidates, a.n_ctx, a.device)
    for text, (_, lp, cnt) in zip(a.candidates, res):
        print(format_line(text, lp, cnt))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Text to vector on one MI355X: the ln_f rows of a Falcon model, pooled on the device.

    python examples/falcon_embedding.py --model falcon-7b-q4_0.ggcc -p "The capital of France is Paris."
    python examples/falcon_embedding.py --model falcon-7b-q4_0.ggcc -f texts.txt --out vectors.npy --similarity

One text per line of the file (or the one given with -p). Each text is evaluated from an empty context in chunks of n_batch tokens
through falcon_hip_embed -- an eval that ends after ln_f: no lm_head, no logits -- and becomes one vector of n_embd floats:

  --pool mean   (default) the mean over every token's ln_f row, summed per column in f64 in position order on the device
                (csrc/kernels_embed.hip), at unit length unless --no-normalize;
  --pool last   the last token's row: what the reference's falcon_get_embeddings returns (with GGML_HIP_REFERENCE_ORDER=1 or 2 in
                the environment bit for bit), as it is unless --normalize.

Without --out the vectors are printed as the reference's examples/embedding/embedding.cpp prints its one: every value with "%f "
and a new line. --similarity prints the cosine matrix of the texts."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ggllm_cpp_amd as g  # noqa: E402


def embed_texts(model_path, texts, pool="mean", normalize=True, n_ctx=2048, n_batch=512, device=0, add_bos=False):
    """float32 [len(texts), n_embd]"""
    g.init(device)
    if os.environ.get("GGML_HIP_REFERENCE_ORDER"):
        g.load().ggml_hip_reference_order(int(os.environ["GGML_HIP_REFERENCE_ORDER"]))
    vocab = g.Vocab(model_path)
    try:
        ids = [vocab.tokenize(t, add_bos=add_bos) for t in texts]
    finally:
        vocab.free()
    for t, i in zip(texts, ids):
        if not 1 <= i.size <= n_ctx:
            raise ValueError("%r: %d tokens, the context holds 1..%d" % (t[:40], i.size, n_ctx))
    model = g.FalconModel.from_ggcc(model_path, n_ctx=n_ctx, n_batch=min(n_batch, max(int(i.size) for i in ids)))
    try:
        return np.stack([model.embed(i, pool=pool, normalize=normalize) for i in ids])
    finally:
        model.free()


def format_vector(v):
    """embedding.cpp's loop: printf("%f ", embeddings[i]) for every value, then a new line"""
    return "".join("%f " % float(x) for x in v) + "\n"


def cosine_matrix(v):
    v = v.astype(np.float64)
    n = np.sqrt((v * v).sum(axis=1, keepdims=True))
    return (v / n) @ (v / n).T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("-p", "--prompt")
    src.add_argument("-f", "--file", help="one text per line")
    ap.add_argument("--pool", choices=("mean", "last"), default="mean")
    ap.add_argument("--normalize", dest="normalize", action="store_true", default=None)
    ap.add_argument("--no-normalize", dest="normalize", action="store_false")
    ap.add_argument("--out", help="write the vectors to this .npy file instead of printing them")
    ap.add_argument("--similarity", action="store_true", help="print the cosine matrix of the texts")
    ap.add_argument("--n-ctx", type=int, default=2048)
    ap.add_argument("--n-batch", type=int, default=512)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    texts = [a.prompt] if a.prompt is not None else [line.rstrip("\n") for line in open(a.file, encoding="utf-8") if line.strip()]
    normalize = (a.pool == "mean") if a.normalize is None else a.normalize
    v = embed_texts(a.model, texts, a.pool, normalize, a.n_ctx, a.n_batch, a.device)
    if a.out:
        np.save(a.out, v)
    else:
        for row in v:
            sys.stdout.write(format_vector(row))
    if a.similarity:
        for row in cosine_matrix(v):
            print(" ".join("%8.5f" % x for x in row))


if __name__ == "__main__":
    main()

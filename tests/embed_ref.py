"""The pooled text vector of csrc/fq_embed.h restated in numpy: the statement tests/test_embed_cpu.py pins by hand and tests/test_gpu_embed.py
holds the kernels (csrc/kernels_embed.hip) against, bit for bit.

    acc[col]  = ((0.0 + row[0][col]) + row[1][col]) + ...          one f64 chain per column, in row order, carried across calls
    mean[col] = float32(acc[col] / float64(count))
    s         = the f64 sum of float64(mean[col])**2: THREADS strided partial chains (columns t, t + THREADS, ...), then the partials in order
    out[col]  = float32(float64(mean[col]) / sqrt(s))

np.cumsum adds sequentially, which is the chain; np.sum is pairwise and is not.
"""
import numpy as np

THREADS = 256         # FQ_EMBED_THREADS


def accumulate(rows, acc=None, count=0):
    """(acc float64 [n_embd], count) after the rows (float32 [n, n_embd]) were added to a running (acc, count)"""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and rows.ndim == 2
    start = np.zeros((1, rows.shape[1]), np.float64) if acc is None else np.asarray(acc, np.float64).reshape(1, -1)
    chain = np.cumsum(np.concatenate([start, rows.astype(np.float64)]), axis=0, dtype=np.float64)
    return chain[-1].copy(), int(count) + rows.shape[0]


def mean(acc, count):
    assert count > 0
    return (np.asarray(acc, np.float64) / np.float64(count)).astype(np.float32)


def sum_squares(m):
    """s in the kernel's order"""
    sq = np.asarray(m, np.float32).astype(np.float64) ** 2            # (a 24-bit value squared is exact in f64)
    pad = np.zeros((-sq.size) % THREADS, np.float64)                  # (a chain that ends early adds nothing; + 0.0 changes no sum of squares)
    part = np.cumsum(np.concatenate([sq, pad]).reshape(-1, THREADS), axis=0, dtype=np.float64)[-1]
    return np.cumsum(part, dtype=np.float64)[-1]


def unit(m):
    s = sum_squares(m)
    assert s > 0
    return (np.asarray(m, np.float32).astype(np.float64) / np.sqrt(s)).astype(np.float32)


def pooled(rows, normalize, splits=None):
    """the vector of the rows, accumulated in one call or in the consecutive pieces splits = [n0, n1, ...]"""
    acc, n, at = None, 0, 0
    for k in (splits or [len(rows)]):
        acc, n = accumulate(rows[at:at + k], acc, n)
        at += k
    assert at == len(rows)
    m = mean(acc, n)
    return unit(m) if normalize else m


def sum_squares_orders(m):
    """the f64 sum of squares in three other orders: index order, reversed, numpy's pairwise"""
    sq = np.asarray(m, np.float32).astype(np.float64) ** 2
    return np.cumsum(sq, dtype=np.float64)[-1], np.cumsum(sq[::-1], dtype=np.float64)[-1], np.sum(sq, dtype=np.float64)


def order_free(m):
    """True when the unit vector's f32 values do not depend on the order of s: the three orders above and the kernel's give the same bits"""
    m = np.asarray(m, np.float32).astype(np.float64)
    outs = [(m / np.sqrt(s)).astype(np.float32) for s in sum_squares_orders(m) + (sum_squares(m),)]
    return all(np.array_equal(outs[0].view(np.uint32), o.view(np.uint32)) for o in outs[1:])


# ---- the recorded models of tests/golden/embedding.npz (tests/gen_embedding_golden.py) and the rows the oracle gives for them
MODELS = {"mqa_q4_0": ("HP_TINY_MQA", "Q4_0"), "gqa_q5_1": ("HP_TINY_GQA", "Q5_1"), "gqa_q4_k": ("HP_TINY_GQA", "Q4_K")}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def golden_model(oracle, name):
    """(hparams, weights) of a recorded model, from its seed"""
    import synth
    from oracle import binding as ob
    hp_name, t_name = MODELS[name]
    hp = getattr(synth, hp_name)
    return hp, synth.make_model(oracle, hp, getattr(ob, t_name), seed=4321)


def oracle_rows(oracle, w, tokens, pieces, n_ctx=32):
    """the ln_f rows of every position in the reference's order, the tokens evaluated in the consecutive pieces [n0, n1, ...]: float32 [sum(pieces), n_embd]"""
    mo, at, out = oracle.model(w, n_ctx), 0, []
    for n in pieces:
        _, hid = mo.eval(tokens[at:at + n], at, want_hidden=True)
        out.append(oracle.layer_norm(hid[-1], w["out_norm_w"], w["out_norm_b"]))
        at += n
    return np.concatenate(out)


# ---- the operator cases of tests/test_gpu_embed.py, drawn here so that the CPU test checks the very inputs the device sees
ORDER_COLUMN = np.array([2.0 ** 60, 1.0, -2.0 ** 60], np.float32)     # in this order 0 (the 1 is lost under 2^60), with the 1 last 1


def case_rows(n_embd, n_rows, seed):
    """float32 [n_rows, n_embd]: N(0, 1) rows; from 3 rows up the order-sensitive column at columns 0, 63, 64 (where the width has them) and n_embd - 1,
    in rows 0, 1 and n_rows - 1 with zeros between"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_rows, n_embd)).astype(np.float32)
    if n_rows >= 3:
        for col in sorted({0, 63, 64, n_embd - 1}):
            if col < n_embd:
                x[:, col] = 0.0
                x[0, col], x[1, col], x[n_rows - 1, col] = ORDER_COLUMN
    return x


CASE_SHAPES = [(e, n) for e in (64, 256, 4544, 8192) for n in (1, 2, 65, 513)]


def case_splits(n_rows):
    """the same rows over three calls, 1 + 64 + the rest (fewer where there are fewer rows)"""
    out, left = [], n_rows
    for k in (1, 64):
        if left > 0:
            out.append(min(k, left))
            left -= out[-1]
    if left > 0:
        out.append(left)
    return out


def case_seed(n_embd, n_rows):
    """the first seed from 1000 * n_embd + n_rows upwards whose rows give an order-free unit vector (chosen on the CPU, never on the device)"""
    seed = 1000 * n_embd + n_rows
    while not order_free(mean(*accumulate(case_rows(n_embd, n_rows, seed)))):
        seed += 1
    return seed

"""Draft-and-verify decode restated in Python (ggllm.cpp_amd/csrc/fq_spec.h): where a pass's drafts come from, and what a run
of passes looks like when the tokens the sampler draws are known. Passes, draws per pass and the histogram are functions of
the token ids alone -- the drafts never change what is drawn."""

LOOKUP, GIVEN = 1, 2

# the lookup rule by hand: (name, history, ngram_min, ngram_max, K) -> drafts, by hand
LOOKUP_CASES = [
    ("no match", [1, 2, 3, 4, 5], 1, 3, 3, [-1, -1, -1]),
    ("only g = 1", [7, 1, 9, 2, 8, 3, 1], 1, 3, 3, [9, 2, 8]),
    ("g = 1 is below ngram_min", [7, 1, 9, 2, 8, 3, 1], 2, 3, 3, [-1, -1, -1]),
    ("two matches: the later wins", [1, 2, 5, 6, 1, 2, 7, 8, 1, 2], 1, 2, 2, [7, 8]),
    ("a longer g wins over a later j", [3, 1, 2, 5, 9, 2, 6, 0, 1, 2], 1, 2, 2, [5, 9]),
    ("the continuation runs into n", [4, 5, 6, 4, 5], 1, 2, 4, [6, 4, 5, -1]),
    ("overlapping occurrences", [2, 2, 2, 2], 1, 3, 3, [2, -1, -1]),
    ("n < g", [5, 5], 3, 3, 2, [-1, -1]),
    ("n == 1", [5], 1, 3, 2, [-1, -1]),
    ("n == 0", [], 1, 3, 2, [-1, -1]),
]


def lookup(h, ngram_min, ngram_max, K):
    """prompt lookup: h = prompt + draws, h[-1] the pending token. For g = ngram_max down to ngram_min the LARGEST j <= n - g - 1
    with h[j:j+g] == h[n-g:n]; the first g with one gives d_i = h[j + g + i - 1], i = 1..K, -1 where that index is >= n"""
    h = [int(t) for t in h]
    n = len(h)
    for g in range(ngram_max, max(ngram_min, 1) - 1, -1):
        for j in range(n - g - 1, -1, -1):
            if h[j:j + g] == h[n - g:n]:
                return [h[j + g + i - 1] if j + g + i - 1 < n else -1 for i in range(1, K + 1)]
    return [-1] * K


def given(q, s, K):
    """the caller's guess q of the continuation, aligned by the draw's number (q[i] guesses draw i): row i of a pass whose first
    draw is number s stands where draw s + i - 1 will, so d_i = q[s + i - 1]; -1 beyond the guess"""
    return [int(q[s + i - 1]) if s + i - 1 < len(q) else -1 for i in range(1, K + 1)]


def simulate(truth, K, source, history=(), ngram=(1, 3), guess=(), pos=None, n_ctx=0):
    """the passes of a run whose draws are `truth` (every one of them made, none ends the row early). Returns (draws per pass,
    histogram [K + 1]: entry d - 1 counts the passes that made d draws). pos / n_ctx: the pending token's position and the cache's
    length -- a row whose position would be >= n_ctx is never accepted"""
    h = [int(t) for t in history]
    truth = [int(t) for t in truth]
    per_pass, s = [], 0
    while s < len(truth):
        d = lookup(h, ngram[0], ngram[1], K) if source == LOOKUP else given(guess, s, K)
        j = 0
        while True:
            draw = truth[s + j]
            left = len(truth) - (s + j + 1)
            nxt = d[j] if j < K else -1
            room = n_ctx <= 0 or pos is None or pos + s + j + 1 < n_ctx
            if not (j < K and left > 0 and nxt >= 0 and draw == nxt and room):
                break
            j += 1
        per_pass.append(j + 1)
        h.extend(truth[s:s + j + 1])
        s += j + 1
    hist = [0] * (K + 1)
    for d in per_pass:
        hist[d - 1] += 1
    return per_pass, hist

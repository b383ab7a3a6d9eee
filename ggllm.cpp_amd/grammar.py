"""Byte automata for constrained decoding (csrc/fq_grammar.h holds the rule the device applies): a small regular-expression compiler,
the "one of these strings" case, and a constructor for a caller's own table. Host-side and pure Python: nothing here touches the device.

A Dfa is n_states states over bytes: trans uint16 [n_states, 256], accept uint8 [n_states], a start state. State 0 is the dead state
(all its transitions are 0, it never accepts); every other state of a Dfa made here can still reach an accepting state.

regex_dfa(pattern): whole-string matching. Strings are taken as their UTF-8 bytes. Supported, and nothing else:
  literals; the escapes \\n \\t \\r \\\\ \\xHH \\d \\w \\s (ASCII sets) and a backslash in front of any ASCII punctuation character;
  .  (any byte but \\n);  [...] and [^...] with ranges (single bytes and \\d \\w \\s inside);
  groups ( ), alternation |, the quantifiers * + ? {m} {m,n} {m,} (one per atom).
Anything else -- anchors, (?...) groups, lazy or possessive quantifiers, back-references, other escapes, a stray ] { } -- raises
ValueError: the compiler never guesses. The pipeline is NFA -> subset construction -> states that cannot reach an accepting state become
state 0 -> minimisation.
"""
import numpy as np

MAX_STATES = 16384          # FQ_GRAMMAR_MAX_STATES

_DIGIT = frozenset(range(0x30, 0x3A))
_WORD = frozenset(list(range(0x30, 0x3A)) + list(range(0x41, 0x5B)) + list(range(0x61, 0x7B)) + [0x5F])
_SPACE = frozenset(b" \t\n\r\f\v")
_ALL = frozenset(range(256))
_PUNCT = frozenset(b"!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~ ")


class Dfa:
    """a byte automaton in the layout the library takes (ggml_hip_dfa)"""

    def __init__(self, trans, accept, start):
        self.trans = np.ascontiguousarray(trans, dtype=np.uint16)
        self.accept = np.ascontiguousarray(accept, dtype=np.uint8)
        self.n_states = int(self.trans.shape[0])
        self.start = int(start)

    def walk(self, state, data):
        """the state after the bytes of data, from state (0 stays 0)"""
        t = self.trans
        for b in bytes(data):
            if state == 0:
                break
            state = int(t[state, b])
        return state

    def accepts(self, data):
        return bool(self.accept[self.walk(self.start, data)])

    def live(self, data):
        """data is a prefix of some accepted string"""
        return self.walk(self.start, data) != 0


def dfa(trans, accept, start=1):
    """a Dfa from a caller's table: trans [n_states][256] with entries < n_states and state 0 dead, accept [n_states]. ValueError otherwise"""
    t = np.asarray(trans)
    a = np.asarray(accept)
    if t.ndim != 2 or t.shape[1] != 256 or not 1 <= t.shape[0] <= MAX_STATES or a.shape != (t.shape[0],):
        raise ValueError("a table of [n_states][256] transitions and [n_states] accept flags, 1 <= n_states <= %d" % MAX_STATES)
    if t.min() < 0 or t.max() >= t.shape[0]:
        raise ValueError("a transition outside [0, n_states)")
    if t[0].any() or a[0]:
        raise ValueError("state 0 is the dead state: no transition leaves it and it does not accept")
    if not 0 <= int(start) < t.shape[0]:
        raise ValueError("start state %d is outside [0, %d)" % (start, t.shape[0]))
    return Dfa(t, a != 0, start)


# ------------------------------------------------------------------------------------------------ parser: pattern -> syntax tree
# nodes: ("set", frozenset of bytes) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, m, n or None)
class _Parser:
    def __init__(self, pattern):
        if isinstance(pattern, str):
            self.units = [ch.encode("utf-8") for ch in pattern]      # one unit per character: a quantifier takes the whole character
        elif isinstance(pattern, (bytes, bytearray)):
            self.units = [bytes([b]) for b in bytes(pattern)]
        else:
            raise TypeError("a pattern is str or bytes")
        self.i = 0

    def err(self, what):
        raise ValueError("regex_dfa: %s at position %d" % (what, self.i))

    def peek(self):
        return self.units[self.i] if self.i < len(self.units) else None

    def take(self):
        u = self.peek()
        if u is None:
            self.err("the pattern ends early")
        self.i += 1
        return u

    def parse(self):
        node = self.alt()
        if self.peek() is not None:
            self.err("unbalanced )")
        return node

    def alt(self):
        parts = [self.cat()]
        while self.peek() == b"|":
            self.i += 1
            parts.append(self.cat())
        return parts[0] if len(parts) == 1 else ("alt", parts)

    def cat(self):
        parts = []
        while self.peek() not in (None, b"|", b")"):
            parts.append(self.rep())
        return ("cat", parts)

    def rep(self):
        node = self.atom()
        u = self.peek()
        if u in (b"*", b"+", b"?"):
            self.i += 1
            node = ("rep", node, 0 if u != b"+" else 1, 1 if u == b"?" else None)
        elif u == b"{":
            self.i += 1
            m = self.number()
            n = m
            if self.peek() == b",":
                self.i += 1
                n = None if self.peek() == b"}" else self.number()
            if self.take() != b"}":
                self.err("a counted repeat is {m}, {m,n} or {m,}")
            if n is not None and n < m:
                self.err("a counted repeat {m,n} with n < m")
            node = ("rep", node, m, n)
        else:
            return node
        if self.peek() in (b"*", b"+", b"?", b"{"):
            self.err("a second quantifier (lazy, possessive and stacked quantifiers are not supported)")
        return node

    def number(self):
        digits = b""
        while self.peek() is not None and self.peek().isdigit() and len(self.peek()) == 1:
            digits += self.take()
        if not digits:
            self.err("a counted repeat is {m}, {m,n} or {m,}")
        return int(digits)

    def escape(self, in_class):
        u = self.take()
        if len(u) != 1:
            self.err("an escaped non-ASCII character")
        c = u[0]
        if u == b"n": return frozenset([0x0A])
        if u == b"t": return frozenset([0x09])
        if u == b"r": return frozenset([0x0D])
        if u == b"d": return _DIGIT
        if u == b"w": return _WORD
        if u == b"s": return _SPACE
        if u == b"x":
            h = b"".join(self.take() for _ in range(2))
            try:
                return frozenset([int(h.decode("ascii"), 16)])
            except (ValueError, UnicodeDecodeError):
                self.err("\\x takes two hexadecimal digits")
        if c in _PUNCT:
            return frozenset([c])
        self.err("an escape this compiler does not know (\\%s)" % u.decode("latin-1"))

    def atom(self):
        u = self.take()
        if u == b"(":
            if self.peek() == b"?":
                self.err("(?...) groups are not supported")
            node = self.alt()
            if self.peek() != b")":
                self.err("unbalanced (")
            self.i += 1
            return node
        if u == b"[":
            return ("set", self.klass())
        if u == b".":
            return ("set", _ALL - frozenset([0x0A]))
        if u == b"\\":
            return ("set", self.escape(False))
        if u in (b"*", b"+", b"?", b"{"):
            self.i -= 1
            self.err("a quantifier with nothing to repeat")
        if u in (b"^", b"$", b"]", b"}"):
            self.i -= 1
            self.err("%s is not supported unescaped" % u.decode("ascii"))
        return ("cat", [("set", frozenset([b])) for b in u]) if len(u) > 1 else ("set", frozenset([u[0]]))

    def klass(self):
        negate = self.peek() == b"^"
        if negate:
            self.i += 1
        if self.peek() == b"]":
            self.err("an empty class (a ] first in a class is not supported: escape it)")
        out = set()
        while True:
            u = self.take()
            if u == b"]":
                break
            if u == b"[":
                self.err("[ inside a class is not supported unescaped")
            if len(u) != 1:
                self.err("a non-ASCII character in a class (a class is a set of bytes)")
            lo = self.escape(True) if u == b"\\" else frozenset([u[0]])
            if self.peek() == b"-" and self.i + 1 < len(self.units) and self.units[self.i + 1] != b"]":
                self.i += 1
                v = self.take()
                if len(v) != 1:
                    self.err("a non-ASCII character in a class (a class is a set of bytes)")
                hi = self.escape(True) if v == b"\\" else frozenset([v[0]])
                if len(lo) != 1 or len(hi) != 1:
                    self.err("a range's ends are single bytes")
                a, b = min(lo), min(hi)
                if b < a:
                    self.err("a range that runs backwards")
                out.update(range(a, b + 1))
            else:
                out.update(lo)
        return frozenset(_ALL - out if negate else out)


# ------------------------------------------------------------------------------------------------ syntax tree -> NFA (Thompson)
class _Nfa:
    def __init__(self):
        self.eps = []           # state -> [states]
        self.edge = []          # state -> [(byte set, state)]

    def new(self):
        self.eps.append([])
        self.edge.append([])
        return len(self.eps) - 1

    def build(self, node):
        """(entry, exit) of a fragment for node"""
        kind = node[0]
        if kind == "set":
            a, b = self.new(), self.new()
            self.edge[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = b = self.new()
            for part in node[1]:
                x, y = self.build(part)
                self.eps[b].append(x)
                b = y
            return a, b
        if kind == "alt":
            a, b = self.new(), self.new()
            for part in node[1]:
                x, y = self.build(part)
                self.eps[a].append(x)
                self.eps[y].append(b)
            return a, b
        _, sub, m, n = node
        a = b = self.new()
        for _ in range(m):
            x, y = self.build(sub)
            self.eps[b].append(x)
            b = y
        if n is None:               # sub*
            x, y = self.build(sub)
            loop = self.new()
            self.eps[b].append(loop)
            self.eps[loop].append(x)
            self.eps[y].append(loop)
            b = loop
        else:                       # up to n - m more, each skippable to the end
            end = self.new()
            for _ in range(n - m):
                x, y = self.build(sub)
                self.eps[b].append(end)
                self.eps[b].append(x)
                b = y
            self.eps[b].append(end)
            b = end
        if len(self.eps) > 1 << 20:
            raise ValueError("regex_dfa: the pattern expands to more than 2^20 NFA states")
        return a, b


def _closure(nfa, states):
    seen = set(states)
    stack = list(states)
    while stack:
        for t in nfa.eps[stack.pop()]:
            if t not in seen:
                seen.add(t)
                stack.append(t)
    return frozenset(seen)


def _byte_classes(sets):
    """bytes that no edge tells apart: class id per byte, one representative per class"""
    sig = [tuple(b in s for s in sets) for b in range(256)]
    ids = {}
    cls = [ids.setdefault(g, len(ids)) for g in sig]
    reps = [cls.index(k) for k in range(len(ids))]
    return cls, reps


def _subset(nfa, entry, exit_):
    sets = list({s for edges in nfa.edge for s, _ in edges})
    cls, reps = _byte_classes(sets)
    start = _closure(nfa, [entry])
    index = {start: 0}
    order = [start]
    trans = []                      # per DFA state: per class, the target (-1: none)
    i = 0
    while i < len(order):
        cur = order[i]
        row = []
        for rb in reps:
            nxt = {t for s in cur for bs, t in nfa.edge[s] if rb in bs}
            if not nxt:
                row.append(-1)
                continue
            key = _closure(nfa, nxt)
            if key not in index:
                index[key] = len(order)
                order.append(key)
                if len(order) > 4 * MAX_STATES:
                    raise ValueError("regex_dfa: more than %d states before minimisation" % (4 * MAX_STATES))
            row.append(index[key])
        trans.append(row)
        i += 1
    return trans, [exit_ in s for s in order], cls


def _finish(trans, accept, cls, start=0):
    """trim and minimise a partial DFA over byte classes (trans[s][k] = target or -1), then lay it out with state 0 dead"""
    n, K = len(trans), len(trans[0]) if trans else 0
    # states that can reach an accepting state
    back = [[] for _ in range(n)]
    for s in range(n):
        for t in trans[s]:
            if t >= 0:
                back[t].append(s)
    live = [bool(a) for a in accept]
    stack = [s for s in range(n) if live[s]]
    while stack:
        for p in back[stack.pop()]:
            if not live[p]:
                live[p] = True
                stack.append(p)
    if not live[start]:
        raise ValueError("regex_dfa: the pattern matches nothing")
    # Moore refinement; block 0 is the dead state (every transition into a state that is not live)
    block = [(2 if accept[s] else 1) if live[s] else 0 for s in range(n)]
    while True:
        sig = {}
        new = []
        for s in range(n):
            if not live[s]:
                new.append(0)
                continue
            key = (block[s],) + tuple(block[t] if t >= 0 and live[t] else 0 for t in trans[s])
            new.append(sig.setdefault(key, len(sig) + 1))
        if len(sig) == len(set(b for b in block if b)):
            block = new
            break
        block = new
    # number the blocks from the start state, breadth first: the start state is 1
    rep = {}
    for s in range(n):
        if live[s]:
            rep.setdefault(block[s], s)
    number = {block[start]: 1}
    queue = [block[start]]
    for b in queue:
        for t in trans[rep[b]]:
            if t >= 0 and live[t] and block[t] not in number:
                number[block[t]] = len(number) + 1
                queue.append(block[t])
    if len(number) + 1 > MAX_STATES:
        raise ValueError("regex_dfa: %d states (at most %d)" % (len(number) + 1, MAX_STATES))
    out = np.zeros((len(number) + 1, 256), dtype=np.uint16)
    acc = np.zeros(len(number) + 1, dtype=np.uint8)
    cls = np.asarray(cls)
    for b, num in number.items():
        s = rep[b]
        acc[num] = 1 if accept[s] else 0
        row = np.array([number[block[t]] if t >= 0 and live[t] else 0 for t in trans[s]], dtype=np.uint16)
        out[num] = row[cls] if K else 0
    return Dfa(out, acc, 1)


def regex_dfa(pattern):
    """the minimal Dfa that accepts exactly the byte strings pattern matches as a whole (see the module's text for the syntax)"""
    tree = _Parser(pattern).parse()
    nfa = _Nfa()
    entry, exit_ = nfa.build(tree)
    trans, accept, cls = _subset(nfa, entry, exit_)
    return _finish(trans, accept, cls)


def choice_dfa(strings):
    """the minimal Dfa that accepts exactly the given strings (bytes, or str as UTF-8): "answer with one of these" without escaping"""
    raw = [bytes(x) if isinstance(x, (bytes, bytearray)) else str(x).encode("utf-8") for x in strings]
    if not raw:
        raise ValueError("choice_dfa: no strings")
    cls = list(range(256))
    trans, accept = [[-1] * 256], [False]
    for word in raw:
        s = 0
        for b in word:
            if trans[s][b] < 0:
                trans[s][b] = len(trans)
                trans.append([-1] * 256)
                accept.append(False)
            s = trans[s][b]
        accept[s] = True
    return _finish(trans, accept, cls)

"""Guided decoding: regex, choice and JSON-schema constraints compiled to byte DFAs.

A constraint is a *minimised, trimmed* deterministic automaton over UTF-8 bytes: the start state
is 0, ``trans[state, cmap[byte]]`` is the next state or ``DEAD``, every state carries an accept
flag and every state can still reach an accepting one.  The sampler masks, per step, every token
whose bytes would leave the automaton (ops/grammar.py; csrc/kernels/grammar.hip on the GPU), so a
finished completion is always a member of the language.

Three sources share one builder (AST -> byte NFA -> subset construction -> trim -> minimise):

* :func:`compile_regex`: full-match semantics over a subset of Python's ``re`` syntax (literals,
  ``\\d \\w \\s \\n \\t \\r \\xHH`` and escaped metacharacters, ``.``, classes, groups, ``|``, ``? * +``
  and counted repetition up to 256).  Within the subset the language equals ``re.fullmatch`` on the
  decoded string; anything else raises a ``ValueError`` naming the construct.
* :func:`compile_choice`: exactly the given strings.
* :func:`compile_json`: a JSON Schema subset (see ``_Json``); unsupported keywords raise.

``.`` and negated classes match one well-formed UTF-8 scalar (RFC 3629: no surrogates, no overlong
forms).  :func:`compile_grammar` caches compiled automata in an LRU keyed by (kind, canonical
source).  :func:`token_bytes` gives the byte string of every vocabulary id, :func:`check_vocab`
the condition under which a live state always admits a token.
"""
from __future__ import annotations

import collections
import hashlib
import json
import threading
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

DEAD = -1
MAX_STATES = 2048          # states of a compiled automaton (the device table's capacity)
WORK_STATES = 4 * MAX_STATES  # subset construction gives up beyond this many states
MAX_REPEAT = 256
CACHE_SIZE = 64

# ------------------------------------------------------------------------------------- AST
# ("set", ((lo, hi), ...))  one code point out of sorted, disjoint, inclusive ranges
# ("byte", b)               one raw byte (only from \xHH >= 0x80 never arises: \xHH is a code point)
# ("cat", [nodes]) ("alt", [nodes]) ("rep", node, m, n or None)
_EPS = ("cat", [])
_MAX_CP = 0x10FFFF
_SURR = (0xD800, 0xDFFF)


def _norm(ranges) -> Tuple[Tuple[int, int], ...]:
    out: List[List[int]] = []
    for lo, hi in sorted(ranges):
        if lo > hi:
            continue
        if out and lo <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return tuple((a, b) for a, b in out)


def _negate(ranges) -> Tuple[Tuple[int, int], ...]:
    out, nxt = [], 0
    for lo, hi in _norm(ranges):
        if lo > nxt:
            out.append((nxt, lo - 1))
        nxt = hi + 1
    if nxt <= _MAX_CP:
        out.append((nxt, _MAX_CP))
    return _norm(out)


def _minus_surrogates(ranges):
    out = []
    for lo, hi in ranges:
        if hi < _SURR[0] or lo > _SURR[1]:
            out.append((lo, hi))
            continue
        if lo < _SURR[0]:
            out.append((lo, _SURR[0] - 1))
        if hi > _SURR[1]:
            out.append((_SURR[1] + 1, hi))
    return out


_uni_tables: Dict[str, tuple] = {}
_uni_lock = threading.Lock()


def _unicode_class(name: str) -> Tuple[Tuple[int, int], ...]:
    """The code points Python's ``re`` matches with ``\\d`` / ``\\w`` / ``\\s`` on ``str`` patterns
    (``str.isdecimal``, ``str.isalnum`` or ``_``, ``str.isspace``), computed once."""
    with _uni_lock:
        if not _uni_tables:
            d, w, s = [], [], []
            for c in range(_MAX_CP + 1):
                ch = chr(c)
                if ch.isalnum() or c == 0x5F:
                    w.append(c)
                    if ch.isdecimal():
                        d.append(c)
                elif ch.isspace():
                    s.append(c)

            def runs(v):
                a = np.asarray(v)
                cut = np.nonzero(np.diff(a) != 1)[0]
                lo = np.concatenate([[a[0]], a[cut + 1]])
                hi = np.concatenate([a[cut], [a[-1]]])
                return tuple((int(x), int(y)) for x, y in zip(lo, hi))
            _uni_tables.update(d=runs(d), w=runs(w), s=runs(s))
    return _uni_tables[name]


# ------------------------------------------------------------------------------- regex parser
_META = set(".^$*+?{}[]\\|()")
_SIMPLE_ESC = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11, "a": 7, "0": 0}


class _Regex:
    def __init__(self, pat: str):
        if not isinstance(pat, str):
            raise ValueError("guided_regex must be a string")
        self.p, self.i = pat, 0

    def err(self, what: str):
        raise ValueError(f"guided_regex: unsupported construct: {what} (at offset {self.i} of {self.p!r})")

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.err("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.i < len(self.p) and self.p[self.i] == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.p[self.i] not in "|)":
            items.append(self.quantified())
        return items[0] if len(items) == 1 else ("cat", items)

    def quantified(self):
        atom = self.atom()
        while self.i < len(self.p):
            c = self.p[self.i]
            if c == "?":
                m, n = 0, 1
            elif c == "*":
                m, n = 0, None
            elif c == "+":
                m, n = 1, None
            elif c == "{":
                m, n = self.braces()
            else:
                break
            if c != "{":
                self.i += 1
            if self.i < len(self.p) and self.p[self.i] == "?":
                self.err("lazy quantifier")
            if self.i < len(self.p) and self.p[self.i] == "+":
                self.err("possessive quantifier")
            if self.i < len(self.p) and self.p[self.i] in "*{":
                self.err("multiple repeat")
            atom = ("rep", atom, m, n)
        return atom

    def braces(self):
        j = self.p.find("}", self.i)
        body = self.p[self.i + 1:j] if j > 0 else ""
        lo, sep, hi = body.partition(",")
        if j < 0 or not lo.isascii() or not lo.isdigit() or (hi and (not hi.isascii() or not hi.isdigit())):
            self.err("malformed quantifier '{'")
        m = int(lo)
        n = m if not sep else (int(hi) if hi else None)
        if m > MAX_REPEAT or (n is not None and (n > MAX_REPEAT or n < m)):
            self.err(f"repetition bound outside 0..{MAX_REPEAT}")
        self.i = j + 1
        return m, n

    def escape(self, in_class: bool):
        """After a backslash → ("set", ranges) for a class escape or an int code point."""
        if self.i >= len(self.p):
            self.err("trailing backslash")
        c = self.p[self.i]
        self.i += 1
        if c in "dws":
            return ("set", _unicode_class(c))
        if c == "x":
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or any(x not in "0123456789abcdefABCDEF" for x in h):
                self.err("malformed \\x escape")
            self.i += 2
            return int(h, 16)
        if c in "ntr":
            return _SIMPLE_ESC[c]
        if not (c.isascii() and (c.isalnum() or c == "_")):
            return ord(c)  # an escaped metacharacter or punctuation mark is itself
        if c.isdigit():
            self.i -= 1
            self.err("back-reference or octal escape \\" + c)
        if c in "bBAZ":
            self.i -= 1
            self.err("anchor \\" + c)
        self.i -= 1
        self.err("escape \\" + c)

    def atom(self):
        c = self.p[self.i]
        if c == "(":
            self.i += 1
            if self.p.startswith("?", self.i):
                if self.p.startswith("?:", self.i):
                    self.i += 2
                else:
                    nxt = self.p[self.i + 1:self.i + 3]
                    what = ("lookahead" if nxt[:1] in "=!" else "lookbehind" if nxt in ("<=", "<!")
                            else "named group" if nxt[:1] in "P<" else "comment" if nxt[:1] == "#"
                            else "inline flag")
                    self.err(f"{what} '(?{nxt}'")
            node = self.alt()
            if self.i >= len(self.p) or self.p[self.i] != ")":
                self.err("unbalanced '('")
            self.i += 1
            return node
        if c == "[":
            return self.klass()
        if c == ".":
            self.i += 1
            return ("set", _negate([(10, 10)]))
        if c in "^$":
            self.err(f"anchor '{c}'")
        if c in "*+?":
            self.err(f"quantifier '{c}' with nothing to repeat")
        if c == "{":
            self.err("quantifier '{' with nothing to repeat")
        if c in "}]":
            self.err(f"unescaped '{c}'")
        self.i += 1
        if c == "\\":
            e = self.escape(False)
            return e if isinstance(e, tuple) else ("set", ((e, e),))
        return ("set", ((ord(c), ord(c)),))

    def klass(self):
        self.i += 1
        neg = self.p.startswith("^", self.i)
        self.i += neg
        ranges: List[Tuple[int, int]] = []
        first = True
        while True:
            if self.i >= len(self.p):
                self.err("unterminated character class")
            c = self.p[self.i]
            if c == "]" and not first:
                self.i += 1
                break
            if c == "[" and self.p.startswith("[:", self.i):
                self.err("POSIX class '[:'")
            first = False
            self.i += 1
            lo = self.escape(True) if c == "\\" else ord(c)
            if isinstance(lo, tuple):
                ranges.extend(lo[1])
                if self.p.startswith("-", self.i) and not self.p.startswith("-]", self.i):
                    self.err("range from a class escape")
                continue
            if self.p.startswith("-", self.i) and not self.p.startswith("-]", self.i) and self.i + 1 < len(self.p):
                self.i += 1
                c2 = self.p[self.i]
                self.i += 1
                hi = self.escape(True) if c2 == "\\" else ord(c2)
                if isinstance(hi, tuple):
                    self.err("range to a class escape")
                if hi < lo:
                    self.err("reversed character range")
                ranges.append((lo, hi))
            else:
                ranges.append((lo, lo))
        rs = _negate(ranges) if neg else _norm(ranges)
        return ("set", rs)


# --------------------------------------------------------------------------------- JSON schema
_IGNORED = {"required", "additionalProperties", "title", "description", "default", "examples", "$schema", "$id",
            "$comment", "$defs", "definitions"}
_REJECTED = ("$ref", "$dynamicRef", "$recursiveRef", "pattern", "patternProperties", "format", "oneOf", "allOf",
             "not", "minimum", "maximum", "exclusiveMinimum", "exclusiveMaximum", "multipleOf", "if", "then", "else",
             "prefixItems", "contains", "uniqueItems", "minProperties", "maxProperties", "propertyNames",
             "dependentRequired", "dependentSchemas", "unevaluatedProperties", "unevaluatedItems")
_KNOWN = {"type", "properties", "items", "minItems", "maxItems", "enum", "const", "minLength", "maxLength", "anyOf"}
_TYPES = ("object", "array", "string", "integer", "number", "boolean", "null")


def _lit(text: str):
    return ("cat", [("set", ((ord(c), ord(c)),)) for c in text])


def _cls(spec: str):
    """A small class from a string of characters and a-b ranges (ASCII, no escapes)."""
    out, i = [], 0
    while i < len(spec):
        if i + 2 < len(spec) and spec[i + 1] == "-":
            out.append((ord(spec[i]), ord(spec[i + 2])))
            i += 3
        else:
            out.append((ord(spec[i]), ord(spec[i])))
            i += 1
    return ("set", _norm(out))


def _opt(node):
    return ("rep", node, 0, 1)


class _Json:
    """JSON Schema → AST.  ``type`` (one of object, array, string, integer, number, boolean, null,
    or a list of them), ``properties`` (all emitted, in declaration order), ``items`` with
    ``minItems`` / ``maxItems``, ``enum`` / ``const`` of scalars, ``minLength`` / ``maxLength``,
    ``anyOf``, nested.  At most one space after ``:`` and ``,``, none elsewhere."""

    DIGIT = _cls("0-9")
    INT = ("cat", [_opt(_lit("-")), ("alt", [_lit("0"), ("cat", [_cls("1-9"), ("rep", _cls("0-9"), 0, 17)])])])
    NUM = ("cat", [INT, _opt(("cat", [_lit("."), ("rep", _cls("0-9"), 1, 17)])),
                   _opt(("cat", [_cls("eE"), _opt(_cls("+-")), ("rep", _cls("0-9"), 1, 3)]))])
    HEX = _cls("0-9a-fA-F")
    CHAR = ("alt", [("set", _negate([(0, 0x1F), (0x22, 0x22), (0x5C, 0x5C)])),
                    ("cat", [_lit("\\"), ("alt", [_cls("\"\\/bfnrt"), ("cat", [_lit("u"), ("rep", HEX, 4, 4)])])])])
    SP = _opt(_lit(" "))

    def __init__(self):
        self.depth = 0

    def err(self, what: str):
        raise ValueError(f"guided_json: unsupported schema keyword: {what}")

    def node(self, s):
        if s is True or s == {}:
            raise ValueError("guided_json: a schema without 'type', 'enum', 'const' or 'anyOf' is not supported "
                             "(any JSON value is not a regular language)")
        if not isinstance(s, dict):
            raise ValueError("guided_json: a schema must be an object")
        for k in _REJECTED:
            if k in s:
                self.err(repr(k))
        for k in s:
            if k not in _KNOWN and k not in _IGNORED:
                self.err(repr(k))
        self.depth += 1
        if self.depth > 64:
            raise ValueError("guided_json: schema nested deeper than 64 levels")
        try:
            return self._node(s)
        finally:
            self.depth -= 1

    def _node(self, s: dict):
        if "const" in s:
            return self.scalar(s["const"], "const")
        if "enum" in s:
            if not isinstance(s["enum"], list) or not s["enum"]:
                raise ValueError("guided_json: 'enum' must be a non-empty list")
            return ("alt", [self.scalar(v, "enum") for v in s["enum"]])
        if "anyOf" in s:
            if not isinstance(s["anyOf"], list) or not s["anyOf"]:
                raise ValueError("guided_json: 'anyOf' must be a non-empty list")
            return ("alt", [self.node(x) for x in s["anyOf"]])
        t = s.get("type")
        if t is None and "properties" in s:
            t = "object"
        if isinstance(t, list) and t:
            return ("alt", [self._node({**s, "type": x}) for x in t])
        if t not in _TYPES:
            raise ValueError(f"guided_json: 'type' must be one of {', '.join(_TYPES)} (got {t!r})")
        return getattr(self, "t_" + t)(s)

    def scalar(self, v, kw: str):
        if v is not None and not isinstance(v, (str, int, float, bool)):
            raise ValueError(f"guided_json: '{kw}' supports scalars only")
        return _lit(json.dumps(v))

    def _count(self, s, lo_key, hi_key):
        lo, hi = (int(v) if isinstance(v, float) and v == int(v) else v  # a protobuf Struct carries floats
                  for v in (s.get(lo_key, 0), s.get(hi_key)))
        for k, v in ((lo_key, lo), (hi_key, hi)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 0):
                raise ValueError(f"guided_json: '{k}' must be a non-negative integer")
        if hi is not None and hi < lo:
            raise ValueError(f"guided_json: '{hi_key}' is below '{lo_key}'")
        if lo > MAX_REPEAT or (hi is not None and hi > MAX_REPEAT):
            raise ValueError(f"guided_json: '{lo_key}' / '{hi_key}' above {MAX_REPEAT}")
        return lo, hi

    def t_string(self, s):
        lo, hi = self._count(s, "minLength", "maxLength")
        return ("cat", [_lit('"'), ("rep", self.CHAR, lo, hi), _lit('"')])

    def t_integer(self, s):
        return self.INT

    def t_number(self, s):
        return self.NUM

    def t_boolean(self, s):
        return ("alt", [_lit("true"), _lit("false")])

    def t_null(self, s):
        return _lit("null")

    def t_object(self, s):
        props = s.get("properties", {})
        if not isinstance(props, dict):
            raise ValueError("guided_json: 'properties' must be an object")
        parts = [_lit("{")]
        for i, (k, sub) in enumerate(props.items()):
            if i:
                parts += [_lit(","), self.SP]
            parts += [_lit(json.dumps(str(k))), _lit(":"), self.SP, self.node(sub)]
        return ("cat", parts + [_lit("}")])

    def t_array(self, s):
        if "items" not in s:
            raise ValueError("guided_json: an array needs 'items'")
        lo, hi = self._count(s, "minItems", "maxItems")
        item = self.node(s["items"])
        more = ("cat", [_lit(","), self.SP, item])
        if hi == 0:
            body = _EPS
        else:
            body = ("cat", [item, ("rep", more, max(lo - 1, 0), None if hi is None else hi - 1)])
            if lo == 0:
                body = _opt(body)
        return ("cat", [_lit("["), body, _lit("]")])


# ------------------------------------------------------------------------------ UTF-8 ranges
def _enc(cp: int) -> bytes:
    return chr(cp).encode("utf-8")


def _utf8_split(lo: int, hi: int, n: int, out: list) -> None:
    for i in range(1, n):
        m = (1 << (6 * i)) - 1
        if (lo & ~m) != (hi & ~m):
            if lo & m:
                _utf8_split(lo, lo | m, n, out)
                _utf8_split((lo | m) + 1, hi, n, out)
                return
            if (hi & m) != m:
                _utf8_split(lo, (hi & ~m) - 1, n, out)
                _utf8_split(hi & ~m, hi, n, out)
                return
    out.append(tuple(zip(_enc(lo), _enc(hi))))


def utf8_sequences(ranges) -> List[tuple]:
    """Code point ranges → byte-range sequences whose union is exactly their well-formed UTF-8."""
    out: list = []
    for lo, hi in _minus_surrogates(_norm(ranges)):
        for a, b, n in ((0, 0x7F, 1), (0x80, 0x7FF, 2), (0x800, 0xFFFF, 3), (0x10000, _MAX_CP, 4)):
            x, y = max(lo, a), min(hi, b)
            if x <= y:
                _utf8_split(x, y, n, out)
    return out


# ------------------------------------------------------------------------------------- NFA
class _NFA:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.edges: List[List[Tuple[int, int, int]]] = []  # (lo byte, hi byte, target)
        self._set_cache: Dict[tuple, List[tuple]] = {}

    def new(self) -> int:
        self.eps.append([])
        self.edges.append([])
        if len(self.eps) > 400000:
            raise ValueError("grammar too large: more than 400000 NFA states")
        return len(self.eps) - 1

    def build(self, node, src: int) -> int:
        """Adds ``node`` starting at state ``src``; returns its end state."""
        kind = node[0]
        if kind == "set":
            seqs = self._set_cache.get(node[1])
            if seqs is None:
                seqs = self._set_cache[node[1]] = utf8_sequences(node[1])
            dst = self.new()
            for seq in seqs:
                cur = src
                for j, (lo, hi) in enumerate(seq):
                    nxt = dst if j == len(seq) - 1 else self.new()
                    self.edges[cur].append((lo, hi, nxt))
                    cur = nxt
            return dst
        if kind == "cat":
            for x in node[1]:
                src = self.build(x, src)
            return src
        if kind == "alt":
            dst = self.new()
            for x in node[1]:
                s = self.new()
                self.eps[src].append(s)
                self.eps[self.build(x, s)].append(dst)
            return dst
        if kind == "rep":
            _, x, m, n = node
            for _ in range(m):
                src = self.build(x, src)
            if n is None:
                a = self.new()
                self.eps[src].append(a)
                b = self.build(x, a)
                self.eps[b].append(a)
                dst = self.new()
                self.eps[a].append(dst)
                return dst
            dst = self.new()
            self.eps[src].append(dst)
            for _ in range(n - m):
                s = self.new()
                self.eps[src].append(s)
                src = self.build(x, s)
                self.eps[src].append(dst)
            return dst
        raise AssertionError(kind)


class CompiledGrammar:
    """A minimised, trimmed byte DFA.  ``cmap`` uint8[256] maps a byte to its class,
    ``trans`` int16[n_states, n_classes] holds the next state or ``DEAD``, ``accept`` bool[n_states]."""

    def __init__(self, kind: str, source: str, cmap: np.ndarray, trans: np.ndarray, accept: np.ndarray):
        self.kind, self.source = kind, source
        self.cmap, self.trans, self.accept = cmap, trans, accept
        self.n_states, self.n_classes = trans.shape
        live = (trans != DEAD).any(axis=0)
        self.live_bytes = frozenset(int(b) for b in range(256) if live[cmap[b]])
        h = hashlib.sha256()
        for a in (cmap, trans, accept.astype(np.uint8)):
            h.update(a.tobytes())
        h.update(repr(trans.shape).encode())
        self.key = h.hexdigest()
        self._vocab_ok: Dict[int, bool] = {}

    def step(self, state: int, byte: int) -> int:
        return DEAD if state < 0 else int(self.trans[state, self.cmap[byte]])

    def walk(self, state: int, data: bytes) -> int:
        t, c = self.trans, self.cmap
        for b in data:
            if state < 0:
                return DEAD
            state = int(t[state, c[b]])
        return state

    def accepts(self, data) -> bool:
        if isinstance(data, str):
            data = data.encode("utf-8")
        s = self.walk(0, data)
        return s >= 0 and bool(self.accept[s])

    def is_trimmed(self) -> bool:
        """Every state is reachable from 0 and reaches an accepting state."""
        S = self.n_states
        fwd = [set(int(x) for x in row if x >= 0) for row in self.trans]
        seen, todo = {0}, [0]
        while todo:
            for y in fwd[todo.pop()]:
                if y not in seen:
                    seen.add(y)
                    todo.append(y)
        back: List[set] = [set() for _ in range(S)]
        for x in range(S):
            for y in fwd[x]:
                back[y].add(x)
        good = set(int(x) for x in np.nonzero(self.accept)[0])
        todo = list(good)
        while todo:
            for y in back[todo.pop()]:
                if y not in good:
                    good.add(y)
                    todo.append(y)
        return len(seen) == S and len(good) == S


def _compile_ast(kind: str, source: str, ast) -> CompiledGrammar:
    nfa = _NFA()
    start = nfa.new()
    final = nfa.build(ast, start)
    n = len(nfa.eps)
    # byte classes: the coarsest partition of 0..255 no edge label cuts
    cuts = {0, 256}
    for es in nfa.edges:
        for lo, hi, _ in es:
            cuts.add(lo)
            cuts.add(hi + 1)
    bounds = sorted(cuts)
    cmap = np.zeros(256, dtype=np.uint8)
    for ci in range(len(bounds) - 1):
        cmap[bounds[ci]:bounds[ci + 1]] = ci
    C = len(bounds) - 1
    cedges: List[Dict[int, List[int]]] = []
    for es in nfa.edges:
        d: Dict[int, List[int]] = {}
        for lo, hi, t in es:
            for ci in range(int(cmap[lo]), int(cmap[hi]) + 1):
                d.setdefault(ci, []).append(t)
        cedges.append(d)
    closure_cache: Dict[int, frozenset] = {}

    def closure(states) -> frozenset:
        out = set()
        for s in states:
            c = closure_cache.get(s)
            if c is None:
                seen, todo = {s}, [s]
                while todo:
                    for y in nfa.eps[todo.pop()]:
                        if y not in seen:
                            seen.add(y)
                            todo.append(y)
                # only states with byte edges (or the final one) matter to the subset's identity
                c = closure_cache[s] = frozenset(x for x in seen if cedges[x] or x == final)
            out |= c
        return frozenset(out)

    s0 = closure([start])
    index = {s0: 0}
    order = [s0]
    rows: List[List[int]] = []
    i = 0
    while i < len(order):
        cur = order[i]
        i += 1
        moves: Dict[int, set] = {}
        for x in cur:
            for ci, ts in cedges[x].items():
                moves.setdefault(ci, set()).update(ts)
        row = [DEAD] * C
        for ci, ts in moves.items():
            nxt = closure(ts)
            j = index.get(nxt)
            if j is None:
                j = index[nxt] = len(order)
                order.append(nxt)
                if j >= WORK_STATES:
                    raise ValueError(f"{kind} grammar too large: more than {WORK_STATES} states before minimisation "
                                     f"(at most {MAX_STATES} after it)")
            row[ci] = j
        rows.append(row)
    S = len(order)
    trans = np.asarray(rows, dtype=np.int32).reshape(S, C)
    accept = np.fromiter((final in st for st in order), dtype=bool, count=S)
    # trim: drop states that cannot reach an accepting one
    good = accept.copy()
    while True:
        reach = (np.where(trans >= 0, good[np.maximum(trans, 0)], False)).any(axis=1) | good
        if (reach == good).all():
            break
        good = reach
    if not good[0]:
        raise ValueError(f"{kind} grammar matches nothing")
    trans = np.where((trans >= 0) & good[np.maximum(trans, 0)], trans, DEAD)
    keep = np.nonzero(good)[0]
    remap = np.full(S + 1, DEAD, dtype=np.int32)
    remap[keep] = np.arange(keep.size)
    trans = remap[trans[keep]]  # DEAD (-1) indexes the last element of remap: DEAD
    accept = accept[keep]
    # minimise (Moore): refine {accepting, not} by the classes of the successors; DEAD is its own class
    S = keep.size
    part = accept.astype(np.int64) + 1
    nparts = len(np.unique(part))
    # A round compares 64-bit mixes of the signature rows (a chain of n states needs n rounds, and
    # sorting whole rows every round is what made that slow); a collision can only delay a split,
    # so the loop ends on a round that compares the rows themselves.
    mult = np.random.default_rng(0x5EED).integers(1, 1 << 62, size=C + 1, dtype=np.uint64) | np.uint64(1)
    exact = False
    while True:
        ext = np.concatenate([part, [0]])  # index -1 → class 0 = DEAD
        sig = np.column_stack([part, ext[trans]])
        if exact:
            _, part2 = np.unique(sig, axis=0, return_inverse=True)
            part = part2.reshape(-1).astype(np.int64) + 1
        else:  # split every class by the mix: always a refinement of the current partition
            h = (sig.astype(np.uint64) * mult).sum(axis=1, dtype=np.uint64)
            idx = np.lexsort((h, part))
            ps, hs = part[idx], h[idx]
            new = np.concatenate([[True], (ps[1:] != ps[:-1]) | (hs[1:] != hs[:-1])])
            part2 = np.empty(S, dtype=np.int64)
            part2[idx] = np.cumsum(new)
            part = part2
        n2 = int(part.max())
        if n2 == nparts:
            if exact:
                break
            exact = True
        else:
            exact = False
        nparts = n2
    # one representative per class, numbered breadth-first from the start state (canonical)
    rep = {}
    for s in range(S):
        rep.setdefault(int(part[s]), s)
    newid = {int(part[0]): 0}
    queue = [int(part[0])]
    qi = 0
    out_rows = []
    while qi < len(queue):
        p = queue[qi]
        qi += 1
        row = []
        for t in trans[rep[p]]:
            if t < 0:
                row.append(DEAD)
                continue
            q = int(part[t])
            if q not in newid:
                newid[q] = len(queue)
                queue.append(q)
            row.append(newid[q])
        out_rows.append(row)
    M = len(queue)
    if M > MAX_STATES:
        raise ValueError(f"{kind} grammar too large: {M} states after minimisation (at most {MAX_STATES})")
    mtrans = np.asarray(out_rows, dtype=np.int16).reshape(M, C)
    maccept = np.fromiter((accept[rep[p]] for p in queue), dtype=bool, count=M)
    # merge byte classes with identical columns
    cols, inv = np.unique(mtrans, axis=1, return_inverse=True)
    inv = inv.reshape(-1)
    return CompiledGrammar(kind, source, inv[cmap].astype(np.uint8), np.ascontiguousarray(cols), maccept)


# ------------------------------------------------------------------------------------ public
def compile_regex(pattern: str) -> CompiledGrammar:
    return _compile_ast("guided_regex", pattern, _Regex(pattern).parse())


def compile_choice(choices: Sequence[str]) -> CompiledGrammar:
    if isinstance(choices, (str, bytes)) or not isinstance(choices, (list, tuple)) or not choices:
        raise ValueError("guided_choice must be a non-empty list of non-empty strings")
    if any(not isinstance(c, str) or not c for c in choices):
        raise ValueError("guided_choice must be a non-empty list of non-empty strings")
    uniq = sorted(set(choices))
    return _compile_ast("guided_choice", json.dumps(uniq), ("alt", [_lit(c) for c in uniq]))


def canonical_json(schema) -> str:
    if isinstance(schema, (str, bytes)):
        try:
            schema = json.loads(schema)
        except ValueError as e:
            raise ValueError(f"guided_json: not valid JSON: {e}") from None
    if not isinstance(schema, dict):
        raise ValueError("guided_json must be a JSON Schema object (a dict or its JSON text)")
    # key order is kept: the properties of an object are emitted in the order they stand here
    return json.dumps(schema)


def compile_json(schema, suffix: str = "") -> CompiledGrammar:
    """``suffix``: literal text that must follow the value (a forced tool call's closing)."""
    src = canonical_json(schema)
    ast = _Json().node(json.loads(src))
    if suffix:
        ast = ("cat", [ast, _lit(suffix)])
    return _compile_ast("guided_json", src + suffix, ast)


_cache: "collections.OrderedDict[tuple, CompiledGrammar]" = collections.OrderedDict()
_cache_lock = threading.Lock()
cache_stats = {"hits": 0, "misses": 0}


def compile_grammar(kind: str, source, suffix: str = "") -> CompiledGrammar:
    """``kind``: regex | choice | json.  LRU-cached by (kind, canonical source)."""
    if kind == "regex":
        if not isinstance(source, str):
            raise ValueError("guided_regex must be a string")
        canon = source
    elif kind == "choice":
        if isinstance(source, (str, bytes)) or not isinstance(source, (list, tuple)):
            raise ValueError("guided_choice must be a non-empty list of non-empty strings")
        canon = json.dumps(list(source))
    elif kind == "json":
        canon = canonical_json(source)
    else:
        raise ValueError(f"unknown grammar kind {kind!r}")
    key = (kind, canon, suffix)
    with _cache_lock:
        g = _cache.get(key)
        if g is not None:
            _cache.move_to_end(key)
            cache_stats["hits"] += 1
            return g
    g = (compile_regex(source) if kind == "regex" else compile_choice(list(source)) if kind == "choice"
         else compile_json(canon, suffix))
    with _cache_lock:
        cache_stats["misses"] += 1
        _cache[key] = g
        while len(_cache) > CACHE_SIZE:
            _cache.popitem(last=False)
    return g


def grammar_for(params) -> Optional[CompiledGrammar]:
    """The compiled constraint of a request's ``SamplingParams`` (None when it has none)."""
    if getattr(params, "guided_regex", None) is not None:
        return compile_grammar("regex", params.guided_regex)
    if getattr(params, "guided_choice", None):
        return compile_grammar("choice", list(params.guided_choice))
    if getattr(params, "guided_json", None) is not None:
        return compile_grammar("json", params.guided_json, getattr(params, "guided_suffix", "") or "")
    return None


# ------------------------------------------------------------------------------ vocabularies
def _gpt2_unicode_to_byte() -> Dict[str, int]:
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(bs, cs)}


def _hf_token_bytes(tok, V: int) -> List[bytes]:
    spec = json.loads(tok.to_str())

    def has(node, name) -> bool:
        if not isinstance(node, dict):
            return False
        if node.get("type") == name:
            return True
        return any(has(x, name) for x in node.get("decoders", []) + node.get("pretokenizers", []))
    byte_level = has(spec.get("decoder"), "ByteLevel") or has(spec.get("pre_tokenizer"), "ByteLevel")
    added = {a["id"]: a for a in spec.get("added_tokens", [])}
    u2b = _gpt2_unicode_to_byte()
    out = [b""] * V
    for text, i in tok.get_vocab(with_added_tokens=True).items():
        if not 0 <= i < V:
            continue
        a = added.get(i)
        if a is not None:
            out[i] = b"" if a.get("special") else text.encode("utf-8")
        elif byte_level:
            out[i] = bytes(u2b[c] for c in text) if all(c in u2b for c in text) else b""
        elif len(text) == 6 and text.startswith("<0x") and text.endswith(">"):
            try:
                out[i] = bytes([int(text[3:5], 16)])
            except ValueError:
                out[i] = text.encode("utf-8")
        else:
            out[i] = text.replace("▁", " ").encode("utf-8")
    return out


def token_bytes(tokenizer, vocab_size: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """→ (``off`` int32[V+1], ``bytes`` uint8[off[V]]): id ``t`` spells ``bytes[off[t]:off[t+1]]``.
    Special tokens and ids the tokenizer does not define spell nothing."""
    V = int(vocab_size if vocab_size is not None else tokenizer.vocab_size)
    if hasattr(tokenizer, "tok"):
        toks = _hf_token_bytes(tokenizer.tok, V)
    elif hasattr(tokenizer, "offset"):
        toks = [b""] * V
        for b in range(256):
            if 0 <= tokenizer.offset + b < V:
                toks[tokenizer.offset + b] = bytes([b])
        for sp in (tokenizer.bos_token_id, tokenizer.eos_token_id):
            if 0 <= sp < V:
                toks[sp] = b""
    else:
        raise ValueError(f"no byte table for tokenizer {type(tokenizer).__name__}")
    off = np.zeros(V + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(t) for t in toks])
    data = np.frombuffer(b"".join(toks), dtype=np.uint8).copy()
    return off, data


def single_byte_tokens(off: np.ndarray, data: np.ndarray) -> frozenset:
    one = np.nonzero(np.diff(off) == 1)[0]
    return frozenset(int(b) for b in data[off[one]])


def check_vocab(g: CompiledGrammar, singles: frozenset) -> None:
    """Every byte on a live transition must itself be a token, so that a live state always admits
    at least one token (ByteTokenizer, byte-fallback and byte-level vocabularies do)."""
    missing = g._vocab_ok.get(id(singles))
    if missing is None:
        missing = g._vocab_ok[id(singles)] = sorted(g.live_bytes - singles)[:8]
    if missing:
        raise ValueError(f"{g.kind}: the vocabulary has no single-byte token for byte(s) "
                         f"{', '.join(hex(b) for b in missing)} the grammar needs")

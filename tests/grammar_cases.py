"""Guided decoding: the cases the compiler and the kernels are held to.

* the regex subset: patterns covering every construct, an alphabet with a 2-byte and a 3-byte
  character, and the constructs that must be refused by name;
* JSON schemas with conforming instances, near misses and a small hand-written checker;
* the inputs of the kernel test (tests/kernels/test_grammar.py): synthetic vocabularies, two
  tables at pool entries 0 and N_TABLES - 1, rows at the states that matter, and the *mutants*
  (deliberate defects of the reference, ops/reference.py ``mutant=``) those inputs must tell
  from the reference (tests/unit/test_grammar_cases.py).
"""
import functools
import json

import numpy as np
import torch

from polykey_service_amd.engine import grammar as G
from polykey_service_amd.ops import reference as ref

# ----------------------------------------------------------------------------------- regex
ALPHABET = ["a", "b", "1", " ", "é", "€"]  # é: 2 bytes, €: 3 bytes
MAX_LEN = 5
REGEX_PATTERNS = [
    r"abc", r"a|b|", r"(ab)*1", r"(?:a|b1)+", r"a?b*1+", r"a{2}", r"a{1,}", r"a{0,3}b", r"[ab1]", r"[^a]", r"[a-b]+",
    r".", r".*", r"a.b", r"\d+", r"\w*", r"\s?a", r"\n|\t|\r| ", r"\x61+", r"\.|\*|\(a\)", r"[^\d]", r"[é]+", r"[^é€]*",
    r"é€|€é", r"[\w-]+", r"[]a]", r"(a|b)(1|é)", r"[a\-1]", r"(a*)*", r"(|a)b", r"[0-9a]{2,3}", r"\w\d", r"[\s€]",
    r"(a|b){2}( |€)?", r"[^\w\s]+", r"(ab|a)(b1|1)",
]
UNSUPPORTED_REGEX = [  # (pattern, a word its error must carry)
    (r"^a", "anchor"), (r"a$", "anchor"), (r"\bfoo", "anchor"), (r"(?=a)b", "lookahead"), (r"(?!a)b", "lookahead"),
    (r"(?<=a)b", "lookbehind"), (r"(a)\1", "back-reference"), (r"a*?", "lazy"), (r"a+?", "lazy"), (r"a{1,2}?", "lazy"),
    (r"a*+", "possessive"), (r"(?i)a", "flag"), (r"(?P<n>a)", "named group"), (r"a{1,300}", "repetition bound"),
    (r"\D", r"escape \D"), (r"a{,3}", "quantifier"), (r"[a", "unterminated"), (r"(a", "unbalanced"),
]

# ------------------------------------------------------------------------------------ JSON
ADDRESS = {"type": "object", "properties": {"street": {"type": "string"}, "zip": {"type": "integer"}}}
JSON_SCHEMAS = {
    "flat": {"type": "object", "properties": {"name": {"type": "string"}, "age": {"type": "integer"}},
             "required": ["name"], "additionalProperties": False},
    "nested": {"type": "object", "properties": {"id": {"type": "integer"}, "home": ADDRESS,
                                                "tags": {"type": "array", "items": {"type": "string"}}}},
    "array_bounds": {"type": "array", "items": {"type": "integer"}, "minItems": 1, "maxItems": 3},
    "array_of_objects": {"type": "array", "items": ADDRESS, "maxItems": 2},
    "enum": {"type": "object", "properties": {"unit": {"enum": ["celsius", "fahrenheit", 5, None, True]},
                                              "kind": {"const": "weather"}}},
    "lengths": {"type": "object", "properties": {"code": {"type": "string", "minLength": 2, "maxLength": 4}}},
    "any_of": {"anyOf": [{"type": "number"}, {"type": "null"}, {"type": "array", "items": {"type": "boolean"}}]},
    "number": {"type": "number"},
    "string": {"type": "string"},
    "empty_object": {"type": "object", "properties": {}},
}
JSON_INSTANCES = {
    "flat": [{"name": "Ada", "age": 36}, {"name": "é€ \"q\" \\ \n", "age": -7}],
    "nested": [{"id": 0, "home": {"street": "Main St", "zip": 12345}, "tags": []},
               {"id": 99, "home": {"street": "", "zip": -1}, "tags": ["a", "b c"]}],
    "array_bounds": [[1], [1, -2, 30]],
    "array_of_objects": [[], [{"street": "x", "zip": 1}, {"street": "y", "zip": 2}]],
    "enum": [{"unit": "celsius", "kind": "weather"}, {"unit": None, "kind": "weather"}, {"unit": 5, "kind": "weather"}],
    "lengths": [{"code": "ab"}, {"code": "é€cd"}],
    "any_of": [1.5, -2e10, None, [True, False], 0],
    "number": [0, -1, 3.25, 1e-3, 123456789],
    "string": ["", "héllo", "tab\there"],
    "empty_object": [{}],
}
JSON_NEAR_MISSES = {  # texts one edit away from conforming
    "flat": ['{"name": "Ada"}', '{"age": 36, "name": "Ada"}', '{"name": "Ada", "age": "36"}', '{"name": "Ada", "age": 36,}',
             '{"name":  "Ada", "age": 36}', '{"name": "Ada",  "age": 36}', ' {"name": "Ada", "age": 36}',
             '{"name": "Ada", "age": 36} ', '{"name": "Ada", "age": 036}', '{"name": "Ada", "age": 36, "x": 1}'],
    "array_bounds": ["[]", "[1, 2, 3, 4]", "[1,]", "[1 , 2]", "[1.5]"],
    "enum": ['{"unit": "kelvin", "kind": "weather"}', '{"unit": "celsius", "kind": "news"}'],
    "lengths": ['{"code": "a"}', '{"code": "abcde"}'],
    "any_of": ['"x"', "[1]", "nul"],
    "string": ['"a', '"a"b"', '"\\x"', '"\n"'],
    "number": ["01", "1.", ".5", "1e", "+1", "--1"],
}
UNSUPPORTED_JSON = [  # (schema, the keyword its error must name)
    ({"$ref": "#/defs/a"}, "$ref"), ({"type": "string", "pattern": "a+"}, "pattern"),
    ({"type": "string", "format": "date"}, "format"), ({"oneOf": [{"type": "null"}]}, "oneOf"),
    ({"allOf": [{"type": "null"}]}, "allOf"), ({"not": {"type": "null"}}, "not"),
    ({"type": "integer", "minimum": 0}, "minimum"), ({"type": "number", "exclusiveMaximum": 1}, "exclusiveMaximum"),
    ({"type": "object", "properties": {"a": {"type": "integer", "multipleOf": 2}}}, "multipleOf"),
]


def conforms(schema, x) -> bool:
    """The supported JSON Schema subset, checked by hand on a parsed value."""
    if "const" in schema:
        return type(x) is type(schema["const"]) and x == schema["const"]
    if "enum" in schema:
        return any(type(x) is type(v) and x == v for v in schema["enum"])
    if "anyOf" in schema:
        return any(conforms(s, x) for s in schema["anyOf"])
    t = schema["type"]
    if t == "object":
        props = schema.get("properties", {})
        return isinstance(x, dict) and list(x) == list(props) and all(conforms(props[k], x[k]) for k in props)
    if t == "array":
        return (isinstance(x, list) and schema.get("minItems", 0) <= len(x) <= schema.get("maxItems", 1 << 30)
                and all(conforms(schema["items"], v) for v in x))
    if t == "string":
        return isinstance(x, str) and schema.get("minLength", 0) <= len(x) <= schema.get("maxLength", 1 << 30)
    if t == "integer":
        return isinstance(x, int) and not isinstance(x, bool)
    if t == "number":
        return isinstance(x, (int, float)) and not isinstance(x, bool)
    if t == "boolean":
        return isinstance(x, bool)
    return t == "null" and x is None


def random_accepted(g, rng, max_len: int = 400) -> bytes:
    """A random walk over the automaton that always ends in acceptance: random live bytes for a
    while, then along a shortest path to an accepting state."""
    dist = distances_to_accept(g)
    state, out = 0, bytearray()
    budget = int(rng.integers(0, 40))
    while True:
        live = [b for b in range(256) if g.trans[state, g.cmap[b]] >= 0]
        if g.accept[state] and (budget <= 0 or not live):
            return bytes(out)
        if budget > 0 and len(out) < max_len:
            b = live[int(rng.integers(len(live)))]
        else:  # not accepting: every step along a shortest path brings acceptance one byte closer
            b = min(live, key=lambda x: dist[g.trans[state, g.cmap[x]]])
        budget -= 1
        out.append(b)
        state = int(g.trans[state, g.cmap[b]])


def distances_to_accept(g) -> np.ndarray:
    dist = np.where(g.accept, 0, 1 << 30).astype(np.int64)
    for _ in range(g.n_states):
        nxt = np.where(g.trans >= 0, dist[np.maximum(g.trans, 0)], 1 << 30).min(axis=1) + 1
        new = np.minimum(dist, nxt)
        if (new == dist).all():
            break
        dist = new
    return dist


# ---------------------------------------------------------------------------- kernel inputs
MUTANTS_MASK = ["from_state_0", "drop_last_byte", "keep_empty", "keep_end", "next_table"]
MUTANTS_ADVANCE = ["advance_on_end"]
N_TABLES = ref.GRAMMAR_N_TABLES
CHAIN = r"(a{256}){7}a{255}"  # 2047 x 'a': a MAX_STATES-sized table whose last state is an accepting sink
WORDS = r"[a-d]*(e|xyz)"      # any run of a-d, then one of two endings: an accepting sink after either
SHAPES = [(259, 1), (1000, 64), (128259, 5)]  # (V, B): V no multiple of a block or vector width
EOS = 1


@functools.lru_cache(maxsize=None)
def tables():
    """pool entry -> compiled grammar: different grammars at entries 0 and N_TABLES - 1, and a
    third one at entry 1 (what the "table of entry g + 1" mutant reads for entry 0)."""
    a, b = G.compile_grammar("regex", WORDS), G.compile_grammar("regex", CHAIN)
    assert b.n_states == ref.GRAMMAR_MAX_STATES and b.accept[-1] and not (b.trans[-1] >= 0).any()
    return {0: a, 1: G.compile_grammar("choice", ["ab", "ba"]), N_TABLES - 1: b}


def make_vocab(V: int, seed: int):
    """Token lengths 0, 1, 2, 7 and 40 over an alphabet in which most strings survive WORDS or
    CHAIN for a while; a few ids are set by hand: survivors of every length, and tokens that die
    on their first and on their last byte."""
    rng = np.random.default_rng(seed)
    lens = rng.choice([0, 1, 2, 7, 40], size=V, p=[0.1, 0.3, 0.3, 0.2, 0.1])
    toks = []
    for n in lens:
        kind = rng.integers(4)
        if kind == 0:
            toks.append(b"a" * int(n))
        elif kind == 1:
            toks.append(rng.choice(list(b"abcd"), size=n).astype(np.uint8).tobytes())
        else:
            toks.append(rng.choice(list(b"abcdexyzq\xc3\xa9"), size=n).astype(np.uint8).tobytes())
    fixed = [b"", b"", b"a", b"b", b"e", b"aa", b"ab", b"xy", b"z", b"a" * 7, b"abcdabc", b"a" * 40, b"abcd" * 10,
             b"q" + b"a" * 39, b"a" * 39 + b"q", b"abcdab" + b"q", b"q" + b"abcdab", b"abcdxyz", b"x", b"yz", b"c", b"d",
             b"y", b"abcd" * 9 + b"xyz" + b"a", b"abcd" * 9 + b"axyz"]
    toks[:len(fixed)] = fixed
    toks = toks[:V]
    off = np.zeros(V + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(t) for t in toks])
    return off, np.frombuffer(b"".join(toks), dtype=np.uint8).copy()


@functools.lru_cache(maxsize=None)
def kernel_case(V: int, B: int, seed: int = 0):
    """→ dict: vocabulary, slot seed entries, the batch's slots (permuted; -1 and table-less
    slots interleaved), the fp32 rows before the mask."""
    rng = np.random.default_rng(1000 * seed + B)
    off, data = make_vocab(V, seed + V)
    t = tables()
    ga, gb = t[0], t[N_TABLES - 1]
    n_slots = B + 3
    stride = (V + 7) // 8 * 8 + 8  # columns >= V exist and must stay untouched
    kinds = [(0, 0), None, (N_TABLES - 1, gb.n_states - 1), (-1, 0), (N_TABLES - 1, 0), (0, -1),
             (0, ga.walk(0, b"abe")), (N_TABLES - 1, gb.n_states - 8), (0, ga.walk(0, b"abx")), (N_TABLES - 1, 5)]
    perm = rng.permutation(n_slots)
    slots = np.full(B, -1, dtype=np.int32)
    entries = []
    for r in range(B):
        kind = kinds[r % len(kinds)] if B > 1 else kinds[0]
        if kind is None:
            continue
        slots[r] = perm[r]
        ends = [EOS] if r % 3 else [EOS, 4, 9]  # ids with bytes can be end ids too
        if r % len(kinds) == 5:
            ends = [EOS] + list(range(30, 46))  # all 17
        entries.append([int(perm[r]), kind[0], kind[1], len(ends)] + ends + [-1] * (ref.GRAMMAR_MAX_END - len(ends)))
    out0 = torch.from_numpy(rng.standard_normal((n_slots, stride)).astype(np.float32))
    return dict(V=V, B=B, off=off, data=data, n_slots=n_slots, stride=stride, slots=slots,
                entries=np.asarray(entries, dtype=np.int32).reshape(-1, ref.GRAMMAR_SEED_WORDS), out0=out0)


def poison(case) -> torch.Tensor:
    """The rows before the mask, with NaN sentinels where nothing may be written: rows whose slot is
    not in the batch or holds no table, and the columns >= V of every row."""
    out = case["out0"].clone()
    out[:, case["V"]:] = float("nan")
    live = {int(e[0]) for e in case["entries"] if e[1] >= 0} & {int(s) for s in case["slots"]}
    for s in range(case["n_slots"]):
        if s not in live:
            out[s] = float("nan")
    return out


def cpu_state(case):
    """(pool, rec) on the CPU with the case's tables loaded and slots seeded."""
    pool = torch.zeros((N_TABLES, ref.GRAMMAR_TABLE_WORDS), dtype=torch.int32)
    for entry, g in tables().items():
        ref.grammar_load(pool, entry, 0, ref.grammar_pack(g.cmap, g.trans, g.accept))
    rec = torch.full((case["n_slots"], ref.GRAMMAR_SLOT_WORDS), -1, dtype=torch.int32)
    ref.grammar_seed(rec, case["entries"])
    return pool, rec


def reference_mask(case, pool, rec, out=None, mutant=None) -> torch.Tensor:
    out = poison(case) if out is None else out
    ref.grammar_mask(out, case["V"], pool, rec, torch.from_numpy(case["slots"]), case["B"], case["off"],
                     case["data"], mutant=mutant)
    return out


def pick_tokens(case, masked: torch.Tensor, step: int = 0) -> np.ndarray:
    """One sampled id per row from what the mask kept: every third row an end id when one
    survived, otherwise a kept id chosen by the row and ``step``; rows without a slot get id 2."""
    toks = np.full(case["B"], 2, dtype=np.int32)
    ends = {int(e[0]): [int(x) for x in e[4:4 + e[3]]] for e in case["entries"]}
    for r, slot in enumerate(case["slots"]):
        if slot < 0:
            continue
        kept = np.nonzero(np.isfinite(masked[slot, :case["V"]].numpy()))[0]
        e = ends.get(int(slot), [])
        e = [t for t in e if t in kept]
        if (r + step) % 3 == 0 and e:
            toks[r] = e[-1]  # the last one: an end id that has bytes where the row has several
        elif kept.size:
            toks[r] = kept[(3 * kept.size // 4 + 7 * r + 13 * step) % kept.size]
    return toks


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)

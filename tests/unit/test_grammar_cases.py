"""The grammar compiler against Python's ``re`` and ``json``, and the kernel test's inputs against
the mutants they must reject (tests/grammar_cases.py)."""
import itertools
import json
import re
import time

import numpy as np
import pytest
import torch

from polykey_service_amd.engine import grammar as G
from polykey_service_amd.engine.tokenizer import ByteTokenizer
from polykey_service_amd.ops import reference as ref
from tests import grammar_cases as gc


def _strings():
    for n in range(gc.MAX_LEN + 1):
        for t in itertools.product(gc.ALPHABET, repeat=n):
            yield "".join(t)


STRINGS = list(_strings())


def _check(g):
    assert g.is_trimmed() and 1 <= g.n_states <= G.MAX_STATES
    assert g.trans.dtype == np.int16 and g.trans.min() >= G.DEAD and g.trans.max() < g.n_states


@pytest.mark.parametrize("pattern", gc.REGEX_PATTERNS)
def test_regex_equals_re_fullmatch_on_every_short_string(pattern):
    t0 = time.perf_counter()
    g = G.compile_regex(pattern)
    dt = time.perf_counter() - t0
    _check(g)
    print(f"{pattern!r}: {g.n_states} states, {g.n_classes} byte classes, compiled in {dt * 1e3:.1f} ms")
    rx = re.compile(pattern)
    wrong = [s for s in STRINGS if g.accepts(s) != (rx.fullmatch(s) is not None)]
    assert not wrong, wrong[:5]
    assert len(STRINGS) == sum(6 ** n for n in range(6))


def test_regex_control_characters_and_dot():
    for pattern, strings in ((r"\n|\t|\r| ", ["\n", "\t", "\r", " ", "n", ""]), (r"a.b", ["a\nb", "a\rb", "aéb", "a€b"]),
                             (r"[^a]", ["\n", "\U0001F600", "a"])):
        g = G.compile_regex(pattern)
        for s in strings:
            assert g.accepts(s) == (re.fullmatch(pattern, s) is not None), (pattern, s)


def test_ill_formed_utf8_is_never_accepted():
    g = G.compile_regex(r".*")
    for bad in (b"\xc0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xe2\x82", b"\x80", b"\xff"):
        assert not g.accepts(bad), bad
    assert g.accepts("a€\U0001F600é".encode())


@pytest.mark.parametrize("pattern,word", gc.UNSUPPORTED_REGEX)
def test_unsupported_regex_constructs_name_themselves(pattern, word):
    with pytest.raises(ValueError, match=re.escape(word)):
        G.compile_regex(pattern)


def test_choice_is_exactly_its_strings():
    g = G.compile_choice(["yes", "no", "né€", "yes!"])
    _check(g)
    for s in ("yes", "no", "né€", "yes!"):
        assert g.accepts(s)
    for s in ("", "y", "ye", "yesno", "nope", "né", "NO"):
        assert not g.accepts(s)
    for bad in ([], [""], "yes", ["a", 1], None):
        with pytest.raises(ValueError, match="guided_choice"):
            G.compile_choice(bad)


@pytest.mark.parametrize("name", list(gc.JSON_SCHEMAS))
def test_json_random_walks_parse_and_conform(name):
    schema = gc.JSON_SCHEMAS[name]
    t0 = time.perf_counter()
    g = G.compile_json(schema)
    dt = time.perf_counter() - t0
    _check(g)
    print(f"{name}: {g.n_states} states, {g.n_classes} byte classes, compiled in {dt * 1e3:.1f} ms")
    rng = np.random.default_rng(11)
    for _ in range(200):
        text = gc.random_accepted(g, rng).decode("utf-8")
        assert gc.conforms(schema, json.loads(text)), text
    for x in gc.JSON_INSTANCES[name]:
        assert gc.conforms(schema, x)
        for text in (json.dumps(x), json.dumps(x, separators=(",", ":")), json.dumps(x, ensure_ascii=False)):
            assert g.accepts(text), text
    for text in gc.JSON_NEAR_MISSES.get(name, []):
        assert not g.accepts(text), text


@pytest.mark.parametrize("schema,keyword", gc.UNSUPPORTED_JSON)
def test_unsupported_schema_keywords_name_themselves(schema, keyword):
    with pytest.raises(ValueError, match=re.escape(keyword)):
        G.compile_json(schema)


def test_json_takes_text_and_rejects_recursion_free_nonsense():
    assert G.compile_json('{"type": "boolean"}').accepts("true")
    for bad in ("{", "[1]", {"type": "thing"}, {"type": "array"}, {}):
        with pytest.raises(ValueError, match="guided_json"):
            G.compile_json(bad)


def test_state_limit_and_work_bound():
    g = G.compile_regex(gc.CHAIN)
    assert g.n_states == G.MAX_STATES
    with pytest.raises(ValueError, match="too large"):
        G.compile_regex(gc.CHAIN + "a")          # 2049 states after minimisation
    t0 = time.perf_counter()
    with pytest.raises(ValueError, match="too large"):
        G.compile_regex(r"(a|b)*a(a|b){20}")     # 2^21 subsets: stopped at the working bound
    assert time.perf_counter() - t0 < 5.0


def test_cache_is_keyed_by_kind_and_canonical_source():
    a = G.compile_grammar("json", {"type": "integer"})
    assert G.compile_grammar("json", '{"type":   "integer"}') is a
    assert G.compile_grammar("regex", "-?[0-9]+") is not a
    c = G.compile_grammar("choice", ["a", "b"])
    assert G.compile_grammar("choice", ("a", "b")) is c and G.compile_grammar("regex", "a|b").key == c.key


def test_vocabulary_check():
    tok = ByteTokenizer(300)
    off, data = G.token_bytes(tok)
    assert off.dtype == np.int32 and off.size == 301 and data.dtype == np.uint8
    assert [bytes(data[off[t]:off[t + 1]]) for t in (0, 1, 2, 3, 3 + 65, 258, 259)] == [b"", b"", b"", b"\x00", b"A", b"\xff", b""]
    singles = G.single_byte_tokens(off, data)
    G.check_vocab(G.compile_regex(r".*"), singles)
    few = G.single_byte_tokens(*G.token_bytes(ByteTokenizer(100)))  # bytes 0..96 only
    G.check_vocab(G.compile_regex(r"[A-Z]+"), few)
    with pytest.raises(ValueError, match="single-byte token"):
        G.check_vocab(G.compile_regex(r"[a-z]+"), few)


def _hf(model, decoder, pre=None, specials=()):
    import tokenizers
    from tokenizers import AddedToken

    class T:  # what token_bytes reads of engine.tokenizer.HFTokenizer
        pass
    t = T()
    t.tok = tokenizers.Tokenizer(model)
    t.tok.decoder = decoder
    if pre is not None:
        t.tok.pre_tokenizer = pre
    t.tok.add_special_tokens([AddedToken(s, special=True) for s in specials])
    t.vocab_size = t.tok.get_vocab_size()
    return t


def test_token_bytes_of_a_byte_level_bpe_vocabulary():
    from tokenizers import decoders, models, pre_tokenizers
    u2b = G._gpt2_unicode_to_byte()
    b2u = {b: u for u, b in u2b.items()}
    assert len(b2u) == 256
    vocab = {b2u[b]: b for b in range(256)}
    vocab.update({b2u[0x20] + "hi": 256, b2u[0xC3] + b2u[0xA9]: 257, "ab": 258})
    t = _hf(models.BPE(vocab=vocab, merges=[]), decoders.ByteLevel(), pre_tokenizers.ByteLevel(add_prefix_space=False),
            specials=["<|end|>"])
    off, data = G.token_bytes(t, 264)
    spell = [bytes(data[off[i]:off[i + 1]]) for i in range(264)]
    assert spell[:256] == [bytes([b]) for b in range(256)]
    assert spell[256:] == [b" hi", "é".encode(), b"ab", b"", b"", b"", b"", b""]
    assert len(G.single_byte_tokens(off, data)) == 256


def test_token_bytes_of_a_sentencepiece_style_vocabulary():
    from tokenizers import decoders, models
    vocab = {"<unk>": 0, "<s>": 1, "</s>": 2}
    vocab.update({f"<0x{b:02X}>": 3 + b for b in range(256)})
    vocab.update({"▁the": 259, "▁": 260, "é": 261, "a▁b": 262})
    t = _hf(models.BPE(vocab=vocab, merges=[], unk_token="<unk>", byte_fallback=True),
            decoders.Sequence([decoders.Replace("▁", " "), decoders.ByteFallback(), decoders.Fuse()]),
            specials=["<unk>", "<s>", "</s>"])
    off, data = G.token_bytes(t)
    spell = [bytes(data[off[i]:off[i + 1]]) for i in range(t.vocab_size)]
    assert spell[:3] == [b"", b"", b""] and spell[3:259] == [bytes([b]) for b in range(256)]
    assert spell[259:] == [b" the", b" ", "é".encode(), b"a b"]


# ------------------------------------------------------------------- the kernel test's inputs
@pytest.fixture(scope="module")
def references():
    out = {}
    for V, B in gc.SHAPES[:2]:
        case = gc.kernel_case(V, B)
        pool, rec = gc.cpu_state(case)
        out[(V, B)] = (case, pool, rec, gc.reference_mask(case, pool, rec))
    return out


def test_kernel_inputs_cover_what_they_claim(references):
    case, pool, rec, want = references[(1000, 64)]
    V = case["V"]
    lens = set(np.diff(case["off"]).tolist())
    assert lens == {0, 1, 2, 7, 40}
    assert (case["slots"] < 0).any() and (case["entries"][:, 1] < 0).any()          # -1 and table-less slots
    assert {0, gc.N_TABLES - 1} <= set(case["entries"][:, 1].tolist())
    states = {(int(e[1]), int(e[2])) for e in case["entries"]}
    assert (0, 0) in states and (gc.N_TABLES - 1, ref.GRAMMAR_MAX_STATES - 1) in states and (0, -1) in states
    # untouched: NaN rows stay NaN, columns >= V stay NaN, a kept word keeps its bits
    before = gc.poison(case)
    assert bool(torch.isnan(want[:, V:]).all())
    same = ~torch.isinf(want)
    assert torch.equal(gc.bits(want)[same], gc.bits(before)[same])
    # tokens that die on their first and on their last byte, at the start state of WORDS
    ga = gc.tables()[0]
    spell = lambda t: bytes(case["data"][case["off"][t]:case["off"][t + 1]])
    assert ga.walk(0, spell(13)[:1]) < 0 and ga.walk(0, spell(14)[:-1]) >= 0 and ga.walk(0, spell(14)) < 0
    assert len(states) >= 9 and (case["entries"][:, 3] == 17).any()  # every kind of row; all 17 end ids


@pytest.mark.parametrize("mutant", gc.MUTANTS_MASK)
def test_mask_mutants_are_rejected(references, mutant):
    hits = 0
    for case, pool, rec, want in references.values():
        got = gc.reference_mask(case, pool, rec, mutant=mutant)
        hits += int(not torch.equal(gc.bits(got), gc.bits(want)))
    assert hits, f"the kernel test's inputs cannot tell the mutant {mutant!r} from the reference"


@pytest.mark.parametrize("mutant", gc.MUTANTS_ADVANCE)
def test_advance_mutants_are_rejected(references, mutant):
    hits = 0
    for case, pool, rec, want in references.values():
        toks = gc.pick_tokens(case, want)
        a, b = rec.clone(), rec.clone()
        ref.grammar_advance(pool, a, case["slots"], toks, case["B"], case["off"], case["data"], case["V"])
        ref.grammar_advance(pool, b, case["slots"], toks, case["B"], case["off"], case["data"], case["V"], mutant=mutant)
        assert not torch.equal(a, rec) or case["B"] == 1  # the true advance moves something
        hits += int(not torch.equal(a, b))
    assert hits, f"the kernel test's inputs cannot tell the mutant {mutant!r} from the reference"

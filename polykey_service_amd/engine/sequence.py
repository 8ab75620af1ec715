"""Request / sequence state for the continuous-batching engine."""
from __future__ import annotations

import dataclasses
import enum
import itertools
import json
import math
import time
from typing import List, Optional, Sequence as Seq


MAX_LOGPROBS = 20  # longest top_logprobs list (the logprobs kernel's compile-time constant)
MAX_GUIDED_STOP_IDS = 16  # plus eos: the 17 end ids of a grammar slot (ops/grammar.py)
MAX_LOGIT_BIAS = 300  # longest logit_bias list (the penalty kernels' per-slot table, ops/penalties.py)
MAX_N = 16  # most choices of one request (parallel sampling): one fork fits one copy launch


def _norm_logit_bias(v) -> tuple:
    """dict with string or int keys (the OpenAI / Struct forms) or a list of (id, value) pairs →
    a tuple of (int id, float value) sorted by id.  Duplicates are kept for ``validate`` to reject."""
    items = v.items() if isinstance(v, dict) else v
    out = []
    try:
        for k, b in items:
            if isinstance(k, bool) or isinstance(b, bool) or (isinstance(k, float) and k != int(k)):
                raise ValueError
            out.append((int(k), float(b)))
    except (TypeError, ValueError):
        raise ValueError("logit_bias must map token ids to numbers") from None
    return tuple(sorted(out))


@dataclasses.dataclass
class SamplingParams:
    max_tokens: int = 16
    temperature: float = 0.0      # 0 → greedy
    top_p: float = 1.0
    top_k: int = 0
    min_p: float = 0.0
    seed: Optional[int] = None
    stop_token_ids: Seq[int] = ()
    ignore_eos: bool = False
    stop: Seq[str] = ()           # stop strings (checked on detokenized text)
    cache_salt: Optional[str] = None  # prefix-cache namespace (e.g. a tenant id); None = shared
    # per-token log-probabilities from the raw logits: None = off, 0 = the sampled token only,
    # 1..20 = plus that many top alternatives (ops/sampler.py logprobs)
    logprobs: Optional[int] = None
    # penalties, applied to a copy of the logits before sampling (logprobs stay raw), in this
    # order: repetition (Hugging Face rule over prompt + generated tokens), frequency and presence
    # (OpenAI rule over generated tokens), logit_bias.  1 / 0 / 0 / () = off.
    repetition_penalty: float = 1.0
    frequency_penalty: float = 0.0
    presence_penalty: float = 0.0
    logit_bias: Seq = ()          # sorted tuple of (token id, bias) pairs (from_dict also takes a dict)
    # guided decoding (engine/grammar.py): at most one of a regex the completion must full-match, a
    # list of strings it must be one of, or a JSON Schema (canonical JSON text) it must conform to
    guided_regex: Optional[str] = None
    guided_choice: Seq[str] = ()
    guided_json: Optional[str] = None
    guided_suffix: str = ""       # literal text after the guided_json value (a forced tool call's closing)
    # the LoRA adapter the request runs on (a name from EngineConfig.lora_modules); None = the base model
    lora: Optional[str] = None
    # speculative decoding (engine/spec.py): None = the engine's setting, False = never draft for this
    # request; True on an engine without speculation is ignored
    speculative: Optional[bool] = None
    # parallel sampling: the request yields n choices, index 0 .. n-1, each an ordinary sequence with
    # these parameters (choice i samples with seed + i); 1 .. MAX_N and at most the engine's max_num_seqs
    n: int = 1
    # log-probabilities of the *prompt* tokens (teacher forcing): None = off, 0 = each prompt token's
    # logprob and rank, 1..20 = plus that many top alternatives; from the raw logits of the row
    # before the token (ops/sampler.py prompt_logprobs).  Only choice 0 of an n > 1 request computes.
    # An init-only variable kept as a plain attribute, not a dataclass field: ``dataclasses.fields`` /
    # ``asdict`` -- and with them the remote-engine frame of a request that does not ask -- are what
    # they were; ``dataclasses.replace`` carries it, ``from_dict`` and the wire name it explicitly
    prompt_logprobs: dataclasses.InitVar[Optional[int]] = None

    def __post_init__(self, prompt_logprobs=None):
        self.prompt_logprobs = prompt_logprobs

    @property
    def has_penalties(self) -> bool:
        return (self.repetition_penalty != 1.0 or self.frequency_penalty != 0.0 or self.presence_penalty != 0.0
                or len(self.logit_bias) > 0)

    @property
    def guided(self) -> bool:
        return self.guided_regex is not None or len(self.guided_choice) > 0 or self.guided_json is not None

    def validate(self, max_model_len: int) -> None:
        if self.max_tokens < 1:
            raise ValueError("max_tokens must be >= 1")
        if self.temperature < 0:
            raise ValueError("temperature must be >= 0")
        if isinstance(self.n, bool) or not isinstance(self.n, int) or not 1 <= self.n <= MAX_N:
            raise ValueError(f"n must be an integer in [1, {MAX_N}]")
        if not 0 < self.top_p <= 1:
            raise ValueError("top_p must be in (0, 1]")
        if self.top_k < 0:
            raise ValueError("top_k must be >= 0")
        if not 0 <= self.min_p < 1:
            raise ValueError("min_p must be in [0, 1)")
        if self.logprobs is not None and (isinstance(self.logprobs, bool) or not isinstance(self.logprobs, int)
                                          or not 0 <= self.logprobs <= MAX_LOGPROBS):
            raise ValueError(f"logprobs must be an integer in [0, {MAX_LOGPROBS}]")
        pl = self.prompt_logprobs
        if pl is not None and (isinstance(pl, bool) or not isinstance(pl, int) or not 0 <= pl <= MAX_LOGPROBS):
            raise ValueError(f"prompt_logprobs must be an integer in [0, {MAX_LOGPROBS}]")
        for name in ("frequency_penalty", "presence_penalty"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not -2 <= v <= 2:
                raise ValueError(f"{name} must be in [-2, 2]")
        r = self.repetition_penalty
        if isinstance(r, bool) or not isinstance(r, (int, float)) or not math.isfinite(r) or not r > 0:
            raise ValueError("repetition_penalty must be finite and > 0")
        if self.logit_bias:
            lb = _norm_logit_bias(self.logit_bias)
            if len(lb) > MAX_LOGIT_BIAS:
                raise ValueError(f"logit_bias holds at most {MAX_LOGIT_BIAS} entries")
            if len({t for t, _ in lb}) != len(lb):
                raise ValueError("logit_bias token ids must be unique")
            if any(t < 0 for t, _ in lb):
                raise ValueError("logit_bias token id out of range")
            if any(not math.isfinite(b) or not -100 <= b <= 100 for _, b in lb):
                raise ValueError("logit_bias values must be in [-100, 100]")
            self.logit_bias = lb
        if self.guided_regex is not None and not isinstance(self.guided_regex, str):
            raise ValueError("guided_regex must be a string")
        gc = self.guided_choice
        if isinstance(gc, (str, bytes)) or not isinstance(gc, (list, tuple)) or any(
                not isinstance(c, str) or not c for c in gc):
            raise ValueError("guided_choice must be a non-empty list of non-empty strings")
        self.guided_choice = tuple(gc)
        if isinstance(self.guided_json, dict):
            self.guided_json = json.dumps(self.guided_json, sort_keys=True)
        if self.guided_json is not None and not isinstance(self.guided_json, str):
            raise ValueError("guided_json must be a JSON Schema (a dict, or its JSON text)")
        if self.lora is not None and (not isinstance(self.lora, str) or not self.lora):
            raise ValueError("lora must be the name of a served adapter")
        if self.speculative is not None and not isinstance(self.speculative, bool):
            raise ValueError("speculative must be a boolean")
        if not isinstance(self.guided_suffix, str) or (self.guided_suffix and self.guided_json is None):
            raise ValueError("guided_suffix needs guided_json")
        if (self.guided_regex is not None) + bool(gc) + (self.guided_json is not None) > 1:
            raise ValueError("at most one of guided_regex, guided_choice and guided_json may be set")
        if self.guided:
            if self.ignore_eos:
                raise ValueError("guided decoding cannot be combined with ignore_eos")
            if len(self.stop_token_ids) > MAX_GUIDED_STOP_IDS:
                raise ValueError(f"a guided request takes at most {MAX_GUIDED_STOP_IDS} stop_token_ids")
            from . import grammar  # compiled here (and cached) so that every front end rejects it early
            grammar.grammar_for(self)

    @classmethod
    def from_dict(cls, d: dict) -> "SamplingParams":
        kw = {}
        for f in dataclasses.fields(cls):
            if f.name in d and d[f.name] is not None:
                v = d[f.name]
                if f.name in ("max_tokens", "top_k"):
                    v = int(v)
                elif f.name in ("temperature", "top_p", "min_p"):
                    v = float(v)
                elif f.name in ("repetition_penalty", "frequency_penalty", "presence_penalty"):
                    if isinstance(v, (bool, str)):
                        raise ValueError(f"{f.name} must be a number")
                    v = float(v)
                elif f.name == "logit_bias":
                    v = _norm_logit_bias(v)
                elif f.name == "seed":
                    v = int(v)
                elif f.name == "n":
                    if isinstance(v, (bool, str)) or (isinstance(v, float) and v != int(v)):
                        raise ValueError(f"n must be an integer in [1, {MAX_N}]")
                    v = int(v)
                elif f.name in ("stop_token_ids",):
                    v = tuple(int(x) for x in v)
                elif f.name == "stop":
                    v = (v,) if isinstance(v, str) else tuple(v)
                elif f.name == "ignore_eos":
                    v = bool(v)
                elif f.name == "cache_salt":
                    v = str(v)
                elif f.name == "guided_regex":
                    if not isinstance(v, str):
                        raise ValueError("guided_regex must be a string")
                elif f.name == "guided_choice":
                    # (an empty list is the unset field as it comes back over the remote-engine wire)
                    if isinstance(v, (str, bytes)) or not isinstance(v, (list, tuple)) or any(
                            not isinstance(c, str) or not c for c in v):
                        raise ValueError("guided_choice must be a non-empty list of non-empty strings")
                    v = tuple(v)
                elif f.name == "guided_json":
                    if isinstance(v, str):
                        try:
                            v = json.loads(v)
                        except ValueError:
                            raise ValueError("guided_json is not valid JSON") from None
                    if not isinstance(v, dict):
                        raise ValueError("guided_json must be a JSON Schema (a dict, or its JSON text)")
                    v = json.dumps(v, sort_keys=True)
                elif f.name == "guided_suffix":
                    v = str(v)
                elif f.name == "lora":
                    if not isinstance(v, str) or not v:
                        raise ValueError("lora must be the name of a served adapter")
                elif f.name == "speculative":
                    if not isinstance(v, bool):
                        raise ValueError("speculative must be a boolean")
                elif f.name == "logprobs":
                    if isinstance(v, bool) or (isinstance(v, float) and v != int(v)):
                        raise ValueError(f"logprobs must be an integer in [0, {MAX_LOGPROBS}]")
                    v = int(v)
                kw[f.name] = v
        v = d.get("prompt_logprobs")
        if v is not None:
            if isinstance(v, (bool, str)) or (isinstance(v, float) and v != int(v)):
                raise ValueError(f"prompt_logprobs must be an integer in [0, {MAX_LOGPROBS}]")
            kw["prompt_logprobs"] = int(v)
        return cls(**kw)


def check_n(llm, params: SamplingParams) -> None:
    """``params.n`` against the sequence cap of the engine behind ``llm`` (an AsyncLLM or a pool of
    them), where a front end can see it; the engine checks again at ``add_request``."""
    eng = getattr(llm, "engine", None)
    cap = eng.cfg.max_num_seqs if eng is not None else None
    if cap is not None and params.n > cap:
        raise ValueError(f"n must be at most max_num_seqs ({cap}), got {params.n}")


class SeqStatus(enum.Enum):
    WAITING = 0
    RUNNING = 1
    FINISHED = 2


class FinishReason(str, enum.Enum):
    LENGTH = "length"
    STOP = "stop"
    ABORT = "abort"
    ERROR = "error"


_ids = itertools.count(1)


class Sequence:
    __slots__ = ("seq_id", "request_id", "prompt_ids", "output_ids", "params", "status", "num_computed",
                 "arrival", "first_scheduled", "first_token_time", "finish_time", "finish_reason",
                 "num_preemptions", "eos_token_id", "token_times", "user", "num_cached_tokens",
                 "cache_salt", "logprobs", "grammar", "spec_state", "spec_drafted", "spec_accepted",
                 "index", "choices", "forked_tokens", "prompt_logprobs", "prompt_lp_missing",
                 "prompt_lp_delivered")

    def __init__(self, request_id: str, prompt_ids: List[int], params: SamplingParams, eos_token_id: int = -1,
                 user=None, cache_salt: Optional[str] = None, index: int = 0):
        self.seq_id = next(_ids)
        self.request_id = request_id
        # parallel sampling: the choice this sequence is of its request, every choice of the request
        # (None for n = 1), and the prompt tokens whose KV it got from choice 0's by a fork
        self.index = index
        self.choices: Optional[List["Sequence"]] = None
        self.forked_tokens = 0
        self.prompt_ids = list(prompt_ids)
        self.output_ids: List[int] = []
        self.params = params
        self.status = SeqStatus.WAITING
        self.num_computed = 0
        self.arrival = time.monotonic()
        self.first_scheduled: Optional[float] = None
        self.first_token_time: Optional[float] = None
        self.finish_time: Optional[float] = None
        self.finish_reason: Optional[FinishReason] = None
        self.num_preemptions = 0
        self.num_cached_tokens = 0  # tokens whose KV came from the prefix cache
        self.eos_token_id = eos_token_id
        self.token_times: List[float] = []
        # one (logprob, [(id, logprob) x n]) per output token; None unless params.logprobs is set
        self.logprobs: Optional[list] = [] if getattr(params, "logprobs", None) is not None else None
        # prompt logprobs (choice 0 only): entry i = (logprob, rank, [(id, logprob) x n]) of prompt_ids[i]
        # given prompt_ids[:i], entry 0 None; entries fill in as prefill chunks complete and survive a
        # preemption.  ``prompt_lp_missing`` counts the entries still to compute (0: not asking)
        ask = getattr(params, "prompt_logprobs", None) is not None and index == 0
        self.prompt_logprobs: Optional[list] = [None] * len(self.prompt_ids) if ask else None
        self.prompt_lp_missing = len(self.prompt_ids) - 1 if ask else 0
        self.prompt_lp_delivered = False
        self.grammar = None  # the request's compiled constraint (engine/grammar.py), set by add_request
        # speculative decoding: the proposer's per-sequence state, and draft tokens proposed / accepted
        # (None on an engine without speculation: seq_metrics then reports neither)
        self.spec_state = None
        self.spec_drafted: Optional[int] = None
        self.spec_accepted: Optional[int] = None
        self.user = user
        # prefix-cache namespace (Scheduler._salt); None = the request's params.cache_salt
        self.cache_salt = cache_salt if cache_salt is not None else getattr(params, "cache_salt", None)

    @property
    def num_tokens(self) -> int:
        return len(self.prompt_ids) + len(self.output_ids)

    @property
    def num_pending(self) -> int:
        """Tokens whose KV is not yet in the cache."""
        return self.num_tokens - self.num_computed

    def token_slice(self, start: int, end: int) -> List[int]:
        n = len(self.prompt_ids)
        if end <= n:
            return self.prompt_ids[start:end]
        if start >= n:
            return self.output_ids[start - n:end - n]
        return self.prompt_ids[start:] + self.output_ids[:end - n]

    @property
    def key(self):
        """The scheduler's registry key: the request id for choice 0 (so n = 1 is as ever), (id, index) beyond."""
        return self.request_id if self.index == 0 else (self.request_id, self.index)

    @property
    def seed(self) -> int:
        return (self.params.seed + self.index if self.params.seed is not None
                else self.seq_id * 2654435761) & 0x7FFFFFFF

    def is_finished(self) -> bool:
        return self.status == SeqStatus.FINISHED

    def append_token(self, tok: int, now: float) -> Optional[FinishReason]:
        self.output_ids.append(tok)
        self.token_times.append(now)
        if self.first_token_time is None:
            self.first_token_time = now
        p = self.params
        if not p.ignore_eos and (tok == self.eos_token_id or tok in p.stop_token_ids):
            return FinishReason.STOP
        if len(self.output_ids) >= p.max_tokens:
            return FinishReason.LENGTH
        return None


@dataclasses.dataclass
class RequestOutput:
    request_id: str
    new_token_ids: List[int]
    finished: bool
    finish_reason: Optional[str] = None
    num_prompt_tokens: int = 0
    num_output_tokens: int = 0
    metrics: Optional[dict] = None
    # the choice of the request (parallel sampling) this output belongs to; ``finished`` and
    # ``finish_reason`` refer to that choice.  Keyword-only: the positional order ends with logprobs
    index: int = dataclasses.field(default=0, kw_only=True)
    # the request's prompt logprobs (SamplingParams.prompt_logprobs): one entry per prompt token, the
    # first None, the others (logprob, rank, [(id, logprob) x n]); set once, on the index-0 output
    # that carries the first generated token.  Keyword-only too
    prompt_logprobs: Optional[list] = dataclasses.field(default=None, kw_only=True)
    # one (logprob, [(id, logprob) x n]) per entry of new_token_ids when the request asked for them
    logprobs: Optional[list] = None


def seq_metrics(s: Sequence) -> dict:
    t0 = s.arrival
    ttft = (s.first_token_time - t0) if s.first_token_time else None
    e2e = (s.finish_time - t0) if s.finish_time else None
    itl = None
    if len(s.token_times) > 1:
        itl = (s.token_times[-1] - s.token_times[0]) / (len(s.token_times) - 1)
    m = {
        "queue_s": (s.first_scheduled - t0) if s.first_scheduled else None,
        "ttft_s": ttft, "e2e_s": e2e, "mean_itl_s": itl, "preemptions": s.num_preemptions,
        "cached_prompt_tokens": s.num_cached_tokens,
    }
    if s.choices is not None:  # a choice of an n > 1 request
        m["forked_prompt_tokens"] = s.forked_tokens
    if s.spec_drafted is not None:  # an engine with speculative decoding configured
        m["spec_drafted"] = s.spec_drafted
        m["spec_accepted"] = s.spec_accepted
    return m

"""LoRA adapters (Hugging Face PEFT format) and their device-resident store.

An adapter targets any of the seven projections q, k, v, o, gate, up, down of every layer:

    t     = bf16(A xn)                 fp32 products and sums, one rounding
    delta = s * (B t)                  fp32, s = lora_alpha / r  (rsLoRA: lora_alpha / sqrt(r))
    y     = W xn + delta

:class:`LoraAdapter` is one adapter on the host (load / save / random); :class:`LoraState` holds
every configured adapter on the device, one slot each, zero-padded to ``max_lora_rank``, stacked and
ordered as the fused projections they accompany (qkv: A of q | k | v stacked along the rank axis, B
rows in q | k | v order; gate_up: A of gate | up stacked, B rows interleaved by 16 like the weight),
and applies the deltas through the shrink / expand kernels (ops/lora.py).  All adapters are
resident; there is no run-time load, unload or eviction.
"""
from __future__ import annotations

import dataclasses
import json
import logging
import math
import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ..ops import gemm
from ..ops import lora as lora_ops
from .config import ModelConfig

TARGETS = ("q", "k", "v", "o", "gate", "up", "down")
MAX_SLOTS = 32
_KEY = re.compile(r"^base_model\.model\.model\.layers\.(\d+)\.(self_attn|mlp)\.(\w+)_proj\.lora_([AB])\.weight$")
_BLOCK = {"q": "self_attn", "k": "self_attn", "v": "self_attn", "o": "self_attn", "gate": "mlp", "up": "mlp",
          "down": "mlp"}


def proj_dims(cfg: ModelConfig, p: str) -> Tuple[int, int]:
    """(K, N) of projection ``p`` of the base model."""
    H, I = cfg.hidden_size, cfg.intermediate_size
    return {"q": (H, cfg.q_size), "k": (H, cfg.kv_size), "v": (H, cfg.kv_size), "o": (cfg.q_size, H),
            "gate": (H, I), "up": (H, I), "down": (I, H)}[p]


def lora_bytes(cfg: ModelConfig, slots: int, max_rank: int) -> int:
    """slots x max_rank x sum_p (K_p + N_p) x 2 bytes x layers."""
    return slots * max_rank * sum(sum(proj_dims(cfg, p)) for p in TARGETS) * 2 * cfg.num_layers


class LoraAdapter:
    """One adapter on the host: ``tensors[(layer, p)] = (A [r, K], B [N, r])`` bf16."""

    def __init__(self, rank: int, alpha: float, targets: Sequence[str], tensors: Dict[Tuple[int, str], tuple],
                 use_rslora: bool = False):
        self.rank, self.alpha, self.use_rslora = int(rank), float(alpha), bool(use_rslora)
        self.targets = tuple(p for p in TARGETS if p in set(targets))
        self.tensors = tensors

    @property
    def scale(self) -> float:
        return self.alpha / math.sqrt(self.rank) if self.use_rslora else self.alpha / self.rank

    # ------------------------------------------------------------------ PEFT directory
    @classmethod
    def load(cls, path: str, cfg: ModelConfig, max_rank: int = 64) -> "LoraAdapter":
        """Read ``adapter_config.json`` + ``adapter_model.safetensors``; ValueError (naming the
        offending key) for what this engine does not serve."""
        from safetensors import safe_open
        with open(os.path.join(path, "adapter_config.json")) as f:
            ac = json.load(f)
        if ac.get("use_dora"):
            raise ValueError(f"LoRA adapter {path}: use_dora is not supported")
        if ac.get("bias", "none") != "none":
            raise ValueError(f"LoRA adapter {path}: bias={ac['bias']!r} is not supported (bias must be \"none\")")
        for key in ("rank_pattern", "alpha_pattern", "modules_to_save"):
            if ac.get(key):
                raise ValueError(f"LoRA adapter {path}: a non-empty {key} is not supported")
        rank = int(ac.get("r", 0))
        if not 1 <= rank <= max_rank:
            raise ValueError(f"LoRA adapter {path}: rank r={rank} is outside 1..max_lora_rank={max_rank}")
        tm = ac.get("target_modules") or []
        tm = [tm] if isinstance(tm, str) else list(tm)
        targets = []
        for m in tm:
            p = m[:-5] if m.endswith("_proj") else m
            if p not in TARGETS:
                raise ValueError(f"LoRA adapter {path}: target module {m!r} is not supported (only "
                                 f"{', '.join(t + '_proj' for t in TARGETS)})")
            targets.append(p)
        found: Dict[Tuple[int, str], dict] = {}
        with safe_open(os.path.join(path, "adapter_model.safetensors"), framework="pt") as f:
            for key in f.keys():
                m = _KEY.match(key)
                if m is None or m.group(3) not in TARGETS or _BLOCK[m.group(3)] != m.group(2):
                    raise ValueError(f"LoRA adapter {path}: unsupported tensor {key!r} (only lora_A / lora_B of "
                                     f"{', '.join(t + '_proj' for t in TARGETS)} in the decoder layers)")
                layer, p, ab = int(m.group(1)), m.group(3), m.group(4)
                if layer >= cfg.num_layers:
                    raise ValueError(f"LoRA adapter {path}: {key!r} names layer {layer}, the base model has "
                                     f"{cfg.num_layers}")
                K, N = proj_dims(cfg, p)
                t = f.get_tensor(key)
                want = (rank, K) if ab == "A" else (N, rank)
                if tuple(t.shape) != want:
                    raise ValueError(f"LoRA adapter {path}: {key!r} has shape {tuple(t.shape)}, the base model "
                                     f"needs {want}")
                found.setdefault((layer, p), {})[ab] = t.to(torch.bfloat16)
        tensors = {}
        for (layer, p), ab in found.items():
            if set(ab) != {"A", "B"}:
                raise ValueError(f"LoRA adapter {path}: layer {layer} {p}_proj has lora_{'A' if 'A' in ab else 'B'} "
                                 f"without its pair")
            tensors[(layer, p)] = (ab["A"], ab["B"])
            if p not in targets:
                targets.append(p)
        return cls(rank, ac.get("lora_alpha", rank), targets, tensors, bool(ac.get("use_rslora")))

    @classmethod
    def random(cls, cfg: ModelConfig, rank: int = 8, alpha: float = 16.0, seed: int = 0,
               targets: Sequence[str] = TARGETS, b_std: float = 0.02) -> "LoraAdapter":
        """A random adapter (A ~ N(0, 1/K), B ~ N(0, b_std^2); b_std = 0: B = 0, the PEFT initialisation)."""
        g = torch.Generator().manual_seed(1000 + seed)
        tensors = {}
        for layer in range(cfg.num_layers):
            for p in TARGETS:
                if p not in targets:
                    continue
                K, N = proj_dims(cfg, p)
                A = (torch.randn((rank, K), generator=g) * K ** -0.5).to(torch.bfloat16)
                B = (torch.randn((N, rank), generator=g) * b_std).to(torch.bfloat16)
                tensors[(layer, p)] = (A, B)
        return cls(rank, alpha, targets, tensors)

    def save(self, path: str, base_model: str = "") -> None:
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        ac = {"peft_type": "LORA", "task_type": "CAUSAL_LM", "base_model_name_or_path": base_model, "r": self.rank,
              "lora_alpha": self.alpha, "use_rslora": self.use_rslora, "use_dora": False, "bias": "none",
              "target_modules": [p + "_proj" for p in self.targets], "rank_pattern": {}, "alpha_pattern": {},
              "modules_to_save": None, "lora_dropout": 0.0, "fan_in_fan_out": False}
        with open(os.path.join(path, "adapter_config.json"), "w") as f:
            json.dump(ac, f, indent=1)
        sd = {}
        for (layer, p), (A, B) in self.tensors.items():
            k = f"base_model.model.model.layers.{layer}.{_BLOCK[p]}.{p}_proj."
            sd[k + "lora_A.weight"] = A.contiguous()
            sd[k + "lora_B.weight"] = B.contiguous()
        save_file(sd, os.path.join(path, "adapter_model.safetensors"))

    def merged_delta(self, layer: int, p: str) -> Optional[torch.Tensor]:
        """s * B A as fp32 [N, K] (tests: the merged-weight reference), None when not targeted."""
        ab = self.tensors.get((layer, p))
        return None if ab is None else self.scale * (ab[1].float() @ ab[0].float())


@dataclasses.dataclass
class LoraProj:
    """The stacked adapters of one fused projection: ``A`` [slots, R, K], ``B`` [slots, N, seg_r]."""
    A: torch.Tensor
    B: torch.Tensor
    seg: lora_ops.Segments


class LoraState:
    """Every configured adapter on the device, plus the per-step row indices and the scratch."""

    def __init__(self, cfg: ModelConfig, adapters: Sequence[Tuple[str, LoraAdapter]], max_rank: int, max_rows: int,
                 device: torch.device, gu_elems: int = 0,
                 dtype: torch.dtype = torch.bfloat16):
        if not 1 <= len(adapters) <= MAX_SLOTS:
            raise ValueError(f"between 1 and {MAX_SLOTS} LoRA adapters can be resident (got {len(adapters)})")
        if not 1 <= max_rank <= lora_ops.MAX_SEG_RANK:
            raise ValueError(f"max_lora_rank must be in 1..{lora_ops.MAX_SEG_RANK} (got {max_rank})")
        self.names = [n for n, _ in adapters]
        if len(set(self.names)) != len(self.names):
            raise ValueError(f"LoRA adapter names must be unique (got {self.names})")
        self.slot_of = {n: i for i, n in enumerate(self.names)}
        self.max_rank = max_rank
        self.seg_r = (max_rank + 7) // 8 * 8
        self.device = device
        S, r = len(adapters), self.seg_r
        for name, ad in adapters:
            if ad.rank > max_rank:
                raise ValueError(f"LoRA adapter {name}: rank r={ad.rank} is above max_lora_rank={max_rank}")
        self.scale = torch.tensor([ad.scale for _, ad in adapters], dtype=torch.float32, device=device)
        self.ranks = torch.tensor([ad.rank for _, ad in adapters], dtype=torch.int32, device=device)
        q_sz, kv_sz, I = cfg.q_size, cfg.kv_size, cfg.intermediate_size
        fused = {"qkv": (("q", "k", "v"), lora_ops.Segments(q_sz, q_sz + kv_sz, 0)),
                 "o": (("o",), None), "gate_up": (("gate", "up"), lora_ops.Segments(2 * I, 2 * I, 16)),
                 "down": (("down",), None)}
        self.layers: List[Dict[str, Optional[LoraProj]]] = []
        for layer in range(cfg.num_layers):
            projs: Dict[str, Optional[LoraProj]] = {}
            for fname, (subs, seg) in fused.items():
                if not any((layer, p) in ad.tensors for _, ad in adapters for p in subs):
                    projs[fname] = None  # no adapter targets it: no launches, a delta of exactly zero
                    continue
                K = proj_dims(cfg, subs[0])[0]
                Ns = [proj_dims(cfg, p)[1] for p in subs]
                A = torch.zeros((S, len(subs) * r, K), dtype=torch.bfloat16)
                Bs = [torch.zeros((S, n, r), dtype=torch.bfloat16) for n in Ns]
                for s, (_, ad) in enumerate(adapters):
                    for j, p in enumerate(subs):
                        ab = ad.tensors.get((layer, p))
                        if ab is not None:
                            A[s, j * r: j * r + ad.rank] = ab[0]
                            Bs[j][s, :, :ad.rank] = ab[1]
                if fname == "gate_up":  # rows interleaved by 16 like the weight (gemm.interleave_gate_up)
                    B = torch.stack([gemm.interleave_gate_up(Bs[0][s], Bs[1][s]) for s in range(S)])
                else:
                    B = torch.cat(Bs, dim=1)
                projs[fname] = LoraProj(A.to(device), B.contiguous().to(device),
                                        seg or lora_ops.Segments.single(B.shape[1]))
            self.layers.append(projs)
        # t scratch of the LoRA state's own (never the split-K workspace: the chain keeps a pending
        # Partial alive there across launches); the widest t is the fused qkv's 3 rank blocks
        self.t = torch.zeros(max_rows * 3 * r, dtype=dtype, device=device)
        # row index of every token of the step: the runner points this at its staging section
        self.idx = torch.full((max_rows,), -1, dtype=torch.int32, device=device)
        # slabs of the chain's gate_up (split over K so that the SiLU slab reduce consumes them)
        self.ws_gu = (torch.empty(gu_elems, dtype=torch.float32, device=device)
                      if gu_elems and device.type == "cuda" else None)
        # whether the step being launched runs in the LoRA form (set by the runner per step)
        self.active = False
        self.nbytes = lora_bytes(cfg, S, max_rank)
        held = sum(t.numel() * t.element_size() for pr in self.layers for p in pr.values() if p is not None
                   for t in (p.A, p.B))
        logging.getLogger(__name__).info(
            "LoRA: %d adapters (%s), max rank %d, %d bytes by the formula, %d bytes held (+ %d scratch)",
            S, ", ".join(self.names), max_rank, self.nbytes, held,
            self.t.numel() * 2 + (0 if self.ws_gu is None else self.ws_gu.numel() * 4))

    def to(self, device: torch.device) -> "LoraState":
        """The same adapters on another device (tests: the CPU twin of a GPU engine)."""
        import copy
        new = copy.copy(self)
        new.device = device
        mv = lambda t: None if t is None else t.to(device)
        new.scale, new.ranks, new.t, new.idx = mv(self.scale), mv(self.ranks), mv(self.t), mv(self.idx)
        new.ws_gu = None
        new.layers = [{k: None if p is None else LoraProj(mv(p.A), mv(p.B), p.seg) for k, p in pr.items()}
                      for pr in self.layers]
        return new

    def _t(self, x: torch.Tensor, pr: LoraProj) -> torch.Tensor:
        return lora_ops.shrink(x, pr.A, self.idx, self.t, self.seg_r, ranks=self.ranks)

    def add_bf16(self, x: torch.Tensor, out: torch.Tensor, layer: int, name: str) -> torch.Tensor:
        """bf16 form: ``out`` [M, N] (the projection's bf16 result) += delta of input ``x``."""
        pr = self.layers[layer][name]
        if pr is not None:
            lora_ops.expand(out, self._t(x, pr), pr.B, self.scale, self.idx, pr.seg, ranks=self.ranks)
        return out

    def add_slab(self, x: torch.Tensor, p: gemm.Partial, layer: int, name: str) -> gemm.Partial:
        """slab form: slab 0 of ``p`` += delta of input ``x`` (between a split-K GEMM and its consumer)."""
        pr = self.layers[layer][name]
        if pr is not None:
            lora_ops.expand(lora_ops.slab0(p), self._t(x, pr), pr.B, self.scale, self.idx, pr.seg,
                            ranks=self.ranks)
        return p

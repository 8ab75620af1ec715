"""Cases and the checker of the KV block copy (pk_kv_copy_blocks / reference.kv_copy_blocks), shared by
tests/unit/test_kv_fork_cases.py (CPU: the checker accepts the reference and rejects five mutants) and
tests/kernels/test_kv_copy.py (GPU: the same cases through the HIP kernel).

Caches of ``layers = 2`` in the engine's two layouts (K [blocks, nkv, bs, 128], V [blocks, nkv, 128, bs]),
bf16 or FP8 bytes.  Every 16-bit word (byte for FP8) is position-coded from (tensor, block, offset) and
compared as an integer; destination blocks start as NaN patterns (0xFFFF, 0x7F for FP8).  The checker
demands that every dst block equals its src bit for bit in all 2 x layers tensors and that every other
block is bit-for-bit untouched."""
import itertools

import numpy as np
import torch

LAYERS = 2
HEAD_DIM = 128
FP8 = torch.float8_e4m3fn

# name -> (num_blocks, pairs)
PAIR_SETS = {
    "one": (6, [(1, 4)]),
    "fanout3": (6, [(2, 0), (2, 3), (2, 5)]),
    "pairs32": (40, [(i % 8, 8 + i) for i in range(32)]),
}
SHAPES = list(itertools.product((1, 4), (16, 32), ("bf16", "fp8")))  # (nkv, bs, dtype)


def case_id(nkv, bs, dtype, pairs):
    return f"nkv{nkv}-bs{bs}-{dtype}-{pairs}"


def CASES():
    return [(nkv, bs, dt, name) for (nkv, bs, dt), name in itertools.product(SHAPES, PAIR_SETS)]


def _raw(t: torch.Tensor) -> torch.Tensor:
    """The cache's words as integers: int16 per bf16 element, uint8 per FP8 byte."""
    return t.view(torch.uint8) if t.dtype == FP8 else t.view(torch.int16)


def make_caches(num_blocks: int, nkv: int, bs: int, dtype: str, pairs, device="cpu"):
    """-> [(k, v)] x LAYERS: word ``o`` of block ``b`` of tensor ``t`` holds a code of (t, b, o) that
    differs between neighbouring tensors, blocks and offsets and is never the NaN fill; the dst blocks
    of ``pairs`` hold the fill."""
    fp8 = dtype == "fp8"
    per_block = nkv * bs * HEAD_DIM
    o = np.arange(per_block, dtype=np.int64)[None, :]
    b = np.arange(num_blocks, dtype=np.int64)[:, None]
    out = []
    for layer in range(LAYERS):
        kv = []
        for which in range(2):
            t = 2 * layer + which
            code = o * 7 + b * 131 + t * 1031 + 1
            if fp8:
                words = (code % 251).astype(np.uint8)       # 0..250
                words[words == 0x7F] = 0xFB                 # the fill value never occurs as a code
                x = torch.from_numpy(words)
            else:
                words = (code % 65521).astype(np.uint16)    # < 0xFFFF
                x = torch.from_numpy(words.view(np.int16))
            shape = (num_blocks, nkv, bs, HEAD_DIM) if which == 0 else (num_blocks, nkv, HEAD_DIM, bs)
            x = x.reshape(shape).contiguous()
            for _, d in pairs:
                x[d] = 0x7F if fp8 else -1              # 0x7F / 0xFFFF: NaN in e4m3 / bf16
            x = x.to(device)
            kv.append(x.view(FP8) if fp8 else x.view(torch.bfloat16))
        out.append(tuple(kv))
    return out


def snapshot(caches):
    return [tuple(_raw(t).cpu().clone() for t in kv) for kv in caches]


def check(before, caches, pairs) -> None:
    """AssertionError unless ``caches`` is ``before`` (a :func:`snapshot`) with every dst block replaced
    by its src block, in all 2 x LAYERS tensors, and nothing else changed."""
    dst_of = {d: s for s, d in pairs}
    for layer, (kv0, kv1) in enumerate(zip(before, caches)):
        for which, (old, new) in enumerate(zip(kv0, kv1)):
            new = _raw(new).cpu()
            assert new.shape == old.shape
            for blk in range(old.shape[0]):
                want = old[dst_of[blk]] if blk in dst_of else old[blk]
                if not torch.equal(new[blk], want):
                    bad = int((new[blk] != want).sum())
                    what = f"copy of block {dst_of[blk]}" if blk in dst_of else "untouched"
                    raise AssertionError(f"layer {layer} {'KV'[which]} block {blk} ({what}): {bad} of "
                                         f"{want.numel()} words differ")


# ---------------------------------------------------------------------------------------- mutants
def _copy(t, s, d, frac=1.0):
    raw = t.view(torch.uint8)
    flat_s, flat_d = raw[s].reshape(-1), raw[d].reshape(-1)
    n = int(flat_s.numel() * frac)
    flat_d[:n] = flat_s[:n]


def mutant_copy(caches, pairs, mutant: str) -> None:
    """Wrong copies the checker must reject."""
    nb = caches[0][0].shape[0]
    for layer, (k, v) in enumerate(caches):
        if mutant == "layer0_only" and layer != 0:
            continue
        for which, t in enumerate((k, v)):
            if mutant == "k_only" and which == 1:
                continue
            for s, d in pairs:
                if mutant == "swapped":
                    _copy(t, d, s)
                elif mutant == "dst_plus_1":
                    _copy(t, s, (d + 1) % nb)
                else:
                    _copy(t, s, d, 0.5 if mutant == "first_half" else 1.0)


MUTANTS = ("k_only", "layer0_only", "first_half", "swapped", "dst_plus_1")

"""The KV block copy's checker (tests/kv_fork_cases.py) on the CPU: it accepts ops/reference.py
kv_copy_blocks on every case and rejects five wrong copies, so the GPU test that runs the same cases
through pk_kv_copy_blocks can fail for each of them."""
import pytest
import torch

from polykey_service_amd.ops import kv as kv_ops
from polykey_service_amd.ops import reference
from tests import kv_fork_cases as C


@pytest.mark.parametrize("nkv,bs,dtype,pairs", C.CASES())
def test_checker_accepts_the_reference(nkv, bs, dtype, pairs):
    nb, pr = C.PAIR_SETS[pairs]
    caches = C.make_caches(nb, nkv, bs, dtype, pr)
    before = C.snapshot(caches)
    reference.kv_copy_blocks(caches, pr)
    C.check(before, caches, pr)


@pytest.mark.parametrize("mutant", C.MUTANTS)
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_checker_rejects_mutants(mutant, dtype):
    nb, pr = C.PAIR_SETS["fanout3"]
    caches = C.make_caches(nb, 4, 32, dtype, pr)
    before = C.snapshot(caches)
    C.mutant_copy(caches, pr, mutant)
    with pytest.raises(AssertionError):
        C.check(before, caches, pr)


def test_checker_rejects_a_missing_copy_and_a_stray_write():
    nb, pr = C.PAIR_SETS["one"]
    caches = C.make_caches(nb, 1, 16, "bf16", pr)
    before = C.snapshot(caches)
    with pytest.raises(AssertionError):
        C.check(before, caches, pr)  # nothing copied: dst still holds the NaN fill
    reference.kv_copy_blocks(caches, pr)
    caches[1][1].view(torch.int16)[0, 0, 0, 0] ^= 1  # one bit of an unrelated block
    with pytest.raises(AssertionError):
        C.check(before, caches, pr)


def test_reference_refusals_leave_the_caches_unchanged():
    caches = C.make_caches(6, 1, 16, "bf16", [])
    before = C.snapshot(caches)
    bad = [[(0, 0)], [(0, 6)], [(-1, 2)], [(0, 2), (1, 2)], [(0, 1), (1, 2)], [(i % 2, 2) for i in range(33)]]
    for pairs in bad:
        with pytest.raises(ValueError):
            reference.kv_copy_blocks(caches, pairs)
        assert kv_ops.try_copy_blocks(caches, pairs) == -1
        C.check(before, caches, [])
    assert kv_ops.try_copy_blocks(caches, []) == 0
    C.check(before, caches, [])

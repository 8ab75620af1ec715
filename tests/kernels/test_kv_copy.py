"""pk_kv_copy_blocks (csrc/kernels/kv_copy.hip) on the GPU: the cases of tests/kv_fork_cases.py -- one
pair, one src to three dst, 32 pairs; nkv 1 and 4, block size 16 and 32, bf16 and FP8 bytes, K and V
layouts -- held bit for bit by the checker that tests/unit/test_kv_fork_cases.py shows rejects a copy of
K only, of layer 0 only, of half a block, with src and dst swapped, or into dst + 1; and the refusals,
each returning -1 with the caches unchanged."""
import pytest
import torch

from polykey_service_amd.ops import kv as kv_ops
from polykey_service_amd.ops import native
from tests import kv_fork_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nkv,bs,dtype,pairs", C.CASES())
def test_copy_is_exact_and_touches_nothing_else(nkv, bs, dtype, pairs):
    nb, pr = C.PAIR_SETS[pairs]
    caches = C.make_caches(nb, nkv, bs, dtype, pr, device="cuda")
    before = C.snapshot(caches)
    kv_ops.copy_blocks(caches, pr)
    torch.cuda.synchronize()
    C.check(before, caches, pr)


def test_refusals_return_minus_one_and_write_nothing():
    caches = C.make_caches(40, 1, 16, "bf16", [], device="cuda")
    before = C.snapshot(caches)
    table = kv_ops.pointer_table(caches)
    bad = {
        "src == dst": [(3, 3)],
        "dst out of range": [(0, 40)],
        "src negative": [(-1, 2)],
        "duplicate dst": [(0, 2), (1, 2)],
        "dst is also a src": [(0, 1), (1, 2)],
        "33 pairs": [(i % 4, 4 + i) for i in range(33)],
    }
    for what, pairs in bad.items():
        assert kv_ops.try_copy_blocks(caches, pairs, table) == -1, what
    flat = (native.ctypes.c_int * 2)(0, 1)
    rc = native.lib().pk_kv_copy_blocks(table.data_ptr(), 4, 24, 40, flat, 1, native.stream_ptr())
    assert rc == -1, "block_bytes % 16 != 0"
    assert kv_ops.try_copy_blocks(caches, [], table) == 0  # zero pairs: no launch
    torch.cuda.synchronize()
    C.check(before, caches, [])

"""The multi-LoRA shrink / expand kernels (csrc/kernels/lora.hip) on the GPU: the exact grid cases
through both kernels and both add forms, bit for bit against the float64 reference, in NaN-filled
over-sized buffers; random values within the derived bound; one real-width case; and a captured
graph replayed with the index buffer rewritten between replays.

tests/unit/test_lora_cases.py proves on the CPU that these inputs reject wrong kernels."""
import pytest
import torch

from polykey_service_amd.ops import lora as lora_ops
from polykey_service_amd.ops.gemm import RowScale
from tests import lora_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")
FORMS = ("slab", "bf16")


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bitwise equality of values, NaN == NaN."""
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a.double().cpu(), nan=-12345.0),
                                              torch.nan_to_num(b.double().cpu(), nan=-12345.0))


class Dev:
    """A case's operands on the device, x keeping its row stride and NaN padding."""

    def __init__(self, c: lc.Case):
        buf = torch.full((c.M, c.K + 8), NAN, dtype=BF16)
        buf[:, :c.K] = c.x
        self.x = buf.to(DEV)[:, :c.K]
        self.A, self.B = c.A.to(DEV), c.B.to(DEV)
        self.scale, self.ranks, self.idx = c.scale.to(DEV), c.ranks.to(DEV), c.idx.to(DEV)
        self.rs = None if c.parts is None else RowScale(c.parts.to(DEV), c.eps)
        self.seg = lora_ops.Segments(*c.seg)
        # t scratch: NaN-filled and over-sized; rows without a slot must stay NaN
        self.t = torch.full((c.M * c.R + 64,), NAN, dtype=BF16, device=DEV)


def run(c: lc.Case, d: Dev, form: str, init: torch.Tensor):
    """shrink + expand -> (t [M, R], the whole over-sized output buffer, its [.., M, N] view)."""
    tv = lora_ops.shrink(d.x, d.A, d.idx, d.t, c.seg_r, ranks=d.ranks, rowscale=d.rs)
    if form == "slab":
        buf = torch.full((2 * c.M * c.N + 64,), NAN, dtype=torch.float32, device=DEV)
        view = buf[: 2 * c.M * c.N].view(2, c.M, c.N)
        view.copy_(init)
        target = view[0]
    else:  # bf16 rows with a row stride of N + 8
        buf = torch.full((c.M, c.N + 8), NAN, dtype=BF16, device=DEV)
        view = buf[:, :c.N]
        view.copy_(init)
        target = view
    lora_ops.expand(target, tv, d.B, d.scale, d.idx, d.seg, ranks=d.ranks)
    return tv, buf, view


@pytest.mark.parametrize("r", lc.RANKS)
@pytest.mark.parametrize("K", lc.KS)
@pytest.mark.parametrize("kind", list(lc.KINDS))
def test_grid_cases_bit_for_bit(kind, K, r):
    for c in lc.grid_cases(kind, K, r):
        d = Dev(c)
        want_t = lc.reference_t(c).to(BF16)
        valid = c.idx >= 0
        for form in FORMS:
            init = lc.initial_out(c, form)
            want = lc.reference_out(c, form, init)
            d.t.fill_(NAN)
            tv, buf, view = run(c, d, form, init)
            assert same(tv, want_t), (c.name, "t")                       # rows without a slot: still NaN
            assert bool(d.t[c.M * c.R:].isnan().all()), (c.name, "t past [M, R]")
            assert same(view, want), (c.name, form)
            assert not bool(view.isnan().any()), (c.name, form, "a NaN row of x poisoned the output")
            got = view.cpu()
            if form == "slab":
                assert bool(buf[2 * c.M * c.N:].isnan().all())
                assert torch.equal(got[1], init[1]) and torch.equal(got[0][~valid], init[0][~valid])
            else:
                assert bool(buf[:, c.N:].isnan().all())
                assert torch.equal(got[~valid], init[~valid])
        # x itself is never written
        assert same(d.x, c.x)


def test_ranks_none_reads_the_zero_padding():
    """Without the rank table both kernels walk the whole padded rank: same values."""
    c = lc.grid_case("qkv", 512, 8, 17, rowscale=True)
    d = Dev(c)
    d.ranks = None
    init = lc.initial_out(c, "slab")
    tv, _, view = run(c, d, "slab", init)
    assert same(tv, lc.reference_t(c).to(BF16)) and same(view, lc.reference_out(c, "slab", init))


def test_uniform_tiles_take_the_shared_path():
    """Rows that share one adapter per 8-row tile (a prefill sequence): the tile path of the shrink
    and the register-resident B of the expand, against the same reference."""
    c = lc.grid_case("gate_up", 2048, 16, 65, rowscale=True)
    c.idx = torch.tensor([(1, 1, 0, 2)[(m // 8) % 4] for m in range(c.M)], dtype=torch.int32)
    x = torch.nan_to_num(c.x.float(), nan=1.0).to(BF16)  # every row has a slot now: give it values
    buf = torch.full((c.M, c.K + 8), NAN, dtype=BF16)
    buf[:, :c.K] = x
    c.x = buf[:, :c.K]
    d = Dev(c)
    for form in FORMS:
        init = lc.initial_out(c, form)
        tv, _, view = run(c, d, form, init)
        assert same(tv, lc.reference_t(c).to(BF16)), form
        assert same(view, lc.reference_out(c, form, init)), form


RANDOM = [("qkv", 512, 768, (16, 64, 32), 17), ("gate_up", 2048, 2048, (32, 16, 64), 5),
          ("single", 14336, 4096, (16, 16, 16), 4)]  # the last: one real-width case (8B down projection)


@pytest.mark.parametrize("kind,K,N,ranks,M", RANDOM)
def test_random_values_within_the_derived_bound(kind, K, N, ranks, M):
    """Against the float64 value with no intermediate rounding (lora_cases.true_out), per element:

        |err| <= s sum_j |B[n,j]| (2^-9 |t_j| + K 2^-24 sum_k |x_k A_jk|) + r 2^-24 s sum_j |B[n,j] t_j|

    plus half a bf16 ulp of the result in the bf16 form (lora_cases.error_bound).  The first term is
    the one rounding of t, the second the shrink's fp32 sums in any order, the third the expand's.
    2^-9 |t| is bf16's half ulp at the upper end of a binade (2^-8 at the lower end), so the bound
    holds for sums over many rank columns, not for a single one: the cases use ranks of 16 and
    more, and tests/unit/test_lora_cases.py checks that the reference ops sit inside 0.9 of it."""
    c = lc.random_case(kind, K, N, ranks, M)
    d = Dev(c)
    for form in FORMS:
        init = lc.initial_out(c, form)
        tv, _, view = run(c, d, form, init)
        got = (view[0] if form == "slab" else view).double().cpu()
        err = (got - lc.true_out(c, form, init)).abs()
        bound = lc.error_bound(c, form, init)
        worst = float((err / bound.clamp_min(1e-30)).max())
        print(f"{c.name} {form}: max err / bound = {worst:.3f}, max err = {float(err.max()):.3e}")
        assert (err <= bound).all(), (form, worst)
        assert (err[c.idx < 0] == 0).all()
        assert bool(tv[d.idx < 0].isnan().all())


def test_graph_replay_with_rewritten_indices():
    """Both launches captured once; the index buffer is rewritten between replays (the grid does
    not depend on its contents), including to all -1."""
    c = lc.grid_case("qkv", 512, 16, 17, rowscale=True)
    # every row of x holds values: any row may get a slot in a later replay
    g = torch.Generator().manual_seed(3)
    buf = torch.full((c.M, c.K + 8), NAN, dtype=BF16)
    buf[:, :c.K] = torch.randint(-2, 3, (c.M, c.K), generator=g).to(BF16)
    c.x = buf[:, :c.K]
    d = Dev(c)
    init = lc.initial_out(c, "slab")
    slab = torch.empty((2, c.M, c.N), dtype=torch.float32, device=DEV)
    init_d = init.to(DEV)

    def step():
        slab.copy_(init_d)
        tv = lora_ops.shrink(d.x, d.A, d.idx, d.t, c.seg_r, ranks=d.ranks, rowscale=d.rs)
        lora_ops.expand(slab[0], tv, d.B, d.scale, d.idx, d.seg, ranks=d.ranks)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    patterns = [c.idx.clone(), torch.roll(c.idx, 1), torch.full_like(c.idx, -1), torch.full_like(c.idx, 2),
                torch.tensor([(0, 1, 2)[m % 3] for m in range(c.M)], dtype=torch.int32)]
    for pat in patterns:
        d.idx.copy_(pat.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        c.idx = pat
        assert same(slab, lc.reference_out(c, "slab", init)), pat.tolist()

"""The IPC expert all-to-all (csrc/comm/ep_alltoall.hip) bit for bit against the CPU model of its
contract (tests/ep_cases.py), and the EP MoE layer (parallel/ep.py, _ep_moe_ipc) against float64, with
2, 3, 4 and 8 ranks sharing cuda:0.

Rows are bit patterns (NaN and -0 among them), the "expert" between dispatch and return is an XOR
with a key of (destination rank, expert id), the receive and return regions start out as sentinels,
and every comparison is ``torch.equal`` of integers: see ep_cases for what a returned row proves and
tests/unit/test_ep_cases.py for the wrong kernels these checks reject.  Shapes A, B, C reach the
second trip of the row, column, id-copy and padding loops.

Each worker runs four phases.  1: stepped -- sentinels, barrier, dispatch, check at once (the kernel's
completion is the promise that every peer's rows have landed), expert, return, check.  2: the same
calls back to back with no host synchronisation and no refill, every call's regions copied to a log by
the stream, rank r putting r large copies between its calls so the ranks drift apart.  3: dispatch,
expert and return captured once as a graph and replayed with other send data, a zero-row call and a
small call after a full one among them.  4 (8 % world == 0): ``ep.ep_moe`` on integer operands with
NaN in unused experts, in the receive regions and in ret_x, within the 4.25 u B of moe_cases.check_moe
of the single-rank float64 layer; deferred combine and a repeat are bit-equal.  Every wait is bounded
by the all-to-all's own timeout (20 s), and the parent ends stragglers.

Records on the MI355X.  Phase 4 prints ``ratio ep_moe <world> <largest error / (u B)>`` (run with
-s); measured 0.5253 (2 ranks), 0.4463 (4), 0.4967 (8), the same in every run, against the bound of
4.25.  No kernel bug was found; two
deliberately wrong builds of the kernels (the padding loop's second trip dropped; the return ignoring
the offsets of remote sources) failed at ('recv_e', source 0, row 16384, 7 instead of -1) and at
('ret_x', row 20, sent to rank 1).  Time per test: 3.3 to 3.6 s at 2, 3 and 4 ranks, 5.5 s at 8, of
which the four phases take 1.0 to 1.4 s and the rest is starting and ending the processes.
"""
import os
import queue
import socket
import time

import pytest
import torch
import torch.multiprocessing as mp

from tests import ep_cases as ec
from tests import moe_cases as mc

pytestmark = pytest.mark.gpu

BF, I16, I32 = torch.bfloat16, torch.int16, torch.int32
GRAPH_CALLS = (1, 2, 4, 5)  # full, small after full, odd ranks idle, even ranks idle
DRIFT_BYTES = 64 << 20


def _port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fill(a2a):
    a2a.recv_x.view(I16).fill_(ec.SENT_X)
    a2a.recv_e.fill_(ec.SENT_E)
    a2a.ret_x.view(I16).fill_(ec.SENT_X)


def _expert(a2a, rank):
    return ec.expert_bits(rank, a2a.recv_x.view(I16), a2a.recv_e).view(BF)


def _stepped(a2a, rank, world, shape, sends, dsends, barrier):
    C, H = ec.SHAPES[shape]
    sent_x = torch.full((world * C, H), ec.SENT_X, dtype=I16)
    sent_r = torch.full((C, H), ec.SENT_X, dtype=I16)
    for call in range(len(ec.CALLS)):
        _fill(a2a)
        torch.cuda.synchronize()
        barrier()
        a2a.dispatch(*dsends[shape, call])
        torch.cuda.synchronize()
        ec.check_dispatch(rank, world, C, a2a.recv_x.view(I16).cpu(), a2a.recv_e.cpu(), sends[shape, call], sent_x)
        y = _expert(a2a, rank)
        back = a2a.return_(y)
        torch.cuda.synchronize()
        assert back.data_ptr() == a2a.ret_x.data_ptr()
        ec.check_return(rank, world, C, back.view(I16).cpu(), sends[shape, call], sent_r)
    assert a2a.error() == 0, ("stepped", shape)


def _back_to_back(a2a, rank, world, shape, sends, dsends, barrier, dev):
    C, H = ec.SHAPES[shape]
    calls = len(ec.CALLS)
    log_x = torch.empty((calls, world * C, H), dtype=I16, device=dev)
    log_e = torch.empty((calls, world * C), dtype=I32, device=dev)
    log_r = torch.empty((calls, C, H), dtype=I16, device=dev)
    drift = torch.empty((2, DRIFT_BYTES), dtype=torch.uint8, device=dev)
    _fill(a2a)
    torch.cuda.synchronize()
    barrier()
    for call in range(calls):
        a2a.dispatch(*dsends[shape, call])
        log_x[call].copy_(a2a.recv_x.view(I16))
        log_e[call].copy_(a2a.recv_e)
        a2a.return_(_expert(a2a, rank))
        log_r[call].copy_(a2a.ret_x.view(I16))
        for _ in range(rank):
            drift[1].copy_(drift[0])
    torch.cuda.synchronize()
    assert a2a.error() == 0, ("back to back", shape)
    log_x, log_e, log_r = log_x.cpu(), log_e.cpu(), log_r.cpu()
    want_x = torch.full((world * C, H), ec.SENT_X, dtype=I16)
    want_r = torch.full((C, H), ec.SENT_X, dtype=I16)
    for call in range(calls):
        try:
            want_x, _ = ec.check_dispatch(rank, world, C, log_x[call], log_e[call], sends[shape, call], want_x)
            want_r = ec.check_return(rank, world, C, log_r[call], sends[shape, call], want_r)
        except AssertionError as e:
            raise AssertionError(("back to back", shape, call, *e.args)) from None


def _graph(a2a, rank, world, shape, sends, dsends, barrier, dev):
    C, H = ec.SHAPES[shape]
    gx = torch.zeros((C, H), dtype=BF, device=dev)
    ge = torch.zeros((C,), dtype=I32, device=dev)
    goff = torch.zeros((world + 1,), dtype=I32, device=dev)
    log_x = torch.zeros((world * C, H), dtype=I16, device=dev)
    log_e = torch.zeros((world * C,), dtype=I32, device=dev)
    log_r = torch.zeros((C, H), dtype=I16, device=dev)

    def step():
        a2a.dispatch(gx, ge, goff)
        log_x.copy_(a2a.recv_x.view(I16))
        log_e.copy_(a2a.recv_e)
        a2a.return_(_expert(a2a, rank))
        log_r.copy_(a2a.ret_x.view(I16))

    _fill(a2a)
    torch.cuda.synchronize()
    barrier()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # a zero-row call of every rank: recv_x and ret_x stay sentinels
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    want_x = torch.full((world * C, H), ec.SENT_X, dtype=I16)
    want_r = torch.full((C, H), ec.SENT_X, dtype=I16)
    for call in GRAPH_CALLS:
        sx, se, so = dsends[shape, call]
        n = sx.shape[0]
        gx[:n].copy_(sx)
        ge[:n].copy_(se)
        goff.copy_(so)
        graph.replay()
        torch.cuda.synchronize()
        try:
            want_x, _ = ec.check_dispatch(rank, world, C, log_x.cpu(), log_e.cpu(), sends[shape, call], want_x)
            want_r = ec.check_return(rank, world, C, log_r.cpu(), sends[shape, call], want_r)
        except AssertionError as e:
            raise AssertionError(("graph", shape, call, *e.args)) from None
    assert a2a.error() == 0, ("graph", shape)
    assert any(sends[shape, c][rank].x.shape[0] == 0 for c in GRAPH_CALLS), "no zero-row replay for this rank"


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(I16), b.view(I16))


def _moe_layer(st, rank, world, barrier, dev):
    """ep.ep_moe over the IPC regions against the float64 layer over all E experts -> largest ratio."""
    from polykey_service_amd.ops import moe as moe_ops
    from polykey_service_amd.parallel import ep, ep_ipc
    E, k, H = ec.MOE_E, ec.MOE_K, ec.MOE_H
    per = E // world
    st.ep_a2a = ep_ipc.maybe_create(st, ec.MOE_C, H)
    assert st.ep_a2a is not None and st.ep_a2a_prefill is None, "the IPC expert all-to-all was not created"
    a2a = st.ep_a2a
    worst = 0.0
    for rnd, tokens in enumerate(ec.MOE_TOKENS[world]):
        xs, router, w13, w2 = ec.moe_operands(world, rnd)
        T = tokens[rank]
        assert xs[rank].shape[0] == T
        st.ep_step_rows = max(tokens)
        x, rt = xs[rank].to(dev), router.to(dev)
        local = slice(rank * per, (rank + 1) * per)
        w13_l, w2_l = w13[local].contiguous().to(dev), w2[local].contiguous().to(dev)
        a2a.recv_x.fill_(float("nan"))
        a2a.ret_x.fill_(float("nan"))
        torch.cuda.synchronize()
        barrier()
        out = ep.ep_moe(x, rt, w13_l, w2_l, k)
        torch.cuda.synchronize()
        out = out.clone()
        again = ep.ep_moe(x, rt, w13_l, w2_l, k)
        torch.cuda.synchronize()
        again = again.clone()
        pend = ep.ep_moe(x, rt, w13_l, w2_l, k, defer_combine=True)
        assert isinstance(pend, moe_ops.PendingCombine) == (T > 0)
        deferred = pend.combine() if T > 0 else pend
        torch.cuda.synchronize()
        assert out.shape == (T, H) and out.dtype == BF, (tuple(out.shape), out.dtype)
        assert _same_bits(out, again), "a second call with the same inputs differs"
        assert _same_bits(out, deferred), "deferred combine differs from the direct result"
        # the layer went through the IPC regions: they hold exactly the rows routed to this rank's
        # experts, ids local and the rest -1, and the padding rows still hold the poison
        routed = [e for r, n in enumerate(tokens) for pair in ec.moe_routes(r, n) for e in pair]
        mine = sum(rank * per <= e < (rank + 1) * per for e in routed)
        ids = a2a.recv_e.cpu()
        assert int((ids >= 0).sum()) == mine and bool(((ids >= -1) & (ids < per)).all()), (mine, ids.unique().tolist())
        assert bool(torch.isnan(a2a.recv_x.float()).all(-1).cpu()[ids < 0].all()), "a padding row was written"
        if T > 0:
            ref, B = mc.moe64(xs[rank], router, w13, w2, k, 0, E)
            worst = max(worst, mc.check_moe(out.cpu(), ref, B))
    assert a2a.error() == 0, "moe"
    return worst


def _worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK="0", LOCAL_WORLD_SIZE=str(world), POLYKEY_CUSTOM_AR_TIMEOUT_S="20")
        torch.set_num_threads(2)
        import torch.distributed as dist

        from polykey_service_amd.parallel.ep_ipc import EpAllToAll, EpAllToAllError
        from polykey_service_amd.parallel.state import destroy_parallel, init_parallel
        times = {}
        t0 = time.monotonic()
        st = init_parallel(tp=1, ep=world, device="cuda", backend="gloo", timeout_s=120.0)
        dev = st.device

        def barrier():
            dist.barrier(group=st.ep_cpu_group)

        ctx = {shape: EpAllToAll(st.ep_cpu_group, rank, world, dev, C, H, timeout_s=20.0)
               for shape, (C, H) in ec.SHAPES.items()}
        sends = {(shape, call): ec.make_sends(world, shape, call)
                 for shape in ec.SHAPES for call in range(len(ec.CALLS))}
        dsends = {kc: (v[rank].x.to(dev).view(BF), v[rank].e.to(dev), v[rank].off.to(dev)) for kc, v in sends.items()}
        torch.cuda.synchronize()
        times["setup"] = time.monotonic() - t0
        t0 = time.monotonic()
        for shape in ec.SHAPES:
            _stepped(ctx[shape], rank, world, shape, sends, dsends, barrier)
        times["stepped"] = time.monotonic() - t0
        t0 = time.monotonic()
        for shape in ("A", "B"):
            _back_to_back(ctx[shape], rank, world, shape, sends, dsends, barrier, dev)
        times["back_to_back"] = time.monotonic() - t0
        t0 = time.monotonic()
        _graph(ctx["B"], rank, world, "B", sends, dsends, barrier, dev)
        times["graph"] = time.monotonic() - t0
        t0 = time.monotonic()
        ratio = _moe_layer(st, rank, world, barrier, dev) if 8 % world == 0 else None
        times["moe"] = time.monotonic() - t0
        torch.cuda.synchronize()
        for a2a in ctx.values():
            assert a2a.error() == 0
            a2a.check()
        barrier()
        # last, with no GPU call following: the host-side failure word
        a2a = ctx["A"]
        a2a.fail()
        assert a2a.error() == 1
        try:
            a2a.check()
            raise AssertionError("check() did not raise")
        except EpAllToAllError:
            pass
        barrier()
        for a2a in ctx.values():
            a2a.close()
        barrier()
        destroy_parallel()
        q.put((rank, ("ok", ratio, times)))
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put((rank, (repr(e) + " " + traceback.format_exc()[-2000:], None, None)))


@pytest.mark.parametrize("world", ec.WORLDS)
def test_expert_all_to_all_exact(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, deadline = {}, time.monotonic() + 240
    try:
        while len(res) < world:
            r, m = q.get(timeout=max(1.0, deadline - time.monotonic()))
            res[r] = m
    except queue.Empty:
        pass
    for p in procs:
        p.join(timeout=30)
    for p in procs:
        if p.is_alive():
            p.kill()
            p.join()
    assert {r: m[0] for r, m in res.items()} == {r: "ok" for r in range(world)}, res
    if 8 % world == 0:
        print(f"ratio ep_moe {world} {max(m[1] for m in res.values()):.4g}")
    print(f"phases ep_alltoall {world} " + " ".join(f"{k}={max(m[2][k] for m in res.values()):.2f}s"
                                                    for k in res[0][2]))

"""The in-process "threads" transport in its barrier mode (kfx_comm_create_threads, csrc/slab_comm.hip), driven through the function
pointers of its kfx_comm tables from three host threads that share the GPU: every collective against the same operation in numpy,
bit for bit; a collective that fails on one rank -- or on all -- returns the SAME status on every rank and leaves the group usable
(the errors live in two sets, by the parity of the collective's sequence number); kfx_comm::dup.

The errors provoked here are argument errors, refused on the host before any device work.  A rank thread that does not come back
within 20 s is a failed assertion (the threads are daemons: a barrier bug must not hang the test run)."""
import ctypes as C
import threading

import numpy as np
import pytest

import kfx_testlib as T  # noqa: F401  (puts the repository on sys.path)

pytestmark = pytest.mark.gpu

W, N = 3, 256                     # ranks, elements per rank and buffer
MIN_I64, SUM_F32, SUM_I32 = 0, 1, 2   # KFX_COMM_* (include/kfx_slab.h)
E_NULL, E_SHAPE, E_RANGE = -1, -2, -4  # KFX_E_* (include/kfx.h)
V = C.c_void_p
hung_ranks = []   # rank threads left inside a collective: their group must not be destroyed under them


def on_ranks(fn, world=W):
    """fn(rank) on `world` daemon threads; their results in rank order."""
    out = [None] * world

    def body(r):
        out[r] = fn(r)
    threads = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(20.0)
    hung = [r for r, t in enumerate(threads) if t.is_alive()]
    hung_ranks.extend(hung)
    assert not hung, "rank threads %s did not return from a collective within 20 s" % hung
    return out


@pytest.fixture
def group():
    import torch
    from kangaroo_amd import slab
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    comms = slab.Comm.threads(W)
    yield comms
    if not hung_ranks:
        torch.cuda.synchronize()
        comms[0].destroy()


def dev(arrays):
    """one device tensor per rank, filled from the numpy arrays"""
    import torch
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    torch.cuda.synchronize()
    return t


def host(tensors):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def all_reduce(comms, bufs, op, count=N):
    return on_ranks(lambda r: comms[r].c.all_reduce(comms[r].ref(), V(bufs[r].data_ptr()) if bufs[r] is not None else None, count, op, None))


def i32_inputs(seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(-2 ** 20, 2 ** 20, N, dtype=np.int32) for _ in range(W)]


def check_good_sum(comms, seed):
    """a correct all-reduce on the group: status 0 on every rank and the sums of numpy"""
    a = i32_inputs(seed)
    bufs = dev(a)
    assert all_reduce(comms, bufs, SUM_I32) == [0] * W
    want = a[0] + a[1] + a[2]
    for got in host(bufs):
        assert np.array_equal(got, want)


def test_all_reduce_gives_numpys_bits(group):
    rng = np.random.default_rng(1)
    # minimum of int64 (the composite's keys)
    a = [rng.integers(-2 ** 62, 2 ** 62, N, dtype=np.int64) for _ in range(W)]
    bufs = dev(a)
    assert all_reduce(group, bufs, MIN_I64) == [0] * W
    want = np.minimum(np.minimum(a[0], a[1]), a[2])
    for got in host(bufs):
        assert np.array_equal(got, want)
    # float sum, in rank order
    a = [rng.standard_normal(N).astype(np.float32) * np.float32(10.0 ** (r - 1)) for r in range(W)]
    bufs = dev(a)
    assert all_reduce(group, bufs, SUM_F32) == [0] * W
    want = (a[0] + a[1]) + a[2]
    assert want.dtype == np.float32
    for got in host(bufs):
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # integer sum of float bit patterns: NaN and -0.0f contributed by exactly one rank survive
    a = i32_inputs(2)
    special = np.array([np.nan, -0.0, np.inf, -np.inf, 1.0, -1.5], np.float32).view(np.int32)
    for k in range(N // 2):
        owner = k % W
        for r in range(W):
            a[r][k] = special[k % len(special)] if r == owner else 0
    bufs = dev(a)
    assert all_reduce(group, bufs, SUM_I32) == [0] * W
    want = a[0] + a[1] + a[2]
    assert np.array_equal(want[:N // 2], np.resize(special, N // 2))
    for got in host(bufs):
        assert np.array_equal(got, want)
    # nothing to reduce: still a collective of all ranks
    assert all_reduce(group, [None] * W, SUM_I32, count=0) == [0] * W


def test_broadcast_from_rank_one(group):
    rng = np.random.default_rng(3)
    a = [rng.standard_normal(N).astype(np.float32) for _ in range(W)]
    bufs = dev(a)
    st = on_ranks(lambda r: group[r].c.broadcast(group[r].ref(), V(bufs[r].data_ptr()), N * 4, 1, None))
    assert st == [0] * W
    for got in host(bufs):
        assert np.array_equal(got.view(np.int32), a[1].view(np.int32))


def test_all_to_all_and_all_gather(group):
    # chunk c of rank r's send buffer holds r * 1000 + c * 10 + a ramp: every (rank, chunk) is distinct
    send = [np.stack([np.float32(r * 1000 + c * 10) + np.arange(N, dtype=np.float32) / np.float32(N) for c in range(W)]) for r in range(W)]
    sbuf = dev(send)
    rbuf = dev([np.zeros((W, N), np.float32) for _ in range(W)])
    st = on_ranks(lambda r: group[r].c.all_to_all(group[r].ref(), V(sbuf[r].data_ptr()), V(rbuf[r].data_ptr()), N * 4, None))
    assert st == [0] * W
    for r, got in enumerate(host(rbuf)):
        want = np.stack([send[src][r] for src in range(W)])   # chunk src <- chunk r of rank src's send
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
    rbuf = dev([np.zeros((W, N), np.float32) for _ in range(W)])
    st = on_ranks(lambda r: group[r].c.all_gather(group[r].ref(), V(sbuf[r].data_ptr()), V(rbuf[r].data_ptr()), N * 4, None))
    assert st == [0] * W
    want = np.stack([send[src][0] for src in range(W)])       # chunk src <- rank src's send (its first N elements)
    for got in host(rbuf):
        assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_exchange_v_with_unequal_legs(group):
    UP, DOWN = 96, 160   # elements a rank sends to its upper / to its lower neighbour; the end ranks' outward legs are empty
    rng = np.random.default_rng(4)
    up = [rng.standard_normal(N).astype(np.float32) for _ in range(W)]
    down = [rng.standard_normal(N).astype(np.float32) for _ in range(W)]
    s_hi, s_lo = dev(up), dev(down)
    r_lo = dev([np.full(N, -7.0, np.float32) for _ in range(W)])
    r_hi = dev([np.full(N, -9.0, np.float32) for _ in range(W)])

    def call(r):
        lo, hi = r > 0, r + 1 < W
        c = group[r].c
        return c.exchange_v(group[r].ref(), V(s_lo[r].data_ptr()) if lo else None, DOWN * 4 if lo else 0, V(r_lo[r].data_ptr()) if lo else None, UP * 4 if lo else 0,
                            V(s_hi[r].data_ptr()) if hi else None, UP * 4 if hi else 0, V(r_hi[r].data_ptr()) if hi else None, DOWN * 4 if hi else 0, None)
    assert on_ranks(call) == [0] * W
    got_lo, got_hi = host(r_lo), host(r_hi)
    for r in range(W):
        want_lo, want_hi = np.full(N, -7.0, np.float32), np.full(N, -9.0, np.float32)
        if r > 0:
            want_lo[:UP] = up[r - 1][:UP]        # what rank - 1 sends upwards
        if r + 1 < W:
            want_hi[:DOWN] = down[r + 1][:DOWN]  # what rank + 1 sends downwards
        assert np.array_equal(got_lo[r].view(np.int32), want_lo.view(np.int32)), r
        assert np.array_equal(got_hi[r].view(np.int32), want_hi.view(np.int32)), r


def test_every_rank_returns_the_same_error_and_the_group_survives(group):
    # one rank's null buffer is every rank's KFX_E_NULL
    bufs = dev(i32_inputs(5))
    assert all_reduce(group, [bufs[0], None, bufs[2]], SUM_I32) == [E_NULL] * W
    check_good_sum(group, 6)
    # an unknown op
    assert all_reduce(group, bufs, 99) == [E_RANGE] * W
    check_good_sum(group, 7)
    # a root outside the group
    st = on_ranks(lambda r: group[r].c.broadcast(group[r].ref(), V(bufs[r].data_ptr()), N * 4, 7, None))
    assert st == [E_RANGE] * W
    check_good_sum(group, 8)
    # two ranks name different byte counts (buffers of W * N elements: every copy made before the disagreement is noticed fits)
    sbuf = dev([np.zeros((W, N), np.float32) for _ in range(W)])
    rbuf = dev([np.zeros((W, N), np.float32) for _ in range(W)])
    nbytes = [N * 4, N * 2, N * 4]
    st = on_ranks(lambda r: group[r].c.all_to_all(group[r].ref(), V(sbuf[r].data_ptr()), V(rbuf[r].data_ptr()), nbytes[r], None))
    assert st == [E_SHAPE] * W
    check_good_sum(group, 9)
    # two failures in a row fill both parity sets; both are clean again afterwards
    assert all_reduce(group, bufs, 99) == [E_RANGE] * W
    assert all_reduce(group, [None, bufs[1], bufs[2]], SUM_I32) == [E_NULL] * W
    check_good_sum(group, 10)
    check_good_sum(group, 11)


def test_dup_gives_a_second_group_over_the_same_threads(group):
    from kangaroo_amd import slab
    copy = (slab.KfxComm * W)()
    assert on_ranks(lambda r: group[r].c.dup(group[r].ref(), C.byref(copy[r]))) == [0] * W
    for r in range(W):
        assert (copy[r].rank, copy[r].world) == (r, W) and copy[r].impl != group[r].c.impl
    send = [np.float32(r + 1) * np.arange(1, N + 1, dtype=np.float32) for r in range(W)]
    sbuf = dev(send)
    want = np.stack(send)
    for table in ([copy[r] for r in range(W)], [group[r].c for r in range(W)]):
        rbuf = dev([np.zeros((W, N), np.float32) for _ in range(W)])
        st = on_ranks(lambda r: table[r].all_gather(C.byref(table[r]), V(sbuf[r].data_ptr()), V(rbuf[r].data_ptr()), N * 4, None))
        assert st == [0] * W
        for got in host(rbuf):
            assert np.array_equal(got.view(np.int32), want.view(np.int32))
    copy[0].destroy(C.byref(copy[0]))   # (rank 0 destroys the copy, as it does the original: the fixture)

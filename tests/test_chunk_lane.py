"""Native chunk lane: ring doorbells, RingHub, ChunkLane, the chunk_done
parser, and the map road end to end with MODAL_AMD_NATIVE_LANE on and off."""

from __future__ import annotations

import os
import select
import subprocess
import sys
import time

import msgpack
import pytest

# the project's own native module: a build that cannot be imported is an
# error here, not a skip
from modal_amd import _core as core

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# helpers: both ends of every ring live in this process


class FakeWorker:
    """Consumer of the scheduler->worker ring, producer of the reverse one."""

    def __init__(self, tmp_path, slot, hub, lane, capacity=1 << 20):
        self.slot = slot
        inp, outp = str(tmp_path / f"in.{slot}"), str(tmp_path / f"out.{slot}")
        self.to_worker_tx = core.ShmRing(inp, capacity, True)
        self.to_worker_rx = core.ShmRing(inp, 0, False)
        self.from_worker_tx = core.ShmRing(outp, capacity, True)
        self.from_worker_rx = core.ShmRing(outp, 0, False)
        hub.add_ring(slot, self.from_worker_rx)
        lane.add_worker(slot, self.to_worker_tx)

    def received(self):
        return [msgpack.unpackb(b, raw=False) for b in self.to_worker_rx.pop_all()]

    def done(self, token, count=64, **extra):
        msg = {
            "t": "chunk_done", "token": token, "call_id": "fc-1", "chunk_id": token[2:],
            "function_id": "fu-1", "count": count, "data": b"ok", "cis": None,
        }
        msg.update(extra)
        assert self.from_worker_tx.push(msgpack.packb(msg, use_bin_type=True))


def frame(token, pad=0):
    return msgpack.packb({"t": "inputs_chunk", "token": token, "pad": b"x" * pad}, use_bin_type=True)


@pytest.fixture()
def rig(tmp_path):
    hub = core.RingHub(str(tmp_path / "hub.bell"), 20)
    lane = core.ChunkLane()
    yield tmp_path, hub, lane
    hub.close()


def test_lane_credit_least_loaded_fifo_and_refill(rig):
    tmp_path, hub, lane = rig
    w0, w1 = FakeWorker(tmp_path, 0, hub, lane), FakeWorker(tmp_path, 1, hub, lane)
    lane.set_cap(0, 128, 1)  # 128 items, i.e. two 64-item chunks per worker
    assert lane.submit(0, "g:a", 64, frame("g:a")) == -1  # nobody eligible yet
    lane.set_eligible(0, 0, True)
    lane.set_eligible(0, 1, True)
    assert lane.kick(0) == [("g:a", 0)]  # ties go to the lowest slot
    # least outstanding items first: w1 (0) before w0 (64), then alternate
    assert [lane.submit(0, f"g:{i}", 64, frame(f"g:{i}")) for i in range(3)] == [1, 0, 1]
    # credit is spent: everything else queues, FIFO, and `front` jumps it
    assert [lane.submit(0, f"g:q{i}", 64, frame(f"g:q{i}")) for i in range(3)] == [-1, -1, -1]
    assert lane.submit(0, "g:front", 64, frame("g:front"), front=True) == -1
    assert lane.queued(0) == 4
    for w in (w0, w1):
        assert lane.outstanding_items(0, w.slot) == 128  # never above the cap
    assert [m["token"] for m in w0.received()] == ["g:a", "g:1"]
    assert [m["token"] for m in w1.received()] == ["g:0", "g:2"]
    # one completion on w1: the refill happens inside drain, front entry first
    w1.done("g:0")
    completions, raw, assignments = lane.drain(hub)
    assert raw == []
    assert completions == [(1, ("g:0", "fc-1", "0", "fu-1", 64, b"ok", None))]
    assert assignments == [("g:front", 1)]
    assert [m["token"] for m in w1.received()] == ["g:front"]  # already on the ring
    assert lane.outstanding_items(0, 1) == 128
    # an unclean chunk_done returns credit too, and stays raw for Python
    w0.done("g:a", failed=True)
    completions, raw, assignments = lane.drain(hub)
    assert completions == [] and assignments == [("g:q0", 0)]
    assert [msgpack.unpackb(b)["failed"] for _s, b in raw] == [True]
    # the rest drain in FIFO order as credit returns
    w0.done("g:1")
    w0.done("g:q0")
    _c, _r, assignments = lane.drain(hub)
    assert assignments == [("g:q1", 0), ("g:q2", 0)]
    assert lane.queued(0) == 0 and lane.outstanding_items(0, 0) == 128


def test_lane_min_chunks_keeps_a_successor_in_flight(rig):
    tmp_path, hub, lane = rig
    FakeWorker(tmp_path, 0, hub, lane)
    lane.set_eligible(0, 0, True)
    lane.set_cap(0, 256, 1)
    assert [lane.submit(0, f"g:{i}", 256, frame(f"g:{i}")) for i in range(4)] == [0, -1, -1, -1]
    assert lane.kick(0) == []
    lane.set_cap(0, 256, 2)  # max(item cap, 2 chunks)
    assert lane.kick(0) == [("g:1", 0)]  # one prefetched chunk, never a third
    assert lane.outstanding_items(0, 0) == 512
    # the tail is not prefetched: with a backlog no deeper than the number of
    # eligible workers a chunk waits for a worker under its item cap
    assert lane.complete(0, "g:0") == [("g:2", 0)]
    assert lane.complete(0, "g:1") == []
    assert lane.queued(0) == 1
    assert lane.complete(0, "g:2") == [("g:3", 0)]


def test_lane_remove_worker_and_cancel(rig):
    tmp_path, hub, lane = rig
    FakeWorker(tmp_path, 0, hub, lane)
    FakeWorker(tmp_path, 1, hub, lane)
    lane.set_cap(0, 64, 1)
    lane.set_eligible(0, 0, True)
    lane.set_eligible(0, 1, True)
    placed = {t: lane.submit(0, t, 64, frame(t)) for t in ("g:a", "g:b", "g:c", "g:d", "g:e")}
    assert placed == {"g:a": 0, "g:b": 1, "g:c": -1, "g:d": -1, "g:e": -1}
    assert lane.cancel(["g:d", "g:a", "g:nope"]) == ["g:d"]  # only queued entries drop
    assert lane.queued(0) == 2
    assert lane.remove_worker(1) == ["g:b"]  # exactly what was in flight there
    assert lane.remove_worker(1) == []
    assert lane.inflight(0) == 1
    # the dead worker is no longer eligible: the requeue waits for worker 0
    assert lane.submit(0, "g:b", 64, frame("g:b"), front=True) == -1
    assert lane.complete(0, "g:a") == [("g:b", 0)]
    assert lane.complete(0, "g:b") == [("g:c", 0)]
    assert lane.complete(0, "g:c") == [("g:e", 0)]


def test_ring_wraparound_through_hub(tmp_path):
    """64 KiB ring, 1-4 KiB frames: many wraps, every frame intact, in order."""
    hub = core.RingHub(str(tmp_path / "bell"), 20)
    path = str(tmp_path / "ring")
    tx, rx = core.ShmRing(path, 64 << 10, True), core.ShmRing(path, 0, False)
    hub.add_ring(7, rx)
    sent, got = [], []
    for i in range(600):
        body = bytes([i % 251]) * (1024 + (i * 977) % 3072)
        while not tx.push(body):
            got.extend(hub.drain())
        sent.append((7, body))
    got.extend(hub.drain())
    hub.close()
    assert got == sent
    assert sum(len(b) for _s, b in sent) > 10 * (64 << 10)


def test_full_ring_preserves_lane_order(rig):
    """A worker ring with no room: the lane keeps the queue in order and
    resumes from its head when space returns."""
    tmp_path, hub, lane = rig
    w = FakeWorker(tmp_path, 0, hub, lane, capacity=8 << 10)
    lane.set_cap(0, 1 << 30, 1)
    lane.set_eligible(0, 0, True)
    tokens = [f"g:{i}" for i in range(12)]
    placed = [lane.submit(0, t, 1, frame(t, pad=3000)) for t in tokens]
    assert placed[:2] == [0, 0] and placed[2:] == [-1] * 10  # 8 KiB holds two
    # a small frame would fit, but must not overtake the queue
    assert lane.submit(0, "g:small", 1, frame("g:small")) == -1
    seen = [m["token"] for m in w.received()]
    while lane.queued(0):
        assert lane.kick(0)
        seen += [m["token"] for m in w.received()]
    assert seen == tokens + ["g:small"]


def test_connection_waits_for_ring_space_in_order(tmp_path):
    """Connection.send on a lane connection with a full ring: senders wait
    for space and their frames arrive in send order."""
    import asyncio

    from modal_amd.scheduler.transport import Connection

    async def handler(_msg):
        pass

    async def run():
        conn = Connection(None, None, handler)
        path = str(tmp_path / "ring")
        conn.ring_out = core.ShmRing(path, 8 << 10, True)
        conn.ring_in = core.ShmRing(str(tmp_path / "unused"), 8 << 10, True)
        conn._lane = True
        rx = core.ShmRing(path, 0, False)
        sends = [
            asyncio.ensure_future(conn.send({"i": i, "pad": b"p" * (3000 if i % 3 else 10)}))
            for i in range(30)
        ]
        got = []
        while len(got) < 30:
            await asyncio.sleep(0.002)
            got += [msgpack.unpackb(b)["i"] for b in rx.pop_all(1)]
        await asyncio.gather(*sends)
        # senders that arrive while others wait, one per loop turn, so some
        # run between a waiter's release of the lock and the next one's wake-up
        late = []
        got_late = []
        for i in range(40):
            late.append(asyncio.ensure_future(conn.send({"i": i, "pad": b"p" * 2500})))
            await asyncio.sleep(0)
            if i % 3 == 2:
                got_late += [msgpack.unpackb(b)["i"] for b in rx.pop_all(1)]
        while len(got_late) < 40:
            await asyncio.sleep(0.001)
            got_late += [msgpack.unpackb(b)["i"] for b in rx.pop_all(1)]
        await asyncio.gather(*late)
        assert got_late == list(range(40))
        assert conn._lane_waiting == 0
        with pytest.raises(RuntimeError):
            await conn.send({"pad": b"p" * (9 << 10)})  # can never fit: not sent
        return got

    assert asyncio.run(run()) == list(range(30))


CHILD = """
import sys, time
sys.path.insert(0, {repo!r})
from modal_amd import _core as core
ring = core.ShmRing({ring!r}, 0, False)
ring.set_shared_bell(core.BellFile({bell!r}, False))
time.sleep(0.2)   # the parent's hub is asleep on the bell by now
t_push = time.time()
assert ring.push(b"from-child")
open({stamp!r}, "w").write(repr(t_push))
"""


def test_doorbell_wakes_hub_across_processes(tmp_path):
    ring_path, bell_path = str(tmp_path / "ring"), str(tmp_path / "bell")
    rx = core.ShmRing(ring_path, 1 << 16, True)
    # no consumer waiting: pushes make no wake syscall
    tx = core.ShmRing(ring_path, 0, False)
    for _ in range(10):
        assert tx.push(b"quiet")
    assert tx.bell_wakes() == 0
    assert len(rx.pop_all()) == 10
    hub = core.RingHub(bell_path, 20)
    try:
        hub.add_ring(0, rx)
        assert hub.stats()["producer_wakes"] == 0
        stamp = str(tmp_path / "t_push")
        child = subprocess.Popen(
            [sys.executable, "-c",
             CHILD.format(repo=REPO, ring=ring_path, bell=bell_path, stamp=stamp)]
        )
        ready, _, _ = select.select([hub.fd()], [], [], 30.0)  # covers interpreter start
        t_signal = time.time()
        assert child.wait(timeout=30) == 0
        t_push = float(open(stamp).read())  # same machine, same clock
        assert ready, "the hub never signalled"
        assert t_signal - t_push < 1.0, f"signal {t_signal - t_push:.3f} s after the push"
        assert hub.drain() == [(0, b"from-child")]
        stats = hub.stats()
        assert stats["notifies"] >= 1
        assert stats["producer_wakes"] >= 1  # the flag was set: one FUTEX_WAKE
        # the eventfd is level-cleared by drain
        assert select.select([hub.fd()], [], [], 0.05)[0] == []
    finally:
        hub.close()


def test_doorbell_latency_within_a_second(tmp_path):
    """In-process producer: the hub signals well within 1 s of the push
    (its futex wait is woken, not timed out)."""
    hub = core.RingHub(str(tmp_path / "bell"), 20)
    path = str(tmp_path / "ring")
    tx, rx = core.ShmRing(path, 1 << 16, True), core.ShmRing(path, 0, False)
    tx.set_shared_bell(core.BellFile(str(tmp_path / "bell"), False))
    hub.add_ring(3, rx)
    time.sleep(0.05)
    try:
        for i in range(5):
            t0 = time.time()
            assert tx.push(b"%d" % i)
            assert select.select([hub.fd()], [], [], 1.0)[0], "no signal within 1 s"
            assert time.time() - t0 < 1.0
            assert hub.drain() == [(3, b"%d" % i)]
            time.sleep(0.03)  # let the waiter go back to sleep
    finally:
        hub.close()


# ---------------------------------------------------------------------------
# parser

def test_parser_clean_frame_is_a_tuple():
    msg = {
        "t": "chunk_done", "token": "g:ck-1", "call_id": "fc-1", "chunk_id": "ck-1",
        "function_id": "fu-1", "count": 64, "data": b"\x80\x04N.", "cis": [0, 2, 5],
    }
    assert core.parse_chunk_done(msgpack.packb(msg, use_bin_type=True)) == (
        "g:ck-1", "fc-1", "ck-1", "fu-1", 64, b"\x80\x04N.", [0, 2, 5]
    )
    for extra in ({"failed": True}, {"exceptions": {"1": [b"x", "boom"]}}, {"items": {}}):
        assert core.parse_chunk_done(msgpack.packb({**msg, **extra}, use_bin_type=True)) is None
    assert core.parse_chunk_done(msgpack.packb({**msg, "t": "outputs"}, use_bin_type=True)) is None
    assert core.parse_chunk_done(msgpack.packb({**msg, "token": "g:\u00e9"}, use_bin_type=True)) is None


# ---------------------------------------------------------------------------
# end to end, lane on and off


@pytest.fixture(params=["1", "0"], ids=["lane-on", "lane-off"])
def lane_client(request, run_dir, monkeypatch):
    """An in-process scheduler with exactly two CPU workers."""
    monkeypatch.setenv("MODAL_AMD_NATIVE_LANE", request.param)
    monkeypatch.setenv("MODAL_AMD_CHUNK_ITEMS", "64")
    from modal_amd._sync import synchronizer
    from modal_amd.client import _Client
    from modal_amd.scheduler.core import Scheduler

    async def make():
        scheduler = Scheduler(run_dir=run_dir)
        await scheduler.start()
        c = _Client(scheduler, "client")
        _Client.set_default(c)
        for _ in range(2):
            await scheduler.pool.spawn_worker()
        return c

    c = synchronizer.run(make())
    pool = c.svc.pool
    deadline = time.time() + 60
    lane_on = request.param == "1"
    # this thread watches the loop thread's registration: a handle appears in
    # pool.workers a moment before its rings are attached
    while len(pool.workers) < 2 or (
        lane_on and len(pool._lane_workers) < 2
    ):
        assert time.time() < deadline, "workers never connected"
        time.sleep(0.02)
    assert (pool._lane is not None) == lane_on
    assert all((w.hub_slot is not None) == lane_on for w in list(pool.workers.values()))
    c.lane_on = request.param == "1"
    yield c
    synchronizer.run(c.close())
    _Client._singleton = None


def lane_pushed(client) -> int:
    lane = client.svc.pool._lane
    return lane.pushed() if lane is not None else 0


def test_e2e_ordered_batched_map(lane_client):
    import modal_amd as modal

    app = modal.App("lane-batched")

    @app.function()
    @modal.batched(max_batch_size=16, wait_ms=1)
    def triple(xs):
        return [3 * x for x in xs]

    with app.run(client=lane_client):
        assert list(triple.map(range(3000))) == [3 * x for x in range(3000)]
        pool = lane_client.svc.pool
        if lane_client.lane_on:
            assert lane_pushed(lane_client) >= 3000 // 64  # chunks rode the lane
            assert not pool._lane_groups  # nothing left behind
            assert all(not w.inflight for w in pool.workers.values())
            assert all(sum(w.outstanding.values()) == 0 for w in pool.workers.values())


def test_e2e_batched_calls_never_overlap_in_a_worker(lane_client):
    """Several chunks are in flight per worker, yet a batched function
    without @concurrent runs one call at a time in each process (its body
    may use per-process scratch state, as the benchmark's pinned buffer)."""
    import modal_amd as modal

    app = modal.App("lane-batched-serial")

    @app.function()
    @modal.batched(max_batch_size=16, wait_ms=1)
    def guarded(xs):
        import builtins
        import threading
        import time as _t

        lock = builtins.__dict__.setdefault("_lane_test_lock", threading.Lock())
        overlapped = not lock.acquire(blocking=False)
        try:
            _t.sleep(0.002)
            return [(x, overlapped) for x in xs]
        finally:
            if not overlapped:
                lock.release()

    with app.run(client=lane_client):
        out = list(guarded.map(range(1200)))
    assert [x for x, _o in out] == list(range(1200))
    assert not any(o for _x, o in out), "two batched calls ran at once in one worker"


def test_e2e_item_exceptions_and_return_exceptions(lane_client):
    import modal_amd as modal

    app = modal.App("lane-exc")

    @app.function()
    def picky(x):
        if x % 50 == 7:
            raise ValueError(f"bad {x}")
        return x + 1

    with app.run(client=lane_client):
        res = list(picky.map(range(400), return_exceptions=True))
        assert len(res) == 400
        for x, r in enumerate(res):
            if x % 50 == 7:
                assert isinstance(r, Exception) and f"bad {x}" in str(r)
            else:
                assert r == x + 1
        # whichever failing item completes first surfaces
        with pytest.raises(Exception, match=r"bad (\d*[05])?7$"):
            list(picky.map(range(400)))
        assert picky.remote(1) == 2


def test_e2e_early_break_and_cancel(lane_client):
    import modal_amd as modal

    app = modal.App("lane-break")

    @app.function()
    def ident(x):
        return x

    @app.function()
    def slow(x):
        import time as _t

        _t.sleep(0.01)
        return x

    with app.run(client=lane_client):
        seen = 0
        for _v in ident.map(range(10_000), order_outputs=False):
            seen += 1
            if seen >= 50:
                break
        assert seen == 50
        assert ident.remote(7) == 7
        # cancel a spawned map with most chunks still queued
        pool = lane_client.svc.pool
        fc = slow.spawn_map(range(2000))
        deadline = time.time() + 20
        while not any(w.inflight for w in pool.workers.values()):
            assert time.time() < deadline, "spawned map never started"
            time.sleep(0.01)
        fc.cancel()
        if lane_client.lane_on:
            # queued chunks are dropped at once, not run to completion
            assert all(pool._lane.queued(s) == 0 for s in pool._lane_fn_slots.values())
        # the pool recovers: credit is free again for the next map
        assert sorted(ident.map(range(300), order_outputs=False)) == list(range(300))
        if lane_client.lane_on:
            # chunks still in flight at the cancel and at the break finish on
            # their own; nothing may stay pinned by the lane's bookkeeping
            deadline = time.time() + 30
            while pool._lane_groups and time.time() < deadline:
                time.sleep(0.02)
            assert not pool._lane_groups


def test_e2e_worker_sigkill_recovers_every_item(lane_client, run_dir):
    import modal_amd as modal

    app = modal.App("lane-kill")
    marker = os.path.join(run_dir, "killed")

    @app.function()
    def kill_once(x, path):
        import os as _os
        import signal as _signal

        if x == 700 and not _os.path.exists(path):
            open(path, "w").write("x")
            _os.kill(_os.getpid(), _signal.SIGKILL)
        return x

    with app.run(client=lane_client):
        out = sorted(kill_once.map(range(1500), kwargs={"path": marker}, order_outputs=False))
        assert out == list(range(1500))
        assert os.path.exists(marker)


def test_e2e_mixed_per_item_and_chunk_traffic(lane_client):
    """One function serving a chunked map and per-item calls at once."""
    import threading

    import modal_amd as modal

    app = modal.App("lane-mixed")

    @app.function()
    def sq(x):
        return x * x

    results = {}
    with app.run(client=lane_client):
        def mapper():
            results["map"] = list(sq.map(range(2000)))

        t = threading.Thread(target=mapper)
        t.start()
        results["unary"] = [sq.remote(x) for x in range(40)]
        results["spawned"] = [fc.get(timeout=60) for fc in [sq.spawn(x) for x in range(40)]]
        t.join(timeout=120)
        assert not t.is_alive()
    assert results["map"] == [x * x for x in range(2000)]
    assert results["unary"] == results["spawned"] == [x * x for x in range(40)]


@pytest.mark.gpu
def test_gpu_batched_op_through_the_lane(run_dir, monkeypatch):
    """2,000 items of the benchmark's batched op (4096-vector bf16 scale +
    4-element sum) at chunk 64 on two GPU workers equal 4*(x%7+1)."""
    import modal_amd as modal
    from modal_amd._sync import synchronizer
    from modal_amd.client import _Client
    from modal_amd.scheduler.core import Scheduler

    monkeypatch.setenv("MODAL_AMD_CHUNK_ITEMS", "64")

    async def make():
        scheduler = Scheduler(run_dir=run_dir)
        await scheduler.start()
        c = _Client(scheduler, "client")
        _Client.set_default(c)
        for _ in range(2):
            await scheduler.pool.spawn_worker(gpu_index=0)
        return c

    c = synchronizer.run(make())
    try:
        pool = c.svc.pool
        deadline = time.time() + 120
        while len(pool.workers) < 2 or len(pool._lane_workers) < 2:
            assert time.time() < deadline, "GPU workers never connected"
            time.sleep(0.05)
        app = modal.App("lane-gpu")

        @app.function(gpu=1)
        @modal.batched(max_batch_size=64, wait_ms=1)
        def scale_sum(xs):
            import torch

            cache = torch.ones(4096, device="cuda", dtype=torch.bfloat16)
            ks = torch.tensor([float(x % 7 + 1) for x in xs], dtype=torch.float32).to(
                "cuda", dtype=torch.bfloat16
            )
            t = ks[:, None] * cache[None, :]
            return t[:, :4].float().sum(dim=1).cpu().tolist()

        with app.run(client=c):
            out = list(scale_sum.map(range(2000)))
        assert out == [float(4 * (x % 7 + 1)) for x in range(2000)]
        assert pool._lane is not None and pool._lane.pushed() >= 2000 // 64
    finally:
        synchronizer.run(c.close())
        _Client._singleton = None

"""Profile the event loop that carries Function.map on the batched path.

The loop thread runs the client pump, the in-process scheduler and every
worker connection, and it is what bounds map items/s. This script runs the
same shape as bench.py (batched function, chunked map_batches, unordered)
with cProfile switched on INSIDE the loop thread and prints:

  * items/s over the profiled steps (under the profiler, so lower than bench),
  * loop time per chunk (wall time minus time parked in epoll.poll),
  * the epoll.poll share of the loop thread's wall time,
  * loop callbacks (asyncio Handle._run) per chunk,
  * the top entries by cumulative time.

With a GPU the function is bench.py's batched op; without one it is a
batched no-op on CPU workers, which isolates the loop cost.

  python scripts/prof_map_loop.py [--workers 4] [--items 100000] [--chunk 256]
                                  [--steps 3] [--top 25]
  MODAL_AMD_NATIVE_LANE=0 python scripts/prof_map_loop.py   # socket path
"""

from __future__ import annotations

import argparse
import cProfile
import os
import pstats
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def noop_batched(xs: list) -> list:
    return xs


def gpu_batched(xs: list) -> list:
    import torch

    cache = getattr(torch, "_ma_prof_cache", None)
    if cache is None:
        cache = torch.ones(4096, device="cuda", dtype=torch.bfloat16)
        torch._ma_prof_cache = cache
    ks = torch.tensor([float(x % 7 + 1) for x in xs], dtype=torch.float32).to(
        "cuda", dtype=torch.bfloat16
    )
    t = ks[:, None] * cache[None, :]
    return t[:, :4].float().sum(dim=1).cpu().tolist()


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--workers", type=int, default=4)
    parser.add_argument("--items", type=int, default=100_000)
    parser.add_argument("--chunk", type=int, default=256)
    parser.add_argument("--steps", type=int, default=3)
    parser.add_argument("--warmup", type=int, default=1)
    parser.add_argument("--top", type=int, default=25)
    args = parser.parse_args()

    os.environ["MODAL_AMD_CHUNK_ITEMS"] = str(args.chunk)
    run_dir = tempfile.mkdtemp(prefix="modal-amd-prof-")
    os.environ["MODAL_AMD_RUN_DIR"] = run_dir

    import torch

    has_gpu = torch.cuda.is_available()

    import modal_amd as modal
    from modal_amd._sync import synchronizer
    from modal_amd.client import _Client
    from modal_amd.scheduler.core import Scheduler

    async def boot():
        scheduler = Scheduler(run_dir=run_dir)
        await scheduler.start()
        client = _Client(scheduler, "client")
        _Client.set_default(client)
        for _ in range(args.workers):
            await scheduler.pool.spawn_worker(gpu_index=0 if has_gpu else None)
        return scheduler, client

    scheduler, client = synchronizer.run(boot())
    deadline = time.time() + 180
    while len(scheduler.pool.workers) < args.workers:
        if time.time() > deadline:
            raise RuntimeError("workers never connected")
        time.sleep(0.05)

    app = modal.App("prof-map-loop")
    fn = app.function(gpu=1 if has_gpu else None)(
        modal.batched(max_batch_size=64, wait_ms=1)(gpu_batched if has_gpu else noop_batched)
    )

    def step() -> None:
        async def consume() -> None:
            n = 0
            async for batch in fn.map_batches.aio(range(args.items), order_outputs=False):
                n += len(batch)
            assert n == args.items

        synchronizer.run(consume())

    prof = cProfile.Profile()

    async def prof_on() -> None:
        prof.enable()  # cProfile is per thread: this is the loop thread

    async def prof_off() -> None:
        prof.disable()

    with app.run(client=client):
        for _ in range(args.warmup):
            step()
        synchronizer.run(prof_on())
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        wall = time.perf_counter() - t0
        synchronizer.run(prof_off())
        lane = sum(1 for w in scheduler.pool.workers.values() if w.hub_slot is not None)
        ring_sent = sum(w.conn.ring_frames_sent for w in scheduler.pool.workers.values())
        ring_recv = sum(w.conn.ring_frames_received for w in scheduler.pool.workers.values())
        hub_stats = scheduler.pool._hub.stats() if scheduler.pool._hub is not None else None
    synchronizer.run(client.close())

    stats = pstats.Stats(prof)
    poll_s = 0.0
    callbacks = 0
    for (filename, _line, name), (_cc, ncalls, tottime, _cum, _callers) in stats.stats.items():
        if name == "<method 'poll' of 'select.epoll' objects>":
            poll_s += tottime
        elif name == "_run" and filename.endswith("events.py"):
            callbacks += ncalls
    chunks = args.steps * ((args.items + args.chunk - 1) // args.chunk)
    total_items = args.steps * args.items
    print(
        f"device={'gpu' if has_gpu else 'cpu'} workers={args.workers} "
        f"lane_workers={lane} chunk={args.chunk} items/step={args.items} steps={args.steps}"
    )
    print(f"items/s under profiler: {total_items / wall:,.0f}")
    print(f"loop time per chunk:    {(wall - poll_s) / chunks * 1e6:.1f} us  ({chunks} chunks)")
    print(f"epoll.poll share:       {100.0 * poll_s / wall:.1f}%  ({poll_s * 1e3:.0f} of {wall * 1e3:.0f} ms)")
    print(f"loop callbacks/chunk:   {callbacks / chunks:.2f}")
    print(f"ring frames sent/received by the scheduler: {ring_sent}/{ring_recv}")
    if hub_stats is not None:
        print(f"hub: {hub_stats}")
    stats.sort_stats("cumulative").print_stats(args.top)


if __name__ == "__main__":
    main()

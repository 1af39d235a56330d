"""Worker-plane transport: length-prefixed msgpack frames over Unix sockets.

This replaces the reference's gRPC/HTTP2 control plane
(/root/reference/py/modal/_utils/grpc_utils.py) with a single-node design:
4-byte little-endian length + msgpack body, no TLS, no HTTP framing. Payload
bytes ride inside msgpack bin values (zero re-encoding). An RPC layer on top
gives workers access to scheduler services (queues, dicts, volumes, blobs)
with the same semantics user code sees in the client process.
"""

from __future__ import annotations

import asyncio
import os
import itertools
import struct
from collections import deque
from typing import Any, Awaitable, Callable, Optional

import msgpack

_LEN = struct.Struct("<I")

MAX_FRAME = 1 << 31  # 2 GiB guard

# frames above this ride the shared-memory ring (modal_amd._core.ShmRing)
# with only a doorbell on the socket; below it the socket round-trip is
# lower-latency than a ring poll
RING_MIN_FRAME = int(os.environ.get("MODAL_AMD_RING_MIN", 32 * 1024))
RING_CAPACITY = 64 << 20  # 64 MiB per direction per worker

try:
    from .. import _core  # C++ native core (built in-tree)
except ImportError:  # pragma: no cover - source-only checkout
    _core = None


def native_lane_enabled() -> bool:
    """MODAL_AMD_NATIVE_LANE=0 keeps every frame below RING_MIN_FRAME on the
    socket, as before the lane existed (docs/TUNING.md)."""
    if _core is None or not hasattr(_core, "RingHub"):
        return False
    return os.environ.get("MODAL_AMD_NATIVE_LANE", "1").lower() not in ("0", "false", "no")


_RPC_REPLY_KINDS = ("rpc_r", "rpc_e")


def pack(msg: dict) -> bytes:
    body = msgpack.packb(msg, use_bin_type=True)
    return _LEN.pack(len(body)) + body


async def read_frame(reader: asyncio.StreamReader) -> Optional[dict]:
    try:
        header = await reader.readexactly(4)
    except (asyncio.IncompleteReadError, ConnectionResetError):
        return None
    (length,) = _LEN.unpack(header)
    if length > MAX_FRAME:
        raise ValueError(f"Frame too large: {length}")
    try:
        body = await reader.readexactly(length)
    except (asyncio.IncompleteReadError, ConnectionResetError):
        return None
    return msgpack.unpackb(body, raw=False, strict_map_key=False)


class Connection:
    """One framed connection with an RPC request/response layer.

    Both directions can send one-way messages (dispatched to ``handler``) and
    RPCs (``call``), multiplexed by message type:
      {"t": <kind>, ...}                     one-way
      {"t": "rpc", "i": id, "m": method, "p": params}  request
      {"t": "rpc_r", "i": id, "r": result} / {"t": "rpc_e", "i": id, "e": msg}
    """

    def __init__(
        self,
        reader: asyncio.StreamReader,
        writer: asyncio.StreamWriter,
        handler: Callable[[dict], Awaitable[None]],
        rpc_target: Optional[Any] = None,
    ):
        self.reader = reader
        self.writer = writer
        self.handler = handler
        self.rpc_target = rpc_target  # object whose async methods serve inbound RPCs
        self._rpc_seq = itertools.count(1)
        self._pending: dict[int, asyncio.Future] = {}
        self._send_lock = asyncio.Lock()
        self._closed = asyncio.Event()
        self._reader_task: Optional[asyncio.Task] = None
        self._loop: Optional[asyncio.AbstractEventLoop] = None
        # shm ring pair: our producer side and our consumer side
        self.ring_out: Any = None
        self.ring_in: Any = None
        self.ring_frames_sent = 0
        self.ring_frames_received = 0
        # native lane: once enabled, EVERY outbound frame rides ring_out and
        # the peer's RingHub is woken through the ring's doorbell
        self._lane = False
        self._own_hub: Any = None  # a worker end owns a one-ring hub
        # handles the hot one-way kinds without a coroutine; returns True
        # when it consumed the frame
        self.sync_handler: Optional[Callable[[dict], bool]] = None
        # ring frames whose handler may suspend run here, one after another
        self._inbox: deque = deque()
        self._lane_waiting = 0  # senders waiting for ring space (or queued behind one)
        self._inbox_task: Optional[asyncio.Task] = None

    def attach_rings(self, out_path: Optional[str], in_path: Optional[str], create: bool) -> bool:
        """Attach the shared-memory bulk channel (both sides call this)."""
        if _core is None or not out_path or not in_path:
            return False
        try:
            self.ring_out = _core.ShmRing(out_path, RING_CAPACITY, create)
            self.ring_in = _core.ShmRing(in_path, RING_CAPACITY, create)
            return True
        except Exception:
            self.ring_out = None
            self.ring_in = None
            return False

    def enable_lane(self, shared_bell: Optional[str] = None, own_hub: bool = False) -> bool:
        """Route every outbound frame through ring_out from now on.

        ``shared_bell``: bell file of the peer's hub, bumped after each push
        (worker end). ``own_hub``: start a one-ring hub on ring_in and read
        it from this loop (worker end); the scheduler end registers ring_in
        with the pool's hub instead and feeds ``on_ring_frame``.

        Whether the lane is used is the scheduler's decision
        (``native_lane_enabled`` when it starts its hub); a worker end follows
        the ``hello_ack`` and does not consult its own environment. False
        means this end cannot serve the lane: the caller must not go on as
        if it could, since the peer already puts every frame on the ring."""
        if _core is None or self.ring_out is None or self.ring_in is None:
            return False
        try:
            if shared_bell:
                self.ring_out.set_shared_bell(_core.BellFile(shared_bell, False))
            if own_hub:
                hub = _core.RingHub("", 20)
                hub.add_ring(0, self.ring_in)
                asyncio.get_running_loop().add_reader(hub.fd(), self._on_own_hub_ready)
                self._own_hub = hub
        except Exception:
            self._drop_own_hub()
            return False
        self._lane = True
        return True

    def _on_own_hub_ready(self) -> None:
        hub = self._own_hub
        if hub is None:
            return
        for _slot, body in hub.drain():
            self.on_ring_frame(body)

    def _drop_own_hub(self) -> None:
        hub, self._own_hub = self._own_hub, None
        if hub is not None:
            try:
                asyncio.get_running_loop().remove_reader(hub.fd())
            except Exception:
                pass
            hub.close()

    def on_ring_frame(self, body: bytes) -> None:
        """One frame popped from ring_in by a hub drain (loop thread)."""
        self.ring_frames_received += 1
        msg = msgpack.unpackb(body, raw=False, strict_map_key=False)
        if self._inbox_task is None:
            # nothing queued ahead of it: the hot kinds finish inline
            if msg.get("t") in _RPC_REPLY_KINDS:
                self._on_rpc_reply(msg)
                return
            if self.sync_handler is not None and self.sync_handler(msg):
                return
            self._inbox_task = asyncio.get_running_loop().create_task(self._run_inbox())
        self._inbox.append(msg)

    async def _run_inbox(self) -> None:
        try:
            while self._inbox:
                msg = self._inbox.popleft()
                try:
                    await self._dispatch(msg)
                except asyncio.CancelledError:
                    raise
                except Exception:
                    pass  # one bad frame does not stall those behind it
        finally:
            self._inbox_task = None
            if self._inbox and not self._closed.is_set():
                self._inbox_task = asyncio.get_running_loop().create_task(self._run_inbox())

    async def _send_lane(self, body: bytes) -> None:
        if self._closed.is_set():
            raise ConnectionError("connection closed")
        ring = self.ring_out
        # Frame order on a connection is push order. A sender that finds the
        # ring full waits for space holding the (FIFO) lock, and while any
        # sender waits, for space or for the lock, every later frame queues
        # behind it: the count, unlike Lock.locked(), stays up between one
        # waiter's release and the next one's wake-up. A frame that can
        # never fit raises from push() and is not sent at all.
        if self._lane_waiting == 0 and ring.push(body):
            self.ring_frames_sent += 1
            return
        self._lane_waiting += 1
        try:
            async with self._send_lock:
                while not ring.push(body):
                    if self._closed.is_set():
                        raise ConnectionError("connection closed")
                    await asyncio.sleep(0.001)
                self.ring_frames_sent += 1
        finally:
            self._lane_waiting -= 1

    def start(self) -> None:
        self._loop = asyncio.get_running_loop()
        self._reader_task = self._loop.create_task(self._read_loop())

    @property
    def closed(self) -> bool:
        return self._closed.is_set()

    async def wait_closed(self) -> None:
        await self._closed.wait()

    async def send(self, msg: dict, via_socket: bool = False) -> None:
        """``via_socket`` forces the socket (the hello_ack of a lane
        connection: the peer attaches its rings only on reading it)."""
        body = msgpack.packb(msg, use_bin_type=True)
        if self._lane and not via_socket:
            await self._send_lane(body)
            return
        if self.ring_out is not None and len(body) >= RING_MIN_FRAME and not via_socket:
            # bulk path: payload through the shm ring, doorbell on the socket
            pushed = self.ring_out.push(body)
            if pushed:
                self.ring_frames_sent += 1
                async with self._send_lock:
                    self.writer.write(pack({"t": "rb"}))
                    await self.writer.drain()
                return
            # ring full: fall through to the socket
        data = _LEN.pack(len(body)) + body
        async with self._send_lock:
            self.writer.write(data)
            await self.writer.drain()

    async def call(self, method: str, params: Any = None, timeout: Optional[float] = None) -> Any:
        # RPCs may originate on another event loop (e.g. the synchronizer loop
        # driving user code's handles inside a worker); bridge to the loop that
        # owns this connection's streams.
        running = asyncio.get_running_loop()
        if self._loop is not None and running is not self._loop:
            fut = asyncio.run_coroutine_threadsafe(self.call(method, params, timeout), self._loop)
            return await asyncio.wrap_future(fut)
        rpc_id = next(self._rpc_seq)
        fut: asyncio.Future = asyncio.get_running_loop().create_future()
        self._pending[rpc_id] = fut
        try:
            await self.send({"t": "rpc", "i": rpc_id, "m": method, "p": params})
            if timeout is not None:
                return await asyncio.wait_for(fut, timeout)
            return await fut
        finally:
            self._pending.pop(rpc_id, None)

    async def _dispatch(self, msg: dict) -> None:
        kind = msg.get("t")
        if kind == "rpc":
            asyncio.get_running_loop().create_task(self._serve_rpc(msg))
        elif kind in _RPC_REPLY_KINDS:
            self._on_rpc_reply(msg)
        else:
            await self.handler(msg)

    def _on_rpc_reply(self, msg: dict) -> None:
        fut = self._pending.get(msg["i"])
        if fut is None or fut.done():
            return
        if msg["t"] == "rpc_r":
            fut.set_result(msg.get("r"))
        else:
            fut.set_exception(RemoteRPCError(msg.get("e", "remote error"), msg.get("c")))

    async def _serve_rpc(self, msg: dict) -> None:
        rpc_id = msg["i"]
        method = msg["m"]
        try:
            if self.rpc_target is None:
                raise RuntimeError("No RPC target on this end")
            fn = getattr(self.rpc_target, method, None)
            if fn is None or method.startswith("_"):
                raise RuntimeError(f"Unknown RPC method {method!r}")
            params = msg.get("p") or {}
            result = await fn(**params)
            await self.send({"t": "rpc_r", "i": rpc_id, "r": result})
        except asyncio.CancelledError:
            raise
        except BaseException as exc:  # report, keep connection alive
            await self.send(
                {"t": "rpc_e", "i": rpc_id, "e": f"{type(exc).__name__}: {exc}", "c": type(exc).__name__}
            )

    async def _read_loop(self) -> None:
        try:
            while True:
                msg = await read_frame(self.reader)
                if msg is None:
                    break
                if msg.get("t") == "rb":
                    # doorbell: drain the inbound ring and dispatch its frames
                    if self.ring_in is not None:
                        for body in self.ring_in.pop_all():
                            self.ring_frames_received += 1
                            await self._dispatch(
                                msgpack.unpackb(body, raw=False, strict_map_key=False)
                            )
                    continue
                await self._dispatch(msg)
        except asyncio.CancelledError:
            pass
        except Exception:
            pass
        finally:
            if self._lane and self.ring_in is not None:
                # the peer pushed its last frames, then closed the socket
                try:
                    for body in self.ring_in.pop_all():
                        self.on_ring_frame(body)
                except Exception:
                    pass
            self._drop_own_hub()
            self._closed.set()
            for fut in self._pending.values():
                if not fut.done():
                    fut.set_exception(ConnectionError("connection closed"))
            try:
                self.writer.close()
            except Exception:
                pass

    async def close(self) -> None:
        if self._reader_task is not None:
            self._reader_task.cancel()
        self._drop_own_hub()
        try:
            self.writer.close()
            await self.writer.wait_closed()
        except Exception:
            pass
        self._closed.set()


class RemoteRPCError(Exception):
    def __init__(self, message: str, code: Optional[str] = None):
        super().__init__(message)
        self.code = code

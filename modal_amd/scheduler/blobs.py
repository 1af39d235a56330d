"""Content-addressed blob store (the local data plane).

Replaces the reference's presigned-URL S3/R2 blob plane
(/root/reference/py/modal/_utils/blob_utils.py): payloads above the inline
threshold (2 MiB, blob_utils.py:36) go into a content-addressed store on local
disk (tmpfs/NVMe) keyed by SHA-256, and only the blob id crosses the control
plane. Hashing uses the CDNA4 HIP sha256 kernel when a GPU is present and the
payload clears the crossover size; CPU hashlib below it (small payloads must
bypass GPU kernels — SURVEY.md §7 hard part 7).
"""

from __future__ import annotations

import hashlib
import os
import tempfile
from typing import Union

INLINE_LIMIT = 2 * 1024 * 1024  # parity: blob_utils.py:36
SPAWN_INLINE_LIMIT = 8 * 1024  # parity: blob_utils.py:39  (async spawn payloads)
BLOB_FILE_THRESHOLD = 4 * 1024 * 1024  # parity: blob_utils.py:43
HASH_CHUNK = 64 * 1024  # parity: hash_utils.py:11
BLOCK_SIZE = 8 * 1024 * 1024  # parity: volume v2 block size, blob_utils.py:63


def _hash_bytes(data: Union[bytes, memoryview]) -> str:
    """Content digest; routed to the HIP sha256 kernel for large buffers
    (ops/hashing.py: plain SHA-256 below the crossover, tree digest above)."""
    from ..ops.hashing import content_digest

    return content_digest(bytes(data))


class BlobStore:
    """CAS on the local filesystem: blobs/<aa>/<sha256>."""

    def __init__(self, root: str):
        self.root = root
        os.makedirs(root, exist_ok=True)

    def _path(self, digest: str) -> str:
        return os.path.join(self.root, digest[:2], digest)

    def _zpath(self, digest: str) -> str:
        # the compressed/raw bit lives in the FILENAME (".z" suffix), never in
        # the payload: raw content that happens to begin with the MALZ41 magic
        # round-trips untouched (advisor finding, round 1)
        return os.path.join(self.root, digest[:2], digest + ".z")

    COMPRESS_MIN = 1024 * 1024  # GPU (de)compression pays above ~1 MiB

    def _store(self, digest: str, data: Union[bytes, memoryview]) -> None:
        if self.has(digest):
            return
        payload = bytes(data)
        compressed = False
        if len(payload) >= self.COMPRESS_MIN:
            # HIP LZ4 kernels; digest stays the digest of the RAW content
            try:
                from ..ops.compress import compress_buffer

                z = compress_buffer(payload)
                if z is not None:
                    payload = z
                    compressed = True
            except Exception:
                pass
        self._store_prepared(digest, payload, compressed)

    def put(self, data: Union[bytes, memoryview]) -> str:
        digest = _hash_bytes(data)
        self._store(digest, data)
        return digest

    PIPELINE_MIN_BYTES = 96 * 1024 * 1024  # pipelined windows pay above this

    def put_many(self, buffers: list) -> list[str]:
        """Batched put: one GPU hash dispatch over all buffers' leaves AND
        one batched compression pass over the new large blocks (the
        volume-upload hot path). Large uploads take the PIPELINED path
        (ops/pipeline.py): H2D / digest+compress kernels / D2H / container
        assembly + CAS writes overlapped across 64 MiB windows."""
        from ..ops import gpu_available
        from ..ops.hashing import GPU_MIN_BYTES, content_digests_batch

        total_bytes = sum(len(b) for b in buffers)
        if total_bytes >= self.PIPELINE_MIN_BYTES and gpu_available():
            try:
                return self._put_many_pipelined(buffers)
            except Exception:
                pass  # serial fallback below

        # stage once: the digest and compression passes share one pinned
        # H2D of all buffers (LEAF_SIZE alignment satisfies both kernels)
        staged = None
        total = sum(len(b) for b in buffers)
        if total >= GPU_MIN_BYTES and gpu_available():
            try:
                from ..ops.hashing import LEAF_SIZE
                from ..ops.staging import stage_many_to_gpu

                staged = stage_many_to_gpu(buffers, align=LEAF_SIZE)
            except Exception:
                staged = None
        digests = content_digests_batch(buffers, staged=staged)
        # compress only blocks that are big enough and not already stored
        todo = [
            i for i, (digest, data) in enumerate(zip(digests, buffers))
            if len(data) >= self.COMPRESS_MIN and not self.has(digest)
        ]
        compressed: dict[int, bytes] = {}
        if todo:
            try:
                from ..ops.compress import compress_buffers

                if staged is not None:
                    payloads = compress_buffers(buffers, staged=staged, only=todo)
                else:
                    payloads = [None] * len(buffers)
                    for i, payload in zip(todo, compress_buffers([buffers[i] for i in todo])):
                        payloads[i] = payload
                for i in todo:
                    if payloads[i] is not None:
                        compressed[i] = payloads[i]
            except Exception:
                pass  # store raw on any kernel/driver hiccup
        for i, (digest, data) in enumerate(zip(digests, buffers)):
            if i in compressed:
                self._store_prepared(digest, compressed[i], True)
            else:
                self._store_prepared(digest, bytes(data), False)
        return digests

    def _put_many_pipelined(self, buffers: list) -> list[str]:
        from ..ops.pipeline import hash_compress_blocks

        def store(i: int, digest: str, payload: bytes, compressed: bool) -> None:
            if self.has(digest):
                return
            if len(buffers[i]) < self.COMPRESS_MIN and compressed:
                # parity with the serial path: tiny blocks store raw
                self._store_prepared(digest, buffers[i], False)
                return
            self._store_prepared(digest, payload, compressed)

        digests, _containers = hash_compress_blocks(buffers, compress=True, store=store)
        return digests

    def _store_prepared(self, digest: str, payload: bytes, compressed: bool = False) -> None:
        """Store an already-encoded payload under digest; ``compressed`` says
        whether it is an LZ4 container (recorded as a ``.z`` filename suffix,
        out-of-band of the bytes)."""
        path = self._zpath(digest) if compressed else self._path(digest)
        if os.path.exists(path):
            return
        os.makedirs(os.path.dirname(path), exist_ok=True)
        fd, tmp = tempfile.mkstemp(dir=os.path.dirname(path))
        try:
            with os.fdopen(fd, "wb") as f:
                f.write(payload)
            os.replace(tmp, path)
        except BaseException:
            try:
                os.unlink(tmp)
            except OSError:
                pass
            raise

    def put_prepared(self, digest: str, payload: bytes, compressed: bool) -> bool:
        """Store a block its producer already hashed and encoded (the device
        codec, ops/devcodec.py). False, and nothing written, when the CAS
        already has the digest in either form."""
        if self.has(digest):
            return False
        self._store_prepared(digest, payload, compressed)
        return True

    def get_stored(self, digest: str) -> tuple[bytes, bool]:
        """The stored form, NOT decompressed: (payload, compressed)."""
        path = self._path(digest)
        if os.path.exists(path):
            with open(path, "rb") as f:
                return f.read(), False
        with open(self._zpath(digest), "rb") as f:
            return f.read(), True

    def put_file(self, src_path: str) -> str:
        # Same CAS key as put(): plain SHA-256 below the GPU threshold, the
        # domain-separated tree digest above (advisor finding: the two paths
        # previously diverged, breaking dedup for identical content).
        from ..ops.hashing import GPU_MIN_BYTES, content_digest

        size = os.path.getsize(src_path)
        if size < GPU_MIN_BYTES:
            h = hashlib.sha256()
            with open(src_path, "rb") as f:
                while True:
                    chunk = f.read(1 << 20)
                    if not chunk:
                        break
                    h.update(chunk)
            digest = h.hexdigest()
        else:
            import mmap

            with open(src_path, "rb") as f:
                with mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
                    digest = content_digest(memoryview(mm))
        path = self._path(digest)
        if not os.path.exists(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
            fd, tmp = tempfile.mkstemp(dir=os.path.dirname(path))
            os.close(fd)
            import shutil

            shutil.copyfile(src_path, tmp)
            os.replace(tmp, path)
        return digest

    def get(self, digest: str) -> bytes:
        path = self._path(digest)
        if os.path.exists(path):
            with open(path, "rb") as f:
                return f.read()
        zpath = self._zpath(digest)
        with open(zpath, "rb") as f:
            blob = f.read()
        from ..ops.compress import decompress_buffer

        return decompress_buffer(blob)

    def open_path(self, digest: str) -> str:
        """Path to the RAW content on disk (consumers sendfile/mmap it).

        A compressed-only blob is decompressed once into the raw path and
        cached there; subsequent calls hit the raw file directly."""
        path = self._path(digest)
        if os.path.exists(path):
            return path
        zpath = self._zpath(digest)
        if not os.path.exists(zpath):
            raise FileNotFoundError(f"blob {digest} not in store")
        self._store_prepared(digest, self.get(digest), False)
        return path

    def materialize(self, digest: str, dest: str) -> None:
        """Produce the RAW content at dest: hard-link when the stored form is
        raw, write a decompressed copy when only the ``.z`` form exists."""
        os.makedirs(os.path.dirname(dest), exist_ok=True)
        src = self._path(digest)
        if not os.path.exists(src):
            if not os.path.exists(self._zpath(digest)):
                raise FileNotFoundError(f"blob {digest} not in store")
            data = self.get(digest)
            with open(dest, "wb") as f:
                f.write(data)
            return
        try:
            if os.path.exists(dest):
                os.unlink(dest)
            os.link(src, dest)
        except OSError:
            import shutil

            shutil.copyfile(src, dest)

    def has(self, digest: str) -> bool:
        return os.path.exists(self._path(digest)) or os.path.exists(self._zpath(digest))

    def size(self, digest: str) -> int:
        """On-disk (stored) size — compressed size for ``.z`` blobs."""
        path = self._path(digest)
        if os.path.exists(path):
            return os.stat(path).st_size
        return os.stat(self._zpath(digest)).st_size

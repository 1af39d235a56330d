"""The segmented container under MALZ41 (ops/compress.py) and MAFP10
(ops/fpcodec.py): a fixed header, a ``<u4`` table with one length per 4 KiB
segment of the raw bytes (0: stored raw), the segments back to back. What
follows from that alone lives here once and imports neither codec; a codec
adds its magic, its own header fields and checks, and its kernels.
"""

from __future__ import annotations

import struct
from typing import Any, Callable, Optional, Sequence

from . import load_lib

SEG_SIZE = 4096
OUT_STRIDE = SEG_SIZE + 256
MIN_GAIN = 0.95  # store raw unless compression saves >=5%
STATUS_CLEAN = 2**31 - 1  # decode status word when no segment is corrupt


def worth_keeping(payload_len: Any, raw_len: Any) -> Any:
    """THE keep/raw rule: a container is kept only when its payload saves
    at least 1 - MIN_GAIN of the raw bytes (scalars or numpy arrays)."""
    return payload_len < raw_len * MIN_GAIN


def seg_raw_lens(n_seg: int, raw_len: int) -> Any:
    """Raw length of every segment (int64 array)."""
    import numpy as np

    seg_raw = np.full(n_seg, SEG_SIZE, dtype=np.int64)
    if n_seg:
        seg_raw[-1] = raw_len - (n_seg - 1) * SEG_SIZE
    return seg_raw


def effective_lens(comp_lens: Any, raw_len: int) -> Any:
    """Bytes every segment takes in the payload (int64 array): its comp_len,
    or the raw segment length where comp_len is 0."""
    import numpy as np

    comp_lens = np.asarray(comp_lens)
    raw = seg_raw_lens(len(comp_lens), raw_len)
    return np.where(comp_lens == 0, raw, comp_lens.astype(np.int64))


def read_header(
    blob: bytes, raw_len: Optional[int], what: str, magic: bytes, header_fixed: int,
    n_seg_at: int, after_magic: Callable[[], None] = lambda: None,
    after_n_seg: Callable[[], None] = lambda: None,
) -> tuple[int, int, Any, int]:
    """The checks every container gets: magic and length, raw_len (the u64
    after the magic) against the caller's when given, n_seg (the u32 at
    ``n_seg_at``) against raw_len, the table inside the blob; a format's own
    checks of its fixed fields run in between, where they always ran. Returns
    (raw_len, n_seg, the ``<u4`` table, payload offset); ValueError names ``what``."""
    import numpy as np

    n = len(blob)
    if n < header_fixed or bytes(blob[: len(magic)]) != magic:
        raise ValueError(f"{what}: not a {magic.decode()} container")
    after_magic()
    (hdr_raw,) = struct.unpack_from("<Q", blob, len(magic))
    (n_seg,) = struct.unpack_from("<I", blob, n_seg_at)
    if raw_len is not None and hdr_raw != raw_len:
        raise ValueError(f"{what}: container raw_len {hdr_raw} != manifest {raw_len}")
    if n_seg != -(-hdr_raw // SEG_SIZE):
        raise ValueError(f"{what}: container has {n_seg} segments for {hdr_raw} bytes")
    after_n_seg()
    off = header_fixed + 4 * n_seg
    if n < off:
        raise ValueError(f"{what}: container truncated inside its segment table")
    return hdr_raw, n_seg, np.frombuffer(blob, dtype="<u4", count=n_seg, offset=header_fixed), off


def check_size(blob: bytes, off: int, payload: int, what: str) -> None:
    if off + payload != len(blob):
        raise ValueError(f"{what}: container is {len(blob)} bytes, header says {off + payload}")


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed: hipError {rc}")


def to_dev(arr: Any) -> Any:
    import numpy as np
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


class Workspace:
    """Device buffers of one ``compress_spans_gpu`` call: the strided encoder
    output (OUT_STRIDE per segment), comp_lens and seg_off per segment, and
    the dense containers."""

    def __init__(self, n_seg: int, dense_bytes: int) -> None:
        import torch

        self.n_seg = n_seg
        self.stride = torch.empty(n_seg * OUT_STRIDE, dtype=torch.uint8, device="cuda")
        self.dense = torch.empty(dense_bytes, dtype=torch.uint8, device="cuda")
        self.comp_lens = torch.empty(n_seg, dtype=torch.int32, device="cuda")
        self.seg_off = torch.empty(n_seg, dtype=torch.int64, device="cuda")

    @classmethod
    def for_lengths(cls, raw_lens: Sequence[int], header_fixed: int) -> "Workspace":
        """Sized to one call: every span kept would still fit the dense part."""
        n_seg = sum(-(-n // SEG_SIZE) for n in raw_lens)
        return cls(n_seg, len(raw_lens) * header_fixed + 4 * n_seg + sum(raw_lens))


def span_tables(spans: Sequence[tuple[int, int]], first_seg: Any) -> tuple:
    """Per span, on the device: first segment in the workspace, raw_len, offset."""
    import numpy as np

    first_d = to_dev(np.asarray(first_seg, dtype=np.int32))
    raw_d = to_dev(np.array([ln for _off, ln in spans], dtype=np.int64))
    return first_d, raw_d, to_dev(np.array([off for off, _ln in spans], dtype=np.int64))


def finish_containers(
    lib: Any, spans: Sequence[tuple[int, int]], ws: Workspace, first_d: Any, raw_d: Any,
    n_segs: Any, header_fixed: int, assemble: Callable[[Any], None],
) -> list:
    """The encoder's tail, once every segment is in its stride slot with its
    comp_len (``n_segs``: segments per span): one plan launch, ONE sync (the
    payload totals), the keep decision, the codec's ``assemble(out_off_d)``
    launch into ``ws.dense`` (-1: span not kept) and one D2H of the dense
    containers, on the current stream. Returns the container per span or None."""
    import numpy as np
    import torch

    from .staging import copy_from_device

    out: list = [None] * len(spans)
    payload_d = torch.empty(len(spans), dtype=torch.int64, device="cuda")
    rc = lib.ma_malz_plan(
        ws.comp_lens.data_ptr(), first_d.data_ptr(), raw_d.data_ptr(), ws.seg_off.data_ptr(),
        payload_d.data_ptr(), len(spans), torch.cuda.current_stream().cuda_stream,
    )
    check(rc, "malz plan kernel")
    totals = payload_d.cpu().numpy()  # the one sync
    keep = worth_keeping(totals, np.array([ln for _off, ln in spans], dtype=np.int64))
    sizes = np.where(keep, header_fixed + 4 * np.asarray(n_segs, dtype=np.int64) + totals, 0)
    ends = np.cumsum(sizes)
    out_off = np.where(keep, ends - sizes, -1)  # -1: the kernel skips the span
    dense_len = int(ends[-1])
    if dense_len == 0:
        return out
    if dense_len > ws.dense.numel():
        raise RuntimeError("dense containers exceed the workspace")
    assemble(to_dev(out_off))
    dense = copy_from_device(ws.dense.data_ptr(), dense_len)
    for j in np.flatnonzero(keep):
        out[j] = dense[out_off[j] : out_off[j] + sizes[j]]
    return out


def decode_status(launch: Callable[[int, int], int], what: str) -> int:
    """Run a decode kernel, ``launch(status pointer, stream)`` -> hipError: 0,
    or 1 + the first corrupt segment (the kernels take the min over them, so
    no lane order decides). The stream has drained either way."""
    import torch

    status = torch.full((1,), STATUS_CLEAN, dtype=torch.int32, device="cuda")
    check(launch(status.data_ptr(), torch.cuda.current_stream().cuda_stream), what)
    first_bad = int(status.item())  # syncs: the caller's tables may be freed
    return 0 if first_bad == STATUS_CLEAN else first_bad


def decompress_buffer_gpu(codec: Any, blob: bytes) -> bytes:
    """Raw bytes of one container, decoded on the device by ``codec`` (a codec module)."""
    hdr = codec.validate_container(blob)  # before any launch
    lib = load_lib(required=True)
    import torch

    from .staging import fetch_from_gpu, stage_to_gpu

    comp = stage_to_gpu(memoryview(blob)[hdr.payload_off :])
    dst = torch.empty(hdr.raw_len, dtype=torch.uint8, device="cuda")
    bad = codec.decompress_run_gpu(lib, comp.data_ptr(), [hdr], dst.data_ptr())
    if bad:
        raise ValueError(codec.corrupt_message(bad))
    return fetch_from_gpu(dst)

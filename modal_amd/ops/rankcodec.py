"""The rank-plane codec under MAFP10 (ops/fpcodec.py) and MAFB10
(ops/bytecodec.py): what the two formats share, written once.

Both code the TOP byte of every ``es``-byte element (at ``es`` 1 the whole
element) as its rank in a per-block frequency order, pack the ranks at a
fixed width chosen per 4 KiB segment, escape the rare ranks and leave the low
``es - 1`` bytes alone. The two modules hold the layouts; they differ in the
magic, in the element sizes a reader admits and in the encode and decode
kernels, and a ``Format`` says exactly that. Everything else is here: the
fixed header and its validator, the order table, the width rule and the bit
packing, the numpy codec (the model the kernels in csrc/fpz.hip and
csrc/bytez.hip are held to byte for byte, and the reader of GPU-less
processes), the device encoder's launches up to the stride slots, the
assemble launch both formats share, and the decode launch. The segmented
container under it is ops/container.py; no format module is imported here.
"""

from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import Any, NamedTuple, Optional, Sequence

import numpy as np

from . import container, gpu_available, load_lib
from .container import OUT_STRIDE, SEG_SIZE, Workspace, effective_lens, seg_raw_lens, worth_keeping

MAGIC_LEN = 6
HEADER_FIXED = MAGIC_LEN + 8 + 1 + 1 + 4 + 256  # up to the seg_len table


class Header(NamedTuple):
    raw_len: int
    seg_lens: Any  # int32 array
    payload_off: int
    es: int
    order: Any  # uint8[256]


def block_order(data: Any, es: int) -> Any:
    """order[r] = byte value of rank r over the top bytes of the block's
    whole elements: count descending, byte value ascending on ties."""
    whole = (len(data) // es) * es
    counts = np.bincount(data[es - 1 : whole : es], minlength=256)
    return np.lexsort((np.arange(256), -counts)).astype(np.uint8)


def _code_rows(ranks: Any, m: int) -> tuple[Any, Any]:
    """(b, hi) per row of ``ranks`` (n x m): the width that minimises
    1 + ceil(m*b/8) + n_escapes(b), smallest b on ties."""
    widths = np.arange(1, 8)
    esc = np.stack([(ranks >= (1 << b) - 1).sum(axis=1) for b in widths], axis=1)
    cost = 1 + (m * widths + 7) // 8 + esc
    pick = cost.argmin(axis=1)  # the first minimum: the smallest b
    return widths[pick], cost[np.arange(len(pick)), pick]


def _pack_rows(ranks: Any, b: int) -> Any:
    """Rows of ranks (n x m) -> n x ceil(m*b/8) code bytes at width b."""
    codes = np.minimum(ranks, (1 << b) - 1).astype(np.uint8)
    bits = np.unpackbits(codes[:, :, None], axis=2, bitorder="little")[:, :, :b]
    return np.packbits(bits.reshape(len(ranks), -1), axis=1, bitorder="little")


@dataclass(frozen=True)
class Format:
    """One rank-plane format, and the codec for it. A format module makes one
    and binds its public names to the methods."""

    magic: bytes
    elem_sizes: tuple  # the element sizes a container of this format may have
    sizes_text: str  # how the element-size error names them
    label: str  # the kernels' name in error messages
    encode_entry: str  # library entries: segments -> stride slots,
    decode_entry: str  # a run of containers -> raw bytes
    es_in_abi: bool  # those entries take the element size (False: they know it)
    min_hi: int = 2  # the fewest bytes a coded segment has after its low bytes

    def __post_init__(self) -> None:
        # a full segment is a whole number of elements: validator and kernels count on it
        if len(self.magic) != MAGIC_LEN or any(SEG_SIZE % es for es in self.elem_sizes):
            raise ValueError("a format has a 6-byte magic and element sizes that divide a segment")

    def is_container(self, blob: bytes) -> bool:
        return bytes(blob[:MAGIC_LEN]) == self.magic

    def _check_es(self, es: int, what: str = "") -> None:
        if es not in self.elem_sizes:
            raise ValueError(f"{what}element size {es} is not {self.sizes_text}")

    def validate_container(
        self, blob: bytes, raw_len: Optional[int] = None, what: str = "container"
    ) -> Header:
        """Parse a container and bound everything a decoder indexes with.
        Raises ValueError naming ``what``."""
        es, order = 0, None  # set by the two checks that run inside the shared reader

        def elem_fields() -> None:
            nonlocal es
            es, reserved = struct.unpack_from("<BB", blob, MAGIC_LEN + 8)
            self._check_es(es, f"{what}: ")
            if reserved != 0:
                raise ValueError(f"{what}: reserved byte is not 0")

        def order_table() -> None:
            nonlocal order
            order = np.frombuffer(blob, dtype=np.uint8, count=256, offset=HEADER_FIXED - 256)
            if not np.array_equal(np.sort(order), np.arange(256, dtype=np.uint8)):
                raise ValueError(f"{what}: order table is not a permutation")

        hdr_raw, n_seg, seg_lens, off = container.read_header(
            blob, raw_len, what, self.magic, HEADER_FIXED, MAGIC_LEN + 10, elem_fields, order_table
        )
        seg_lens = seg_lens.astype(np.int64)
        L = seg_raw_lens(n_seg, hdr_raw)
        coded = seg_lens != 0
        # every element size divides SEG_SIZE: only the last segment can be odd
        if n_seg and coded[-1] and L[-1] % es:
            raise ValueError(f"{what}: coded segment is not a whole number of elements")
        lo = (L // es) * (es - 1)
        if np.any(coded & ((seg_lens < lo + self.min_hi) | (seg_lens >= L))):
            raise ValueError(f"{what}: segment seg_len out of range")
        container.check_size(blob, off, int(np.where(coded, seg_lens, L).sum()), what)
        return Header(hdr_raw, seg_lens.astype(np.int32), off, es, order)

    def corrupt_message(self, status: int) -> str:
        return f"{self.magic.decode()} container corrupt at segment {status - 1}"

    # -----------------------------------------------------------------------
    # the numpy model
    # -----------------------------------------------------------------------

    def _header(self, raw_len: int, es: int, order: Any, seg_lens: Any) -> bytes:
        return (
            self.magic
            + struct.pack("<QBBI", raw_len, es, 0, len(seg_lens))
            + np.asarray(order, dtype=np.uint8).tobytes()
            + np.asarray(seg_lens, dtype="<u4").tobytes()
        )

    def compress_buffer_cpu(self, data: Any, es: int) -> Optional[bytes]:
        """The container of ``data`` at element size ``es``, or None when it
        does not save 5 %."""
        self._check_es(es)
        data = np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8)
        n = len(data)
        if n == 0:
            return None
        n_seg = -(-n // SEG_SIZE)
        order = block_order(data, es)
        rank_of = np.empty(256, dtype=np.uint8)
        rank_of[order] = np.arange(256, dtype=np.uint8)

        # pass 1: every segment's width and seg_len; full segments together,
        # then the short last one, through the same steps
        seg_lens = np.zeros(n_seg, dtype=np.int64)
        widths = np.zeros(n_seg, dtype=np.int64)
        groups = [(0, n // SEG_SIZE, SEG_SIZE), (n // SEG_SIZE, 1 if n % SEG_SIZE else 0, n % SEG_SIZE)]
        groups = [(first, count, L) for first, count, L in groups if count and L % es == 0]
        ranks_of_group = {}
        for first, count, L in groups:
            m = L // es
            tops = data[first * SEG_SIZE : first * SEG_SIZE + count * L].reshape(count, m, es)[:, :, es - 1]
            ranks = ranks_of_group[first] = rank_of[tops]
            b_row, hi = _code_rows(ranks, m)
            coded = hi < m
            widths[first : first + count] = np.where(coded, b_row, 0)
            seg_lens[first : first + count] = np.where(coded, m * (es - 1) + hi, 0)
        eff = effective_lens(seg_lens, n)
        if not worth_keeping(int(eff.sum()), n):
            return None

        # pass 2: the payload, every segment at its offset
        offs = np.cumsum(eff) - eff
        payload = np.empty(int(eff.sum()), dtype=np.uint8)
        for s in np.flatnonzero(seg_lens == 0):
            payload[offs[s] : offs[s] + eff[s]] = data[s * SEG_SIZE : s * SEG_SIZE + eff[s]]
        for first, count, L in groups:
            m = L // es
            lo = m * (es - 1)
            elems = data[first * SEG_SIZE : first * SEG_SIZE + count * L].reshape(count, m, es)
            for b in np.unique(widths[first : first + count]):
                if b == 0:
                    continue
                b = int(b)
                rows = np.flatnonzero(widths[first : first + count] == b)
                at = offs[first + rows][:, None]
                nbytes = (m * b + 7) // 8
                payload[at + np.arange(lo)] = elems[rows, :, : es - 1].reshape(len(rows), lo)
                payload[at[:, 0] + lo] = b
                ranks = ranks_of_group[first][rows]
                payload[at + (lo + 1) + np.arange(nbytes)] = _pack_rows(ranks, b)
                esc = ranks >= (1 << b) - 1
                nth = np.cumsum(esc, axis=1) - 1  # an escape's place among its segment's
                payload[(at + (lo + 1 + nbytes) + nth)[esc]] = elems[rows, :, es - 1][esc]
        return self._header(n, es, order, seg_lens) + payload.tobytes()

    def decompress_buffer_cpu(self, blob: bytes) -> bytes:
        """Raw bytes of a container; ValueError on a malformed header or a
        corrupt segment (the first one is named)."""
        hdr = self.validate_container(blob)
        es, n = hdr.es, hdr.raw_len
        buf = np.frombuffer(blob, dtype=np.uint8)
        out = np.empty(n, dtype=np.uint8)
        seg_lens = hdr.seg_lens.astype(np.int64)
        L_of = seg_raw_lens(len(seg_lens), n)
        eff = effective_lens(seg_lens, n)
        offs = hdr.payload_off + np.cumsum(eff) - eff
        for s in np.flatnonzero(seg_lens == 0):
            out[s * SEG_SIZE : s * SEG_SIZE + eff[s]] = buf[offs[s] : offs[s] + eff[s]]

        coded = np.flatnonzero(seg_lens)
        lo_of = (L_of // es) * (es - 1)
        b_of = np.zeros(len(seg_lens), dtype=np.int64)
        b_of[coded] = buf[offs[coded] + lo_of[coded]]
        nbytes_of = ((L_of // es) * b_of + 7) // 8
        ok = (b_of >= 1) & (b_of <= 7) & (lo_of + 1 + nbytes_of <= seg_lens)
        bad = coded[~ok[coded]].tolist()
        # segments of one length and one width decode together
        for L, b in sorted({(int(L_of[s]), int(b_of[s])) for s in coded if ok[s]}):
            rows = coded[(L_of[coded] == L) & (b_of[coded] == b) & ok[coded]]
            m = L // es
            lo, nbytes = m * (es - 1), (m * b + 7) // 8
            at = offs[rows][:, None]
            bits = np.unpackbits(buf[at + (lo + 1) + np.arange(nbytes)], axis=1, bitorder="little")
            bits = bits[:, : m * b].reshape(len(rows), m, b)
            codes = np.packbits(bits, axis=2, bitorder="little").reshape(len(rows), m)
            esc = codes == (1 << b) - 1
            fits = esc.sum(axis=1) == seg_lens[rows] - lo - 1 - nbytes
            bad += rows[~fits].tolist()
            rows, at, codes, esc = rows[fits], at[fits], codes[fits], esc[fits]
            elems = np.empty((len(rows), m, es), dtype=np.uint8)
            elems[:, :, : es - 1] = buf[at + np.arange(lo)].reshape(len(rows), m, es - 1)
            tops = hdr.order[codes]
            nth = np.cumsum(esc, axis=1) - 1
            tops[esc] = buf[(at + (lo + 1 + nbytes) + nth)[esc]]
            elems[:, :, es - 1] = tops
            if L == SEG_SIZE:
                out[: (n // SEG_SIZE) * SEG_SIZE].reshape(-1, SEG_SIZE)[rows] = elems.reshape(-1, L)
            elif len(rows):
                out[rows[0] * SEG_SIZE :] = elems.reshape(-1)
        if bad:
            raise ValueError(
                f"{self.corrupt_message(min(bad) + 1)}: bad code width or escape count"
            )
        return out.tobytes()

    # -----------------------------------------------------------------------
    # GPU paths
    # -----------------------------------------------------------------------

    def compress_spans_gpu(
        self, lib: Any, base: int, spans: Sequence[tuple[int, int]], es: int, ws: Workspace,
        counts: Any = None,
    ) -> list:
        """Containers of the device bytes ``(base + offset, raw_len)`` per
        span, None where the container is not kept. One histogram, one rank
        and one encode launch for all spans, then
        ``container.finish_containers`` (one plan launch, ONE sync, one
        assemble launch, one D2H of the dense containers), all on the current
        stream. ``counts``, a contiguous ``len(spans) x 256`` int32 device
        tensor, is the spans' histograms at ``es`` where the caller has them
        (``fpcodec.probe_spans_gpu``): no histogram launch then."""
        import torch

        self._check_es(es)
        if not spans:
            return []
        stream = torch.cuda.current_stream().cuda_stream
        n_segs = np.array([-(-ln // SEG_SIZE) for _off, ln in spans], dtype=np.int64)
        ends_seg = np.cumsum(n_segs)
        if int(ends_seg[-1]) > ws.n_seg:
            raise RuntimeError("compress spans exceed the workspace")
        first_d, raw_d, src_off_d = container.span_tables(spans, ends_seg - n_segs)
        tables = torch.empty(2, len(spans) * 256, dtype=torch.uint8, device="cuda")
        order_d, rank_d = tables[0], tables[1]
        if counts is None:
            counts = torch.zeros(len(spans) * 256, dtype=torch.int32, device="cuda")
            rc = lib.ma_rank_hist(
                base, src_off_d.data_ptr(), raw_d.data_ptr(), es, counts.data_ptr(),
                order_d.data_ptr(), rank_d.data_ptr(), len(spans), stream,
            )
        else:
            if (
                counts.dtype != torch.int32 or counts.numel() != len(spans) * 256
                or not counts.is_cuda or not counts.is_contiguous()
            ):
                raise ValueError("counts is a contiguous int32 device tensor of len(spans) x 256")
            rc = lib.ma_fpz_rank_counts(
                counts.data_ptr(), order_d.data_ptr(), rank_d.data_ptr(), len(spans), stream
            )
        container.check(rc, f"{self.label} histogram/rank kernels")
        es_arg = (es,) if self.es_in_abi else ()
        container.check(
            getattr(lib, self.encode_entry)(
                base, src_off_d.data_ptr(), raw_d.data_ptr(), first_d.data_ptr(),
                rank_d.data_ptr(), *es_arg, ws.stride.data_ptr(), OUT_STRIDE,
                ws.comp_lens.data_ptr(), len(spans), int(n_segs.max()), stream,
            ),
            f"{self.label} encode kernel",
        )

        def assemble(out_off_d: Any) -> None:
            rc = lib.ma_rank_assemble(
                base, src_off_d.data_ptr(), ws.stride.data_ptr(), OUT_STRIDE,
                ws.comp_lens.data_ptr(), ws.seg_off.data_ptr(), first_d.data_ptr(),
                raw_d.data_ptr(), order_d.data_ptr(), int.from_bytes(self.magic, "little"), es,
                ws.dense.data_ptr(), out_off_d.data_ptr(), len(spans), stream,
            )
            container.check(rc, f"{self.label} assemble kernel")

        return container.finish_containers(
            lib, spans, ws, first_d, raw_d, n_segs, HEADER_FIXED, assemble
        )

    def decompress_run_gpu(self, lib: Any, comp: int, headers: Sequence[Header], dst: int) -> int:
        """Decompress a run of VALIDATED containers, ``headers`` what
        ``validate_container`` returned for each, whose payloads lie back to
        back at device pointer ``comp`` and whose raw bytes are consecutive at
        ``dst``, on the current stream. Returns 0, or 1 + the run's first
        segment found corrupt; the stream has drained either way."""
        if not sum(len(h.seg_lens) for h in headers):
            return 0
        offs_d, ints_d, order_d, n_segments = container.run_tables(headers)
        es_arg: tuple = ()
        if self.es_in_abi:  # the element size of every container of the run
            es_d = container.to_dev(np.array([h.es for h in headers], dtype=np.uint8))
            es_arg = (es_d.data_ptr(),)
        return container.decode_status(
            lambda status, stream: getattr(lib, self.decode_entry)(
                comp, offs_d[0].data_ptr(), offs_d[1].data_ptr(), ints_d[0].data_ptr(),
                ints_d[1].data_ptr(), ints_d[2].data_ptr(), order_d.data_ptr(),
                *es_arg, dst, status, n_segments, stream,
            ),
            f"{self.label} decode kernel",
        )

    def decompress_buffer_gpu(self, blob: bytes) -> bytes:
        return container.decompress_buffer_gpu(self, blob)

    # -----------------------------------------------------------------------
    # dispatching front door
    # -----------------------------------------------------------------------

    def compress_buffer_gpu(self, data: bytes, es: int) -> Optional[bytes]:
        if len(data) == 0:
            return None
        lib = load_lib(required=True)
        from .staging import stage_to_gpu

        src = stage_to_gpu(data)
        ws = Workspace.for_lengths([len(data)], HEADER_FIXED)
        return self.compress_spans_gpu(lib, src.data_ptr(), [(0, len(data))], es, ws)[0]

    def compress_buffer(self, data: bytes, es: int) -> Optional[bytes]:
        """GPU when present, else the numpy codec: the same container either way."""
        if gpu_available():
            return self.compress_buffer_gpu(data, es)
        return self.compress_buffer_cpu(data, es)

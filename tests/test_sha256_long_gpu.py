"""The wavefront SHA-256 (csrc/sha256w.hip, hashing.sha256_long_gpu) against
hashlib.sha256 of the same host bytes: the padding edges inside a block, the
padding block that opens a new batch, exact batch multiples, enough batches to
cycle the prefetch, unaligned sources that end at their tensor's last byte,
many messages in one launch, and the tail block of devcodec's public path.
Every comparison is exact."""

from __future__ import annotations

import hashlib

import numpy as np
import pytest

from modal_amd.ops import hashing

pytestmark = pytest.mark.gpu

B = hashing.LONG_BATCH
MiB = 1 << 20
LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, B - 65, B - 64, B - 10, B - 9, B - 8, B - 1, B, B + 1,
           2 * B - 9, 2 * B, 3 * B + 777, MiB + 3]


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (before the library, as in test_digest_gpu.py)

    from modal_amd.ops import load_lib

    return load_lib(required=True)


def _random_device(nbytes: int, seed: int):
    import torch

    host = np.random.default_rng(seed).integers(0, 256, max(nbytes, 1), dtype=np.uint8)[:nbytes]
    dev = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")[:nbytes]
    dev.copy_(torch.from_numpy(host))
    assert dev.data_ptr() % 256 == 0
    return host, dev


def _i64(values) -> np.ndarray:
    return np.array(values, dtype=np.int64)


@pytest.mark.parametrize("length", LENGTHS)
def test_lengths(lib, length):
    host, dev = _random_device(length, 1000 + length)
    got = hashing.sha256_long_gpu(lib, dev.data_ptr(), _i64([0]), _i64([length]))
    assert got.shape == (1, 32) and got.dtype == np.uint8
    assert got[0].tobytes() == hashlib.sha256(host.tobytes()).digest()


@pytest.mark.parametrize("length", [B - 9, 2 * B + 1])
@pytest.mark.parametrize("mis", [1, 2, 3, 5, 8])
def test_unaligned_source_ending_at_the_tensor_end(lib, mis, length):
    host, dev = _random_device(mis + length, 2000 + 16 * mis + length)
    got = hashing.sha256_long_gpu(lib, dev.data_ptr(), _i64([mis]), _i64([length]))
    assert got[0].tobytes() == hashlib.sha256(host[mis:].tobytes()).digest()


def test_many_messages_in_one_launch(lib):
    import torch

    lengths = [0, 1, B, 70000, 64, 3 * B + 777, 200000]
    offsets, at = [], 13
    for n in lengths:
        offsets.append(at)
        at += n + 7  # arbitrary alignments, no two messages adjacent
    host, dev = _random_device(at, 3000)
    want = [hashlib.sha256(host[o : o + n].tobytes()).digest() for o, n in zip(offsets, lengths)]
    got = hashing.sha256_long_gpu(lib, dev.data_ptr(), _i64(offsets), _i64(lengths))
    assert [row.tobytes() for row in got] == want

    # a second call on a subset writes its own rows of `out` and no others
    subset = [3, 0, 6]
    out = torch.from_numpy(got.copy()).cuda()
    off_d = torch.from_numpy(_i64([offsets[i] for i in subset])).cuda()
    len_d = torch.from_numpy(_i64([lengths[i] for i in subset])).cuda()
    rc = lib.ma_sha256_long(dev.data_ptr(), off_d.data_ptr(), len_d.data_ptr(), out.data_ptr(),
                            len(subset), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    rows = [row.tobytes() for row in out.cpu().numpy()]
    assert rows == [want[i] for i in subset] + want[len(subset):]
    assert lib.ma_sha256_long(0, 0, 0, 0, 0, 0) == 0  # n <= 0: no launch


def test_tail_block_through_devcodec(lib):
    import torch

    from modal_amd.ops import devcodec

    nbytes = 8 * MiB + devcodec.LONG_MIN + 5
    host, dev = _random_device(nbytes, 4000)
    blocks = devcodec.encode_tensor(dev)
    assert [b.raw_len for b in blocks] == [8 * MiB, devcodec.LONG_MIN + 5]
    assert blocks[1].digest == hashing.content_digest(host[8 * MiB :].tobytes())
    out = torch.full_like(dev, 0xA5)
    devcodec.decode_tensor(blocks, out, verify=True)
    assert torch.equal(out, dev)
    out[nbytes - 3] ^= 0x01
    with pytest.raises(ValueError, match="block 1 digest mismatch"):
        devcodec.verify_device([(out.data_ptr(), [(b.digest, b.raw_len) for b in blocks])])

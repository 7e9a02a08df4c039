"""The segmented CRC-32 on the GPU (csrc/crc32.hip, ops.crc32_rows) against zlib.crc32: integer work, so every checksum is
EQUAL to zlib's.  The kernel cuts a row into pieces of 64 bytes, a workgroup takes 256 of them (16384 bytes), and a row of
several workgroups is folded by a second kernel: the lengths sit on both sides of each of those sizes."""

import functools
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PIECE, SPAN = 64, 16384
PITCH = 3 * SPAN + 849                                     # 50001, odd: consecutive rows start on every byte alignment
LENS = [0, 1, 3, 4, 5, PIECE - 1, PIECE, PIECE + 1, SPAN - 1, SPAN, SPAN + 1, 0, 2 * SPAN + 4097, PITCH, PITCH - 1]
FILL, GUARD = 0xA5, 0x5A5A5A5A
IDAT = zlib.crc32(b"IDAT")


@functools.lru_cache(maxsize=None)
def rows_of(kind):
    """(len(LENS), PITCH) uint8: row i's first LENS[i] bytes are the data, the bytes behind them a pattern that must not count."""
    assert PITCH % 2 == 1 and {(i * PITCH) % 4 for i in range(len(LENS))} == {0, 1, 2, 3}
    if kind == "random":
        a = np.random.default_rng(5).integers(0, 256, (len(LENS), PITCH), dtype=np.uint8)
    else:
        a = np.full((len(LENS), PITCH), 0x00 if kind == "zeros" else 0xFF, dtype=np.uint8)
    for i, n in enumerate(LENS):
        a[i, n:] = FILL if kind != "random" else a[i, n:] ^ 0x3C
    a.setflags(write=False)
    return a


def seeds_of(kind):
    if kind == "none":
        return None
    if kind == "zero":
        return np.zeros(len(LENS), dtype=np.uint32)
    mixed = [IDAT, 0xFFFFFFFF, 0, 1, 0x80000000, zlib.crc32(b"fdAT\0\0\0\2")]
    return np.array([mixed[i % len(mixed)] for i in range(len(LENS))], dtype=np.uint32)


def gpu_crc(data, lens, seeds, ws_short=0):
    """-> uint32 (n,); the word in front of and behind the n results must stay as it was."""
    from vdpp_amd.hip import ops
    n, pitch = data.shape
    d = torch.from_numpy(np.array(data)).to(DEV)
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
    sd = None if seeds is None else torch.from_numpy(np.array(seeds).view(np.int32)).to(DEV)
    out = torch.from_numpy(np.full(n + 2, GUARD, dtype=np.uint32).view(np.int32)).to(DEV)
    ws = torch.empty(ops.crc32_ws_bytes(n, pitch) - ws_short, dtype=torch.uint8, device=DEV)
    ops.crc32_rows(d, ln, out[1:n + 1], ws, seed=sd)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert got[0] == GUARD and got[-1] == GUARD, "a word outside crc[0 .. n) was written"
    return got[1:-1]


def want_crc(data, lens, seeds):
    return np.array([zlib.crc32(data[i, :max(0, min(n, data.shape[1]))].tobytes(), 0 if seeds is None else int(seeds[i]))
                     for i, n in enumerate(lens)], dtype=np.uint32)


@pytest.mark.parametrize("seed_kind", ("none", "zero", "mixed"))
@pytest.mark.parametrize("data_kind", ("random", "zeros", "ones"))
def test_rows_of_every_length_equal_zlib(data_kind, seed_kind):
    data, seeds = rows_of(data_kind), seeds_of(seed_kind)
    got, want = gpu_crc(data, LENS, seeds), want_crc(data, LENS, seeds)
    bad = [(LENS[i], hex(int(got[i])), hex(int(want[i]))) for i in range(len(LENS)) if got[i] != want[i]]
    assert not bad, f"{data_kind} data, {seed_kind} seeds: (length, got, zlib) {bad}"
    if seed_kind != "none":
        assert all(got[i] == seeds[i] for i, n in enumerate(LENS) if n == 0), "a length of 0 gives the seed"


def test_one_row_and_rows_shorter_than_a_word():
    rng = np.random.default_rng(9)
    for pitch in (1, 2, 3, 5, PIECE + 1):
        data = rng.integers(0, 256, (7, pitch), dtype=np.uint8)
        lens = [pitch, 0, 1, pitch - 1, pitch, min(2, pitch), pitch]
        seeds = np.array([IDAT] * 7, dtype=np.uint32)
        assert np.array_equal(gpu_crc(data, lens, seeds), want_crc(data, lens, seeds)), f"pitch {pitch}"
    one = rng.integers(0, 256, (1, 5 * SPAN + 3), dtype=np.uint8)
    assert np.array_equal(gpu_crc(one, [one.shape[1]], None), want_crc(one, [one.shape[1]], None))


def test_lengths_outside_the_row_count_as_its_nearer_end():
    data = rows_of("random")[:4]
    lens = [-1, PITCH + 1, 2 ** 31 - 1, -2 ** 31]
    seeds = np.array([IDAT, 7, 0xFFFFFFFF, 0], dtype=np.uint32)
    got = gpu_crc(data, lens, seeds)
    assert np.array_equal(got, want_crc(data, [0, PITCH, PITCH, 0], seeds))


def test_refusals():
    from vdpp_amd.hip import ops
    data = rows_of("zeros")[:2]
    with pytest.raises(Exception):
        gpu_crc(data, [1, 2], None, ws_short=4)
    d = torch.zeros((2, 8), dtype=torch.uint8, device=DEV)
    ln = torch.zeros(2, dtype=torch.int32, device=DEV)
    ws = torch.empty(ops.crc32_ws_bytes(2, 8), dtype=torch.uint8, device=DEV)
    with pytest.raises(Exception):
        ops.crc32_rows(d, ln, torch.zeros(2, dtype=torch.float32, device=DEV), ws)
    with pytest.raises(Exception):
        ops.crc32_rows(d, ln.long(), torch.zeros(2, dtype=torch.int32, device=DEV), ws)
    with pytest.raises(Exception):
        ops.crc32_rows(d, ln, torch.zeros(1, dtype=torch.int32, device=DEV), ws)
    assert ops.crc32_ws_bytes(0, 8) == 0 and ops.crc32_ws_bytes(2, 0) == 0 and ops.crc32_ws_bytes(2, 2 ** 31) == 0
    assert ops.crc32_ws_bytes(3, SPAN) == 12 and ops.crc32_ws_bytes(3, SPAN + 1) == 24

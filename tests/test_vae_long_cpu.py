"""The query-row block plan of the VAE's mid-block attention above 16,384 tokens per frame
(``models/vae_hip.py::attn_row_blocks``): pure arithmetic, no GPU."""

import pytest

from vdpp_amd.models.vae_hip import ATTN_LONG_FROM, ATTN_SCRATCH_ELEMS, attn_row_blocks

HWS = (256, 768, 9216, 16640, 20736, 36864)


def _caps(hw):
    # from one 256-row block of scratch to the whole [hw][hw] matrix, with values between and off every multiple
    caps = {256 * hw, 256 * hw + 1, 257 * hw, 511 * hw, 512 * hw, 1024 * hw - 1, 1024 * hw, hw * hw // 3, hw * hw - 1, hw * hw}
    return sorted(c for c in caps if 256 * hw <= c <= hw * hw)


@pytest.mark.parametrize("hw", HWS)
def test_blocks_cover_every_row_once_in_order_within_the_cap(hw):
    for cap in _caps(hw):
        r, blocks = attn_row_blocks(hw, cap)
        assert r % 256 == 0 and r >= 256, (hw, cap, r)
        assert r * hw <= cap, (hw, cap, r)
        assert (r + 256) * hw > cap or r >= hw, "R is the largest that fits"
        assert blocks[0][0] == 0 and blocks[-1][1] == hw
        for (a0, a1), (b0, b1) in zip(blocks, blocks[1:]):
            assert a1 == b0, "blocks are contiguous and ordered"
        assert all(0 < r1 - r0 <= r for r0, r1 in blocks)
        assert all(r1 - r0 == r for r0, r1 in blocks[:-1]), "only the last block may be short"
        assert sum(r1 - r0 for r0, r1 in blocks) == hw
        assert all((r1 - r0) % 256 == 0 for r0, r1 in blocks), "hw and R are multiples of 256, so every block is"
    # the whole matrix allowed: one block
    assert attn_row_blocks(hw, hw * hw)[1] == [(0, hw)]


@pytest.mark.parametrize("hw", HWS)
def test_a_cap_below_one_block_forces_256_rows(hw):
    for cap in (1, hw, 256 * hw - 1):
        r, blocks = attn_row_blocks(hw, cap)
        assert r == 256 and blocks == [(r0, r0 + 256) for r0 in range(0, hw, 256)]


def test_default_cap_is_the_native_decodes_matrix():
    assert ATTN_LONG_FROM == 16384 and ATTN_SCRATCH_ELEMS == 9216 * 9216
    r, blocks = attn_row_blocks(20736)
    assert r == 4096 and len(blocks) == 6 and blocks[-1] == (20480, 20736)
    r, blocks = attn_row_blocks(9216)
    assert r == 9216 and blocks == [(0, 9216)]
    r, blocks = attn_row_blocks(36864)
    assert r == 2304 and len(blocks) == 16 and r * 36864 <= ATTN_SCRATCH_ELEMS
    r, blocks = attn_row_blocks(16640)
    assert r == 4864 and [b[1] - b[0] for b in blocks] == [4864, 4864, 4864, 2048]


def test_nonsense_is_refused():
    with pytest.raises(ValueError):
        attn_row_blocks(0, 100)
    with pytest.raises(ValueError):
        attn_row_blocks(256, 0)

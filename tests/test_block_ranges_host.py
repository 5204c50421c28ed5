"""Host arithmetic of the two-range dense blocks (densenet.block_ranges): for every spot count 1..64 on the 4 x 4 and 8 x 8
maps the plan is one range, or two ranges that every launcher takes - never an illegal pair.  The legality rules are restated
here from include/gridnext_hip.h (gnx_dense_block_ranges): whole spots, whole 128-row tiles in both ranges, whole 256-pixel
Winograd tiles in the first range on the 8 x 8 map."""
import pytest

from gridnext_amd.densenet import RANGE_ROWS, block_ranges


def _legal(r0, r1, s):
    return r0 > 0 and r1 > 0 and r0 % (s * s) == 0 and r1 % (s * s) == 0 and r0 % 128 == 0 and r1 % 128 == 0 and \
        (s < 8 or r0 % 256 == 0)


def _round(s, unit_rows):
    """rows of one round: 2 units on the 8 x 8 map, 1 on the 4 x 4 map, in whole groups of 8 spots"""
    r, g = unit_rows * (2 if s == 8 else 1), 8 * s * s
    while r % g:
        r += unit_rows * (2 if s == 8 else 1)
    return r


@pytest.mark.parametrize("s", [4, 8])
def test_every_plan_is_one_range_or_a_legal_pair(s):
    split = 0
    for n in range(1, 65):
        M = n * s * s
        for unit_rows in (128, 512, RANGE_ROWS):
            r0 = block_ranges(n, s, unit_rows)
            rnd = _round(s, unit_rows)
            assert 0 <= r0 < M
            if r0:
                assert _legal(r0, M - r0, s), (n, s, unit_rows, r0)
                assert r0 % rnd == 0 and r0 % (8 * s * s) == 0    # whole rounds, whole groups of 8 spots
                assert r0 <= M - r0 < r0 + 2 * rnd               # as many as fit into half the rows
                split += 1
            else:
                # one range: fewer than two rounds, or a second range that would not be whole 128-row tiles
                assert M < 2 * rnd or (M - M // 2 // rnd * rnd) % 128 != 0, (n, s, unit_rows)
        assert block_ranges(n, s) == 0                          # 64 spots are far below two rounds
    assert split > 0


def test_other_maps_and_the_headline():
    assert all(block_ranges(4096, s, 128) == 0 for s in (2, 7, 14, 16, 32, 64))
    # the benchmark's array after skip_empty, 4 432 or 4 456 spots, and whole, 4 992: two rounds of conv1 / Winograd tiles on the
    # 8 x 8 map, one round of the direct conv2 on the 4 x 4 map - 2 048 spots either way
    for n in (4432, 4456, 4992):
        assert block_ranges(n, 8) == 2048 * 64 == 2 * 65536 and block_ranges(n, 4) == 2048 * 16 == RANGE_ROWS
    # from two rounds on
    assert block_ranges(2048, 8) == 1024 * 64 and block_ranges(2040, 8) == 0
    assert block_ranges(4096, 4) == 2048 * 16 and block_ranges(4088, 4) == 0
    assert block_ranges(3 * 4096, 4) == 3 * RANGE_ROWS and block_ranges(3 * 4096 + 8, 8) == 6 * 65536

"""Host arithmetic of the empty-spot compaction of the DenseNet eval forward (densenet.compacted_spots): how many spots run
for (N, n_fg, chunk), and when the compaction is declined.  No device."""
import pytest

from gridnext_amd.densenet import EMPTY_GRANULE, compacted_spots

G = EMPTY_GRANULE


def brute(N, n_fg, g):
    """The smallest count that holds every non-empty spot and one empty one and is congruent to N modulo g."""
    n = n_fg + 1
    while n % g != N % g:
        n += 1
    return n


def test_granule_is_one_128_row_tile_of_4x4_maps():
    assert G * 4 * 4 == 128


@pytest.mark.parametrize("N", [4992, 304, 301, 4096, 17, 9])
def test_sweep_of_foreground_counts(N):
    """Every n_fg from 0 to N: taken iff the padded count is below N; the count holds n_fg + 1 spots, keeps N's remainder
    modulo the granule (so every launch keeps its kernel class) and wastes less than one granule."""
    taken = 0
    for n_fg in range(0, N + 1):
        n = compacted_spots(N, n_fg, N)
        want = brute(N, n_fg, G) if n_fg < N else None
        if want is not None and want >= N:
            want = None
        assert n == want, (N, n_fg, n, want)
        if n is not None:
            taken += 1
            assert n_fg + 1 <= n < N and n % G == N % G and n - (n_fg + 1) < G
    assert compacted_spots(N, N, N) is None                    # no empty spot: nothing to skip
    assert taken == max(0, N - G)                              # n_fg = 0 .. N - G - 1 leave at least a granule to save


def test_values_around_each_multiple_of_the_granule():
    N = 4992
    for k in range(0, N // G + 1):
        for n_fg in (k * G - 2, k * G - 1, k * G, k * G + 1):
            if not 0 <= n_fg <= N:
                continue
            n = compacted_spots(N, n_fg, N)
            # n_fg = 8k - 1 plus the one empty spot is exactly k granules; n_fg = 8k needs k + 1 of them
            want = ((n_fg + 1 + G - 1) // G) * G
            assert n == (want if want < N else None), (n_fg, n, want)
    assert compacted_spots(N, 0, N) == G                       # all empty: one granule of empty spots
    assert compacted_spots(N, 4429, N) == 4432 and compacted_spots(N, 4449, N) == 4456      # the benchmark's two arrays
    assert compacted_spots(N, N - G - 1, N) == N - G and compacted_spots(N, N - G, N) is None


def test_declined_where_the_uncompacted_call_mixes_kernel_classes():
    """Chunked calls: taken when every chunk of the uncompacted call holds whole granules (so do the compacted chunks);
    declined when its chunks are ragged, or whole with a ragged rest - rows would change kernel class."""
    assert compacted_spots(4992, 4000, 1000) == 4008           # 8 | 1000, 8 | 4992
    assert compacted_spots(4992, 4000, 1001) is None           # ragged chunks
    assert compacted_spots(4990, 4000, 1000) is None           # whole chunks, ragged rest
    assert compacted_spots(4990, 4000, 4990) == 4006           # one chunk: 4006 = 4990 (mod 8), the class is kept
    assert compacted_spots(4990, 4000, 6000) == 4006


def test_other_granules():
    for g in (1, 2, 128):
        for N in (g * 5, g * 5 + 3):
            for n_fg in range(0, N + 1):
                n = compacted_spots(N, n_fg, N, g)
                want = brute(N, n_fg, g) if n_fg < N else N
                assert n == (want if want < N else None)

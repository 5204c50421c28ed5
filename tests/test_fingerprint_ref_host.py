"""tests/fingerprint_ref.py - the numpy restatement of the content fingerprint of include/gridnext_hip.h - on the host:
known answers, and the properties the row cache relies on (length-, order- and bit-sensitivity).  No GPU."""
import numpy as np

import fingerprint_ref as R

# (bytes, lane 0, lane 1).  The empty buffer's lane 0 is mix(K0; M1, M2): the first output of splitmix64 seeded with 0,
# 0xE220A8397B1DCDAF in every published table of that generator - an anchor from outside this repository.  The others were
# worked out with the plain-integer restatement (fingerprint128_int) and are pinned here.
KNOWN = [
    (b'', 0xE220A8397B1DCDAF, 0xEB1A588FDEE91CD7),
    (b'\0', 0xB382A305F4414F5E, 0xCAE0479D1DA90B22),
    (b'a', 0x7BC8EE98091BBDD8, 0x1624641BB4797105),
    (b'gridnext', 0x13D4A51B630CE300, 0x2201F100B773E4AA),
    (b'gridnext!', 0x36FEA20D2793B7DB, 0xC7C4DF25C2314CAB),
    (bytes(range(17)), 0xD2387A1C14C717CB, 0x991C2A68638B92E6),
    (bytes(range(256)) * 3 + b'xyz', 0x86E5F0BE16036DBB, 0x87A13361A4569210),
]


def test_known_answers():
    for data, f0, f1 in KNOWN:
        assert R.fingerprint128(data) == (f0, f1), len(data)
        assert R.fingerprint128_int(data) == (f0, f1), len(data)


def test_numpy_and_integer_restatements_agree_on_random_buffers():
    rng = np.random.default_rng(3)
    for n in (2, 15, 16, 31, 1000, 4097):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert R.fingerprint128(data) == R.fingerprint128_int(data)


def test_zero_buffers_of_lengths_0_to_17_are_all_distinct():
    """Background spots are zero-filled: the value must still depend on the length (1 .. 8 zero bytes are the same single
    zero word, 9 .. 16 the same two)."""
    fps = [R.fingerprint128(bytes(n)) for n in range(18)]
    assert len(set(fps)) == 18
    assert len(set(f[0] for f in fps)) == 18 and len(set(f[1] for f in fps)) == 18


def test_swapping_two_unequal_words_changes_both_lanes():
    rng = np.random.default_rng(4)
    w = rng.integers(0, 2 ** 63, 64, dtype=np.uint64)
    base = R.fingerprint128(w.tobytes())
    for i, j in ((0, 1), (0, 63), (17, 40), (62, 63)):
        assert w[i] != w[j]
        v = w.copy()
        v[i], v[j] = w[j], w[i]
        got = R.fingerprint128(v.tobytes())
        assert got[0] != base[0] and got[1] != base[1], (i, j)
    # a buffer of two different words against its reverse, the smallest case
    assert R.fingerprint128(b'A' * 8 + b'B' * 8) != R.fingerprint128(b'B' * 8 + b'A' * 8)


def test_single_flipped_bit_changes_the_value_at_4096_positions():
    """64 KiB of random bytes; one bit flipped at 4 096 random positions: every flip changes BOTH lanes (mix is a bijection,
    so the one changed term differs in each sum) and no two flips collide.  The sums are updated term by term from the
    restatement's own pieces, and a sample of the flips is checked against the whole function."""
    rng = np.random.default_rng(5)
    buf = rng.integers(0, 256, 65536, dtype=np.uint8)
    base = R.fingerprint128(buf.tobytes())
    w = R.words(buf.tobytes())
    pos = np.arange(1, len(w) + 1, dtype=np.uint64)
    n1 = np.uint64(len(buf) + 1)
    with np.errstate(over='ignore'):
        t0, t1 = R.mix(w ^ (pos * R.K0), R.M1, R.M2), R.mix(w ^ (pos * R.K1), R.M2, R.M1)
        s0, s1 = np.sum(t0, dtype=np.uint64), np.sum(t1, dtype=np.uint64)
        bits = rng.choice(65536 * 8, 4096, replace=False)
        seen = set()
        for k, bit in enumerate(bits):
            i, b = int(bit) // 64, np.uint64(int(bit) % 64)
            wi = w[i] ^ (np.uint64(1) << b)
            n0 = s0 - t0[i] + R.mix(wi ^ (pos[i] * R.K0), R.M1, R.M2)
            n1_ = s1 - t1[i] + R.mix(wi ^ (pos[i] * R.K1), R.M2, R.M1)
            got = (int(R.mix(n0 + n1 * R.K0, R.M1, R.M2)), int(R.mix(n1_ + n1 * R.K1, R.M2, R.M1)))
            assert got[0] != base[0] and got[1] != base[1], bit
            seen.add(got)
            if k % 256 == 0:                                   # the shortcut is the function: 16 whole evaluations
                flipped = buf.copy()
                flipped[int(bit) // 8] ^= np.uint8(1 << (int(bit) % 8))
                assert R.fingerprint128(flipped.tobytes()) == got
        assert len(seen) == 4096

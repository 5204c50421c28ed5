"""The 128-bit content fingerprint of include/gridnext_hip.h ("content fingerprint"), restated in numpy uint64 from the
header's formulas alone (test_fingerprint_ref_host.py pins it to known answers; test_gpu_fcache.py holds the kernel to it
bit for bit).  All arithmetic wraps modulo 2^64, as numpy's uint64 does."""
import numpy as np

K0, K1 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xC2B2AE3D27D4EB4F)
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def mix(x, a, b):
    """splitmix64's finalizer with multipliers (a, b) on a uint64 array."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over='ignore'):
        x = (x ^ (x >> np.uint64(30))) * a
        x = (x ^ (x >> np.uint64(27))) * b
        return x ^ (x >> np.uint64(31))


def words(data):
    """The little-endian 64-bit words of a bytes-like object, the last one zero-padded."""
    data = bytes(data)
    pad = (-len(data)) % 8
    return np.frombuffer(data + b'\0' * pad, dtype='<u8').astype(np.uint64)


def fingerprint128(data):
    """(lane 0, lane 1) of the bytes `data` as Python ints."""
    data = bytes(data)
    n = np.uint64(len(data))
    w = words(data)
    pos = np.arange(1, len(w) + 1, dtype=np.uint64)
    with np.errstate(over='ignore'):
        s0 = np.sum(mix(w ^ (pos * K0), M1, M2), dtype=np.uint64)
        s1 = np.sum(mix(w ^ (pos * K1), M2, M1), dtype=np.uint64)
        one = np.uint64(1)
        f0 = mix(np.array([s0 + (n + one) * K0], dtype=np.uint64), M1, M2)[0]
        f1 = mix(np.array([s1 + (n + one) * K1], dtype=np.uint64), M2, M1)[0]
    return int(f0), int(f1)


def fingerprint128_int(data):
    """The same function in plain Python integers (an independent second restatement, for the known-answer test)."""
    mask = (1 << 64) - 1

    def mx(x, a, b):
        x = ((x ^ (x >> 30)) * a) & mask
        x = ((x ^ (x >> 27)) * b) & mask
        return x ^ (x >> 31)
    data = bytes(data)
    k0, k1, m1, m2 = int(K0), int(K1), int(M1), int(M2)
    s0 = s1 = 0
    for i in range((len(data) + 7) // 8):
        w = int.from_bytes(data[8 * i:8 * i + 8].ljust(8, b'\0'), 'little')
        s0 = (s0 + mx(w ^ (((i + 1) * k0) & mask), m1, m2)) & mask
        s1 = (s1 + mx(w ^ (((i + 1) * k1) & mask), m2, m1)) & mask
    n = len(data)
    return mx((s0 + (n + 1) * k0) & mask, m1, m2), mx((s1 + (n + 1) * k1) & mask, m2, m1)

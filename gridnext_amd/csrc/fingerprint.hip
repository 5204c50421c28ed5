// 128-bit content fingerprints of back-to-back byte segments of a device buffer (include/gridnext_hip.h: "Content
// fingerprint" states the function; tests/fingerprint_ref.py restates it in numpy).  A frozen spot classifier maps equal
// arrays to equal rows, so the grid models key their row cache (gridnext_amd/fcache.py) on this value instead of running
// f again; on a cached step this read of the array is the only large device work left, so it is a streaming kernel:
//   * one aligned 16-byte load per thread and pair of words, FP_UNR of them in flight per thread;
//   * a segment is cut into up to FP_MAX_BLOCKS contiguous parts, one workgroup each (one 285 MB array: 2 048 workgroups
//     of ~139 KB), or many segments take one workgroup each (a grid split over segments);
//   * each lane of the fingerprint is a sum modulo 2^64 of per-word terms: any split and any order of the partial sums
//     gives the same bits.  Parts are summed by a second, tiny kernel out of a workspace (plain stores, no atomics).
// The start of a segment may sit at any byte: loads stay 16-byte aligned and the words are cut out of two neighbouring
// pieces with a funnel shift; the (at most two) pieces of a segment that reach outside it are read byte by byte, so no
// byte outside [base, base + n_seg * seg_bytes) is ever touched and the bytes past a segment's end count as zero.
#include "common.h"

namespace {

constexpr int FP_THREADS = 256;
constexpr int FP_UNR = 4;                        // pairs of words per thread in flight
constexpr uint64_t FP_SPLIT_BYTES = 32768;       // one workgroup's share of a segment (gnx_fingerprint128_split_bytes)
constexpr int FP_MAX_BLOCKS = 2048;              // 256 CUs x 8 workgroups

constexpr uint64_t FP_K0 = 0x9E3779B97F4A7C15ull, FP_K1 = 0xC2B2AE3D27D4EB4Full;   // position strides of lane 0 / lane 1
constexpr uint64_t FP_M1 = 0xBF58476D1CE4E5B9ull, FP_M2 = 0x94D049BB133111EBull;   // the multipliers of splitmix64

// splitmix64's finalizer with multipliers (a, b): a bijection of the 64-bit words
__host__ __device__ __forceinline__ uint64_t fp_mix(uint64_t x, uint64_t a, uint64_t b) {
    x ^= x >> 30; x *= a;
    x ^= x >> 27; x *= b;
    x ^= x >> 31;
    return x;
}

// 16-byte piece `j` of the aligned address `a0 + 16 j`; bytes outside [lo, hi) read as zero and are not loaded
__host__ __device__ __forceinline__ uint4 fp_piece(const unsigned char* a0, uint64_t j, const unsigned char* lo, const unsigned char* hi) {
    const unsigned char* p = a0 + 16 * j;
    if (p >= lo && p + 16 <= hi) return *reinterpret_cast<const uint4*>(p);
    unsigned v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < 16; ++b)
        if (p + b >= lo && p + b < hi) v[b >> 2] |= (unsigned)p[b] << (8 * (b & 3));
    return make_uint4(v[0], v[1], v[2], v[3]);
}

__host__ __device__ __forceinline__ uint64_t fp_u64(unsigned lo, unsigned hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }

// One thread's share of both lanes' sums over the pairs [p0, p1) of one segment (pair t = words 2t and 2t + 1): the pairs
// p0 + tid, p0 + tid + FP_THREADS, ...  (Host-callable, so that a host build can walk it under a sanitizer.)
__host__ __device__ __forceinline__ void fp_thread_sums(const unsigned char* seg, uint64_t n_bytes, uint64_t p0, uint64_t p1,
                                                        unsigned tid, uint64_t& s0, uint64_t& s1) {
    const unsigned r = (unsigned)(reinterpret_cast<uintptr_t>(seg) & 15);      // uniform in the workgroup
    const unsigned char* a0 = seg - r;
    const unsigned char* end = seg + n_bytes;
    const uint64_t n_words = (n_bytes + 7) / 8;
    const unsigned sh = 8 * (r & 7);
    for (uint64_t base = p0 + tid; base < p1; base += (uint64_t)FP_THREADS * FP_UNR) {
        uint4 c0[FP_UNR], c1[FP_UNR];
#pragma unroll
        for (int u = 0; u < FP_UNR; ++u) {                     // every load of the round first
            const uint64_t t = base + (uint64_t)u * FP_THREADS;
            c0[u] = c1[u] = make_uint4(0u, 0u, 0u, 0u);
            if (t < p1) {
                c0[u] = fp_piece(a0, t, seg, end);
                if (r != 0) c1[u] = fp_piece(a0, t + 1, seg, end);
            }
        }
#pragma unroll
        for (int u = 0; u < FP_UNR; ++u) {
            const uint64_t t = base + (uint64_t)u * FP_THREADS;
            if (t < p1) {
                uint64_t q0 = fp_u64(c0[u].x, c0[u].y), q1 = fp_u64(c0[u].z, c0[u].w), q2 = fp_u64(c1[u].x, c1[u].y);
                if (r >= 8) { q0 = q1; q1 = q2; q2 = fp_u64(c1[u].z, c1[u].w); }
                const uint64_t wa = sh ? (q0 >> sh) | (q1 << (64 - sh)) : q0;
                const uint64_t wb = sh ? (q1 >> sh) | (q2 << (64 - sh)) : q1;
                const uint64_t ia = 2 * t + 1;                 // word index + 1
                s0 += fp_mix(wa ^ (ia * FP_K0), FP_M1, FP_M2);
                s1 += fp_mix(wa ^ (ia * FP_K1), FP_M2, FP_M1);
                if (2 * t + 1 < n_words) {
                    s0 += fp_mix(wb ^ ((ia + 1) * FP_K0), FP_M1, FP_M2);
                    s1 += fp_mix(wb ^ ((ia + 1) * FP_K1), FP_M2, FP_M1);
                }
            }
        }
    }
}

// Sums of both lanes over the pairs [p0, p1) of one segment, whole workgroup; the result is valid in thread 0.
__device__ __forceinline__ void fp_block_sums(const unsigned char* seg, uint64_t n_bytes, uint64_t p0, uint64_t p1,
                                              uint64_t& s0_out, uint64_t& s1_out) {
    __shared__ uint64_t red[2][FP_THREADS / 64];
    uint64_t s0 = 0, s1 = 0;
    fp_thread_sums(seg, n_bytes, p0, p1, threadIdx.x, s0, s1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor((unsigned long long)s0, o, 64);
        s1 += __shfl_xor((unsigned long long)s1, o, 64);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[0][wid] = s0; red[1][wid] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        s0 = s1 = 0;
        for (int w = 0; w < FP_THREADS / 64; ++w) { s0 += red[0][w]; s1 += red[1][w]; }
        s0_out = s0;
        s1_out = s1;
    }
}

// the length goes in last: a segment of zeros still depends on how long it is
__device__ __forceinline__ void fp_finish(uint64_t s0, uint64_t s1, uint64_t n_bytes, uint64_t* out) {
    out[0] = fp_mix(s0 + (n_bytes + 1) * FP_K0, FP_M1, FP_M2);
    out[1] = fp_mix(s1 + (n_bytes + 1) * FP_K1, FP_M2, FP_M1);
}

// parts == 1: one workgroup per segment writes the fingerprint.  parts > 1: workgroup (segment, part) writes its two
// sums to ws[segment][part][2] and fingerprint_combine_kernel finishes.
__global__ __launch_bounds__(FP_THREADS) void fingerprint_kernel(const unsigned char* __restrict__ base, uint64_t seg_bytes,
                                                                 int parts, uint64_t pairs_per_part,
                                                                 uint64_t* __restrict__ out, uint64_t* __restrict__ ws) {
    const uint64_t seg = blockIdx.x / (unsigned)parts, part = blockIdx.x % (unsigned)parts;
    const uint64_t n_pairs = (seg_bytes + 15) / 16;
    uint64_t p0 = part * pairs_per_part, p1 = p0 + pairs_per_part;
    if (p0 > n_pairs) p0 = n_pairs;
    if (p1 > n_pairs) p1 = n_pairs;
    uint64_t s0 = 0, s1 = 0;
    fp_block_sums(base + seg * seg_bytes, seg_bytes, p0, p1, s0, s1);
    if (threadIdx.x == 0) {
        if (parts == 1) fp_finish(s0, s1, seg_bytes, out + 2 * seg);
        else { ws[2 * blockIdx.x] = s0; ws[2 * blockIdx.x + 1] = s1; }
    }
}

__global__ __launch_bounds__(64) void fingerprint_combine_kernel(const uint64_t* __restrict__ ws, int parts, uint64_t seg_bytes,
                                                                 uint64_t* __restrict__ out) {
    const uint64_t seg = blockIdx.x;
    uint64_t s0 = 0, s1 = 0;
    for (int p = threadIdx.x; p < parts; p += 64) {
        s0 += ws[2 * (seg * parts + p)];
        s1 += ws[2 * (seg * parts + p) + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor((unsigned long long)s0, o, 64);
        s1 += __shfl_xor((unsigned long long)s1, o, 64);
    }
    if (threadIdx.x == 0) fp_finish(s0, s1, seg_bytes, out + 2 * seg);
}

// workgroups per segment: FP_SPLIT_BYTES each, as many as keep the whole grid within FP_MAX_BLOCKS
int fp_parts(uint64_t seg_bytes, int n_seg) {
    uint64_t parts = (seg_bytes + FP_SPLIT_BYTES - 1) / FP_SPLIT_BYTES;
    const uint64_t room = n_seg >= FP_MAX_BLOCKS ? 1 : (uint64_t)(FP_MAX_BLOCKS / n_seg);
    if (parts > room) parts = room;
    return parts < 1 ? 1 : (int)parts;
}

}  // namespace

// Largest segment the one-kernel form takes whatever n_seg is; longer segments are cut into parts while the grid has room.
GNX_EXPORT long gnx_fingerprint128_split_bytes() { return (long)FP_SPLIT_BYTES; }

// Bytes of workspace gnx_fingerprint128_batch needs for these arguments: 0 in the one-kernel form.
GNX_EXPORT long gnx_fingerprint128_batch_workspace(size_t seg_bytes, int n_seg) {
    if (n_seg <= 0) return 0;
    const int parts = fp_parts(seg_bytes, n_seg);
    return parts == 1 ? 0 : (long)n_seg * parts * 16;
}

GNX_EXPORT int gnx_fingerprint128_batch(const void* base, size_t seg_bytes, int n_seg, uint64_t* out, void* workspace,
                                        hipStream_t stream) {
    if (n_seg < 0 || (n_seg > 0 && !out) || (n_seg > 0 && seg_bytes > 0 && !base)) return GNX_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(out) & 7) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return GNX_ERR_BAD_ARG;
    if (n_seg == 0) return GNX_OK;
    const int parts = fp_parts(seg_bytes, n_seg);
    if (parts > 1 && !workspace) return GNX_ERR_BAD_ARG;
    if ((uint64_t)n_seg * (uint64_t)parts > 2147483647ull) return GNX_ERR_UNSUPPORTED;
    const uint64_t n_pairs = (seg_bytes + 15) / 16;
    const uint64_t per_part = (n_pairs + parts - 1) / parts;
    fingerprint_kernel<<<(unsigned)(n_seg * parts), FP_THREADS, 0, stream>>>(
        static_cast<const unsigned char*>(base), seg_bytes, parts, per_part, out, static_cast<uint64_t*>(workspace));
    if (parts > 1)
        fingerprint_combine_kernel<<<(unsigned)n_seg, 64, 0, stream>>>(static_cast<const uint64_t*>(workspace), parts, seg_bytes, out);
    return gnx_launch_status();
}

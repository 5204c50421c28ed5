// Colour-cast removal of a resident whole-slide image (the reference's remove_color_cast / scale_rgb, imgprocess.py:49-67:
// np.percentile(channel, q=99) of the WHOLE slide per channel, then Image.point(i -> i * 255 / p) on every byte).  On the
// device that is two streaming passes over the interleaved uint8 [n_pixels][3] bytes: a 3 x 256 histogram, from which the host
// takes the percentiles and builds Pillow's table clip(round(i * scale), 0, 255), and a 3 x 256 table lookup.  Both are
// integer-only, so the result is numpy's and Pillow's bit for bit.
//
// The unit of work is 48 bytes: a 16-byte load holds no whole number of pixels, three of them hold 16.  The byte at offset o of
// the image belongs to channel o % 3; behind a bytewise head that ends at the first 16-byte boundary every unit starts at the
// same channel phase (head % 3), so the channel of each of a unit's 48 bytes is fixed for the launch.  Head and tail (under 16
// and under 48 bytes) are handled byte by byte by workgroup 0; no byte outside the image is read or written.
//
// Histogram.  A workgroup keeps CC_COPIES interleaved copies of the 3 x 256 counters in the LDS (counter (c, v), copy k at
// [(c * 256 + v) * CC_COPIES + k]: the copies of one counter lie in different banks) and a lane adds into copy lane % CC_COPIES.
// A slide is mostly one background value, so before the LDS add a thread folds runs of equal bytes of one channel among its
// 16 pixels into one add: a constant image costs 3 LDS adds per thread and unit, a random one 48.  The 32-bit counters are
// folded into 64-bit registers (three counters per thread) every CC_FLUSH_PASSES passes - a counter holds at most
// CC_FLUSH_PASSES * 4096 + 62 by then - and each workgroup stores its 768 64-bit partial sums as one slab of the workspace;
// a second, small kernel sums the slabs into hist (plain stores: hist is overwritten, every word of the workspace that is read
// was written by the same call, and integer sums do not depend on the split or its order).
//
// Lookup.  The table sits in the LDS as 768 bytes.  Units are aligned on dst (dwordx4 stores); the source bytes of a unit come
// from aligned dwordx4 loads too, cut out of up to four neighbouring pieces with a funnel shift when src and dst differ
// modulo 16.  The at most two units whose outer pieces would reach outside the source take byte loads.  dst == src (in place)
// is allowed: every thread then reads exactly the bytes it writes.  Ranges that overlap otherwise are refused.
#include "common.h"

namespace {

constexpr int CC_THREADS = 256;
constexpr int CC_UNIT = 48;                      // bytes: 16 pixels, three 16-byte loads
constexpr int CC_UNIT_PIXELS = CC_UNIT / 3;
constexpr int CC_COPIES = 8;                     // copies of each LDS counter: 3 * 256 * 8 * 4 B = 24 KB, 6 workgroups per CU
constexpr int CC_HIST_BLOCKS = 1536;             // 256 CUs x 6 resident workgroups
constexpr int CC_FLUSH_PASSES = 64;              // passes between two folds of the 32-bit counters into 64 bits
constexpr int CC_LUT_BLOCKS = 2048;              // 256 CUs x 8 workgroups
constexpr int CC_BINS = 3 * 256;

// byte j (a compile-time constant at every call) of the 48 bytes of a unit
__device__ __forceinline__ unsigned cc_byte(const uint4 (&p)[3], int j) {
    const uint4& q = p[j >> 4];
    const int d = (j >> 2) & 3;
    const unsigned v = d == 0 ? q.x : d == 1 ? q.y : d == 2 ? q.z : q.w;
    return (v >> (8 * (j & 3))) & 255u;
}

// n_bytes = 3 n_pixels; head = bytes in front of the first 16-byte boundary (<= n_bytes); n_units whole units behind it.
__global__ __launch_bounds__(CC_THREADS) void cc_hist_kernel(const uint8_t* __restrict__ img, uint64_t n_bytes, uint64_t head,
                                                             uint64_t n_units, uint64_t* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) uint32_t cnt[CC_BINS * CC_COPIES];
    const unsigned tid = threadIdx.x, copy = tid & (CC_COPIES - 1);
    for (int i = tid; i < CC_BINS * CC_COPIES; i += CC_THREADS) cnt[i] = 0u;
    uint64_t acc[3] = {0, 0, 0};                 // the counters tid, tid + 256, tid + 512 of [3][256]
    __syncthreads();

    if (blockIdx.x == 0) {                       // ragged head and tail, byte by byte
        for (uint64_t o = tid; o < head; o += CC_THREADS)
            atomicAdd(&cnt[((unsigned)(o % 3) * 256 + img[o]) * CC_COPIES + copy], 1u);
        for (uint64_t o = head + n_units * CC_UNIT + tid; o < n_bytes; o += CC_THREADS)
            atomicAdd(&cnt[((unsigned)(o % 3) * 256 + img[o]) * CC_COPIES + copy], 1u);
    }

    const unsigned ph = (unsigned)(head % 3);    // channel of byte 0 of every unit
    uint32_t* tbl[3];                            // tbl[s]: the counters of the channel of a unit's bytes s, s + 3, s + 6, ...
#pragma unroll
    for (int s = 0; s < 3; ++s) tbl[s] = cnt + ((ph + s) % 3) * 256 * CC_COPIES + copy;
    const uint8_t* mid = img + head;             // 16-byte aligned

    int passes = 0;
    for (uint64_t p = blockIdx.x; p * CC_THREADS < n_units; p += gridDim.x) {        // p: the same in the whole workgroup
        const uint64_t u = p * CC_THREADS + tid;
        if (u < n_units) {
            const uint4* src = reinterpret_cast<const uint4*>(mid + u * CC_UNIT);
            uint4 v[3];
            v[0] = src[0];
            v[1] = src[1];
            v[2] = src[2];
#pragma unroll
            for (int s = 0; s < 3; ++s) {        // one channel: bytes s, s + 3, ..., s + 45; runs of equal bytes are one add
                unsigned cur = cc_byte(v, s), run = 1;
#pragma unroll
                for (int j = s + 3; j < CC_UNIT; j += 3) {
                    const unsigned b = cc_byte(v, j);
                    if (b != cur) {
                        atomicAdd(&tbl[s][cur * CC_COPIES], run);
                        cur = b;
                        run = 0;
                    }
                    ++run;
                }
                atomicAdd(&tbl[s][cur * CC_COPIES], run);
            }
        }
        if (++passes == CC_FLUSH_PASSES) {       // fold before a 32-bit counter can wrap
            passes = 0;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                uint4* c4 = reinterpret_cast<uint4*>(cnt + (tid + k * CC_THREADS) * CC_COPIES);
                const uint4 a = c4[0], b = c4[1];
                acc[k] += (uint64_t)a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
                c4[0] = c4[1] = make_uint4(0u, 0u, 0u, 0u);
            }
            __syncthreads();
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint4* c4 = reinterpret_cast<const uint4*>(cnt + (tid + k * CC_THREADS) * CC_COPIES);
        const uint4 a = c4[0], b = c4[1];
        acc[k] += (uint64_t)a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
        ws[(uint64_t)blockIdx.x * CC_BINS + tid + k * CC_THREADS] = acc[k];
    }
}

// hist[b] = sum over the slabs of ws[slab][b]; workgroup g owns the 16 counters 16 g .. 16 g + 15, 16 threads per counter.
__global__ __launch_bounds__(CC_THREADS) void cc_hist_sum_kernel(const uint64_t* __restrict__ ws, int slabs,
                                                                 uint64_t* __restrict__ hist) {
    __shared__ uint64_t red[CC_THREADS];
    const int tid = threadIdx.x, bin = blockIdx.x * 16 + (tid & 15);
    uint64_t s = 0;
    for (int g = tid >> 4; g < slabs; g += CC_THREADS / 16) s += ws[(uint64_t)g * CC_BINS + bin];
    red[tid] = s;
    __syncthreads();
    if (tid < 16) {
        for (int k = 1; k < CC_THREADS / 16; ++k) s += red[tid + 16 * k];
        hist[bin] = s;
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_lut_kernel(const uint8_t* src, uint8_t* dst, uint64_t n_bytes, uint64_t head,
                                                            uint64_t n_units, const uint8_t* __restrict__ lut) {
    __shared__ uint8_t tab[CC_BINS];
    const unsigned tid = threadIdx.x;
    for (int i = tid; i < CC_BINS; i += CC_THREADS) tab[i] = lut[i];
    __syncthreads();

    if (blockIdx.x == 0) {                       // ragged head and tail: each byte is read and written by one thread
        for (uint64_t o = tid; o < head; o += CC_THREADS) dst[o] = tab[(unsigned)(o % 3) * 256 + src[o]];
        for (uint64_t o = head + n_units * CC_UNIT + tid; o < n_bytes; o += CC_THREADS)
            dst[o] = tab[(unsigned)(o % 3) * 256 + src[o]];
    }

    const unsigned ph = (unsigned)(head % 3);
    const uint8_t* t[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) t[s] = tab + ((ph + s) % 3) * 256;
    const unsigned r = (unsigned)(reinterpret_cast<uintptr_t>(src + head) & 15);     // src against dst modulo 16: uniform
    const unsigned sh = 8 * (r & 7);

    for (uint64_t u = (uint64_t)blockIdx.x * CC_THREADS + tid; u < n_units; u += (uint64_t)gridDim.x * CC_THREADS) {
        const uint64_t off = head + u * CC_UNIT;
        uint64_t w[6];                           // the unit's 48 source bytes
        if (r == 0) {
            const uint4* p = reinterpret_cast<const uint4*>(src + off);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint4 q = p[k];
                w[2 * k] = (uint64_t)q.x | ((uint64_t)q.y << 32);
                w[2 * k + 1] = (uint64_t)q.z | ((uint64_t)q.w << 32);
            }
        } else if (off >= r && off - r + 64 <= n_bytes) {      // the four aligned pieces around it lie inside the source
            const uint4* p = reinterpret_cast<const uint4*>(src + off - r);
            uint64_t q[9];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint4 v = p[k];
                q[2 * k] = (uint64_t)v.x | ((uint64_t)v.y << 32);
                q[2 * k + 1] = (uint64_t)v.z | ((uint64_t)v.w << 32);
            }
            q[8] = 0;
            if (r >= 8) {
#pragma unroll
                for (int k = 0; k < 8; ++k) q[k] = q[k + 1];
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) w[k] = sh ? (q[k] >> sh) | (q[k + 1] << (64 - sh)) : q[k];
        } else {                                 // a unit at either end of the source: byte loads
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                uint64_t x = 0;
#pragma unroll
                for (int b = 0; b < 8; ++b) x |= (uint64_t)src[off + 8 * k + b] << (8 * b);
                w[k] = x;
            }
        }
        uint32_t o32[12];
#pragma unroll
        for (int d = 0; d < 12; ++d) {
            const uint32_t x = (uint32_t)(w[d >> 1] >> (32 * (d & 1)));
            uint32_t y = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) y |= (uint32_t)t[(4 * d + b) % 3][(x >> (8 * b)) & 255u] << (8 * b);
            o32[d] = y;
        }
        uint4* out = reinterpret_cast<uint4*>(dst + off);
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = make_uint4(o32[4 * k], o32[4 * k + 1], o32[4 * k + 2], o32[4 * k + 3]);
    }
}

// bytes in front of the first 16-byte boundary at or behind p, at most n_bytes
uint64_t cc_head(const void* p, uint64_t n_bytes) {
    const uint64_t h = (16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15;
    return h < n_bytes ? h : n_bytes;
}

// workgroups of the histogram for an image of n_pixels, whatever its alignment (a function of n_pixels alone: it sizes the
// workspace); a workgroup without units still stores its slab
int cc_hist_blocks(uint64_t n_pixels) {
    const uint64_t per_pass = (uint64_t)CC_THREADS * CC_UNIT_PIXELS;
    const uint64_t b = (n_pixels + per_pass - 1) / per_pass;
    return b > (uint64_t)CC_HIST_BLOCKS ? CC_HIST_BLOCKS : (int)b;
}

}  // namespace

// Bytes of workspace gnx_rgb_hist_u8 needs for an image of n_pixels: one slab of 768 64-bit sums per workgroup.
GNX_EXPORT long gnx_rgb_hist_u8_workspace(size_t n_pixels) { return (long)cc_hist_blocks(n_pixels) * CC_BINS * 8; }

GNX_EXPORT int gnx_rgb_hist_u8(const uint8_t* img, size_t n_pixels, uint64_t* hist, void* workspace, hipStream_t stream) {
    if (!hist || (reinterpret_cast<uintptr_t>(hist) & 7) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0)
        return GNX_ERR_BAD_ARG;
    if (n_pixels > 0 && (!img || !workspace)) return GNX_ERR_BAD_ARG;
    if (n_pixels > (size_t)1 << 60) return GNX_ERR_UNSUPPORTED;
    const int blocks = cc_hist_blocks(n_pixels);
    if (blocks > 0) {
        const uint64_t n_bytes = 3 * (uint64_t)n_pixels, head = cc_head(img, n_bytes);
        cc_hist_kernel<<<(unsigned)blocks, CC_THREADS, 0, stream>>>(img, n_bytes, head, (n_bytes - head) / CC_UNIT,
                                                                    static_cast<uint64_t*>(workspace));
    }
    cc_hist_sum_kernel<<<CC_BINS / 16, CC_THREADS, 0, stream>>>(static_cast<const uint64_t*>(workspace), blocks, hist);
    return gnx_launch_status();
}

GNX_EXPORT int gnx_rgb_lut_u8(const uint8_t* src, uint8_t* dst, size_t n_pixels, const uint8_t* lut, hipStream_t stream) {
    if (n_pixels > (size_t)1 << 60) return GNX_ERR_UNSUPPORTED;
    if (n_pixels == 0) return GNX_OK;
    if (!src || !dst || !lut) return GNX_ERR_BAD_ARG;
    const uint64_t n_bytes = 3 * (uint64_t)n_pixels;
    const uintptr_t s = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
    if (s != d && s < d + n_bytes && d < s + n_bytes) return GNX_ERR_BAD_ARG;      // overlapping without being equal
    const uint64_t head = cc_head(dst, n_bytes), n_units = (n_bytes - head) / CC_UNIT;
    uint64_t blocks = (n_units + CC_THREADS - 1) / CC_THREADS;
    blocks = blocks < 1 ? 1 : (blocks > (uint64_t)CC_LUT_BLOCKS ? CC_LUT_BLOCKS : blocks);
    cc_lut_kernel<<<(unsigned)blocks, CC_THREADS, 0, stream>>>(src, dst, n_bytes, head, n_units, lut);
    return gnx_launch_status();
}

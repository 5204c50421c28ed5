// Pillow's two-pass fixed-point resampling of 8-bit channels, stated once for the kernels that run it (resize.hip: bilinear on
// planar patches; wsi_patches.hip: bicubic on windows of an interleaved slide).  Per axis a table of int32 coefficients
// k = (int)(+-0.5 + w 2^22) and bounds {first tap, taps} per output index (gridnext_amd/transforms.py: axis_tables); a pass is
// clip((2^21 + sum pixel k) >> 22, 0, 255) with signed k; the horizontal pass runs first and writes BYTES into an LDS image
// of dwords, 4 output bytes each; the vertical pass runs on those bytes, 4 outputs per thread.  Integer-only, so the bytes
// are Pillow's bit for bit.  A workgroup is RU_THREADS lanes: tx = t & 63 walks the dword columns, ty = t >> 6 the rows.
// Every table entry goes through ru_bounds before it is used as an address, so a wrong table gives wrong bytes, never an
// access outside the tensors.  What is NOT here is what differs: which bytes a tile stages and where they lie (the callers'
// indexing), the LDS layout and its size rule, the launch.
#pragma once
#include "fwd_common.h"

namespace {

constexpr int RU_THREADS = 256;
constexpr int RU_PREC = 22;            // Pillow's PRECISION_BITS for 8-bit channels
constexpr int RU_ROUND = 1 << (RU_PREC - 1);   // what an accumulator starts at
constexpr int RU_MAX_KSIZE = 17;       // bilinear reductions up to 8x per axis, bicubic ones up to 4x
constexpr int RU_LDS_SOFT = 40 * 1024; // tile choice: several workgroups per CU
constexpr int RU_LDS_HARD = 160 * 1024;

__device__ __forceinline__ int ru_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int ru_clip8(int acc) { return ru_clamp(acc >> RU_PREC, 0, 255); }

// Stage the byte run [g, g + nbytes) at lds + (address of g modulo 16), which is returned: 16-B loads for the aligned middle
// of the run, byte loads for its ragged head and tail.  `lds` is 16-B aligned with room for nbytes + 15; lane of NL lanes.
template <int NL>
__device__ __forceinline__ int ru_stage(uint8_t* lds, const uint8_t* __restrict__ g, int nbytes, int lane) {
    const int head = (int)(reinterpret_cast<uintptr_t>(g) & 15);
    uint8_t* in = lds + head;
    const int first = min((16 - head) & 15, nbytes);         // ragged head: bytes before the first aligned 16
    const int nchunks = (nbytes - first) >> 4;
    const int tail0 = first + (nchunks << 4);                // ragged tail: bytes behind the last whole 16
    for (int c = lane; c < nchunks; c += NL)
        *reinterpret_cast<uint4*>(in + first + (c << 4)) = *reinterpret_cast<const uint4*>(g + first + (c << 4));
    if (lane < first) in[lane] = g[lane];
    if (lane < nbytes - tail0) in[tail0 + lane] = g[tail0 + lane];
    return head;
}

// {first tap, taps} of output index i, relative to sample `base` of the n staged samples that start there: both clamped
__device__ __forceinline__ void ru_bounds(const int* __restrict__ bnd, int i, int base, int n, int ks, int& first, int& cnt) {
    first = ru_clamp(bnd[2 * i] - base, 0, n);
    cnt = ru_clamp(bnd[2 * i + 1], 0, min(ks, n - first));
}

// the same for the outputs 4 q .. 4 q + 3 of n_out (none behind n_out)
__device__ __forceinline__ void ru_bounds4(const int* __restrict__ bnd, int q, int n_out, int n_in, int ks, int (&xmin)[4],
                                           int (&cnt)[4]) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        xmin[b] = cnt[b] = 0;
        if (4 * q + b < n_out) ru_bounds(bnd, 4 * q + b, 0, n_in, ks, xmin[b], cnt[b]);
    }
}

// horizontal pass: outputs 4 q .. 4 q + 3 of one row whose samples lie STRIDE bytes apart, packed (bytes beyond n_out: zero)
template <int STRIDE>
__device__ __forceinline__ uint32_t ru_hpass4(const uint8_t* row, const int* __restrict__ coef, int q, int n_out, int ks,
                                              const int (&xmin)[4], const int (&cnt)[4]) {
    uint32_t packed = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int xo = 4 * q + b;
        if (xo < n_out) {
            const int* kc = coef + (long)xo * ks;
            int acc = RU_ROUND;
            for (int k = 0; k < cnt[b]; ++k) acc += (int)row[STRIDE * (xmin[b] + k)] * kc[k];
            packed |= (uint32_t)ru_clip8(acc) << (8 * b);
        }
    }
    return packed;
}

// vertical pass: one tap - dword wv of the column, 4 bytes of one row of mid, times its coefficient - onto the 4 accumulators
// of 4 consecutive output bytes, which start at RU_ROUND and end in ru_clip4.  The loop over the taps stays with the caller:
// inside a helper the compiler shapes it on its own, before it sees the clamp of the trip count, and the kernel comes out slower.
__device__ __forceinline__ void ru_vtap4(int (&a)[4], uint32_t wv, int kk) {
    a[0] += (int)(wv & 0xffu) * kk;
    a[1] += (int)((wv >> 8) & 0xffu) * kk;
    a[2] += (int)((wv >> 16) & 0xffu) * kk;
    a[3] += (int)(wv >> 24) * kk;
}
__device__ __forceinline__ void ru_clip4(int (&a)[4]) {
    a[0] = ru_clip8(a[0]), a[1] = ru_clip8(a[1]), a[2] = ru_clip8(a[2]), a[3] = ru_clip8(a[3]);
}

// ToTensor / Normalize of channel c for the float form: nrm = {mean[3], std[3], 1/std[3]}, or null for ToTensor alone
struct RuNorm {
    bool on;
    float mean, sd, rsd;
};
template <bool F32>
__device__ __forceinline__ RuNorm ru_norm(const float* __restrict__ nrm, int c) {
    const bool on = F32 && nrm != nullptr;
    return {on, on ? nrm[c] : 0.f, on ? nrm[3 + c] : 1.f, on ? nrm[6 + c] : 1.f};
}

// store the bytes v of outputs xo .. xo + 3 of a row of n_out at element `off`, as bytes or through u8_pixel as floats: one
// dword / float4 with vec_store (ru_vec_store), else single elements, none behind n_out
template <bool F32>
__device__ __forceinline__ void ru_store4(void* outv, long off, int xo, int n_out, int vec_store, const int (&v)[4],
                                          const RuNorm& nm) {
    if constexpr (F32) {
        float* out = reinterpret_cast<float*>(outv) + off;
        const auto px = [&](int b) { return u8_pixel((float)v[b], nm.on, nm.mean, nm.sd, nm.rsd); };
        const float4 f = make_float4(px(0), px(1), px(2), px(3));
        if (vec_store) {
            *reinterpret_cast<float4*>(out) = f;
        } else {
            out[0] = f.x;
            if (xo + 1 < n_out) out[1] = f.y;
            if (xo + 2 < n_out) out[2] = f.z;
            if (xo + 3 < n_out) out[3] = f.w;
        }
    } else {
        uint8_t* out = reinterpret_cast<uint8_t*>(outv) + off;
        if (vec_store) {
            *reinterpret_cast<uint32_t*>(out) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
        } else {
            out[0] = (uint8_t)v[0];
            if (xo + 1 < n_out) out[1] = (uint8_t)v[1];
            if (xo + 2 < n_out) out[2] = (uint8_t)v[2];
            if (xo + 3 < n_out) out[3] = (uint8_t)v[3];
        }
    }
}

// ---- host ----
// taps per output index of one axis (Pillow: (int)ceil(support) * 2 + 1, support = radius max(in / out, 1); radius 1 bilinear,
// 2 bicubic); an axis whose size does not change is not resampled: 1 (the identity table)
int ru_ksize(int n_in, int n_out, int radius) {
    if (n_in == n_out) return 1;
    const double scale = (double)n_in / n_out;
    const double support = radius * (scale < 1.0 ? 1.0 : scale);
    const int up = (int)support;
    return ((double)up < support ? up + 1 : up) * 2 + 1;
}

// input rows a tile of `tr` consecutive output rows can need: its first tap to behind its last
int ru_rows_bound(int tr, int n_in, int n_out, int radius) {
    if (n_in == n_out) return tr;
    const double scale = (double)n_in / n_out, support = radius * (scale < 1.0 ? 1.0 : scale);
    const double rows = (tr - 1) * scale + 2.0 * support + 3.0;
    return rows < (double)n_in ? (int)rows : n_in;
}

// The tile: the most output rows (32 down to `lo0`, never more than the n_rows there are) whose LDS images leave room for
// several workgroups per CU; else fewer rows (8 down to 1) in up to the whole LDS.  lds_bytes(rows) is the caller's layout for
// `rows` staged input rows.  Returns the tile's rows, with *rows and *lds those of the tile, or 0: nothing fits.
template <class LdsBytes>
int ru_pick_tile(int n_rows, int n_in, int n_out, int radius, int lo0, LdsBytes lds_bytes, int* rows, long* lds) {
    for (int pass = 0; pass < 2; ++pass)
        for (int tr = pass == 0 ? 32 : 8; tr >= (pass == 0 ? lo0 : 1); tr >>= 1) {
            const int trc = tr < n_rows ? tr : n_rows;
            *rows = ru_rows_bound(trc, n_in, n_out, radius);
            *lds = lds_bytes(*rows);
            if (*lds <= (pass == 0 ? RU_LDS_SOFT : RU_LDS_HARD)) return trc;
        }
    return 0;
}

// ru_store4 may store 4 outputs at once: rows are whole groups of 4 and the base is aligned to the group
template <bool F32>
int ru_vec_store(const void* out, int n_out) {
    const uintptr_t o = reinterpret_cast<uintptr_t>(out);
    return n_out % 4 == 0 && (F32 ? (o & 15) == 0 : (o & 3) == 0);
}

}  // namespace

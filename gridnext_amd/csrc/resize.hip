// Resize + CenterCrop of uint8 RGB patches on the device (the first two steps of the tutorials' transform:
// transforms.Resize(256), transforms.CenterCrop(224) in front of ToTensor / Normalize, image_datasets.py:102-105, :113-117).
//
// The arithmetic is Pillow's two-pass fixed-point bilinear resampling (what torchvision.transforms.Resize runs on the PIL images
// the datasets hand it), so the bytes are Pillow's bit for bit: per axis a table of int32 coefficients k = (int)(0.5 + w 2^22)
// and bounds (first tap, taps) per output index; a pass is clip((2^21 + sum pixel k) >> 22, 0, 255); the horizontal pass runs
// first and writes BYTES, the vertical pass runs on those bytes.  The tables are built on the host in double
// (gridnext_amd/transforms.py: axis_tables) for the crop window's columns and rows only - the crop commutes with both passes.
// An axis whose size does not change has the identity table (one tap of 2^22: the pass returns its input).
// The kernel is integer-only.  A workgroup takes one plane and a tile of output rows:
//   1. the contiguous byte range of the input rows the tile needs goes into the LDS - 16-B loads for the aligned middle of the
//      range, byte loads for its ragged head and tail (planes start at any byte address);
//   2. horizontal pass: LDS bytes -> a second LDS image [input rows][ceil(Pw / 4)] dwords, 4 output bytes per thread;
//   3. vertical pass: one dword of that image per tap gives 4 consecutive output bytes, stored as one dword (or as floats:
//      ToTensor / Normalize with u8_pixel, the device function of gnx_u8_to_f32).
// Consecutive tiles re-read the rows they share (L2 holds them).  Every table entry is clamped to the plane and to the staged
// rows before it is used as an address, so a wrong table gives wrong bytes, never an access outside the tensors.
#include "fwd_common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_PREC = 22;            // Pillow's PRECISION_BITS for 8-bit channels
constexpr int RS_MAX_KSIZE = 17;       // reductions up to 8x per axis
constexpr int RS_LDS_SOFT = 40 * 1024; // tile choice: several workgroups per CU
constexpr int RS_LDS_HARD = 160 * 1024;

__device__ __forceinline__ int rs_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int rs_clip8(int acc) { return rs_clamp(acc >> RS_PREC, 0, 255); }

template <bool F32>
__global__ __launch_bounds__(RS_THREADS) void resize_crop_kernel(
    const uint8_t* __restrict__ x, void* __restrict__ outv, int H0, int W0, int Ph, int Pw, const int* __restrict__ hcoef,
    const int* __restrict__ hbnd, int ksw, const int* __restrict__ vcoef, const int* __restrict__ vbnd, int ksh, int TR,
    int ntiles, int max_rows, int mid_off, int vec_store, const float* __restrict__ nrm) {
    extern __shared__ __attribute__((aligned(16))) uint8_t rs_lds[];
    const int t = threadIdx.x, tx = t & 63, ty = t >> 6;
    const long plane = blockIdx.x / ntiles;
    const int tile = blockIdx.x % ntiles;
    const int r0 = tile * TR, r1 = min(r0 + TR, Ph);
    const int y0 = rs_clamp(vbnd[2 * r0], 0, H0);
    const int y1 = rs_clamp(vbnd[2 * (r1 - 1)] + vbnd[2 * (r1 - 1) + 1], y0, H0);
    const int nrows = min(y1 - y0, max_rows);
    const int nq = (Pw + 3) >> 2;

    // 1. stage input rows [y0, y0 + nrows) of the plane: LDS address == global address modulo 16
    const uint8_t* g0 = x + plane * ((long)H0 * W0) + (long)y0 * W0;
    const int nbytes = nrows * W0;
    const int head = (int)(reinterpret_cast<uintptr_t>(g0) & 15);
    uint8_t* in = rs_lds + head;
    const int first = min((16 - head) & 15, nbytes);         // ragged head: bytes before the first aligned 16
    const int nchunks = (nbytes - first) >> 4;
    const int tail0 = first + (nchunks << 4);                // ragged tail: bytes behind the last whole 16
    for (int c = t; c < nchunks; c += RS_THREADS)
        *reinterpret_cast<uint4*>(in + first + (c << 4)) = *reinterpret_cast<const uint4*>(g0 + first + (c << 4));
    if (t < first) in[t] = g0[t];
    if (t < nbytes - tail0) in[tail0 + t] = g0[tail0 + t];
    __syncthreads();

    // 2. horizontal pass -> mid [nrows][nq] dwords (bytes beyond Pw: zero)
    uint32_t* mid = reinterpret_cast<uint32_t*>(rs_lds + mid_off);
    for (int q = tx; q < nq; q += 64) {
        int xmin[4], cnt[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int xo = 4 * q + b;
            xmin[b] = cnt[b] = 0;
            if (xo < Pw) {
                xmin[b] = rs_clamp(hbnd[2 * xo], 0, W0);
                cnt[b] = rs_clamp(hbnd[2 * xo + 1], 0, min(ksw, W0 - xmin[b]));
            }
        }
        for (int r = ty; r < nrows; r += RS_THREADS / 64) {
            const uint8_t* row = in + r * W0;
            uint32_t packed = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int xo = 4 * q + b;
                if (xo < Pw) {
                    const int* kc = hcoef + (long)xo * ksw;
                    int acc = 1 << (RS_PREC - 1);
                    for (int k = 0; k < cnt[b]; ++k) acc += (int)row[xmin[b] + k] * kc[k];
                    packed |= (uint32_t)rs_clip8(acc) << (8 * b);
                }
            }
            mid[r * nq + q] = packed;
        }
    }
    __syncthreads();

    // 3. vertical pass: 4 consecutive output bytes per thread
    const int c = (int)(plane % 3);
    const bool norm = F32 && nrm != nullptr;
    const float mean = norm ? nrm[c] : 0.f, sd = norm ? nrm[3 + c] : 1.f, rsd = norm ? nrm[6 + c] : 1.f;
    for (int rr = r0 + ty; rr < r1; rr += RS_THREADS / 64) {
        const int ymin = rs_clamp(vbnd[2 * rr] - y0, 0, nrows);
        const int cnt = rs_clamp(vbnd[2 * rr + 1], 0, min(ksh, nrows - ymin));
        const int* kc = vcoef + (long)rr * ksh;
        const long orow = (plane * Ph + rr) * (long)Pw;
        for (int q = tx; q < nq; q += 64) {
            int a0 = 1 << (RS_PREC - 1), a1 = a0, a2 = a0, a3 = a0;
            for (int k = 0; k < cnt; ++k) {
                const uint32_t wv = mid[(ymin + k) * nq + q];
                const int kk = kc[k];
                a0 += (int)(wv & 0xffu) * kk;
                a1 += (int)((wv >> 8) & 0xffu) * kk;
                a2 += (int)((wv >> 16) & 0xffu) * kk;
                a3 += (int)(wv >> 24) * kk;
            }
            const int v0 = rs_clip8(a0), v1 = rs_clip8(a1), v2 = rs_clip8(a2), v3 = rs_clip8(a3);
            const int xo = 4 * q;
            if constexpr (F32) {
                float* out = reinterpret_cast<float*>(outv) + orow + xo;
                const float4 f = make_float4(u8_pixel((float)v0, norm, mean, sd, rsd), u8_pixel((float)v1, norm, mean, sd, rsd),
                                             u8_pixel((float)v2, norm, mean, sd, rsd), u8_pixel((float)v3, norm, mean, sd, rsd));
                if (vec_store) {
                    *reinterpret_cast<float4*>(out) = f;
                } else {
                    out[0] = f.x;
                    if (xo + 1 < Pw) out[1] = f.y;
                    if (xo + 2 < Pw) out[2] = f.z;
                    if (xo + 3 < Pw) out[3] = f.w;
                }
            } else {
                uint8_t* out = reinterpret_cast<uint8_t*>(outv) + orow + xo;
                if (vec_store) {
                    *reinterpret_cast<uint32_t*>(out) = (uint32_t)v0 | ((uint32_t)v1 << 8) | ((uint32_t)v2 << 16) | ((uint32_t)v3 << 24);
                } else {
                    out[0] = (uint8_t)v0;
                    if (xo + 1 < Pw) out[1] = (uint8_t)v1;
                    if (xo + 2 < Pw) out[2] = (uint8_t)v2;
                    if (xo + 3 < Pw) out[3] = (uint8_t)v3;
                }
            }
        }
    }
}

// taps per output index of one axis (Pillow: (int)ceil(support) * 2 + 1 with support = max(in / out, 1)); 1 = identity
int rs_ksize(int n_in, int n_out) {
    if (n_in == n_out) return 1;
    const double scale = (double)n_in / n_out;
    const double support = scale < 1.0 ? 1.0 : scale;
    const int up = (int)support;
    return ((double)up < support ? up + 1 : up) * 2 + 1;
}

// input rows a tile of `tr` consecutive output rows can need: its first tap to behind its last
int rs_rows_bound(int tr, int H0, int Hr) {
    if (H0 == Hr) return tr;
    const double scale = (double)H0 / Hr, support = scale < 1.0 ? 1.0 : scale;
    const double rows = (tr - 1) * scale + 2.0 * support + 3.0;
    return rows < (double)H0 ? (int)rows : H0;
}

long rs_lds_bytes(int rows, int W0, int Pw, int* mid_off) {
    const long in_bytes = ((long)rows * W0 + 15 + 15) / 16 * 16;      // up to 15 bytes of alignment shift in front
    *mid_off = (int)in_bytes;
    return in_bytes + (long)rows * ((Pw + 3) / 4) * 4;
}

template <bool F32>
int resize_crop_launch(const uint8_t* x, void* out, long imgs, int H0, int W0, int Hr, int Wr, int top, int left, int Ph, int Pw,
                       const int* hcoef, const int* hbnd, const int* vcoef, const int* vbnd, const float* norm,
                       hipStream_t stream) {
    if (imgs < 0 || H0 <= 0 || W0 <= 0 || Hr <= 0 || Wr <= 0 || Ph <= 0 || Pw <= 0 || top < 0 || left < 0 ||
        (long)top + Ph > Hr || (long)left + Pw > Wr)
        return GNX_ERR_BAD_ARG;
    const int ksw = rs_ksize(W0, Wr), ksh = rs_ksize(H0, Hr);
    if (ksw > RS_MAX_KSIZE || ksh > RS_MAX_KSIZE) return GNX_ERR_UNSUPPORTED;
    if (imgs == 0) return GNX_OK;
    if (!x || !out || !hcoef || !hbnd || !vcoef || !vbnd) return GNX_ERR_BAD_ARG;
    // the tile: the most output rows whose two LDS images leave room for several workgroups per CU; fewer rows, up to the
    // whole LDS, for wide planes and strong reductions
    int TR = 0, rows = 0, mid_off = 0;
    long lds = 0;
    for (int pass = 0; pass < 2 && TR == 0; ++pass)
        for (int tr = pass == 0 ? 32 : 8; tr >= 1; tr >>= 1) {
            const int trc = tr < Ph ? tr : Ph;
            rows = rs_rows_bound(trc, H0, Hr);
            lds = rs_lds_bytes(rows, W0, Pw, &mid_off);
            if (lds <= (pass == 0 ? RS_LDS_SOFT : RS_LDS_HARD)) {
                TR = trc;
                break;
            }
        }
    if (TR == 0) return GNX_ERR_UNSUPPORTED;
    const long ntiles = (Ph + TR - 1) / TR;
    const long blocks = imgs * 3 * ntiles;
    if (blocks >= (1L << 31)) return GNX_ERR_UNSUPPORTED;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(&resize_crop_kernel<F32>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
        return GNX_ERR_LAUNCH;
    const uintptr_t o = reinterpret_cast<uintptr_t>(out);
    const int vec_store = Pw % 4 == 0 && (F32 ? (o & 15) == 0 : (o & 3) == 0);
    resize_crop_kernel<F32><<<(unsigned)blocks, RS_THREADS, (size_t)lds, stream>>>(
        x, out, H0, W0, Ph, Pw, hcoef, hbnd, ksw, vcoef, vbnd, ksh, TR, (int)ntiles, rows, mid_off, vec_store, norm);
    return gnx_launch_status();
}

}  // namespace

GNX_EXPORT int gnx_resize_ksize(int n_in, int n_out) {
    if (n_in <= 0 || n_out <= 0) return GNX_ERR_BAD_ARG;
    return rs_ksize(n_in, n_out);
}

GNX_EXPORT int gnx_resize_crop_u8(const uint8_t* x8, uint8_t* out, long imgs, int H0, int W0, int Hr, int Wr, int top, int left,
                                  int Ph, int Pw, const int* hcoef, const int* hbnd, const int* vcoef, const int* vbnd,
                                  hipStream_t stream) {
    return resize_crop_launch<false>(x8, out, imgs, H0, W0, Hr, Wr, top, left, Ph, Pw, hcoef, hbnd, vcoef, vbnd, nullptr, stream);
}

GNX_EXPORT int gnx_resize_crop_u8_f32(const uint8_t* x8, float* out, long imgs, int H0, int W0, int Hr, int Wr, int top, int left,
                                      int Ph, int Pw, const int* hcoef, const int* hbnd, const int* vcoef, const int* vbnd,
                                      const float* norm, hipStream_t stream) {
    return resize_crop_launch<true>(x8, out, imgs, H0, W0, Hr, Wr, top, left, Ph, Pw, hcoef, hbnd, vcoef, vbnd, norm, stream);
}

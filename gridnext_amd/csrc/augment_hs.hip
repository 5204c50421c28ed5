// Saturation and hue jitter of uint8 patches on the device, Pillow's bytes bit for bit: gnx_patch_augment_u8[_f32]
// (augment.hip: the eight symmetries of the square, the per-channel byte tables, the scatter of the rows) with two more stages
// per patch - ImageEnhance.Color (a blend of every channel with the pixel's grey value) and torchvision's adjust_hue
// (convert('HSV'), H plus a shift modulo 256, convert('RGB')).  The reference reaches these through the `img_transforms` hook of
// its datasets (gridnext/image_datasets.py:102-105, :184-187), i.e. through per-patch PIL calls on the host.
//
// Both stages need a pixel's three channels at once, which augment.hip's unit of work (a tile of ONE plane) cannot give.  Here
// the unit is a 64 x 64 tile of one patch with ALL THREE planes, so the code, the destination row, the three tables, the
// factor and the shift are the same in the whole workgroup; the units are spread over the grid with a stride.  The index map
// is augment.hip's,
//     out[y][x] = in[sy][sx],   t = 0: (sy, sx) = (a ? P-1-y : y,  b ? P-1-x : x)
//                               t = 1: (sy, sx) = (a ? P-1-x : x,  b ? P-1-y : y),   t = code & 1, a = (code >> 1) & 1,
// b = parity(code), and so is the movement: t = 0 moves four neighbouring pixels of a source row to the mirrored row with no
// LDS but the tables; t = 1 puts the three source tiles into the LDS (68-byte rows, 3 x 4352 bytes) and reads them back by
// columns.  Where P % 4 == 0 and both bases are aligned (4 B; 16 B for the float destination) a thread's four pixels are one
// dword load per plane and one dword (float4) store per plane; any other P or alignment takes the same code byte by byte.
//
// The colour stages act on the bytes as they are loaded (a per-pixel map commutes with the permutation), in the order tables,
// saturation, hue.  Their arithmetic is hs_pixel.h, Pillow's float / double expressions without contraction.  What the HSV ->
// RGB step derives from H alone (the sector and the float fraction of h * 6.0 / 255.0) and from S alone (float s / 255.0) are
// 256 values each: a workgroup computes them once, a double division per thread, and keeps them in the LDS, so the pixels'
// own double arithmetic is products and sums (and the one division h / 6.0 of the RGB -> HSV step).
#include "fwd_common.h"
#include "hs_pixel.h"

namespace {

constexpr int HS_THREADS = 256;
constexpr int HS_TILE = 64;                      // pixels per tile edge: 16 threads x 4 pixels across, 16 rows per pass
constexpr int HS_LD = HS_TILE + 4;               // bytes per LDS row of a tile
constexpr int HS_PLANE = HS_TILE * HS_LD;        // bytes per LDS tile of one plane
constexpr int HS_MAX_BLOCKS = 8192;              // 256 CUs x 8 workgroups x 4; further units by the grid stride
constexpr int HS_MAX_P = 32768;                  // P * P * 12 stays far inside 64 bits

struct HsNorm {
    bool on;
    float mean[3], sd[3], rsd[3];
};

// what is uniform in a unit of work
struct HsOp {
    bool lut, sat, inside, hue;
    float fs;
    uint32_t shift;
};

struct HsLds {
    uint8_t tab[3 * 256];                        // the patch's three byte tables
    uint8_t sector[256];                         // hs_hue_sector of every h
    float frac[256];
    float unit[256];                             // hs_sat_unit of every s
};

__device__ __forceinline__ void hs_store4(uint8_t* p, uint32_t w, const HsNorm&, int) { *reinterpret_cast<uint32_t*>(p) = w; }
__device__ __forceinline__ void hs_store4(float* p, uint32_t w, const HsNorm& nm, int c) {
    *reinterpret_cast<float4*>(p) = u8x4_pixels(w, nm.on, nm.mean[c], nm.sd[c], nm.rsd[c]);
}
__device__ __forceinline__ void hs_store1(uint8_t* p, uint32_t v, const HsNorm&, int) { *p = (uint8_t)v; }
__device__ __forceinline__ void hs_store1(float* p, uint32_t v, const HsNorm& nm, int c) {
    *p = u8_pixel((float)v, nm.on, nm.mean[c], nm.sd[c], nm.rsd[c]);
}

// one pixel through tables, saturation, hue
__device__ __forceinline__ void hs_pixel(int& r, int& g, int& b, const HsOp& op, const HsLds& s) {
    if (op.lut) {
        r = s.tab[r];
        g = s.tab[256 + g];
        b = s.tab[512 + b];
    }
    if (op.sat) {
        const int L = hs_grey(r, g, b);
        r = hs_blend(L, r, op.fs, op.inside);
        g = hs_blend(L, g, op.fs, op.inside);
        b = hs_blend(L, b, op.fs, op.inside);
    }
    if (op.hue) {
        int h, sv, v;
        hs_rgb_to_hsv(r, g, b, h, sv, v);
        h = (int)(((uint32_t)h + op.shift) & 255u);
        hs_hsv_to_rgb(s.sector[h], s.frac[h], s.unit[sv], sv, v, r, g, b);
    }
}

// four pixels, one per byte of the planes' dwords
__device__ __forceinline__ void hs_pixel4(uint32_t (&w)[3], const HsOp& op, const HsLds& s) {
    if (!(op.lut || op.sat || op.hue)) return;
    uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int r = (int)((w[0] >> (8 * j)) & 255u), g = (int)((w[1] >> (8 * j)) & 255u), b = (int)((w[2] >> (8 * j)) & 255u);
        hs_pixel(r, g, b, op, s);
        o[0] |= (uint32_t)r << (8 * j);
        o[1] |= (uint32_t)g << (8 * j);
        o[2] |= (uint32_t)b << (8 * j);
    }
    w[0] = o[0];
    w[1] = o[1];
    w[2] = o[2];
}

// nt = tiles per plane edge, units = n * nt * nt; vec: P % 4 == 0 and aligned bases (see above)
template <typename OUT>
__global__ __launch_bounds__(HS_THREADS) void hs_kernel(const uint8_t* __restrict__ src, OUT* __restrict__ dst, int P, long dst_n,
                                                        const uint8_t* __restrict__ codes, const uint8_t* __restrict__ luts,
                                                        const float* __restrict__ sat, const uint8_t* __restrict__ hue,
                                                        const int* __restrict__ dst_rows, const float* __restrict__ nrm, int nt,
                                                        uint64_t units, bool vec) {
    __shared__ HsLds lds;
    __shared__ __attribute__((aligned(16))) uint8_t tile[3 * HS_PLANE];
    const int tid = threadIdx.x, cg = tid & 15, r0 = tid >> 4, x4 = cg * 4;
    const uint64_t plane = (uint64_t)P * P, nt2 = (uint64_t)nt * nt;

    if (hue) {                                                           // the same 256 values for every unit
        int i;
        float f;
        hs_hue_sector(tid, i, f);
        lds.sector[tid] = (uint8_t)i;
        lds.frac[tid] = f;
        lds.unit[tid] = hs_sat_unit(tid);
    }
    HsNorm nm;
    nm.on = nrm != nullptr;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = nm.on ? nrm[c] : 0.f;
        nm.sd[c] = nm.on ? nrm[3 + c] : 1.f;
        nm.rsd[c] = nm.on ? nrm[6 + c] : 1.f;
    }

    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {           // everything up to the loads is workgroup-uniform
        const uint64_t k = u / nt2, tl = u - k * nt2;
        const int ty = (int)(tl / nt), tx = (int)(tl - (uint64_t)ty * nt);
        const long row = dst_rows ? (long)dst_rows[k] : (long)k;
        if (row < 0 || row >= dst_n) continue;                           // checked before it addresses anything
        const unsigned code = codes ? (unsigned)codes[k] & 7u : 0u;
        const bool t = (code & 1u) != 0, a = (code & 2u) != 0, b = (__popc(code) & 1) != 0;
        HsOp op;
        op.lut = luts != nullptr;
        op.sat = sat != nullptr;
        op.fs = op.sat ? sat[k] : 1.f;
        op.inside = op.fs >= 0.f && op.fs <= 1.f;
        op.hue = hue != nullptr;
        op.shift = op.hue ? (uint32_t)hue[k] : 0u;

        const int oy0 = ty * HS_TILE, ox0 = tx * HS_TILE;                // the tile of the OUTPUT planes
        const int th = min(HS_TILE, P - oy0), tw = min(HS_TILE, P - ox0);
        const int sh = t ? tw : th, sw = t ? th : tw;                    // its source rectangle
        const int ys = t ? ox0 : oy0, xs = t ? oy0 : ox0;
        const int sy0 = a ? P - ys - sh : ys, sx0 = b ? P - xs - sw : xs;
        const uint8_t* sp = src + k * 3 * plane;
        OUT* dp = dst + (uint64_t)row * 3 * plane;

        __syncthreads();                                                 // the last unit's reads of the LDS are done
        if (op.lut) {
#pragma unroll
            for (int c = 0; c < 3; ++c) lds.tab[c * 256 + tid] = luts[(k * 3 + c) * 256 + tid];
        }
        __syncthreads();                                                 // (also: the hue tables, before the first unit)

        if (!t) {
#pragma unroll
            for (int i = 0; i < HS_TILE / 16; ++i) {
                const int r = r0 + 16 * i;
                if (r >= sh) break;
                const uint64_t so = (uint64_t)(sy0 + r) * P + sx0;
                const uint64_t dof = (uint64_t)(oy0 + (a ? sh - 1 - r : r)) * P + ox0;
                if (vec) {
                    if (x4 < sw) {
                        uint32_t w[3];
#pragma unroll
                        for (int c = 0; c < 3; ++c) w[c] = *reinterpret_cast<const uint32_t*>(sp + c * plane + so + x4);
                        hs_pixel4(w, op, lds);
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            hs_store4(dp + c * plane + dof + (b ? sw - 4 - x4 : x4), b ? __builtin_bswap32(w[c]) : w[c], nm, c);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int x = x4 + j;
                        if (x < sw) {
                            int pr = sp[so + x], pg = sp[plane + so + x], pb = sp[2 * plane + so + x];
                            hs_pixel(pr, pg, pb, op, lds);
                            const uint64_t d = dof + (b ? sw - 1 - x : x);
                            hs_store1(dp + d, (uint32_t)pr, nm, 0);
                            hs_store1(dp + plane + d, (uint32_t)pg, nm, 1);
                            hs_store1(dp + 2 * plane + d, (uint32_t)pb, nm, 2);
                        }
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < HS_TILE / 16; ++i) {                     // source rows into the LDS, as they lie
                const int r = r0 + 16 * i;
                if (r >= sh) break;
                const uint64_t so = (uint64_t)(sy0 + r) * P + sx0;
                if (vec) {
                    if (x4 < sw) {
                        uint32_t w[3];
#pragma unroll
                        for (int c = 0; c < 3; ++c) w[c] = *reinterpret_cast<const uint32_t*>(sp + c * plane + so + x4);
                        hs_pixel4(w, op, lds);
#pragma unroll
                        for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(&tile[c * HS_PLANE + r * HS_LD + x4]) = w[c];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int x = x4 + j;
                        if (x < sw) {
                            int pr = sp[so + x], pg = sp[plane + so + x], pb = sp[2 * plane + so + x];
                            hs_pixel(pr, pg, pb, op, lds);
                            tile[r * HS_LD + x] = (uint8_t)pr;
                            tile[HS_PLANE + r * HS_LD + x] = (uint8_t)pg;
                            tile[2 * HS_PLANE + r * HS_LD + x] = (uint8_t)pb;
                        }
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < HS_TILE / 16; ++i) {                     // output rows: columns of the LDS tiles
                const int ly = r0 + 16 * i;
                if (ly >= th) break;
                const int rx = b ? sw - 1 - ly : ly;
                const uint64_t dof = (uint64_t)(oy0 + ly) * P + ox0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint8_t* tp = tile + c * HS_PLANE;
                    if (vec) {
                        if (x4 < tw) {
                            uint32_t w = 0;
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int x = x4 + j;
                                w |= (uint32_t)tp[(a ? sh - 1 - x : x) * HS_LD + rx] << (8 * j);
                            }
                            hs_store4(dp + c * plane + dof + x4, w, nm, c);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int x = x4 + j;
                            if (x < tw) hs_store1(dp + c * plane + dof + x, tp[(a ? sh - 1 - x : x) * HS_LD + rx], nm, c);
                        }
                    }
                }
            }
        }
    }
}

bool hs_al(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <typename OUT>
int hs_launch(const uint8_t* src, OUT* dst, long n, int P, long dst_n, const uint8_t* codes, const uint8_t* luts,
              const float* sat, const uint8_t* hue, const int* dst_rows, const float* norm, hipStream_t stream) {
    if (n < 0 || dst_n < 0 || P <= 0) return GNX_ERR_BAD_ARG;
    if (n == 0) return GNX_OK;
    if (!src || !dst) return GNX_ERR_BAD_ARG;
    if (!dst_rows && dst_n < n) return GNX_ERR_BAD_ARG;
    if (sat && !hs_al(sat, 4)) return GNX_ERR_BAD_ARG;
    if (P > HS_MAX_P) return GNX_ERR_UNSUPPORTED;
    const uint64_t plane = (uint64_t)P * P;
    const uint64_t most = ((uint64_t)1 << 62) / (3 * plane * sizeof(OUT));
    if ((uint64_t)n > most || (uint64_t)dst_n > most) return GNX_ERR_UNSUPPORTED;
    const uint64_t src_bytes = (uint64_t)n * 3 * plane, dst_bytes = (uint64_t)dst_n * 3 * plane * sizeof(OUT);
    const uintptr_t s = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
    if (s < d + dst_bytes && d < s + src_bytes) return GNX_ERR_BAD_ARG;  // no in-place form
    if (dst_n == 0) return GNX_OK;                                       // every row index is outside: nothing to write
    const int nt = (P + HS_TILE - 1) / HS_TILE;
    const uint64_t units = (uint64_t)n * nt * nt;
    const bool vec = P % 4 == 0 && hs_al(src, 4) && hs_al(dst, sizeof(OUT) == 1 ? 4 : 16);
    const unsigned blocks = (unsigned)(units < (uint64_t)HS_MAX_BLOCKS ? units : (uint64_t)HS_MAX_BLOCKS);
    hs_kernel<OUT><<<blocks, HS_THREADS, 0, stream>>>(src, dst, P, dst_n, codes, luts, sat, hue, dst_rows, norm, nt, units, vec);
    return gnx_launch_status();
}

}  // namespace

GNX_EXPORT int gnx_patch_augment_hs_u8(const uint8_t* src, uint8_t* dst, long n, int P, long dst_n, const uint8_t* codes,
                                       const uint8_t* luts, const float* sat, const uint8_t* hue, const int* dst_rows,
                                       hipStream_t stream) {
    return hs_launch<uint8_t>(src, dst, n, P, dst_n, codes, luts, sat, hue, dst_rows, nullptr, stream);
}

GNX_EXPORT int gnx_patch_augment_hs_u8_f32(const uint8_t* src, float* dst, long n, int P, long dst_n, const uint8_t* codes,
                                           const uint8_t* luts, const float* sat, const uint8_t* hue, const int* dst_rows,
                                           const float* norm, hipStream_t stream) {
    if (dst && !hs_al(dst, 4)) return GNX_ERR_BAD_ARG;
    return hs_launch<float>(src, dst, n, P, dst_n, codes, luts, sat, hue, dst_rows, norm, stream);
}

// Train-time augmentation of uint8 patches that are already on the device: one of the eight symmetries of the square per patch
// (flips and quarter turns), an optional per-patch, per-channel byte table (brightness / contrast), an optional scatter of the
// rows, and the grey sums the contrast tables are built from.  The reference leaves this to the `img_transforms` hook of its
// datasets (gridnext/image_datasets.py:102-105, :184-187), i.e. to per-patch PIL calls on the host.
//
// code = 4 f + r (low three bits):  out = rot90^r(fliplr^f(x)), torch.rot90 over the last two axes.  Written as one index map
//     out[y][x] = in[sy][sx],   t = 0: (sy, sx) = (a ? P-1-y : y,  b ? P-1-x : x)
//                               t = 1: (sy, sx) = (a ? P-1-x : x,  b ? P-1-y : y)
// with t = code & 1, a = (code >> 1) & 1, b = parity(code):
//     0 identity   1 rot90 (t, b)   2 rot180 (a, b)   3 rot270 (t, a)   4 fliplr (b)   5 transpose (t)   6 flipud (a)
//     7 transverse (t, a, b).
//
// The unit of work is one 64 x 64 tile of one channel plane of one patch, so the code, the destination row and the 256-byte
// table of that plane are the same in the whole workgroup; the units are spread over the grid with a stride.
//   t = 0: a row permutation and / or a reversal within the rows.  A thread moves four neighbouring bytes of a source row to
//          their place in the mirrored row (byte-swapped when b): no LDS but the table.
//   t = 1: the source tile goes into the LDS row by row and is read back by columns, so that global reads and global writes
//          both run along rows.
// Where P % 4 == 0 and both bases are aligned (4 B; 16 B for the float destination) a thread's four bytes are one dword load
// and one dword (float4) store; any other P or alignment takes the same code byte by byte.  The table is applied to the
// bytes as they are loaded: a per-byte map commutes with the permutation.  The float form stores u8_pixel of the byte result,
// the device function of gnx_u8_to_f32.
//
// Grey sums: one workgroup per patch at a time, each thread sums Pillow's L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 over
// its pixels in 64 bits, then one LDS tree per patch: exact integers, a fixed structure, no atomics.
#include "fwd_common.h"

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_TILE = 64;                     // bytes per tile edge: 16 threads x 4 bytes across, 16 rows per pass
constexpr int AUG_LD = AUG_TILE + 4;             // bytes per LDS row of the tile
constexpr int AUG_MAX_BLOCKS = 8192;             // 256 CUs x 8 workgroups x 4; further units by the grid stride
constexpr int AUG_MAX_P = 32768;                 // P * P * 12 stays far inside 64 bits

__device__ __forceinline__ uint32_t aug_lut4(uint32_t w, const uint8_t* tab) {
    return (uint32_t)tab[w & 255u] | ((uint32_t)tab[(w >> 8) & 255u] << 8) | ((uint32_t)tab[(w >> 16) & 255u] << 16) |
           ((uint32_t)tab[w >> 24] << 24);
}

struct AugNorm {
    bool on;
    float mean, sd, rsd;
};

__device__ __forceinline__ void aug_store4(uint8_t* p, uint32_t w, const AugNorm&) { *reinterpret_cast<uint32_t*>(p) = w; }
__device__ __forceinline__ void aug_store4(float* p, uint32_t w, const AugNorm& nm) {
    *reinterpret_cast<float4*>(p) = u8x4_pixels(w, nm.on, nm.mean, nm.sd, nm.rsd);
}
__device__ __forceinline__ void aug_store1(uint8_t* p, uint32_t v, const AugNorm&) { *p = (uint8_t)v; }
__device__ __forceinline__ void aug_store1(float* p, uint32_t v, const AugNorm& nm) {
    *p = u8_pixel((float)v, nm.on, nm.mean, nm.sd, nm.rsd);
}

// nt = tiles per plane edge, units = n * 3 * nt * nt; vec: P % 4 == 0 and aligned bases (see above)
template <typename OUT>
__global__ __launch_bounds__(AUG_THREADS) void aug_kernel(const uint8_t* __restrict__ src, OUT* __restrict__ dst, int P,
                                                          long dst_n, const uint8_t* __restrict__ codes,
                                                          const uint8_t* __restrict__ luts, const int* __restrict__ dst_rows,
                                                          const float* __restrict__ nrm, int nt, uint64_t units, bool vec) {
    __shared__ uint8_t tab[256];
    __shared__ __attribute__((aligned(16))) uint8_t tile[AUG_TILE * AUG_LD];
    const int tid = threadIdx.x, cg = tid & 15, r0 = tid >> 4, x4 = cg * 4;
    const uint64_t plane = (uint64_t)P * P, nt2 = (uint64_t)nt * nt, per_patch = 3 * nt2;

    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {           // everything up to the loads is workgroup-uniform
        const uint64_t k = u / per_patch, rem = u - k * per_patch;
        const int c = (int)(rem / nt2);
        const uint64_t tl = rem - (uint64_t)c * nt2;
        const int ty = (int)(tl / nt), tx = (int)(tl - (uint64_t)ty * nt);
        const long row = dst_rows ? (long)dst_rows[k] : (long)k;
        if (row < 0 || row >= dst_n) continue;                           // checked before it addresses anything
        const unsigned code = codes ? (unsigned)codes[k] & 7u : 0u;
        const bool t = (code & 1u) != 0, a = (code & 2u) != 0, b = (__popc(code) & 1) != 0;

        const int oy0 = ty * AUG_TILE, ox0 = tx * AUG_TILE;              // the tile of the OUTPUT plane
        const int th = min(AUG_TILE, P - oy0), tw = min(AUG_TILE, P - ox0);
        const int sh = t ? tw : th, sw = t ? th : tw;                    // its source rectangle
        const int ys = t ? ox0 : oy0, xs = t ? oy0 : ox0;
        const int sy0 = a ? P - ys - sh : ys, sx0 = b ? P - xs - sw : xs;
        const uint8_t* sp = src + (k * 3 + c) * plane;
        OUT* dp = dst + ((uint64_t)row * 3 + c) * plane;
        AugNorm nm;
        nm.on = nrm != nullptr;
        nm.mean = nm.on ? nrm[c] : 0.f;
        nm.sd = nm.on ? nrm[3 + c] : 1.f;
        nm.rsd = nm.on ? nrm[6 + c] : 1.f;

        __syncthreads();                                                 // the last unit's reads of tab and tile are done
        const bool lut = luts != nullptr;
        if (lut) {
            tab[tid] = luts[(k * 3 + c) * 256 + tid];
            __syncthreads();
        }

        if (!t) {
#pragma unroll
            for (int i = 0; i < AUG_TILE / 16; ++i) {
                const int r = r0 + 16 * i;
                if (r >= sh) break;
                const uint8_t* srow = sp + (uint64_t)(sy0 + r) * P + sx0;
                OUT* drow = dp + (uint64_t)(oy0 + (a ? sh - 1 - r : r)) * P + ox0;
                if (vec) {
                    if (x4 < sw) {
                        uint32_t w = *reinterpret_cast<const uint32_t*>(srow + x4);
                        if (lut) w = aug_lut4(w, tab);
                        if (b) w = __builtin_bswap32(w);
                        aug_store4(drow + (b ? sw - 4 - x4 : x4), w, nm);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int x = x4 + j;
                        if (x < sw) {
                            uint32_t v = srow[x];
                            if (lut) v = tab[v];
                            aug_store1(drow + (b ? sw - 1 - x : x), v, nm);
                        }
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < AUG_TILE / 16; ++i) {                    // source rows into the LDS, as they lie
                const int r = r0 + 16 * i;
                if (r >= sh) break;
                const uint8_t* srow = sp + (uint64_t)(sy0 + r) * P + sx0;
                if (vec) {
                    if (x4 < sw) {
                        uint32_t w = *reinterpret_cast<const uint32_t*>(srow + x4);
                        if (lut) w = aug_lut4(w, tab);
                        *reinterpret_cast<uint32_t*>(&tile[r * AUG_LD + x4]) = w;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int x = x4 + j;
                        if (x < sw) {
                            uint32_t v = srow[x];
                            if (lut) v = tab[v];
                            tile[r * AUG_LD + x] = (uint8_t)v;
                        }
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < AUG_TILE / 16; ++i) {                    // output rows: columns of the LDS tile
                const int ly = r0 + 16 * i;
                if (ly >= th) break;
                const int rx = b ? sw - 1 - ly : ly;
                OUT* drow = dp + (uint64_t)(oy0 + ly) * P + ox0;
                if (vec) {
                    if (x4 < tw) {
                        uint32_t w = 0;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int x = x4 + j;
                            w |= (uint32_t)tile[(a ? sh - 1 - x : x) * AUG_LD + rx] << (8 * j);
                        }
                        aug_store4(drow + x4, w, nm);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int x = x4 + j;
                        if (x < tw) aug_store1(drow + x, tile[(a ? sh - 1 - x : x) * AUG_LD + rx], nm);
                    }
                }
            }
        }
    }
}

__device__ __forceinline__ uint32_t aug_grey(uint32_t r, uint32_t g, uint32_t b) {
    return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16;
}

__global__ __launch_bounds__(AUG_THREADS) void aug_grey_sum_kernel(const uint8_t* __restrict__ src, long n, uint64_t plane,
                                                                   uint64_t* __restrict__ sums, bool vec) {
    __shared__ uint64_t red[AUG_THREADS];
    const int tid = threadIdx.x;
    for (long k = blockIdx.x; k < n; k += gridDim.x) {
        const uint8_t* pr = src + 3 * (uint64_t)k * plane;
        const uint8_t* pg = pr + plane;
        const uint8_t* pb = pg + plane;
        uint64_t acc = 0;
        if (vec) {                                                       // plane % 4 == 0 and a 4-byte aligned base
            for (uint64_t i = tid; i < plane / 4; i += AUG_THREADS) {
                const uint32_t r = reinterpret_cast<const uint32_t*>(pr)[i], g = reinterpret_cast<const uint32_t*>(pg)[i],
                               b = reinterpret_cast<const uint32_t*>(pb)[i];
                uint32_t s = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) s += aug_grey((r >> (8 * j)) & 255u, (g >> (8 * j)) & 255u, (b >> (8 * j)) & 255u);
                acc += s;
            }
        } else {
            for (uint64_t i = tid; i < plane; i += AUG_THREADS) acc += aug_grey(pr[i], pg[i], pb[i]);
        }
        red[tid] = acc;
        __syncthreads();
        for (int s = AUG_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        if (tid == 0) sums[k] = red[0];
        __syncthreads();
    }
}

bool aug_al(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <typename OUT>
int aug_launch(const uint8_t* src, OUT* dst, long n, int P, long dst_n, const uint8_t* codes, const uint8_t* luts,
               const int* dst_rows, const float* norm, hipStream_t stream) {
    if (n < 0 || dst_n < 0 || P <= 0) return GNX_ERR_BAD_ARG;
    if (n == 0) return GNX_OK;
    if (!src || !dst) return GNX_ERR_BAD_ARG;
    if (!dst_rows && dst_n < n) return GNX_ERR_BAD_ARG;
    if (P > AUG_MAX_P) return GNX_ERR_UNSUPPORTED;
    const uint64_t plane = (uint64_t)P * P;
    const uint64_t most = ((uint64_t)1 << 62) / (3 * plane * sizeof(OUT));
    if ((uint64_t)n > most || (uint64_t)dst_n > most) return GNX_ERR_UNSUPPORTED;
    const uint64_t src_bytes = (uint64_t)n * 3 * plane, dst_bytes = (uint64_t)dst_n * 3 * plane * sizeof(OUT);
    const uintptr_t s = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
    if (s < d + dst_bytes && d < s + src_bytes) return GNX_ERR_BAD_ARG;  // no in-place form
    if (dst_n == 0) return GNX_OK;                                       // every row index is outside: nothing to write
    const int nt = (P + AUG_TILE - 1) / AUG_TILE;
    const uint64_t units = (uint64_t)n * 3 * nt * nt;
    const bool vec = P % 4 == 0 && aug_al(src, 4) && aug_al(dst, sizeof(OUT) == 1 ? 4 : 16);
    const unsigned blocks = (unsigned)(units < (uint64_t)AUG_MAX_BLOCKS ? units : (uint64_t)AUG_MAX_BLOCKS);
    aug_kernel<OUT><<<blocks, AUG_THREADS, 0, stream>>>(src, dst, P, dst_n, codes, luts, dst_rows, norm, nt, units, vec);
    return gnx_launch_status();
}

}  // namespace

GNX_EXPORT int gnx_patch_augment_u8(const uint8_t* src, uint8_t* dst, long n, int P, long dst_n, const uint8_t* codes,
                                    const uint8_t* luts, const int* dst_rows, hipStream_t stream) {
    return aug_launch<uint8_t>(src, dst, n, P, dst_n, codes, luts, dst_rows, nullptr, stream);
}

GNX_EXPORT int gnx_patch_augment_u8_f32(const uint8_t* src, float* dst, long n, int P, long dst_n, const uint8_t* codes,
                                        const uint8_t* luts, const int* dst_rows, const float* norm, hipStream_t stream) {
    if (dst && !aug_al(dst, 4)) return GNX_ERR_BAD_ARG;
    return aug_launch<float>(src, dst, n, P, dst_n, codes, luts, dst_rows, norm, stream);
}

GNX_EXPORT int gnx_patch_grey_sum_u8(const uint8_t* src, long n, int P, unsigned long long* sums, hipStream_t stream) {
    if (n < 0 || P <= 0) return GNX_ERR_BAD_ARG;
    if (n == 0) return GNX_OK;
    if (!src || !sums || !aug_al(sums, 8)) return GNX_ERR_BAD_ARG;
    if (P > AUG_MAX_P) return GNX_ERR_UNSUPPORTED;
    const uint64_t plane = (uint64_t)P * P;
    if ((uint64_t)n > ((uint64_t)1 << 62) / (3 * plane)) return GNX_ERR_UNSUPPORTED;
    const bool vec = plane % 4 == 0 && aug_al(src, 4);
    const unsigned blocks = (unsigned)(n < (long)AUG_MAX_BLOCKS ? n : (long)AUG_MAX_BLOCKS);
    aug_grey_sum_kernel<<<blocks, AUG_THREADS, 0, stream>>>(src, n, plane, reinterpret_cast<uint64_t*>(sums), vec);
    return gnx_launch_status();
}

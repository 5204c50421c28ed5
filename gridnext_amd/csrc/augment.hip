// Train-time augmentation of uint8 patches that are already on the device: one of the eight symmetries of the square per patch
// (flips and quarter turns), a colour stage, an optional scatter of the rows, and the grey sums the contrast tables are built
// from.  The reference leaves this to the `img_transforms` hook of its datasets (gridnext/image_datasets.py:102-105, :184-187),
// i.e. to per-patch PIL calls on the host.
//
// code = 4 f + r (low three bits):  out = rot90^r(fliplr^f(x)), torch.rot90 over the last two axes.  Written as one index map
//     out[y][x] = in[sy][sx],   t = 0: (sy, sx) = (a ? P-1-y : y,  b ? P-1-x : x)
//                               t = 1: (sy, sx) = (a ? P-1-x : x,  b ? P-1-y : y)
// with t = code & 1, a = (code >> 1) & 1, b = parity(code):
//     0 identity   1 rot90 (t, b)   2 rot180 (a, b)   3 rot270 (t, a)   4 fliplr (b)   5 transpose (t)   6 flipud (a)
//     7 transverse (t, a, b).
//
// The mover, aug_kernel<OUT, STAGE>.  The unit of work is one 64 x 64 tile of STAGE::PLANES channel planes of one patch, so the
// code, the destination row and the stage's per-patch operands are the same in the whole workgroup; the units are spread over
// the grid with a stride.
//   t = 0: a row permutation and / or a reversal within the rows.  A thread moves four neighbouring bytes of a source row to
//          their place in the mirrored row (byte-swapped when b): no LDS but the stage's.
//   t = 1: the source tile goes into the LDS row by row (68-byte rows, one tile per plane) and is read back by columns, so that
//          global reads and global writes both run along rows.
// Where P % 4 == 0 and both bases are aligned (4 B; 16 B for the float destination) a thread's four bytes are one dword load
// and one dword (float4) store per plane; any other P or alignment takes the same code byte by byte.  The float form stores
// u8_pixel of the byte result, the device function of gnx_u8_to_f32.
//
// The stage is what happens to the bytes between load and store; it acts on them as they are loaded, since a per-pixel map
// commutes with the permutation.  A stage holds its operands, its LDS, what a workgroup computes once (`once`), what it loads
// per unit with the barrier after that load (`load`), and the map of four pixels held as one dword per plane (`map4`) and of
// one pixel (`map1`).
//   AugLut (PLANES = 1, gnx_patch_augment_u8[_f32]): an optional per-patch, per-channel byte table (brightness / contrast).
//   AugHs (PLANES = 3, gnx_patch_augment_hs_u8[_f32]): the tables, then ImageEnhance.Color (a blend of every channel with the
//       pixel's grey value), then torchvision's adjust_hue (convert('HSV'), H plus a shift modulo 256, convert('RGB')), Pillow's
//       bytes bit for bit.  Both need a pixel's three channels at once, hence the three-plane unit.  The arithmetic is
//       hs_pixel.h, Pillow's float / double expressions without contraction.  What the HSV -> RGB step derives from H alone (the
//       sector and the float fraction of h * 6.0 / 255.0) and from S alone (float s / 255.0) are 256 values each: a workgroup
//       computes them once, a double division per thread, and keeps them in the LDS, so the pixels' own double arithmetic is
//       products and sums (and the one division h / 6.0 of the RGB -> HSV step).
//
// Grey sums: one workgroup per patch at a time, each thread sums Pillow's L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 over
// its pixels in 64 bits, then one LDS tree per patch: exact integers, a fixed structure, no atomics.
#include "fwd_common.h"
#include "hs_pixel.h"

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_TILE = 64;                     // bytes per tile edge: 16 threads x 4 bytes across, 16 rows per pass
constexpr int AUG_LD = AUG_TILE + 4;             // bytes per LDS row of a tile
constexpr int AUG_PLANE = AUG_TILE * AUG_LD;     // bytes per LDS tile of one plane
constexpr int AUG_MAX_BLOCKS = 8192;             // 256 CUs x 8 workgroups x 4; further units by the grid stride
constexpr int AUG_MAX_P = 32768;                 // P * P * 12 stays far inside 64 bits

struct AugLut {
    static constexpr int PLANES = 1;
    struct Lds {
        uint8_t tab[256];                        // the plane's byte table
    };
    const uint8_t* luts;

    __device__ __forceinline__ AugLut(const uint8_t* tables, const float*, const uint8_t*) : luts(tables) {}
    __device__ __forceinline__ void once(Lds&, int) {}
    __device__ __forceinline__ void load(Lds& s, uint64_t k, int c, int tid) {
        if (luts) {
            s.tab[tid] = luts[(k * 3 + c) * 256 + tid];
            __syncthreads();
        }
    }
    __device__ __forceinline__ void map4(uint32_t (&w)[1], const Lds& s) const {
        if (luts)
            w[0] = (uint32_t)s.tab[w[0] & 255u] | ((uint32_t)s.tab[(w[0] >> 8) & 255u] << 8) |
                   ((uint32_t)s.tab[(w[0] >> 16) & 255u] << 16) | ((uint32_t)s.tab[w[0] >> 24] << 24);
    }
    __device__ __forceinline__ void map1(uint32_t (&v)[1], const Lds& s) const {
        if (luts) v[0] = s.tab[v[0]];
    }
};

struct AugHs {
    static constexpr int PLANES = 3;
    struct Lds {
        uint8_t tab[3 * 256];                    // the patch's three byte tables
        uint8_t sector[256];                     // hs_hue_sector of every h
        float frac[256];
        float unit[256];                         // hs_sat_unit of every s
    };
    const uint8_t* luts;
    const float* sat;
    const uint8_t* hue;
    float fs;                                    // of the unit (`load`): the factor, whether it is in [0, 1], the shift
    bool inside;
    uint32_t shift;

    __device__ __forceinline__ void once(Lds& s, int tid) {
        if (hue) {                                                       // the same 256 values for every unit
            int i;
            float f;
            hs_hue_sector(tid, i, f);
            s.sector[tid] = (uint8_t)i;
            s.frac[tid] = f;
            s.unit[tid] = hs_sat_unit(tid);
        }
    }
    __device__ __forceinline__ void load(Lds& s, uint64_t k, int, int tid) {
        fs = sat ? sat[k] : 1.f;
        inside = fs >= 0.f && fs <= 1.f;
        shift = hue ? (uint32_t)hue[k] : 0u;
        if (luts) {
#pragma unroll
            for (int c = 0; c < 3; ++c) s.tab[c * 256 + tid] = luts[(k * 3 + c) * 256 + tid];
        }
        __syncthreads();                                                 // (also: the hue tables, before the first unit)
    }
    // one pixel through tables, saturation, hue
    __device__ __forceinline__ void pixel(int& r, int& g, int& b, const Lds& s) const {
        if (luts) {
            r = s.tab[r];
            g = s.tab[256 + g];
            b = s.tab[512 + b];
        }
        if (sat) {
            const int L = hs_grey(r, g, b);
            r = hs_blend(L, r, fs, inside);
            g = hs_blend(L, g, fs, inside);
            b = hs_blend(L, b, fs, inside);
        }
        if (hue) {
            int h, sv, v;
            hs_rgb_to_hsv(r, g, b, h, sv, v);
            h = (int)(((uint32_t)h + shift) & 255u);
            hs_hsv_to_rgb(s.sector[h], s.frac[h], s.unit[sv], sv, v, r, g, b);
        }
    }
    __device__ __forceinline__ void map4(uint32_t (&w)[3], const Lds& s) const {
        if (!(luts || sat || hue)) return;
        uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int r = (int)((w[0] >> (8 * j)) & 255u), g = (int)((w[1] >> (8 * j)) & 255u), b = (int)((w[2] >> (8 * j)) & 255u);
            pixel(r, g, b, s);
            o[0] |= (uint32_t)r << (8 * j);
            o[1] |= (uint32_t)g << (8 * j);
            o[2] |= (uint32_t)b << (8 * j);
        }
        w[0] = o[0];
        w[1] = o[1];
        w[2] = o[2];
    }
    __device__ __forceinline__ void map1(uint32_t (&v)[3], const Lds& s) const {
        int r = (int)v[0], g = (int)v[1], b = (int)v[2];
        pixel(r, g, b, s);
        v[0] = (uint32_t)r;
        v[1] = (uint32_t)g;
        v[2] = (uint32_t)b;
    }
};

// the float store's normalisation of a unit's planes
template <int PLANES>
struct AugNorm {
    bool on;
    float mean[PLANES], sd[PLANES], rsd[PLANES];

    __device__ __forceinline__ AugNorm(const float* nrm, int c0) : on(nrm != nullptr) {
#pragma unroll
        for (int c = 0; c < PLANES; ++c) {
            mean[c] = on ? nrm[c0 + c] : 0.f;
            sd[c] = on ? nrm[3 + c0 + c] : 1.f;
            rsd[c] = on ? nrm[6 + c0 + c] : 1.f;
        }
    }
};

// four bytes / one byte of plane c of the unit
template <typename NORM>
__device__ __forceinline__ void aug_store4(uint8_t* p, uint32_t w, const NORM&, int) { *reinterpret_cast<uint32_t*>(p) = w; }
template <typename NORM>
__device__ __forceinline__ void aug_store4(float* p, uint32_t w, const NORM& nm, int c) {
    *reinterpret_cast<float4*>(p) = u8x4_pixels(w, nm.on, nm.mean[c], nm.sd[c], nm.rsd[c]);
}
template <typename NORM>
__device__ __forceinline__ void aug_store1(uint8_t* p, uint32_t v, const NORM&, int) { *p = (uint8_t)v; }
template <typename NORM>
__device__ __forceinline__ void aug_store1(float* p, uint32_t v, const NORM& nm, int c) {
    *p = u8_pixel((float)v, nm.on, nm.mean[c], nm.sd[c], nm.rsd[c]);
}

// nt = tiles per plane edge, units = n * (3 / PLANES) * nt * nt; vec: P % 4 == 0 and aligned bases (see above).  Three things are
// shaped by the compiler's output: the stages' operands are plain kernel arguments from which the stage is built
// here, not a stage object passed by value, and a row is addressed through a pointer to it, not through a 64-bit offset that
// every access adds to the plane's base - either costs the three-plane float form its seventh wave per SIMD; and the straight
// and the transposing path each keep their loop over the source rows - one loop that tests t inside measured 10-30 % slower.
template <typename OUT, typename STAGE>
__global__ __launch_bounds__(AUG_THREADS) void aug_kernel(const uint8_t* __restrict__ src, OUT* __restrict__ dst, int P,
                                                          long dst_n, const uint8_t* __restrict__ codes,
                                                          const uint8_t* __restrict__ luts, const float* __restrict__ sat,
                                                          const uint8_t* __restrict__ hue, const int* __restrict__ dst_rows,
                                                          const float* __restrict__ nrm, int nt, uint64_t units, bool vec) {
    constexpr int PL = STAGE::PLANES;
    __shared__ typename STAGE::Lds lds;
    __shared__ __attribute__((aligned(16))) uint8_t tile[PL * AUG_PLANE];
    const int tid = threadIdx.x, cg = tid & 15, r0 = tid >> 4, x4 = cg * 4;
    const uint64_t plane = (uint64_t)P * P, nt2 = (uint64_t)nt * nt, per_patch = (3 / PL) * nt2;
    STAGE st{luts, sat, hue};
    st.once(lds, tid);

    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {           // everything up to the loads is workgroup-uniform
        const uint64_t k = u / per_patch, rem = u - k * per_patch;
        const int c0 = PL == 3 ? 0 : (int)(rem / nt2);                   // the unit's first plane
        const uint64_t tl = rem - (uint64_t)c0 * nt2;
        const int ty = (int)(tl / nt), tx = (int)(tl - (uint64_t)ty * nt);
        const long row = dst_rows ? (long)dst_rows[k] : (long)k;
        if (row < 0 || row >= dst_n) continue;                           // checked before it addresses anything
        const unsigned code = codes ? (unsigned)codes[k] & 7u : 0u;
        const bool t = (code & 1u) != 0, a = (code & 2u) != 0, b = (__popc(code) & 1) != 0;

        const int oy0 = ty * AUG_TILE, ox0 = tx * AUG_TILE;              // the tile of the OUTPUT planes
        const int th = min(AUG_TILE, P - oy0), tw = min(AUG_TILE, P - ox0);
        const int sh = t ? tw : th, sw = t ? th : tw;                    // its source rectangle
        const int ys = t ? ox0 : oy0, xs = t ? oy0 : ox0;
        const int sy0 = a ? P - ys - sh : ys, sx0 = b ? P - xs - sw : xs;
        const uint8_t* sp = src + (k * 3 + c0) * plane;
        OUT* dp = dst + ((uint64_t)row * 3 + c0) * plane;
        const AugNorm<PL> nm(nrm, c0);

        __syncthreads();                                                 // the last unit's reads of the LDS are done
        st.load(lds, k, c0, tid);

        if (!t) {
#pragma unroll
            for (int i = 0; i < AUG_TILE / 16; ++i) {
                const int r = r0 + 16 * i;
                if (r >= sh) break;
                const uint8_t* srow = sp + (uint64_t)(sy0 + r) * P + sx0;
                OUT* drow = dp + (uint64_t)(oy0 + (a ? sh - 1 - r : r)) * P + ox0;
                if (vec) {
                    if (x4 < sw) {
                        uint32_t w[PL];
#pragma unroll
                        for (int c = 0; c < PL; ++c) w[c] = *reinterpret_cast<const uint32_t*>(srow + c * plane + x4);
                        st.map4(w, lds);
#pragma unroll
                        for (int c = 0; c < PL; ++c)
                            aug_store4(drow + c * plane + (b ? sw - 4 - x4 : x4), b ? __builtin_bswap32(w[c]) : w[c], nm, c);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int x = x4 + j;
                        if (x < sw) {
                            uint32_t v[PL];
#pragma unroll
                            for (int c = 0; c < PL; ++c) v[c] = srow[c * plane + x];
                            st.map1(v, lds);
#pragma unroll
                            for (int c = 0; c < PL; ++c) aug_store1(drow + c * plane + (b ? sw - 1 - x : x), v[c], nm, c);
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
                        uint32_t w[PL];
#pragma unroll
                        for (int c = 0; c < PL; ++c) w[c] = *reinterpret_cast<const uint32_t*>(srow + c * plane + x4);
                        st.map4(w, lds);
#pragma unroll
                        for (int c = 0; c < PL; ++c)
                            *reinterpret_cast<uint32_t*>(&tile[c * AUG_PLANE + r * AUG_LD + x4]) = w[c];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int x = x4 + j;
                        if (x < sw) {
                            uint32_t v[PL];
#pragma unroll
                            for (int c = 0; c < PL; ++c) v[c] = srow[c * plane + x];
                            st.map1(v, lds);
#pragma unroll
                            for (int c = 0; c < PL; ++c) tile[c * AUG_PLANE + r * AUG_LD + x] = (uint8_t)v[c];
                        }
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < AUG_TILE / 16; ++i) {                    // output rows: columns of the LDS tiles
                const int ly = r0 + 16 * i;
                if (ly >= th) break;
                const int rx = b ? sw - 1 - ly : ly;
                OUT* drow = dp + (uint64_t)(oy0 + ly) * P + ox0;
#pragma unroll
                for (int c = 0; c < PL; ++c) {
                    const uint8_t* tp = tile + c * AUG_PLANE;
                    if (vec) {
                        if (x4 < tw) {
                            uint32_t w = 0;
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int x = x4 + j;
                                w |= (uint32_t)tp[(a ? sh - 1 - x : x) * AUG_LD + rx] << (8 * j);
                            }
                            aug_store4(drow + c * plane + x4, w, nm, c);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int x = x4 + j;
                            if (x < tw) aug_store1(drow + c * plane + x, tp[(a ? sh - 1 - x : x) * AUG_LD + rx], nm, c);
                        }
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

template <typename OUT, typename STAGE>
int aug_launch(const uint8_t* src, OUT* dst, long n, int P, long dst_n, const uint8_t* codes, const uint8_t* luts,
               const float* sat, const uint8_t* hue, const int* dst_rows, const float* norm, hipStream_t stream) {
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
    const uint64_t units = (uint64_t)n * (3 / STAGE::PLANES) * nt * nt;
    const bool vec = P % 4 == 0 && aug_al(src, 4) && aug_al(dst, sizeof(OUT) == 1 ? 4 : 16);
    const unsigned blocks = (unsigned)(units < (uint64_t)AUG_MAX_BLOCKS ? units : (uint64_t)AUG_MAX_BLOCKS);
    aug_kernel<OUT, STAGE>
        <<<blocks, AUG_THREADS, 0, stream>>>(src, dst, P, dst_n, codes, luts, sat, hue, dst_rows, norm, nt, units, vec);
    return gnx_launch_status();
}

// A factor vector off its 4 bytes is refused where it always was: behind the checks that answer GNX_ERR_BAD_ARG themselves or
// find nothing to do (n == 0), before the ones that answer GNX_ERR_UNSUPPORTED.
bool aug_sat_ok(long n, const float* sat) { return n == 0 || !sat || aug_al(sat, 4); }

}  // namespace

GNX_EXPORT int gnx_patch_augment_u8(const uint8_t* src, uint8_t* dst, long n, int P, long dst_n, const uint8_t* codes,
                                    const uint8_t* luts, const int* dst_rows, hipStream_t stream) {
    return aug_launch<uint8_t, AugLut>(src, dst, n, P, dst_n, codes, luts, nullptr, nullptr, dst_rows, nullptr, stream);
}

GNX_EXPORT int gnx_patch_augment_u8_f32(const uint8_t* src, float* dst, long n, int P, long dst_n, const uint8_t* codes,
                                        const uint8_t* luts, const int* dst_rows, const float* norm, hipStream_t stream) {
    if (dst && !aug_al(dst, 4)) return GNX_ERR_BAD_ARG;
    return aug_launch<float, AugLut>(src, dst, n, P, dst_n, codes, luts, nullptr, nullptr, dst_rows, norm, stream);
}

GNX_EXPORT int gnx_patch_augment_hs_u8(const uint8_t* src, uint8_t* dst, long n, int P, long dst_n, const uint8_t* codes,
                                       const uint8_t* luts, const float* sat, const uint8_t* hue, const int* dst_rows,
                                       hipStream_t stream) {
    if (!aug_sat_ok(n, sat)) return GNX_ERR_BAD_ARG;
    return aug_launch<uint8_t, AugHs>(src, dst, n, P, dst_n, codes, luts, sat, hue, dst_rows, nullptr, stream);
}

GNX_EXPORT int gnx_patch_augment_hs_u8_f32(const uint8_t* src, float* dst, long n, int P, long dst_n, const uint8_t* codes,
                                           const uint8_t* luts, const float* sat, const uint8_t* hue, const int* dst_rows,
                                           const float* norm, hipStream_t stream) {
    if (dst && !aug_al(dst, 4)) return GNX_ERR_BAD_ARG;
    if (!aug_sat_ok(n, sat)) return GNX_ERR_BAD_ARG;
    return aug_launch<float, AugHs>(src, dst, n, P, dst_n, codes, luts, sat, hue, dst_rows, norm, stream);
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

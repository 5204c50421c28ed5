// The patch grid of a Visium array cut straight out of the whole-slide image (the reference's grid_from_wsi_visium,
// imgprocess.py:198-236: np.pad(mode='edge') of the slide, one window per in-tissue spot, Image.fromarray(window).resize((P, P)),
// permute to planar, store at the spot's odd-right cell).
//
// The slide is resident as uint8 [Hs][Ws][3] (interleaved, any base alignment).  A spot {x_px, y_px, grid_row, grid_col} owns
// the window of source rows and columns [c - half, c + half), every coordinate clamped to the slide (= the slice of the
// edge-padded slide; no padded copy exists here).  The resize is Pillow's default, BICUBIC, in its two-pass fixed-point form:
// one table pair (gridnext_amd/transforms.py: axis_tables(2 half, P, filter='bicubic')) serves both axes and every spot. 2
// half == P is the identity: a deinterleaving copy, no table is read. The resampler itself - the horizontal pass, the tap of
// the vertical one, the clamps, the staging of a byte run, the 4-wide store, and on the host the tap count, the tile search
// and the limits - is resample_u8.h, shared with resize.hip.  This file holds what is its own: the spots and the geometry in
// the launch arguments, the window's rows staged one by one out of an interleaved slide with a fallback at its edges, the copy
// path, the cell a patch goes to, and the chunked launches.
// A workgroup takes one spot and a tile of output rows:
//   1. the window's source rows the tile needs go into the LDS, interleaved as they lie in the slide.  A window whose columns
//      are inside the slide is a contiguous run of 6 half bytes per row at an arbitrary alignment, and the row sits in the
//      LDS at its global address modulo 16 (ru_stage).  A window that reaches over the left or right edge takes byte loads
//      with clamped columns.  Rows are clamped in both;
//   2. horizontal pass: LDS bytes -> a second LDS image [rows][3][ceil(P / 4)] dwords, deinterleaving as it reads;
//   3. vertical pass: one dword of that image per tap gives 4 consecutive output bytes of one plane, stored as one dword (or
//      as floats: ToTensor / Normalize with u8_pixel), or as single bytes / floats where P % 4 != 0 or the base is unaligned.
// The spots are HOST memory: the entry point checks every grid index before anything is launched, and hands the spots to the
// kernel inside its launch arguments, WP_CHUNK per launch - no device table, no copy, no allocation, nothing read back.
// Every spot coordinate and every table entry is clamped before it is used as an address, and every byte offset into the
// slide and the grid is 64-bit (a real slide exceeds 2^31 bytes).
//
// The _lut forms fold a per-channel byte table (SpaCell's colour-cast removal, imgprocess.py:49-67; the layout gnx_rgb_lut_u8
// takes) into the gather: the table goes into 768 bytes of LDS behind the two images, and between step 1 and the passes that
// read them every staged byte of channel c becomes lut[c][byte], a dword of a row per lane.  A per-pixel map commutes with
// the edge replication, so the bytes are those of the plain kernel run on gnx_rgb_lut_u8(slide, lut) - and the slide itself
// is neither written nor copied.  The kernel is a template on it: without a table there is no extra LDS, pass or barrier.
#include "resample_u8.h"

namespace {

constexpr int WP_CHUNK = 224;          // spots per launch: 3.5 KB of the 4 KB a launch's arguments may take
constexpr int WP_LUT_BYTES = 3 * 256;  // the _lut forms' table in the LDS: [channel][byte]

struct WpSpots {
    int v[WP_CHUNK][4];                // {x_px, y_px, grid_row, grid_col}
};

struct WpGeom {
    int Hs, Ws, half, P, ksize, grid_h, grid_w;
    int TR, ntiles, max_rows, row_stride, mid_off, vec_store, ident;
};

template <bool F32, bool LUT>
__global__ __launch_bounds__(RU_THREADS) void wsi_patch_kernel(const uint8_t* __restrict__ slide, void* __restrict__ outv,
                                                               const WpSpots spots, const WpGeom g,
                                                               const int* __restrict__ coef, const int* __restrict__ bnd,
                                                               const float* __restrict__ nrm, const uint8_t* __restrict__ lut) {
    extern __shared__ __attribute__((aligned(16))) uint8_t wp_lds[];
    const int t = threadIdx.x, tx = t & 63, ty = t >> 6;
    const int spot = blockIdx.x / g.ntiles, tile = blockIdx.x % g.ntiles;
    const int P = g.P, win = 2 * g.half, nq = (P + 3) >> 2;
    const int cx = ru_clamp(spots.v[spot][0], 0, g.Ws - 1), cy = ru_clamp(spots.v[spot][1], 0, g.Hs - 1);
    const int gr = ru_clamp(spots.v[spot][2], 0, g.grid_h - 1), gc = ru_clamp(spots.v[spot][3], 0, g.grid_w - 1);
    const int r0 = tile * g.TR, r1 = min(r0 + g.TR, P);
    // window rows [y0, y0 + nrows) feed output rows [r0, r1)
    int y0 = r0, y1 = r1;
    if (!g.ident) {
        y0 = ru_clamp(bnd[2 * r0], 0, win);
        y1 = ru_clamp(bnd[2 * (r1 - 1)] + bnd[2 * (r1 - 1) + 1], y0, win);
    }
    const int nrows = min(y1 - y0, g.max_rows);
    const int RS = g.row_stride, nbytes = 3 * win;
    const int gx0 = cx - g.half;
    const bool inside = gx0 >= 0 && gx0 + win <= g.Ws;          // the window's columns lie in the slide: rows are contiguous runs

    // the table [3][256] behind the two images (wsi_patch_launch's LDS rule); the barrier after step 1 publishes it with the rows
    [[maybe_unused]] uint8_t* tab = wp_lds + (long)g.max_rows * (g.row_stride + (g.ident ? 0 : 3 * nq * 4));
    if constexpr (LUT)
        for (int i = t; i < WP_LUT_BYTES; i += RU_THREADS) tab[i] = lut[i];

    // 1. stage the interleaved window rows
    for (int r = ty; r < nrows; r += RU_THREADS / 64) {
        const int gy = ru_clamp(cy - g.half + y0 + r, 0, g.Hs - 1);
        const uint8_t* grow = slide + (long)gy * g.Ws * 3;
        if (inside) {
            ru_stage<64>(wp_lds + r * RS, grow + (long)gx0 * 3, nbytes, tx);    // LDS address == global address modulo 16
        } else {
            uint8_t* in = wp_lds + r * RS;
            for (int i = tx; i < nbytes; i += 64) {
                const int px = i / 3, ch = i - 3 * px;
                in[i] = grow[(long)ru_clamp(gx0 + px, 0, g.Ws - 1) * 3 + ch];
            }
        }
    }
    __syncthreads();

    if constexpr (LUT) {
        // 1b. every staged byte through its channel's table: the whole dwords of the LDS row that hold the run's bytes
        // [head, head + nbytes).  The channel of a byte is its index IN THE RUN modulo 3 - ru_stage shifted the run by its
        // address modulo 16, so the row's LDS base says nothing about it; a byte outside the run stays what it was
        for (int r = ty; r < nrows; r += RU_THREADS / 64) {
            const int gy = ru_clamp(cy - g.half + y0 + r, 0, g.Hs - 1);
            const int head = inside ? (int)(reinterpret_cast<uintptr_t>(slide + ((long)gy * g.Ws + gx0) * 3) & 15) : 0;
            uint32_t* roww = reinterpret_cast<uint32_t*>(wp_lds + r * RS);
            for (int d = (head >> 2) + tx; 4 * d < head + nbytes; d += 64) {
                const uint32_t w = roww[d];
                const int i0 = 4 * d - head;                 // index in the run of the dword's first byte: >= -3
                int ch = (i0 + 3) % 3;
                uint32_t o = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uint32_t v = (w >> (8 * b)) & 0xffu;
                    const bool in_run = i0 + b >= 0 && i0 + b < nbytes;
                    o |= (in_run ? (uint32_t)tab[ch * 256 + v] : v) << (8 * b);
                    ch = ch == 2 ? 0 : ch + 1;
                }
                roww[d] = o;
            }
        }
        __syncthreads();
    }

    const long cell = (long)gr * g.grid_w + gc;

    if (g.ident) {
        // the identity size: Pillow returns a copy - deinterleave the staged rows straight into the three planes
        for (int rr = ty; rr < nrows; rr += RU_THREADS / 64) {
            const int gy = ru_clamp(cy - g.half + y0 + rr, 0, g.Hs - 1);
            const int head = inside ? (int)(reinterpret_cast<uintptr_t>(slide + ((long)gy * g.Ws + gx0) * 3) & 15) : 0;
            const uint8_t* row = wp_lds + rr * RS + head;
            for (int e = tx; e < 3 * nq; e += 64) {
                const int c = e / nq, q = e - c * nq, xo = 4 * q;
                const RuNorm nm = ru_norm<F32>(nrm, c);
                int v[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) v[b] = xo + b < P ? (int)row[3 * (xo + b) + c] : 0;
                const long off = ((cell * 3 + c) * P + (r0 + rr)) * (long)P + xo;
                ru_store4<F32>(outv, off, xo, P, g.vec_store, v, nm);
            }
        }
        return;
    }

    // 2. horizontal pass -> mid [nrows][3][nq] dwords, deinterleaving
    uint32_t* mid = reinterpret_cast<uint32_t*>(wp_lds + g.mid_off);
    const int ks = g.ksize;
    for (int q = tx; q < nq; q += 64) {
        int xmin[4], cnt[4];
        ru_bounds4(bnd, q, P, win, ks, xmin, cnt);
        for (int rc = ty; rc < nrows * 3; rc += RU_THREADS / 64) {
            const int r = rc / 3, c = rc - 3 * r;
            const int gy = ru_clamp(cy - g.half + y0 + r, 0, g.Hs - 1);
            const int head = inside ? (int)(reinterpret_cast<uintptr_t>(slide + ((long)gy * g.Ws + gx0) * 3) & 15) : 0;
            mid[rc * nq + q] = ru_hpass4<3>(wp_lds + r * RS + head + c, coef, q, P, ks, xmin, cnt);
        }
    }
    __syncthreads();

    // 3. vertical pass: 4 consecutive output bytes of one plane per thread
    for (int rr = r0 + ty; rr < r1; rr += RU_THREADS / 64) {
        int ymin, cnt;
        ru_bounds(bnd, rr, y0, nrows, ks, ymin, cnt);
        const int* kc = coef + (long)rr * ks;
        for (int e = tx; e < 3 * nq; e += 64) {
            const int c = e / nq, q = e - c * nq, xo = 4 * q;
            const RuNorm nm = ru_norm<F32>(nrm, c);
            int v[4] = {RU_ROUND, RU_ROUND, RU_ROUND, RU_ROUND};
            for (int k = 0; k < cnt; ++k) ru_vtap4(v, mid[((ymin + k) * 3 + c) * nq + q], kc[k]);
            ru_clip4(v);
            ru_store4<F32>(outv, ((cell * 3 + c) * P + rr) * (long)P + xo, xo, P, g.vec_store, v, nm);
        }
    }
}

template <bool F32, bool LUT>
int wsi_patch_launch(const uint8_t* slide, int Hs, int Ws, const int* spots, int n, int half, int P, int grid_h, int grid_w,
                     const int* coef, const int* bnd, int ksize, void* out, const float* norm, const uint8_t* lut,
                     hipStream_t stream) {
    if (Hs <= 0 || Ws <= 0 || n < 0 || half <= 0 || P <= 0 || grid_h <= 0 || grid_w <= 0 || half > (1 << 20) || P > (1 << 14))
        return GNX_ERR_BAD_ARG;
    const int win = 2 * half;
    const int ks = ru_ksize(win, P, 2);
    if (ks > RU_MAX_KSIZE) return GNX_ERR_UNSUPPORTED;
    if (ksize != ks) return GNX_ERR_BAD_ARG;
    if (n == 0) return GNX_OK;
    if (!slide || !spots || !out || (win != P && (!coef || !bnd)) || (LUT && !lut)) return GNX_ERR_BAD_ARG;
    for (int i = 0; i < n; ++i)
        if (spots[4 * i + 2] < 0 || spots[4 * i + 2] >= grid_h || spots[4 * i + 3] < 0 || spots[4 * i + 3] >= grid_w)
            return GNX_ERR_BAD_ARG;
    WpGeom g;
    g.Hs = Hs, g.Ws = Ws, g.half = half, g.P = P, g.ksize = ks, g.grid_h = grid_h, g.grid_w = grid_w;
    g.ident = win == P;
    g.row_stride = (3 * win + 15) / 16 * 16 + 16;               // up to 15 bytes of alignment shift in front of every row
    // the tile: the most output rows whose two LDS images leave room for several workgroups per CU, but no fewer than 4 (a
    // strong reduction would stage every source row many times over); else fewer rows, up to the whole LDS
    long lds = 0;
    g.TR = ru_pick_tile(P, win, P, 2, 4, [&](int nr) {
        const long in_bytes = (long)nr * g.row_stride;
        g.mid_off = (int)in_bytes;
        return in_bytes + (g.ident ? 0 : (long)nr * 3 * ((P + 3) / 4) * 4) + (LUT ? WP_LUT_BYTES : 0);
    }, &g.max_rows, &lds);
    if (g.TR == 0) return GNX_ERR_UNSUPPORTED;
    g.ntiles = (P + g.TR - 1) / g.TR;
    if (gnx_allow_lds<wsi_patch_kernel<F32, LUT>>((size_t)lds) != GNX_OK) return GNX_ERR_LAUNCH;
    g.vec_store = ru_vec_store<F32>(out, P);
    for (int s0 = 0; s0 < n; s0 += WP_CHUNK) {
        const int ns = n - s0 < WP_CHUNK ? n - s0 : WP_CHUNK;
        WpSpots sp;
        for (int i = 0; i < ns; ++i)
            for (int j = 0; j < 4; ++j) sp.v[i][j] = spots[4 * (s0 + i) + j];
        for (int i = ns; i < WP_CHUNK; ++i) sp.v[i][0] = sp.v[i][1] = sp.v[i][2] = sp.v[i][3] = 0;
        wsi_patch_kernel<F32, LUT><<<(unsigned)(ns * g.ntiles), RU_THREADS, (size_t)lds, stream>>>(slide, out, sp, g, coef, bnd, norm,
                                                                                                lut);
        const int rc = gnx_launch_status();
        if (rc != GNX_OK) return rc;
    }
    return GNX_OK;
}

}  // namespace

GNX_EXPORT int gnx_wsi_patch_grid_u8(const uint8_t* slide, int Hs, int Ws, const int* spots, int n, int half, int P, int grid_h,
                                     int grid_w, const int* coef, const int* bnd, int ksize, uint8_t* out, hipStream_t stream) {
    return wsi_patch_launch<false, false>(slide, Hs, Ws, spots, n, half, P, grid_h, grid_w, coef, bnd, ksize, out, nullptr, nullptr,
                                          stream);
}

GNX_EXPORT int gnx_wsi_patch_grid_u8_f32(const uint8_t* slide, int Hs, int Ws, const int* spots, int n, int half, int P,
                                         int grid_h, int grid_w, const int* coef, const int* bnd, int ksize, float* out,
                                         const float* norm, hipStream_t stream) {
    return wsi_patch_launch<true, false>(slide, Hs, Ws, spots, n, half, P, grid_h, grid_w, coef, bnd, ksize, out, norm, nullptr,
                                         stream);
}

GNX_EXPORT int gnx_wsi_patch_grid_u8_lut(const uint8_t* slide, int Hs, int Ws, const int* spots, int n, int half, int P,
                                         int grid_h, int grid_w, const int* coef, const int* bnd, int ksize, uint8_t* out,
                                         const uint8_t* lut, hipStream_t stream) {
    return wsi_patch_launch<false, true>(slide, Hs, Ws, spots, n, half, P, grid_h, grid_w, coef, bnd, ksize, out, nullptr, lut,
                                         stream);
}

GNX_EXPORT int gnx_wsi_patch_grid_u8_f32_lut(const uint8_t* slide, int Hs, int Ws, const int* spots, int n, int half, int P,
                                             int grid_h, int grid_w, const int* coef, const int* bnd, int ksize, float* out,
                                             const float* norm, const uint8_t* lut, hipStream_t stream) {
    return wsi_patch_launch<true, true>(slide, Hs, Ws, spots, n, half, P, grid_h, grid_w, coef, bnd, ksize, out, norm, lut,
                                        stream);
}

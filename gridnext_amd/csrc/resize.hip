// Resize + CenterCrop of uint8 RGB patches on the device (the first two steps of the tutorials' transform:
// transforms.Resize(256), transforms.CenterCrop(224) in front of ToTensor / Normalize, image_datasets.py:102-105, :113-117).
//
// The arithmetic is Pillow's two-pass fixed-point bilinear resampling (what torchvision.transforms.Resize runs on the PIL
// images the datasets hand it), so the bytes are Pillow's bit for bit.  The resampler itself - the horizontal pass, the tap of
// the vertical one, the clamps, the staging of a byte run, the 4-wide store, and on the host the tap count, the tile search
// and the limits - is resample_u8.h, shared with wsi_patches.hip.  This file holds what is its own: planar patches, one table
// pair per axis (built on the host in double, gridnext_amd/transforms.py: axis_tables, for the crop window's columns and rows
// only - the crop commutes with both passes; an axis whose size does not change has the identity table: one tap of 2^22, the
// pass returns its input), and the tiling.
// A workgroup takes one plane and a tile of output rows:
//   1. the input rows the tile needs are ONE contiguous byte run of the plane, at any byte address: it goes into the LDS;
//   2. horizontal pass: LDS bytes -> a second LDS image [input rows][ceil(Pw / 4)] dwords;
//   3. vertical pass: one dword of that image per tap gives 4 consecutive output bytes, stored as bytes (or as floats:
//      ToTensor / Normalize with u8_pixel, the device function of gnx_u8_to_f32).
// Consecutive tiles re-read the rows they share (L2 holds them).
#include "resample_u8.h"

namespace {

template <bool F32>
__global__ __launch_bounds__(RU_THREADS) void resize_crop_kernel(
    const uint8_t* __restrict__ x, void* __restrict__ outv, int H0, int W0, int Ph, int Pw, const int* __restrict__ hcoef,
    const int* __restrict__ hbnd, int ksw, const int* __restrict__ vcoef, const int* __restrict__ vbnd, int ksh, int TR,
    int ntiles, int max_rows, int mid_off, int vec_store, const float* __restrict__ nrm) {
    extern __shared__ __attribute__((aligned(16))) uint8_t rs_lds[];
    const int t = threadIdx.x, tx = t & 63, ty = t >> 6;
    const long plane = blockIdx.x / ntiles;
    const int tile = blockIdx.x % ntiles;
    const int r0 = tile * TR, r1 = min(r0 + TR, Ph);
    const int y0 = ru_clamp(vbnd[2 * r0], 0, H0);
    const int y1 = ru_clamp(vbnd[2 * (r1 - 1)] + vbnd[2 * (r1 - 1) + 1], y0, H0);
    const int nrows = min(y1 - y0, max_rows);
    const int nq = (Pw + 3) >> 2;

    // 1. stage input rows [y0, y0 + nrows) of the plane
    const uint8_t* in = rs_lds + ru_stage<RU_THREADS>(rs_lds, x + plane * ((long)H0 * W0) + (long)y0 * W0, nrows * W0, t);
    __syncthreads();

    // 2. horizontal pass -> mid [nrows][nq] dwords
    uint32_t* mid = reinterpret_cast<uint32_t*>(rs_lds + mid_off);
    for (int q = tx; q < nq; q += 64) {
        int xmin[4], cnt[4];
        ru_bounds4(hbnd, q, Pw, W0, ksw, xmin, cnt);
        for (int r = ty; r < nrows; r += RU_THREADS / 64)
            mid[r * nq + q] = ru_hpass4<1>(in + r * W0, hcoef, q, Pw, ksw, xmin, cnt);
    }
    __syncthreads();

    // 3. vertical pass: 4 consecutive output bytes per thread
    const RuNorm nm = ru_norm<F32>(nrm, (int)(plane % 3));
    for (int rr = r0 + ty; rr < r1; rr += RU_THREADS / 64) {
        int ymin, cnt;
        ru_bounds(vbnd, rr, y0, nrows, ksh, ymin, cnt);
        const int* kc = vcoef + (long)rr * ksh;
        const long orow = (plane * Ph + rr) * (long)Pw;
        for (int q = tx; q < nq; q += 64) {
            int v[4] = {RU_ROUND, RU_ROUND, RU_ROUND, RU_ROUND};
            for (int k = 0; k < cnt; ++k) ru_vtap4(v, mid[(ymin + k) * nq + q], kc[k]);
            ru_clip4(v);
            ru_store4<F32>(outv, orow + 4 * q, 4 * q, Pw, vec_store, v, nm);
        }
    }
}

template <bool F32>
int resize_crop_launch(const uint8_t* x, void* out, long imgs, int H0, int W0, int Hr, int Wr, int top, int left, int Ph, int Pw,
                       const int* hcoef, const int* hbnd, const int* vcoef, const int* vbnd, const float* norm,
                       hipStream_t stream) {
    if (imgs < 0 || H0 <= 0 || W0 <= 0 || Hr <= 0 || Wr <= 0 || Ph <= 0 || Pw <= 0 || top < 0 || left < 0 ||
        (long)top + Ph > Hr || (long)left + Pw > Wr)
        return GNX_ERR_BAD_ARG;
    const int ksw = ru_ksize(W0, Wr, 1), ksh = ru_ksize(H0, Hr, 1);
    if (ksw > RU_MAX_KSIZE || ksh > RU_MAX_KSIZE) return GNX_ERR_UNSUPPORTED;
    if (imgs == 0) return GNX_OK;
    if (!x || !out || !hcoef || !hbnd || !vcoef || !vbnd) return GNX_ERR_BAD_ARG;
    // the two LDS images of `rows` input rows: the byte run with up to 15 bytes of alignment shift in front, then mid
    int rows = 0, mid_off = 0;
    long lds = 0;
    const int TR = ru_pick_tile(Ph, H0, Hr, 1, 1, [&](int nr) {
        const long in_bytes = ((long)nr * W0 + 15 + 15) / 16 * 16;
        mid_off = (int)in_bytes;
        return in_bytes + (long)nr * ((Pw + 3) / 4) * 4;
    }, &rows, &lds);
    if (TR == 0) return GNX_ERR_UNSUPPORTED;
    const long ntiles = (Ph + TR - 1) / TR;
    const long blocks = imgs * 3 * ntiles;
    if (blocks >= (1L << 31)) return GNX_ERR_UNSUPPORTED;
    if (gnx_allow_lds<resize_crop_kernel<F32>>((size_t)lds) != GNX_OK) return GNX_ERR_LAUNCH;
    resize_crop_kernel<F32><<<(unsigned)blocks, RU_THREADS, (size_t)lds, stream>>>(
        x, out, H0, W0, Ph, Pw, hcoef, hbnd, ksw, vcoef, vbnd, ksh, TR, (int)ntiles, rows, mid_off, ru_vec_store<F32>(out, Pw),
        norm);
    return gnx_launch_status();
}

}  // namespace

GNX_EXPORT int gnx_resize_ksize(int n_in, int n_out) {
    if (n_in <= 0 || n_out <= 0) return GNX_ERR_BAD_ARG;
    return ru_ksize(n_in, n_out, 1);
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

// Data gradient of the stem convolution (features.conv0) with respect to the NCHW patches, gfx950:
//   gnx_conv0_dgrad : dX[i][c][y][x] = sum_(o, ky, kx) dS[(i*Ho + yo)*Wo + xo][o] * w[o][c][ky][kx],
//                     yo*stride = y + pad - ky, xo*stride = x + pad - kx, integer yo in [0, Ho), xo in [0, Wo)
// - the adjoint of gnx_conv_stem (7x7 stride 2 pad 3, and the 3x3 stride 1 pad 1 stem of small_inputs), 64 -> 3 channels.
//
// A gather: one thread per input pixel, fp32 FMA, no atomics.  Every pixel sums its terms in ONE order - ky ascending, kx
// ascending, o ascending - whatever the batch, the image's place in it or the grid, so results are bit-reproducible and an
// image's gradient does not depend on its neighbours.  A workgroup takes 16 x 16 pixels of one image: w is staged once per
// workgroup as [tap][o][c] (12 contiguous floats per 4 channels of one tap), the dS rows that reach the tile - 11 x 11 conv0
// positions at stride 2, 18 x 18 at stride 1, zeros outside the map - per tile as [position][o], the position stride padded to
// an odd number of 16-B slots (ds_read_b128 of 16 neighbouring positions: 16 different slots).  At stride 2 the parity of
// (y + pad, x + pad) selects which rows and columns of the window reach a pixel (3 or 4 of the 7), so each of the four waves
// takes ONE parity class of the tile: the tap loop and the w reads are wave-uniform (LDS broadcasts), only dS differs by lane.
#include "common.h"

namespace {

bool al16b(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

constexpr int DG_TILE = 16;        // input pixels per tile side
constexpr int DG_MAX_WGS = 512;    // two workgroups per CU (71 KB of LDS at O = 64, 7x7)

__host__ __device__ constexpr int dg_rows(int stride) { return stride == 2 ? DG_TILE / 2 + 3 : DG_TILE + 2; }
// position stride in floats: O rounded up to 4, then to an odd number of 16-B slots
__host__ __device__ inline int dg_op(int O) { return (((O + 3) / 4) | 1) * 4; }

template <int STRIDE, int KS, int PAD, bool VEC>
__global__ __launch_bounds__(256) void conv0_dgrad_kernel(const float* __restrict__ dS, long ldd, const float* __restrict__ w,
                                                          float* __restrict__ dX, int H, int W, int Ho, int Wo, int O,
                                                          int tiles_x, int tiles_y, long ntiles) {
    constexpr int TR = dg_rows(STRIDE), KK = KS * KS;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int O4 = (O + 3) / 4 * 4, OQ = O4 / 4, OP = dg_op(O);
    float* lw = lds;                         // [KK][O4][3]
    float* ld = lds + KK * O4 * 3;           // [TR * TR][OP]   (KK * O4 * 3 floats: a multiple of 16 B)
    const int tid = threadIdx.x;

    for (int i = tid; i < KK * O4 * 3; i += 256) {
        const int c = i % 3, o = (i / 3) % O4, tap = i / (3 * O4);
        lw[i] = o < O ? w[((long)o * 3 + c) * KK + tap] : 0.f;
    }

    int ly, lx;                              // this thread's pixel in the tile
    if (STRIDE == 2) {
        const int cls = tid >> 6, lane = tid & 63;
        ly = 2 * (lane >> 3) + (cls >> 1);
        lx = 2 * (lane & 7) + (cls & 1);
    } else {
        ly = tid >> 4;
        lx = tid & 15;
    }

    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tx = (int)(t % tiles_x), ty = (int)((t / tiles_x) % tiles_y);
        const long img = t / ((long)tiles_x * tiles_y);
        const int y0 = ty * DG_TILE, x0 = tx * DG_TILE;
        const int yb = y0 / STRIDE - 1, xb = x0 / STRIDE - 1;        // first conv0 row / column that reaches the tile
        __syncthreads();                                             // the previous tile's reads (first tile: lw is whole)
        for (int i = tid; i < TR * TR * OQ; i += 256) {
            const int q = i % OQ, p = i / OQ;
            const int yo = yb + p / TR, xo = xb + p % TR;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (yo >= 0 && yo < Ho && xo >= 0 && xo < Wo) {
                const float* src = dS + ((img * Ho + yo) * Wo + xo) * ldd + 4 * q;
                if (VEC && 4 * q + 3 < O) {
                    v = *reinterpret_cast<const f32x4*>(src);
                } else {                                             // columns past O are not ours to read
                    v.x = src[0];
                    if (4 * q + 1 < O) v.y = src[1];
                    if (4 * q + 2 < O) v.z = src[2];
                    if (4 * q + 3 < O) v.w = src[3];
                }
            }
            *reinterpret_cast<f32x4*>(ld + p * OP + 4 * q) = v;
        }
        __syncthreads();
        const int y = y0 + ly, x = x0 + lx;
        if (y >= H || x >= W) continue;                              // (no barrier below)
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int ky = (y + PAD) % STRIDE; ky < KS; ky += STRIDE) {
            const int r = (y + PAD - ky) / STRIDE - yb;              // in [0, TR): positions outside the map hold zeros
            for (int kx = (x + PAD) % STRIDE; kx < KS; kx += STRIDE) {
                const int cc = (x + PAD - kx) / STRIDE - xb;
                const float* dp = ld + (r * TR + cc) * OP;
                const float* wp = lw + (ky * KS + kx) * O4 * 3;
                for (int q = 0; q < OQ; ++q) {
                    const f32x4 d = *reinterpret_cast<const f32x4*>(dp + 4 * q);
                    const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp + 12 * q);
                    const f32x4 w1 = *reinterpret_cast<const f32x4*>(wp + 12 * q + 4);
                    const f32x4 w2 = *reinterpret_cast<const f32x4*>(wp + 12 * q + 8);
                    a0 = fmaf(d.x, w0.x, a0); a1 = fmaf(d.x, w0.y, a1); a2 = fmaf(d.x, w0.z, a2);
                    a0 = fmaf(d.y, w0.w, a0); a1 = fmaf(d.y, w1.x, a1); a2 = fmaf(d.y, w1.y, a2);
                    a0 = fmaf(d.z, w1.z, a0); a1 = fmaf(d.z, w1.w, a1); a2 = fmaf(d.z, w2.x, a2);
                    a0 = fmaf(d.w, w2.y, a0); a1 = fmaf(d.w, w2.z, a1); a2 = fmaf(d.w, w2.w, a2);
                }
            }
        }
        float* out = dX + ((img * 3 * H + y) * (long)W + x);
        out[0] = a0;
        out[(long)H * W] = a1;
        out[2L * H * W] = a2;
    }
}

template <int STRIDE, int KS, int PAD, bool VEC>
int dgrad_launch(const float* dS, long ldd, const float* w, float* dX, long imgs, int H, int W, int Ho, int Wo, int O,
                 hipStream_t stream) {
    constexpr int TR = dg_rows(STRIDE), KK = KS * KS;
    const size_t lds_max = ((size_t)KK * 64 * 3 + (size_t)TR * TR * dg_op(64)) * sizeof(float);
    if (gnx_allow_lds<conv0_dgrad_kernel<STRIDE, KS, PAD, VEC>>(lds_max) != GNX_OK) return GNX_ERR_LAUNCH;
    const int O4 = (O + 3) / 4 * 4;
    const size_t lds_bytes = ((size_t)KK * O4 * 3 + (size_t)TR * TR * dg_op(O)) * sizeof(float);
    const int tiles_x = gnx_cdiv(W, DG_TILE), tiles_y = gnx_cdiv(H, DG_TILE);
    const long ntiles = imgs * tiles_x * tiles_y;
    const int blocks = (int)(ntiles < DG_MAX_WGS ? ntiles : DG_MAX_WGS);
    conv0_dgrad_kernel<STRIDE, KS, PAD, VEC><<<blocks, 256, lds_bytes, stream>>>(dS, ldd, w, dX, H, W, Ho, Wo, O, tiles_x,
                                                                                tiles_y, ntiles);
    return gnx_launch_status();
}

}  // namespace

// dX [imgs][3][H][W] from dS [imgs*Ho*Wo][O] (ldd) and conv0's weight w [O][3][KH][KW]; every element of dX is written
GNX_EXPORT int gnx_conv0_dgrad(const float* dS, long ldd, const float* w, float* dX, long imgs, int H, int W, int O, int KH,
                               int KW, int stride, int pad, hipStream_t stream) {
    if (!dS || !w || !dX || imgs <= 0 || H <= 0 || W <= 0 || O <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad < 0 ||
        ldd < O)
        return GNX_ERR_BAD_ARG;
    const bool s2 = stride == 2 && KH == 7 && KW == 7 && pad == 3, s1 = stride == 1 && KH == 3 && KW == 3 && pad == 1;
    if (!(s2 || s1) || O > 64) return GNX_ERR_UNSUPPORTED;
    const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
    const bool vec = ldd % 4 == 0 && al16b(dS);
    if (s2)
        return vec ? dgrad_launch<2, 7, 3, true>(dS, ldd, w, dX, imgs, H, W, Ho, Wo, O, stream)
                   : dgrad_launch<2, 7, 3, false>(dS, ldd, w, dX, imgs, H, W, Ho, Wo, O, stream);
    return vec ? dgrad_launch<1, 3, 1, true>(dS, ldd, w, dX, imgs, H, W, Ho, Wo, O, stream)
               : dgrad_launch<1, 3, 1, false>(dS, ldd, w, dX, imgs, H, W, Ho, Wo, O, stream);
}

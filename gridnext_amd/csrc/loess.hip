// Direct loess on the device: the local polynomial fit of log10(variance) on log10(mean) inside the Seurat-v3 gene selection
// (the reference's notebooks/register_hvgs.ipynb: sc.pp.highly_variable_genes(flavor='seurat_v3'), whose genes become
// gridnext/count_datasets.py's select_genes).  The abscissae are sorted; the host has chosen every evaluation point's window
// [lo, lo + cnt), its 1 / h and its degree (gridnext_amd/hvg.py); the weighted sums and the solve are done here.
//
// One wavefront per evaluation point i, x0 = xs[i].  Lane j takes the window's elements j, j + 64, ... in that order:
//     u = (xs[k] - x0) * inv_h,  a = |u|,  w = (1 - a^3)^3 for a < 1, else 0;  inv_h == 0: w = 1 (and u = 0)
//     p1 = w u, p2 = p1 u, p3 = p2 u, p4 = p3 u            (plain products)
//     m0 += w, m1 += p1, m2 += p2, m3 += p3, m4 += p4;    r0 = fma(w, y, r0), r1 = fma(p1, y, r1), r2 = fma(p2, y, r2)
// all in double from 0.0, then the eight sums go through the fixed shuffle tree of wave_sum_d, and lane 0 solves the symmetric
// system M beta = r, M[a][b] = m(a+b), by LDL^T without pivoting, in this order:
//     degree 0:  beta0 = r0 / m0
//     degree 1:  l10 = m1 / m0, d1 = m2 - l10 m1, z1 = r1 - l10 r0, b1 = z1 / d1, beta0 = r0 / m0 - l10 b1
//     degree 2:  l10 = m1 / m0, l20 = m2 / m0, d1 = m2 - l10 m1, l21 = (m3 - l20 m1) / d1, d2 = (m4 - l20 m2) - l21 (l21 d1),
//                z1 = r1 - l10 r0, z2 = (r2 - l20 r0) - l21 z1, b2 = z2 / d2, b1 = z1 / d1 - l21 b2,
//                beta0 = (r0 / m0 - l10 b1) - l20 b2
// This file is compiled under `#pragma clang fp contract(off)`: a product and a sum are fused only where fma is written, so the
// operations above are the operations executed.
// The order depends on the point's window alone: equal inputs give equal bits.  No atomics, out[i] is written exactly once.
//
// Nothing outside [0, n) is read whatever lo and cnt hold: the window is cut to the array in the kernel.  A degree outside 0 .. 2
// cannot be seen by the launcher (the array lives on the device and the launcher never synchronises): that point's result is
// NaN; gridnext_amd/hvg.py refuses such a degree on the host, before the upload.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int LO_THREADS = 256;
constexpr int LO_WAVES = LO_THREADS / 64;
constexpr long LO_MAX = 2147483647L;             // points of one launch: window positions are int32

__device__ __forceinline__ double loess_solve(int degree, double m0, double m1, double m2, double m3, double m4, double r0,
                                              double r1, double r2) {
    if (degree == 0) return r0 / m0;
    const double l10 = m1 / m0;
    const double d1 = m2 - l10 * m1;
    const double z1 = r1 - l10 * r0;
    if (degree == 1) {
        const double b1 = z1 / d1;
        return r0 / m0 - l10 * b1;
    }
    const double l20 = m2 / m0;
    const double l21 = (m3 - l20 * m1) / d1;
    const double d2 = (m4 - l20 * m2) - l21 * (l21 * d1);
    const double z2 = (r2 - l20 * r0) - l21 * z1;
    const double b2 = z2 / d2;
    const double b1 = z1 / d1 - l21 * b2;
    return (r0 / m0 - l10 * b1) - l20 * b2;
}

__global__ __launch_bounds__(LO_THREADS) void loess_fit_kernel(const double* __restrict__ xs, const double* __restrict__ ys, int64_t n,
                                                               const int32_t* __restrict__ lo, const int32_t* __restrict__ cnt,
                                                               const double* __restrict__ inv_h, const int32_t* __restrict__ degree,
                                                               double* __restrict__ out, int64_t n_eval) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * LO_WAVES + (threadIdx.x >> 6);           // the same in the whole wavefront
    if (i >= n_eval) return;
    const double x0 = xs[i], ih = inv_h[i];
    int64_t b = lo[i], e = b + (int64_t)cnt[i];
    b = b < 0 ? 0 : b;                           // the window, cut to the array
    e = e > n ? n : e;
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0, r0 = 0.0, r1 = 0.0, r2 = 0.0;
    for (int64_t k = b + lane; k < e; k += 64) {
        const double u = (xs[k] - x0) * ih, y = ys[k];
        const double a = fabs(u);
        const double c = 1.0 - a * a * a;
        const double w = ih == 0.0 ? 1.0 : (a < 1.0 ? c * c * c : 0.0);
        const double p1 = w * u, p2 = p1 * u, p3 = p2 * u, p4 = p3 * u;
        m0 += w, m1 += p1, m2 += p2, m3 += p3, m4 += p4;
        r0 = fma(w, y, r0), r1 = fma(p1, y, r1), r2 = fma(p2, y, r2);
    }
    m0 = wave_sum_d(m0), m1 = wave_sum_d(m1), m2 = wave_sum_d(m2), m3 = wave_sum_d(m3), m4 = wave_sum_d(m4);
    r0 = wave_sum_d(r0), r1 = wave_sum_d(r1), r2 = wave_sum_d(r2);
    if (lane != 0) return;
    const int d = degree[i];
    out[i] = d < 0 || d > 2 ? __builtin_nan("") : loess_solve(d, m0, m1, m2, m3, m4, r0, r1, r2);
}

}  // namespace

GNX_EXPORT int gnx_loess_fit_f64(const double* xs, const double* ys, long n, const int* lo, const int* cnt, const double* inv_h,
                                 const int* degree, double* out, long n_eval, hipStream_t stream) {
    if (n < 0 || n_eval < 0 || n_eval > n) return GNX_ERR_BAD_ARG;
    if (n > LO_MAX) return GNX_ERR_UNSUPPORTED;
    if (n_eval == 0) return GNX_OK;
    if (!xs || !ys || !lo || !cnt || !inv_h || !degree || !out) return GNX_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(xs) | reinterpret_cast<uintptr_t>(ys) | reinterpret_cast<uintptr_t>(inv_h) |
         reinterpret_cast<uintptr_t>(out)) & 7)
        return GNX_ERR_BAD_ARG;
    loess_fit_kernel<<<(unsigned)gnx_cdiv(n_eval, LO_WAVES), LO_THREADS, 0, stream>>>(xs, ys, n, lo, cnt, inv_h, degree, out, n_eval);
    return gnx_launch_status();
}

// Empty spots of an array: which patches of a batch are all-zero, as ordered index lists.
// A frozen eval-mode network maps every all-zero patch to the same row, so the eval forward (densenet.py) runs the
// non-empty spots plus ONE empty one and copies that row to the others.  This file finds them and does the copy:
//   gnx_spot_compact:         patches (any element type, bytes) -> fg_idx / bg_idx / counts
//   gnx_spot_broadcast_rows:  row bg_idx[0] of a matrix -> rows bg_idx[1 ...]
#include "common.h"

namespace {

constexpr int SC_UNR = 4;          // 16-B pieces per thread and slab after the first one (16 KB slabs)

// empty[spot] = 1 iff every byte of the spot's q16 16-B pieces is zero (bitwise: -0.0 and NaN are not empty).
// One workgroup per spot; it leaves at the first slab holding a non-zero byte (first slab 4 KB, then 16 KB each), so a
// foreground spot costs a few KB of reads and only the empty ones are read whole.
__global__ __launch_bounds__(256) void spot_scan_kernel(const uint4* __restrict__ x, long q16, int* __restrict__ empty) {
    const uint4* __restrict__ p = x + (long)blockIdx.x * q16;
    const int t = threadIdx.x;
    int nonzero = 0;
    long base = 0;
    for (int unr = 1; base < q16 && !nonzero; base += 256L * unr, unr = SC_UNR) {
        unsigned acc = 0u;
#pragma unroll
        for (int u = 0; u < SC_UNR; ++u) {
            const long j = base + 256L * u + t;
            if (u < unr && j < q16) {
                const uint4 v = p[j];
                acc |= v.x | v.y | v.z | v.w;
            }
        }
        nonzero = __syncthreads_or(acc != 0u);
    }
    if (t == 0) empty[blockIdx.x] = nonzero ? 0 : 1;
}

// Ordered compaction of the flags by ONE workgroup (the arrays it serves hold thousands of spots): fg_idx[0 .. n_fg) = the
// non-empty spots ascending, bg_idx[0 .. n_bg) = the empty ones ascending, counts = {n_fg, n_bg}.  Positions are prefix
// sums (wave ballots + a fixed-order sum over the waves), no atomics: the lists are the same on every run.  The rest of
// fg_idx, [n_fg, N), is filled with the first empty spot (0 if there is none): fg_idx[0 .. n) for any n <= N is then a
// list of the non-empty spots padded with an empty one.
__global__ __launch_bounds__(1024) void spot_compact_kernel(const int* __restrict__ empty, long N, int* __restrict__ fg_idx,
                                                            int* __restrict__ bg_idx, int* __restrict__ counts) {
    __shared__ int wf[16], wb[16], first_bg;
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    if (t == 0) first_bg = 0;
    long nf = 0, nb = 0;                                   // running totals, the same in every thread
    for (long start = 0; start < N; start += 1024) {
        const long i = start + t;
        const int e = i < N ? empty[i] : -1;
        const unsigned long long mf = __ballot(e == 0), mb = __ballot(e == 1);
        const unsigned long long below = (1ull << lane) - 1ull;
        __syncthreads();                                   // the previous round's wf / wb reads are done
        if (lane == 0) { wf[wid] = __popcll(mf); wb[wid] = __popcll(mb); }
        __syncthreads();
        int of = 0, ob = 0, tf = 0, tb = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k < wid) { of += wf[k]; ob += wb[k]; }
            tf += wf[k]; tb += wb[k];
        }
        if (e == 0) fg_idx[nf + of + __popcll(mf & below)] = (int)i;
        if (e == 1) {
            const long pos = nb + ob + __popcll(mb & below);
            bg_idx[pos] = (int)i;
            if (pos == 0) first_bg = (int)i;
        }
        nf += tf;
        nb += tb;
    }
    __syncthreads();
    const int fill = first_bg;
    for (long j = nf + t; j < N; j += 1024) fg_idx[j] = fill;
    if (t == 0) { counts[0] = (int)nf; counts[1] = (int)nb; }
}

// rows[bg_idx[r]][0 .. C) = rows[bg_idx[0]][0 .. C) for r = 1 .. n_bg - 1 (entries outside [0, n_rows) are skipped)
__global__ __launch_bounds__(256) void spot_broadcast_rows_kernel(float* __restrict__ rows, long ld, int C,
                                                                  const int* __restrict__ bg_idx, long n_bg, long n_rows) {
    const long src = bg_idx[0];
    if (src < 0 || src >= n_rows) return;
    const long total = (n_bg - 1) * C;
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (long)gridDim.x * blockDim.x) {
        const long r = k / C;
        const int c = (int)(k - r * C);
        const long dst = bg_idx[1 + r];
        if (dst >= 0 && dst < n_rows) rows[dst * ld + c] = rows[src * ld + c];
    }
}

}  // namespace

// x: N spots of spot_bytes bytes each, contiguous (16 | spot_bytes, 16-B aligned; GNX_ERR_UNSUPPORTED otherwise).
// A spot is EMPTY iff all its bytes are zero.  Device ints out: fg_idx [N] (the non-empty spots ascending, then the first
// empty spot repeated up to N), bg_idx [N] (the empty spots ascending in [0, n_bg)), counts {n_fg, n_bg}; flags [N] is scratch.
GNX_EXPORT int gnx_spot_compact(const void* x, long spot_bytes, long N, int* flags, int* fg_idx, int* bg_idx, int* counts,
                                hipStream_t stream) {
    if (!x || !flags || !fg_idx || !bg_idx || !counts || spot_bytes <= 0 || N < 0) return GNX_ERR_BAD_ARG;
    if (spot_bytes % 16 != 0 || (reinterpret_cast<uintptr_t>(x) & 15) != 0 || N > 2147483647L) return GNX_ERR_UNSUPPORTED;
    if (N > 0)
        spot_scan_kernel<<<(unsigned)N, 256, 0, stream>>>(reinterpret_cast<const uint4*>(x), spot_bytes / 16, flags);
    spot_compact_kernel<<<1, 1024, 0, stream>>>(flags, N, fg_idx, bg_idx, counts);
    return gnx_launch_status();
}

// rows [n_rows][C] (ld): copy row bg_idx[0] to the rows bg_idx[1 .. n_bg) (device ints, as gnx_spot_compact wrote them)
GNX_EXPORT int gnx_spot_broadcast_rows(float* rows, long ld, long n_rows, int C, const int* bg_idx, long n_bg,
                                       hipStream_t stream) {
    if (!rows || !bg_idx || ld < C || C <= 0 || n_rows <= 0 || n_bg < 0 || n_bg > n_rows) return GNX_ERR_BAD_ARG;
    if (n_bg <= 1) return GNX_OK;
    long blocks = ((n_bg - 1) * C + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    spot_broadcast_rows_kernel<<<(unsigned)blocks, 256, 0, stream>>>(rows, ld, C, bg_idx, n_bg, n_rows);
    return gnx_launch_status();
}

// A Linear layer over sparse count rows (the first layer of the count classifier, Tutorial_visium_count.ipynb cell 12, without
// the dense operand): forward over the resident CSR, weight gradient over the resident per-array CSCs.  Lines, idx, val and
// lineptr are the ones of sparse_counts.hip.
//
// Both passes are one kernel, a GATHER-SUM: output row r = init row + sum over the kept entries e of line(r), in entry order,
// of val[e] * M[map(idx[e])][.], M a dense row-major matrix.
//   forward          line = a spot, map = gene -> channel, M = the gene-major weight W[G][F], init = the bias;
//   weight gradient  line = a gene of one array's CSC, map = the array's row -> position in the batch, M = dY[B][F],
//                    init = dW as it is (accumulate) or nothing.
// The inverted index (per destination, the list of its contribution rows, in fixed order) replaces the float atomics a
// scatter of val * dY rows into dW would need: every output element has one owner and one summation order.
//
// One workgroup per (output row, slice of F); a thread owns VEC adjacent features of that row and keeps ONE chain per feature:
// acc = 0.0f, then acc = fmaf(val[e], M[row(e)][f], acc) over the kept entries in entry order, then out = init + acc (init is
// 0.0f where there is none).  The chain is a function of the line alone - not of the row's place in the launch, of the other
// lines, of the slice or of VEC - so a row has the same bits alone, in any batch, and at any alignment: VEC = 4 (dwordx4 loads
// of M where M and its leading dimension are 16-byte multiples) and VEC = 1 differ in how the bytes are fetched, never in the
// arithmetic.  Each wavefront reads the line 64 entries at a time (coalesced idx / val loads, one map look-up per lane), takes a
// ballot of the kept entries and walks the hits with the row index and the value broadcast from the owning lane; SL_FLIGHT
// rows of M are requested before the first of their multiply-adds.
#include "sparse_lines.h"

namespace {

constexpr int SL_THREADS = 256;                  // at most; a multiple of 64 that covers the slice
constexpr int SL_FLIGHT = 4;                     // rows of M in flight per wavefront
constexpr long SL_MAX_F = 1L << 20;

template <int VEC>
__device__ __forceinline__ void sl_load(float (&w)[VEC], const float* __restrict__ p, int nf) {
    if constexpr (VEC == 4) {
        if (nf == 4) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(p);
            w[0] = t.x, w[1] = t.y, w[2] = t.z, w[3] = t.w;
            return;
        }
    }
#pragma unroll
    for (int q = 0; q < VEC; ++q) w[q] = q < nf ? p[q] : 0.f;                // the row's last, partial group: dwords
}

// init and out may be the same buffer (the accumulating weight gradient): neither is __restrict__
template <int VEC>
__global__ __launch_bounds__(SL_THREADS) void sl_gather_sum_kernel(const int64_t* __restrict__ lineptr, const int32_t* __restrict__ idx,
                                                                   const float* __restrict__ val, const int32_t* __restrict__ lines,
                                                                   const int32_t* __restrict__ map, const float* __restrict__ M,
                                                                   int64_t ldm, const float* init, int64_t ld_init, float* out,
                                                                   int64_t ld_out, int F, int out_vec) {
    const int lane = threadIdx.x & 63;
    const int64_t row = blockIdx.x;
    const int64_t f0 = ((int64_t)blockIdx.y * blockDim.x + threadIdx.x) * VEC;
    if (f0 - (int64_t)lane * VEC >= F) return;                               // the whole wavefront lies behind F
    const int nf = f0 >= F ? 0 : (F - f0 < VEC ? (int)(F - f0) : VEC);       // 0 .. VEC features of this thread

    float acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.f;

    const LineRange ln = line_range(lineptr, lines, row);
    for (int64_t k0 = ln.b; k0 < ln.e; k0 += 64) {
        const int64_t k = k0 + lane;
        int m = -1;
        float v = 0.f;
        if (k < ln.e) {
            const int32_t j = idx[k];
            m = map ? map[j] : j;
            v = val[k];
        }
        unsigned long long hits = __ballot(m >= 0);
        while (hits) {
            int r[SL_FLIGHT], n = 0, j = 0;
            float x[SL_FLIGHT];
#pragma unroll
            for (int u = 0; u < SL_FLIGHT; ++u) {
                if (hits) {                                                  // wave-uniform
                    j = __builtin_ctzll(hits);
                    hits &= hits - 1;
                    n = u + 1;
                }                                                            // else: the last hit's row again, not added
                r[u] = lane_get(m, j);
                x[u] = lane_get(v, j);
            }
            float w[SL_FLIGHT][VEC];
#pragma unroll
            for (int u = 0; u < SL_FLIGHT; ++u) sl_load<VEC>(w[u], M + (int64_t)r[u] * ldm + f0, nf);
#pragma unroll
            for (int u = 0; u < SL_FLIGHT; ++u) {
                if (u < n) {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) acc[q] = fmaf(x[u], w[u][q], acc[q]);
                }
            }
        }
    }

    if (nf == 0) return;
    float res[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) res[q] = (init && q < nf ? init[row * ld_init + f0 + q] : 0.f) + acc[q];
    float* o = out + row * ld_out + f0;
    if constexpr (VEC == 4) {
        if (nf == 4 && out_vec) {
            *reinterpret_cast<f32x4*>(o) = f32x4{res[0], res[1], res[2], res[3]};
            return;
        }
    }
#pragma unroll
    for (int q = 0; q < VEC; ++q)
        if (q < nf) o[q] = res[q];
}

bool sl_vec_ok(const void* p, long ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; }

int sl_launch(const long long* lineptr, const int* idx, const float* val, const int* lines, long n_rows, const int* map,
              const float* M, long ldm, const float* init, long ld_init, float* out, long ld_out, int F, hipStream_t stream) {
    const bool vec = F >= 4 && sl_vec_ok(M, ldm);
    const int per_thread = vec ? 4 : 1;
    const int want = (gnx_cdiv(F, per_thread) + 63) / 64 * 64;
    const int threads = want < SL_THREADS ? want : SL_THREADS;
    const dim3 grid((unsigned)n_rows, (unsigned)gnx_cdiv(F, (long)threads * per_thread));
    const auto* ptr = reinterpret_cast<const int64_t*>(lineptr);
    if (vec)
        sl_gather_sum_kernel<4><<<grid, threads, 0, stream>>>(ptr, idx, val, lines, map, M, ldm, init, ld_init, out, ld_out, F,
                                                              sl_vec_ok(out, ld_out) ? 1 : 0);
    else
        sl_gather_sum_kernel<1><<<grid, threads, 0, stream>>>(ptr, idx, val, lines, map, M, ldm, init, ld_init, out, ld_out, F, 0);
    return gnx_launch_status();
}

}  // namespace

GNX_EXPORT long gnx_sparse_linear_max_f(void) { return SL_MAX_F; }

GNX_EXPORT int gnx_sparse_linear_fwd_f32(const long long* lineptr, const int* idx, const float* val, const int* lines, long n_lines,
                                         const int* chan_of_idx, const float* W, long ldw, const float* bias, float* out,
                                         long ld_out, long F, hipStream_t stream) {
    const bool bad = F <= 0 || ldw < F || ld_out < F || !W || !out || lines_misaligned(W) || lines_misaligned(out) ||
                     lines_misaligned(bias) || lines_misaligned(val);
    const int go = lines_preamble(n_lines, lineptr, bad, F > SL_MAX_F, idx, val);
    if (go != LINES_GO) return go;
    return sl_launch(lineptr, idx, val, lines, n_lines, chan_of_idx, W, ldw, bias, 0, out, ld_out, (int)F, stream);
}

GNX_EXPORT int gnx_sparse_linear_wgrad_f32(const long long* lineptr, const int* idx, const float* val, const int* gene_lines,
                                           long n_channels, const int* pos_of_idx, const float* dY, long ld_dy, float* dW, long ldw,
                                           long F, int accumulate, hipStream_t stream) {
    const bool bad = F <= 0 || ldw < F || ld_dy < F || !dY || !dW || lines_misaligned(dY) || lines_misaligned(dW) ||
                     lines_misaligned(val);
    const int go = lines_preamble(n_channels, lineptr, bad, F > SL_MAX_F, idx, val);
    if (go != LINES_GO) return go;
    return sl_launch(lineptr, idx, val, gene_lines, n_channels, pos_of_idx, dY, ld_dy, accumulate ? dW : nullptr, ldw, dW, ldw,
                     (int)F, stream);
}

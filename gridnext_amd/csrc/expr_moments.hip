// Per-gene moments of an expression prediction against sparse counts (the evaluation the reference's
// notebooks/counts_from_img.ipynb stops short of: which genes the image predicts - the per-gene Pearson correlation, R^2 and
// MSE between sigmoid(z) and the [0, 1]-scaled counts over held-out spots).  Everything a per-gene statistic needs is five
// sums per gene channel c, kept in double in a table M[G][ld_m]:
//   column 0  sum p      column 1  sum p^2                     over ALL rows of the batch     (dense half: z alone)
//   column 2  sum t      column 3  sum t^2    column 4  sum p t over the STORED entries        (sparse half: t is 0 elsewhere)
// with p = act((double) z) and t = (double) fl32(val * gene_scale[c]).  No dense (B, G) target is ever formed.
//
// Dense half.  One workgroup of 1 024 threads per EM_COLS = 8 adjacent columns: EM_STRIPS = 128 strips of 8 threads, thread
// (strip s, column c).  Strip s adds the rows s, s + 128, s + 256, ... in that order into its own pair of doubles (s1 += p,
// s2 = fma(p, p, s2)), the 128 pairs go to the LDS, and the column's thread of strip 0 adds them in strip order:
// total = ((strip 0 + strip 1) + strip 2) + ... + strip 127, then M = total (accumulate == 0) or M = M + total.  The order is a
// function of B alone - not of G, ldz, the alignment or the other columns.  B is not split over workgroups: there is no
// workspace in the interface, no second launch and no counter.
// The tile is narrow because the sigmoid in double, not the memory, bounds this kernel: at 4 992 x 2 000 the time was
// proportional to 1 / workgroups from 64 columns (32 workgroups, 237 us) down to 8 (250 workgroups on 256 CUs, 39 us), about
// 150 fp64 issue slots per element either way.  A wavefront then reads 8 rows x 32 bytes per load; an order of the tiles that
// keeps neighbours on one XCD changed nothing measurable (37.9 against 38.9 us) and is not there.
//
// Sparse half.  The walk of sc_line_reduce_kernel<ScMoments> (sparse_counts.hip): one wavefront per channel, lane j adds the
// line's entries j, j + 64, ... in that order (the dropped ones skipped), then wave_sum_d's fixed shuffle tree, then lane 0 stores.
//
// No atomics; every store is a vector store of plain C++.  exp() is the device library's double exp, taken to lie within
// 1 ulp; the bound of include/gridnext_hip.h leaves 16 roundings per term for it, the add, the divide and the product.
#include "sparse_lines.h"

namespace {

constexpr int EM_COLS = 8;                       // columns per workgroup: see the note on the tile above
constexpr int EM_THREADS = 1024;
constexpr int EM_STRIPS = EM_THREADS / EM_COLS;  // 128
constexpr int EM_UNROLL = 4;                     // rows of a strip requested before the first of their sums
constexpr int EM_WAVES = 4;                      // lines per workgroup of the sparse half

template <int ACT>
__device__ __forceinline__ double em_act(float z) {
    const double x = (double)z;
    if constexpr (ACT == GNX_ACT_SIGMOID) {
        if (x >= 0.0) return 1.0 / (1.0 + exp(-x));
        const double e = exp(x);
        return e / (1.0 + e);
    }
    return x;
}

template <int ACT>
__global__ __launch_bounds__(EM_THREADS) void em_col_moments_kernel(const float* __restrict__ z, int64_t ldz, int64_t B, int64_t G,
                                                                    double* __restrict__ M, int64_t ld_m, int accumulate) {
    __shared__ double part[EM_STRIPS][2][EM_COLS];
    const int lane = threadIdx.x % EM_COLS, strip = threadIdx.x / EM_COLS;
    const int64_t c = (int64_t)blockIdx.x * EM_COLS + lane;
    const bool live = c < G;
    double s1 = 0.0, s2 = 0.0;
    if (live) {
        const float* col = z + c;
        int64_t r = strip;
        for (; r + (int64_t)(EM_UNROLL - 1) * EM_STRIPS < B; r += (int64_t)EM_UNROLL * EM_STRIPS) {
            float v[EM_UNROLL];
#pragma unroll
            for (int u = 0; u < EM_UNROLL; ++u) v[u] = col[(r + (int64_t)u * EM_STRIPS) * ldz];
#pragma unroll
            for (int u = 0; u < EM_UNROLL; ++u) {
                const double p = em_act<ACT>(v[u]);
                s1 += p;
                s2 = fma(p, p, s2);
            }
        }
        for (; r < B; r += EM_STRIPS) {
            const double p = em_act<ACT>(col[r * ldz]);
            s1 += p;
            s2 = fma(p, p, s2);
        }
    }
    part[strip][0][lane] = s1;
    part[strip][1][lane] = s2;
    __syncthreads();
    if (strip == 0 && live) {
        double t1 = part[0][0][lane], t2 = part[0][1][lane];
#pragma unroll
        for (int s = 1; s < EM_STRIPS; ++s) {
            t1 += part[s][0][lane];
            t2 += part[s][1][lane];
        }
        double* row = M + c * ld_m;
        row[0] = accumulate ? row[0] + t1 : t1;
        row[1] = accumulate ? row[1] + t2 : t2;
    }
}

template <int ACT>
__global__ __launch_bounds__(EM_WAVES * 64) void em_sparse_moments_kernel(const int64_t* __restrict__ lineptr, const int32_t* __restrict__ idx,
                                                                          const float* __restrict__ val, const int32_t* __restrict__ gene_lines,
                                                                          int64_t n_channels, const int32_t* __restrict__ pos_of_idx,
                                                                          const float* __restrict__ gene_scale, const float* __restrict__ z,
                                                                          int64_t ldz, double* __restrict__ M, int64_t ld_m, int accumulate) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * EM_WAVES + (threadIdx.x >> 6);         // the same in the whole wavefront
    if (c >= n_channels) return;
    const LineRange r = line_range(lineptr, gene_lines, c);
    double st = 0.0, stt = 0.0, spt = 0.0;
    const float scale = gene_scale ? gene_scale[c] : 1.f;
    for (int64_t k = r.b + lane; k < r.e; k += 64) {
        const int32_t j = idx[k];
        const int64_t pos = pos_of_idx ? (int64_t)pos_of_idx[j] : (int64_t)j;
        if (pos < 0) continue;
        const float tf = gene_scale ? val[k] * scale : val[k];                      // the fp32 product: the criterion's target
        const double t = (double)tf;
        const double p = em_act<ACT>(z[pos * ldz + c]);
        st += t;
        stt = fma(t, t, stt);
        spt = fma(p, t, spt);
    }
    st = wave_sum_d(st);
    stt = wave_sum_d(stt);
    spt = wave_sum_d(spt);
    if (lane == 0) {
        double* row = M + c * ld_m;
        row[2] = accumulate ? row[2] + st : st;
        row[3] = accumulate ? row[3] + stt : stt;
        row[4] = accumulate ? row[4] + spt : spt;
    }
}

bool em_known(int activation) { return activation == GNX_ACT_NONE || activation == GNX_ACT_SIGMOID; }

}  // namespace

GNX_EXPORT int gnx_act_col_moments_f64(const float* z, long ldz, long B, long G, int activation, double* M, long ld_m,
                                       int accumulate, hipStream_t stream) {
    if (!z || !M || B < 0 || G < 0 || ldz < G || ld_m < 5 || !em_known(activation)) return GNX_ERR_BAD_ARG;
    if (lines_misaligned(M, 8) || lines_misaligned(z)) return GNX_ERR_BAD_ARG;
    if (G > LINES_MAX) return GNX_ERR_UNSUPPORTED;
    if (G == 0) return GNX_OK;
    const unsigned grid = (unsigned)gnx_cdiv(G, EM_COLS);
    if (activation == GNX_ACT_SIGMOID)
        em_col_moments_kernel<GNX_ACT_SIGMOID><<<grid, EM_THREADS, 0, stream>>>(z, ldz, B, G, M, ld_m, accumulate ? 1 : 0);
    else
        em_col_moments_kernel<GNX_ACT_NONE><<<grid, EM_THREADS, 0, stream>>>(z, ldz, B, G, M, ld_m, accumulate ? 1 : 0);
    return gnx_launch_status();
}

GNX_EXPORT int gnx_sparse_pred_moments_f64(const long long* lineptr, const int* idx, const float* val, const int* gene_lines,
                                           long n_channels, const int* pos_of_idx, const float* gene_scale, const float* z,
                                           long ldz, int activation, double* M, long ld_m, int accumulate, hipStream_t stream) {
    const bool bad = !z || !M || ldz < n_channels || ld_m < 5 || !em_known(activation) || lines_misaligned(M, 8) ||
                     lines_misaligned(z) || lines_misaligned(val) || lines_misaligned(gene_scale);
    const int go = lines_preamble(n_channels, lineptr, bad, false, idx, val);
    if (go != LINES_GO) return go;
    const unsigned grid = (unsigned)gnx_cdiv(n_channels, EM_WAVES);
    const auto* ptr = reinterpret_cast<const int64_t*>(lineptr);
    if (activation == GNX_ACT_SIGMOID)
        em_sparse_moments_kernel<GNX_ACT_SIGMOID><<<grid, EM_WAVES * 64, 0, stream>>>(ptr, idx, val, gene_lines, n_channels, pos_of_idx,
                                                                                      gene_scale, z, ldz, M, ld_m, accumulate ? 1 : 0);
    else
        em_sparse_moments_kernel<GNX_ACT_NONE><<<grid, EM_WAVES * 64, 0, stream>>>(ptr, idx, val, gene_lines, n_channels, pos_of_idx,
                                                                                   gene_scale, z, ldz, M, ld_m, accumulate ? 1 : 0);
    return gnx_launch_status();
}

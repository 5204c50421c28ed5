// The genes x genes second-moment matrix X^T X of sparse counts, in double: the one hot part of fitting a PCA on resident counts
// (scripts/fit_pca_unified_cortex.py:33-100: PCA().fit on the normalised, log1p'd, z-scored training arrays; the PCs feed
// use_pcs of count_datasets.py:309-475 and utils.py:197-205).  Lines, idx, val and lineptr are the ones of sparse_counts.hip.
//
// C[a][b] = sum over the spots r of X[r][a] * X[r][b] is walked from gene a's side: the entries (r, v) of gene a's CSC line in
// ONE array, and for each of them the entries (g, u) of spot r's CSR row, adding v * u to column chan(g).  The walk touches
// only pairs of stored values: nnz(line a) * (mean row length) products per row of C, never an N x G operand.
//
// One workgroup per (row a of C, chunk of SG_CHUNK columns) holds SG_WAVES strips of doubles in the LDS, one per wavefront.
// Wavefront w takes the entries k = w, w + SG_WAVES, ... of line a, in that order; its 64 lanes stride the CSR row of the
// entry's spot and add (double)v * (double)u - exact, both being fp32 - into the wavefront's OWN strip at the entry's channel.
// The channel map is injective, so the lanes of one instruction hit 64 different addresses, and a wavefront's LDS operations
// complete in program order: no atomics, in the LDS or in global memory.  After a barrier thread t adds the strips of the
// columns t, t + 256, ... in the order w = 0 .. SG_WAVES - 1 and stores the sum (C + the sum when accumulating).  Every element
// has one owner and one order that depends on the inputs alone: a second call gives equal bits.
//
// A wavefront fetches 64 of its entries at once - the spot, the value and the two ends of the spot's CSR row, one entry per
// lane - and walks them with the three broadcast from the owning lane, so the chain entry -> row pointer -> row is paid once
// per 64 entries and not once per entry; of a row it requests SG_FLIGHT strides of 64 entries before the first addition.  The
// additions keep entry order, then position order within the row, whatever SG_FLIGHT is.
#include "sparse_lines.h"

namespace {

constexpr int SG_WAVES = 4;
constexpr int SG_THREADS = 64 * SG_WAVES;
constexpr int SG_FLIGHT = 4;                     // 64-entry strides of a CSR row requested before the first of their additions
constexpr int SG_CHUNK = 2048;                   // columns per workgroup: SG_WAVES * SG_CHUNK doubles = 64 KB of LDS at most
constexpr long SG_MAX_CHANNELS = 65535L * SG_CHUNK;   // grid.y

__global__ __launch_bounds__(SG_THREADS) void sparse_gram_kernel(const int64_t* __restrict__ csc_ptr, const int32_t* __restrict__ csc_idx,
                                                                 const float* __restrict__ csc_val, const int32_t* __restrict__ gene_lines,
                                                                 const int64_t* __restrict__ csr_ptr, const int32_t* __restrict__ csr_idx,
                                                                 const float* __restrict__ csr_val, int64_t row0,
                                                                 const int32_t* __restrict__ chan, double* C, int64_t ldc,
                                                                 int n_channels, int cols, int accumulate) {
    extern __shared__ double sg_strips[];                                    // [SG_WAVES][cols]
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // w: wave-uniform, scalar
    const int64_t a = blockIdx.x;
    const int c0 = (int)blockIdx.y * SG_CHUNK;
    const int c1 = c0 + (n_channels - c0 < cols ? n_channels - c0 : cols);   // this workgroup's columns [c0, c1)

    for (int i = threadIdx.x; i < SG_WAVES * cols; i += SG_THREADS) sg_strips[i] = 0.0;
    __syncthreads();

    double* mine = sg_strips + (size_t)w * cols;
    const LineRange ln = line_range(csc_ptr, gene_lines, a);
    for (int64_t k0 = ln.b + w; k0 < ln.e; k0 += 64 * SG_WAVES) {                // wave-uniform
        const int64_t k = k0 + (int64_t)lane * SG_WAVES;
        int64_t rb = 0, re = 0;
        float v = 0.f;
        if (k < ln.e) {
            const int64_t r = row0 + csc_idx[k];
            v = csc_val[k];
            rb = csr_ptr[r], re = csr_ptr[r + 1];
        }
        const int64_t left = (ln.e - k0 + SG_WAVES - 1) / SG_WAVES;          // this wavefront's entries from k0 on
        const int n = left < 64 ? (int)left : 64;
        for (int j = 0; j < n; ++j) {
            const int64_t jb = lane_get(rb, j), je = lane_get(re, j);
            const double vj = (double)lane_get(v, j);
            for (int64_t p0 = jb + lane; p0 < je; p0 += 64 * SG_FLIGHT) {    // SG_FLIGHT strides requested, then added
                int32_t c[SG_FLIGHT];
                float u[SG_FLIGHT];
#pragma unroll
                for (int q = 0; q < SG_FLIGHT; ++q) {
                    const int64_t p = p0 + 64 * q;
                    c[q] = p < je ? csr_idx[p] : -1;
                    u[q] = p < je ? csr_val[p] : 0.f;
                }
                if (chan) {
#pragma unroll
                    for (int q = 0; q < SG_FLIGHT; ++q) c[q] = c[q] >= 0 ? chan[c[q]] : -1;
                }
                // two strides never hold one channel (one row, an injective map), and if they did: the read-modify-writes
                // below may alias as far as the compiler knows, so it keeps them in program order
#pragma unroll
                for (int q = 0; q < SG_FLIGHT; ++q)
                    if (c[q] >= c0 && c[q] < c1) mine[c[q] - c0] += vj * (double)u[q];
            }
        }
    }
    __syncthreads();

    double* out = C + a * ldc + c0;
    for (int i = threadIdx.x; i < c1 - c0; i += SG_THREADS) {
        double s = sg_strips[i];
#pragma unroll
        for (int u = 1; u < SG_WAVES; ++u) s += sg_strips[(size_t)u * cols + i];
        out[i] = accumulate ? out[i] + s : s;
    }
}

}  // namespace

GNX_EXPORT long gnx_sparse_gram_chunk(void) { return SG_CHUNK; }

GNX_EXPORT int gnx_sparse_gram_f64(const long long* csc_ptr, const int* csc_idx, const float* csc_val, const int* gene_lines,
                                   long n_channels, const long long* csr_ptr, const int* csr_idx, const float* csr_val, long row0,
                                   const int* chan_of_idx, double* C, long ldc, int accumulate, hipStream_t stream) {
    const bool bad = ldc < n_channels || row0 < 0 || !csr_ptr || !C || lines_misaligned(C, 8) || lines_misaligned(csc_val) ||
                     lines_misaligned(csr_val);
    const int go = lines_preamble(n_channels, csc_ptr, bad, n_channels > SG_MAX_CHANNELS, csc_idx, csc_val);
    if (go != LINES_GO) return go;
    if (!csr_idx || !csr_val) return GNX_ERR_BAD_ARG;
    const int cols = n_channels < SG_CHUNK ? (int)n_channels : SG_CHUNK;
    const dim3 grid((unsigned)n_channels, (unsigned)gnx_cdiv(n_channels, SG_CHUNK));
    sparse_gram_kernel<<<grid, SG_THREADS, (size_t)SG_WAVES * cols * sizeof(double), stream>>>(
        reinterpret_cast<const int64_t*>(csc_ptr), csc_idx, csc_val, gene_lines, reinterpret_cast<const int64_t*>(csr_ptr), csr_idx,
        csr_val, row0, chan_of_idx, C, ldc, (int)n_channels, cols, accumulate);
    return gnx_launch_status();
}

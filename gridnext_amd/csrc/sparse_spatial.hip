// The neighbour sums of Moran's I and Geary's C over one array's CSC (gridnext_amd/spatial.py fixes the statistics).  The
// reference builds the spot graph as an N x N pdist matrix (gridnext/graph_datasets.py:145-157, `0 < d <= 1` after scaling by
// sqrt(3) / 2, its TODO asking for the O(N) enumeration); here the graph is a table nbr[r][k] of rows within the array, -1 where
// spot r has no k-th neighbour, and a label permutation of the spots is the same walk over a relabelled table.
//
// One workgroup owns a line (a gene) at a time.  The line is expanded into n_idx floats of dynamic LDS; then, for every table
// of the workgroup's share, thread j takes the entries j, j + 256, ... : it reads the entry's K table entries, adds the present
// neighbours' LDS values in k order in double and counts them, and accumulates p = fma(v, s, p), d += deg v, q += (deg v) v.
// wave_sum_d, then the four wavefronts' partials through the LDS in wavefront order: one store of three doubles per (table,
// line), no atomics, nothing cleared in front of the launch.
//
// A workgroup walks the rows blockIdx.x, blockIdx.x + gridDim.x, ...  The vector is zeroed ONCE; after a line's tables every
// thread writes 0.0f over exactly the entries it deposited, so the next line starts from zeros again.  Zeroing the whole
// vector per line would cost n_idx / 256 ds_write_b32 per thread and line (20 at Visium's 4 992 spots) where a line of 3 %
// non-zeros deposits - and clears - 150 entries, under one per thread.  The partials' slots alternate with every (table, line),
// so a table costs one barrier: the slots a wavefront writes next are not the ones thread 0 is still adding.
#include "sparse_lines.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr long SP_MAX_IDX = 32768;               // 128 KB of LDS
constexpr long SP_MAX_K = 32;
constexpr long SP_MAX_TABLES = 65535;            // grid.y
constexpr long SP_BLOCKS = 2048;                 // of one launch in x: 256 CUs x 8 workgroups of 4 wavefronts

// One table entry's share of s and deg, without a branch: an absent neighbour reads x[0] and adds +0.0, which leaves s's bits
// as they are (s starts at +0.0 and never becomes -0.0), so the K reads of an entry are issued together.
__device__ __forceinline__ void sp_neighbour(double& s, int& deg, int32_t n, const float* x, int n_idx) {
    const bool present = (uint32_t)n < (uint32_t)n_idx;
    const float xv = x[present ? n : 0];
    s += present ? (double)xv : 0.0;
    deg += present;
}

// KT: the table's width at compile time (the K loads of an entry are issued together), 0: any K at run time.  The sums are
// added in k order in every form.
template <int KT>
__global__ __launch_bounds__(SP_THREADS) void sp_line_spatial_kernel(const int64_t* __restrict__ lineptr, const int32_t* __restrict__ idx,
                                                                     const float* __restrict__ val, const int32_t* __restrict__ lines,
                                                                     int64_t n_lines, int n_idx, const int32_t* __restrict__ nbr,
                                                                     int K_rt, int n_tables, double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float x[];            // [n_idx]
    __shared__ double part[2][SP_WAVES][3];
    const int K = KT ? KT : K_rt;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int s = tid; s < n_idx; s += SP_THREADS) x[s] = 0.f;
    int slot = 0;
    for (int64_t row = blockIdx.x; row < n_lines; row += gridDim.x) {
        const LineRange r = line_range(lineptr, lines, row);
        __syncthreads();                                                  // the zeros, or the last line's clearing
        for (int64_t e = r.b + tid; e < r.e; e += SP_THREADS) {
            const int32_t j = idx[e];
            if ((uint32_t)j < (uint32_t)n_idx) x[j] = val[e];
        }
        __syncthreads();
        for (int t = blockIdx.y; t < n_tables; t += gridDim.y) {
            const int32_t* __restrict__ tab = nbr + (int64_t)t * n_idx * K;
            double p = 0.0, d = 0.0, q = 0.0;
            for (int64_t e = r.b + tid; e < r.e; e += SP_THREADS) {
                const int32_t j = idx[e];
                if ((uint32_t)j >= (uint32_t)n_idx) continue;
                const double v = (double)val[e];
                const int32_t* __restrict__ mine = tab + (int64_t)j * K;
                double s = 0.0;
                int deg = 0;
                if constexpr (KT != 0) {
                    int32_t nb[KT];
#pragma unroll
                    for (int k = 0; k < KT; ++k) nb[k] = mine[k];
#pragma unroll
                    for (int k = 0; k < KT; ++k) sp_neighbour(s, deg, nb[k], x, n_idx);
                } else {
                    for (int k = 0; k < K; ++k) sp_neighbour(s, deg, mine[k], x, n_idx);
                }
                const double dv = (double)deg * v;
                p = fma(v, s, p);
                d += dv;
                q += dv * v;
            }
            if (r.b + (tid & ~63) < r.e) {       // the same in the whole wavefront; one without entries holds +0.0, its own sum
                p = wave_sum_d(p);
                d = wave_sum_d(d);
                q = wave_sum_d(q);
            }
            if (lane == 0) part[slot][wave][0] = p, part[slot][wave][1] = d, part[slot][wave][2] = q;
            __syncthreads();
            if (tid < 3) {
                double sum = part[slot][0][tid];
#pragma unroll
                for (int w = 1; w < SP_WAVES; ++w) sum += part[slot][w][tid];
                out[((int64_t)t * n_lines + row) * 3 + tid] = sum;
            }
            slot ^= 1;
        }
        // every gather of this line lies in front of a barrier: the last table's, or the one after the deposit
        for (int64_t e = r.b + tid; e < r.e; e += SP_THREADS) {
            const int32_t j = idx[e];
            if ((uint32_t)j < (uint32_t)n_idx) x[j] = 0.f;
        }
    }
}

template <int KT>
int sp_launch(const int64_t* lineptr, const int* idx, const float* val, const int* lines, long n_lines, long n_idx, const int* nbr,
              long K, long n_tables, double* out, hipStream_t stream) {
    const size_t lds = (size_t)n_idx * sizeof(float);
    const int allowed = gnx_allow_lds<sp_line_spatial_kernel<KT>>(lds);
    if (allowed != GNX_OK) return allowed;
    // few lines and many tables: the tables are dealt over grid.y until the launch has SP_BLOCKS workgroups
    const long gx = n_lines < SP_BLOCKS ? n_lines : SP_BLOCKS;
    const long want = SP_BLOCKS / gx;
    const long gy = n_tables < want ? n_tables : want;
    sp_line_spatial_kernel<KT><<<dim3((unsigned)gx, (unsigned)gy), SP_THREADS, lds, stream>>>(
        lineptr, idx, val, lines, n_lines, (int)n_idx, nbr, (int)K, (int)n_tables, out);
    return gnx_launch_status();
}

}  // namespace

GNX_EXPORT long gnx_sparse_spatial_max_idx(void) { return SP_MAX_IDX; }

GNX_EXPORT int gnx_sparse_line_spatial_f64(const long long* lineptr, const int* idx, const float* val, const int* lines, long n_lines,
                                           long n_idx, const int* nbr, long K, long n_tables, double* out, hipStream_t stream) {
    const bool bad = !nbr || !out || K < 1 || K > SP_MAX_K || n_tables < 1 || n_idx < 1 || lines_misaligned(out, 8) ||
                     lines_misaligned(nbr);
    const int go = lines_preamble(n_lines, lineptr, bad, n_idx > SP_MAX_IDX || n_tables > SP_MAX_TABLES, idx, val);
    if (go != LINES_GO) return go;
    const int64_t* lp = reinterpret_cast<const int64_t*>(lineptr);
    if (K == 6) return sp_launch<6>(lp, idx, val, lines, n_lines, n_idx, nbr, K, n_tables, out, stream);
    if (K == 18) return sp_launch<18>(lp, idx, val, lines, n_lines, n_idx, nbr, K, n_tables, out, stream);
    return sp_launch<0>(lp, idx, val, lines, n_lines, n_idx, nbr, K, n_tables, out, stream);
}

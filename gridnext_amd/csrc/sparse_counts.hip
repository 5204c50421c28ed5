// Sparse count matrices on the device (the count side of the reference's tutorial, notebooks/Tutorial_visium_count.ipynb:
// an AnnData whose X is scipy-sparse, sc.pp.normalize_total, sc.pp.log1p, X.mean(0) / X.std(0), then
// anndata_to_tensordataset / anndata_to_grids, which densify on the host).  A matrix is a list of LINES - the rows of a CSR or
// the columns of a CSC matrix: line l owns the entries lineptr[l] .. lineptr[l + 1] of idx (int32, strictly increasing within
// a line) and val (fp32); lineptr is int64.
//
// Expand.  One workgroup per (output row, chunk of SC_CHUNK positions).  The chunk is zeroed in the LDS, the threads walk the
// line's entries with coalesced idx / val loads and deposit the ones that land in the chunk, and after a barrier the chunk
// goes out whole: every output element is written exactly once, zeros included, so nothing is cleared in front of the launch.
// The chunk sits in the LDS at the offset (row address / 4) mod 4, so a 16-byte group of the LDS is a 16-byte group of the
// output: the body goes out as dwordx4 stores whatever the row's alignment, the at most three elements on either side as
// dwords.  A row longer than a chunk takes several workgroups, each filtering the same entries.  Two entries of a line on one
// position would race: the caller's map is injective on its non-negative values.
//
// Moments.  One wavefront per line: lane j adds the entries j, j + 64, ... of the line in that order, in double, and the 64
// partial sums go through the fixed shuffle tree of wave_sum_d.  The order depends on the line alone, so equal inputs give
// equal bits; the square of an fp32 value is exact in double.  Maximum: the same walk with fmaxf, started at 0.  Clipped moments:
// the same walk again, every entry cut at its ROW's bound first: t = fmin((double) v, clip[row]), s1 += t, s2 = fma(t, t, s2).
//
// The divisions are IEEE round-to-nearest fp32 divisions (this library is built without fast-math, and HIP's default is the
// correctly rounded divide), log1p is the device library's log1pf.
#include "sparse_lines.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_CHUNK = 8192;                   // positions per workgroup: 32 KB of LDS (+ 16 B for the alignment offset)
constexpr int SC_MAX_BLOCKS = 1 << 16;           // of a grid-stride launch

__global__ __launch_bounds__(SC_THREADS) void sc_expand_kernel(const int64_t* __restrict__ lineptr, const int32_t* __restrict__ idx,
                                                               const float* __restrict__ val, const int32_t* __restrict__ lines,
                                                               const int32_t* __restrict__ pos_of_idx, float* __restrict__ out,
                                                               int64_t ld_out, int64_t L) {
    __shared__ __attribute__((aligned(16))) float buf[SC_CHUNK + 4];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x, p0 = (int64_t)blockIdx.y * SC_CHUNK;
    const int n = (int)(L - p0 < SC_CHUNK ? L - p0 : SC_CHUNK);          // 1 .. SC_CHUNK positions of this chunk
    float* dst = out + row * ld_out + p0;
    const int shift = (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3);  // buf[shift + q] is position p0 + q
    for (int s = tid; s < n + shift; s += SC_THREADS) buf[s] = 0.f;
    __syncthreads();

    const LineRange r = line_range(lineptr, lines, row);
    for (int64_t k = r.b + tid; k < r.e; k += SC_THREADS) {
        const int32_t j = idx[k];
        const int64_t p = (pos_of_idx ? (int64_t)pos_of_idx[j] : (int64_t)j) - p0;
        if (p >= 0 && p < n) buf[shift + (int)p] = val[k];
    }
    __syncthreads();

    // LDS slots shift .. shift + n; the 16-byte groups g with 4 g >= shift and 4 g + 4 <= shift + n go out as one store
    const int g0 = (shift + 3) >> 2, g1 = (shift + n) >> 2;
    if (g1 > g0) {
        const f32x4* src4 = reinterpret_cast<const f32x4*>(buf);
        f32x4* dst4 = reinterpret_cast<f32x4*>(dst - shift);
        for (int g = g0 + tid; g < g1; g += SC_THREADS) dst4[g] = src4[g];
        const int head = 4 * g0 - shift, tail = shift + n - 4 * g1;         // each 0 .. 3
        if (tid < head) dst[tid] = buf[shift + tid];
        if (tid >= 64 && tid - 64 < tail) dst[4 * g1 - shift + tid - 64] = buf[4 * g1 + tid - 64];
    } else {
        for (int q = tid; q < n; q += SC_THREADS) dst[q] = buf[shift + q];  // under two groups: at most 7 dwords
    }
}

// The three reductions of a line's kept entries: what a lane adds an entry to, and how the 64 lanes' values become the row's
// result.  Arg is what a launch hands every row beside the line (nothing, or the rows' bounds); begin() takes the row's share.
struct ScMoments {                               // the sum and the sum of squares, in double
    using Out = double;
    using Arg = const void*;
    double s1 = 0.0, s2 = 0.0;
    __device__ __forceinline__ void begin(Arg, int64_t) {}
    __device__ __forceinline__ void add(float x) {
        const double v = (double)x;
        s1 += v;
        s2 += v * v;
    }
    __device__ __forceinline__ void store(double* __restrict__ out, int64_t row, int lane) {
        s1 = wave_sum_d(s1);
        s2 = wave_sum_d(s2);
        if (lane == 0) out[2 * row] = s1, out[2 * row + 1] = s2;
    }
};

// the largest of 0 - the implicit value of a sparse line - and the line's kept entries: a maximum has no order, the result is exact
struct ScMax {
    using Out = float;
    using Arg = const void*;
    float m = 0.f;
    __device__ __forceinline__ void begin(Arg, int64_t) {}
    __device__ __forceinline__ void add(float x) { m = fmaxf(m, x); }
    __device__ __forceinline__ void store(float* __restrict__ out, int64_t row, int lane) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if (lane == 0) out[row] = m;
    }
};

// ScMoments on min(v, the row's bound): with a bound of +inf t is v and t * t is exact, so the bits are ScMoments'; fmin drops
// a NaN bound (t = v).  The fma rounds once per entry, the square of a bound that is no fp32 number being inexact in double.
struct ScClipMoments {
    using Out = double;
    using Arg = const double*;                   // [n_lines]: row i's bound
    double s1 = 0.0, s2 = 0.0, clip;
    __device__ __forceinline__ void begin(Arg bound, int64_t row) { clip = bound[row]; }
    __device__ __forceinline__ void add(float x) {
        const double t = fmin((double)x, clip);
        s1 += t;
        s2 = fma(t, t, s2);
    }
    __device__ __forceinline__ void store(double* __restrict__ out, int64_t row, int lane) {
        s1 = wave_sum_d(s1);
        s2 = wave_sum_d(s2);
        if (lane == 0) out[2 * row] = s1, out[2 * row + 1] = s2;
    }
};

template <class R>
__global__ __launch_bounds__(SC_THREADS) void sc_line_reduce_kernel(const int64_t* __restrict__ lineptr, const int32_t* __restrict__ idx,
                                                                    const float* __restrict__ val, const int32_t* __restrict__ lines,
                                                                    int64_t n_lines, const uint8_t* __restrict__ idx_mask,
                                                                    typename R::Arg arg, typename R::Out* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * SC_WAVES + (threadIdx.x >> 6);       // the same in the whole wavefront
    if (row >= n_lines) return;
    const LineRange r = line_range(lineptr, lines, row);
    R acc;
    acc.begin(arg, row);
    for (int64_t k = r.b + lane; k < r.e; k += 64) {
        if (idx_mask && idx_mask[idx[k]] == 0) continue;
        acc.add(val[k]);
    }
    acc.store(out, row, lane);
}

template <class R>
int sc_line_reduce(const long long* lineptr, const int* idx, const float* val, const int* lines, long n_lines,
                   const uint8_t* idx_mask, typename R::Arg arg, bool bad, typename R::Out* out, hipStream_t stream) {
    const int go = lines_preamble(n_lines, lineptr, !out || bad, false, idx, val);
    if (go != LINES_GO) return go;
    sc_line_reduce_kernel<R><<<(unsigned)gnx_cdiv(n_lines, SC_WAVES), SC_THREADS, 0, stream>>>(
        reinterpret_cast<const int64_t*>(lineptr), idx, val, lines, n_lines, idx_mask, arg, out);
    return gnx_launch_status();
}

__global__ __launch_bounds__(SC_THREADS) void sc_div_by_line_kernel(const int64_t* __restrict__ lineptr, float* __restrict__ val,
                                                                    int64_t n_lines, const float* __restrict__ divisor) {
    const int lane = threadIdx.x & 63;
    const int64_t line = (int64_t)blockIdx.x * SC_WAVES + (threadIdx.x >> 6);
    if (line >= n_lines) return;
    const int64_t b = lineptr[line], e = lineptr[line + 1];
    const float d = divisor[line];
    for (int64_t k = b + lane; k < e; k += 64) val[k] = val[k] / d;
}

__global__ __launch_bounds__(SC_THREADS) void sc_div_by_idx_kernel(const int32_t* __restrict__ idx, float* __restrict__ val,
                                                                   int64_t n, const float* __restrict__ divisor) {
    for (int64_t k = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x; k < n; k += (int64_t)gridDim.x * SC_THREADS)
        val[k] = val[k] / divisor[idx[k]];
}

__global__ __launch_bounds__(SC_THREADS) void sc_log1p_kernel(float* __restrict__ val, int64_t n) {
    for (int64_t k = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x; k < n; k += (int64_t)gridDim.x * SC_THREADS)
        val[k] = log1pf(val[k]);
}

unsigned sc_stride_blocks(int64_t n) {
    const int64_t b = (n + SC_THREADS - 1) / SC_THREADS;
    return (unsigned)(b > SC_MAX_BLOCKS ? SC_MAX_BLOCKS : b);
}

}  // namespace

GNX_EXPORT long gnx_sparse_expand_chunk(void) { return SC_CHUNK; }

GNX_EXPORT int gnx_sparse_expand_f32(const long long* lineptr, const int* idx, const float* val, const int* lines, long n_lines,
                                     const int* pos_of_idx, float* out, long ld_out, long L, hipStream_t stream) {
    const long chunks = (L + SC_CHUNK - 1) / SC_CHUNK;
    const int go = lines_preamble(n_lines, lineptr, L <= 0 || ld_out < L || !out || lines_misaligned(out), chunks > 65535, idx, val);
    if (go != LINES_GO) return go;
    sc_expand_kernel<<<dim3((unsigned)n_lines, (unsigned)chunks), SC_THREADS, 0, stream>>>(
        reinterpret_cast<const int64_t*>(lineptr), idx, val, lines, pos_of_idx, out, ld_out, L);
    return gnx_launch_status();
}

GNX_EXPORT int gnx_sparse_line_moments_f64(const long long* lineptr, const int* idx, const float* val, const int* lines,
                                           long n_lines, const uint8_t* idx_mask, double* out, hipStream_t stream) {
    return sc_line_reduce<ScMoments>(lineptr, idx, val, lines, n_lines, idx_mask, nullptr, false, out, stream);
}

GNX_EXPORT int gnx_sparse_line_clip_moments_f64(const long long* lineptr, const int* idx, const float* val, const int* lines,
                                                long n_lines, const uint8_t* idx_mask, const double* clip, double* out,
                                                hipStream_t stream) {
    return sc_line_reduce<ScClipMoments>(lineptr, idx, val, lines, n_lines, idx_mask, clip, !clip, out, stream);
}

GNX_EXPORT int gnx_sparse_line_max_f32(const long long* lineptr, const int* idx, const float* val, const int* lines, long n_lines,
                                       const uint8_t* idx_mask, float* out, hipStream_t stream) {
    return sc_line_reduce<ScMax>(lineptr, idx, val, lines, n_lines, idx_mask, nullptr, false, out, stream);
}

GNX_EXPORT int gnx_sparse_div_by_line_f32(const long long* lineptr, float* val, long n_lines, const float* divisor,
                                          hipStream_t stream) {
    const int go = lines_preamble(n_lines, lineptr, false, false, val, divisor);
    if (go != LINES_GO) return go;
    sc_div_by_line_kernel<<<(unsigned)gnx_cdiv(n_lines, SC_WAVES), SC_THREADS, 0, stream>>>(
        reinterpret_cast<const int64_t*>(lineptr), val, n_lines, divisor);
    return gnx_launch_status();
}

GNX_EXPORT int gnx_sparse_div_by_idx_f32(const int* idx, float* val, long n, const float* divisor, hipStream_t stream) {
    if (n < 0) return GNX_ERR_BAD_ARG;
    if (n == 0) return GNX_OK;
    if (!idx || !val || !divisor) return GNX_ERR_BAD_ARG;
    sc_div_by_idx_kernel<<<sc_stride_blocks(n), SC_THREADS, 0, stream>>>(idx, val, n, divisor);
    return gnx_launch_status();
}

GNX_EXPORT int gnx_log1p_f32(float* val, long n, hipStream_t stream) {
    if (n < 0) return GNX_ERR_BAD_ARG;
    if (n == 0) return GNX_OK;
    if (!val) return GNX_ERR_BAD_ARG;
    sc_log1p_kernel<<<sc_stride_blocks(n), SC_THREADS, 0, stream>>>(val, n);
    return gnx_launch_status();
}

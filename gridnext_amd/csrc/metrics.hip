// Evaluation metrics of a finished run, on the device (the numeric half of the reference's gridnext/plotting.py):
//   gnx_confusion_counts  - sklearn's confusion_matrix behind plot_confusion (plotting.py:103-134),
//   gnx_clf_curve         - the one-vs-rest ROC / precision-recall curves and their areas of performance_curves
//                           (plotting.py:14-98; sklearn's _binary_clf_curve, roc_curve, precision_recall_curve, auc),
//   gnx_misclass_density  - the per-spot misclassification map (plotting.py:138-149).
//
// Curve.  Per class the scores are ordered by a radix sort and counted:
//   key      a float's bits as an order-preserving uint32 (-0.0 first becomes +0.0; then non-negatives get the sign bit
//            flipped, negatives all bits), inverted, so that ascending keys are descending scores.  All of it is integer
//            work: denormals keep their order.  An element is the 64-bit word (key << 1 | positive).
//   sort     four LSD passes over 8-bit digits of the key, classes in grid.y.  A class's n elements are cut into tiles of
//            MT_TILE; workgroup g owns the contiguous span of tiles [g * span, (g + 1) * span).  A pass is (1) a digit
//            histogram per workgroup, hist[class][digit][g]; (2) one exclusive prefix per class over (digit, g) in that
//            order, so a workgroup's base for a digit counts every smaller digit and the same digit in the workgroups
//            before it; (3) the scatter.  The scatter is STABLE: within a workgroup a tile's elements are ranked in element
//            order - wave w holds elements [512 w, 512 w + 512) of the tile, 64 consecutive ones per round, a lane's rank among
//            the lanes of equal digit comes from wave ballots (the popcount of the equal-digit mask below the lane), the
//            waves' bases from a prefix over the per-wave digit counts.  No position is a ticket from an atomic; the only
//            atomics are LDS counter increments, whose sums do not depend on their order.
//   counts   group ends (key[i] != key[i + 1], and the last element) and an inclusive scan of the positive flags, both as
//            a two-level scan over the same spans; the group ends are compacted as (tp << 32 | i + 1) into the second sort
//            buffer, the thresholds straight into the output.
//   areas    from the compacted groups k and k - 1: S = sum (fp_k - fp_{k-1}) (tp_k + tp_{k-1}) in int64 and
//            A = sum (tp_k - tp_{k-1}) (p_k + p_{k-1}) in float64, p_k = tp_k / (tp_k + fp_k), p_0 = 1.  Each thread adds
//            its groups in index order, a workgroup folds its 256 sums in a fixed tree, one thread per class adds the
//            workgroups' partial sums in index order: the same input gives the same bits.  No floating-point atomics.
//            auroc = (double)S / (double)(2 P N) (one rounding for 2 P N < 2^53), auprc = A / 2 / P.
// The launch geometry of a class depends on n alone, so a column gives the same bits alone and among others.
#include "common.h"

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_WAVES = MT_THREADS / 64;
constexpr int MT_ITEMS = 8;                         // elements per thread and tile: 16 VGPRs of payload
constexpr int MT_TILE = MT_THREADS * MT_ITEMS;      // 2048 elements per workgroup and step
constexpr int MT_WAVE_ELEMS = 64 * MT_ITEMS;        // a wave's contiguous share of a tile
constexpr int MT_GMAX = 256;                        // workgroups per class: one per CU; above it a workgroup walks several tiles
constexpr int MT_RADIX = 256;                       // 8-bit digits: 5 KB of LDS counters per workgroup
constexpr long MT_NMAX = 2147483647L;               // n < 2^31: positions and counts are 32-bit, 2 P N < 2^63
constexpr int MT_CMAX = 65535;                      // grid.y

constexpr int CF_KMAX = 64;                         // K * K 32-bit LDS counters: 16 KB at the limit
constexpr int CF_BLOCKS = 1024;
constexpr long CF_NMAX = 1L << 40;                  // a workgroup's 32-bit counters hold its share (< 2^31) without wrapping

struct MtGeo {
    long span;   // elements per workgroup (a whole number of tiles)
    int G;       // workgroups per class
};

MtGeo mt_geo(long n) {
    const long ntiles = (n + MT_TILE - 1) / MT_TILE;
    const long per = (ntiles + MT_GMAX - 1) / MT_GMAX;
    MtGeo g;
    g.span = per * MT_TILE;
    g.G = (int)((ntiles + per - 1) / per);
    return g;
}

// byte offsets of the workspace's parts; every part is a multiple of 8 bytes
struct MtWs {
    size_t a, b, hist, part, tot, partial, total;
};

MtWs mt_ws(long n, int C, int G) {
    MtWs w;
    size_t o = 0;
    w.a = o;       o += (size_t)C * (size_t)n * 8;
    w.b = o;       o += (size_t)C * (size_t)n * 8;
    w.hist = o;    o += (size_t)C * MT_RADIX * (size_t)G * 4;
    w.part = o;    o += (size_t)C * (size_t)G * 16;
    w.tot = o;     o += (size_t)C * 16;
    w.partial = o; o += (size_t)C * (size_t)G * 16;
    w.total = o;
    return w;
}

__device__ __forceinline__ uint32_t mt_key(uint32_t bits) {
    if (bits == 0x80000000u) bits = 0u;                                   // -0.0 + 0.0f
    const uint32_t ord = bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
    return ~ord;                                                          // ascending key = descending score
}

__device__ __forceinline__ uint32_t mt_unkey(uint32_t key) {
    const uint32_t ord = ~key;
    return (ord >> 31) ? (ord ^ 0x80000000u) : ~ord;
}

__global__ void mt_zero_word_kernel(unsigned long long* word) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *word = 0ull;
}

// a[c][i] = key(scores[i][c]) << 1 | (y[i] == c); one thread per row, so y and a row's cache lines are read once
__global__ __launch_bounds__(MT_THREADS) void mt_key_kernel(const float* __restrict__ scores, long ld,
                                                            const long long* __restrict__ y, long n, int C,
                                                            uint64_t* __restrict__ a, unsigned long long* bad) {
    const long i = (long)blockIdx.x * MT_THREADS + threadIdx.x;
    int nan = 0;
    if (i < n) {
        const long long yy = y[i];
        const float* row = scores + i * ld;
        for (int c = 0; c < C; ++c) {
            const uint32_t bits = __float_as_uint(row[c]);
            nan += (bits & 0x7fffffffu) > 0x7f800000u;
            a[(size_t)c * n + i] = ((uint64_t)mt_key(bits) << 1) | (uint64_t)(yy == (long long)c);
        }
    }
    nan = wave_sum_i(nan);
    if ((threadIdx.x & 63) == 0 && nan) atomicAdd(bad, (unsigned long long)nan);
}

// hist[c][d][g] = the number of elements of workgroup g's span whose digit is d
__global__ __launch_bounds__(MT_THREADS) void mt_hist_kernel(const uint64_t* __restrict__ in, long n, long span, int shift,
                                                             uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[MT_RADIX];
    const int tid = threadIdx.x, g = blockIdx.x, c = blockIdx.y, G = gridDim.x;
    h[tid] = 0u;
    __syncthreads();
    const uint64_t* src = in + (size_t)c * n;
    const long begin = (long)g * span, end = begin + span < n ? begin + span : n;
    for (long i = begin + tid; i < end; i += MT_THREADS) atomicAdd(&h[(unsigned)(src[i] >> shift) & 255u], 1u);
    __syncthreads();
    hist[((size_t)c * MT_RADIX + tid) * G + g] = h[tid];
}

// in place: hist[c][d][g] -> the number of elements of class c in front of (d, g) in (digit, workgroup) order
__global__ __launch_bounds__(MT_RADIX) void mt_hist_scan_kernel(uint32_t* __restrict__ hist, int G) {
    __shared__ uint32_t s[MT_RADIX];
    const int d = threadIdx.x;
    uint32_t* row = hist + ((size_t)blockIdx.x * MT_RADIX + d) * G;
    uint32_t sum = 0;
    for (int g = 0; g < G; ++g) sum += row[g];
    s[d] = sum;
    __syncthreads();
    for (int o = 1; o < MT_RADIX; o <<= 1) {                     // inclusive scan over the 256 digit sums
        const uint32_t v = d >= o ? s[d - o] : 0u;
        __syncthreads();
        s[d] += v;
        __syncthreads();
    }
    uint32_t run = s[d] - sum;
    for (int g = 0; g < G; ++g) {
        const uint32_t t = row[g];
        row[g] = run;
        run += t;
    }
}

__global__ __launch_bounds__(MT_THREADS) void mt_scatter_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                                long n, long span, int shift,
                                                                const uint32_t* __restrict__ hist) {
    __shared__ uint32_t off[MT_RADIX];                 // next position of digit d for this workgroup
    __shared__ uint32_t wh[MT_WAVES][MT_RADIX];        // per wave: digit counts of the tile, then the wave's next positions
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = blockIdx.x, c = blockIdx.y, G = gridDim.x;
    const uint64_t* src = in + (size_t)c * n;
    uint64_t* dst = out + (size_t)c * n;
    const long begin = (long)g * span, end = begin + span < n ? begin + span : n;
    off[tid] = hist[((size_t)c * MT_RADIX + tid) * G + g];

    for (long tb = begin; tb < end; tb += MT_TILE) {                       // uniform in the workgroup
#pragma unroll
        for (int k = 0; k < MT_WAVES; ++k) wh[k][tid] = 0u;
        __syncthreads();
        uint64_t v[MT_ITEMS];
        const long e0 = tb + (long)w * MT_WAVE_ELEMS + lane;               // element of round r: e0 + 64 r
#pragma unroll
        for (int r = 0; r < MT_ITEMS; ++r) {
            const long i = e0 + 64 * r;
            v[r] = i < end ? src[i] : 0ull;
            if (i < end) atomicAdd(&wh[w][(unsigned)(v[r] >> shift) & 255u], 1u);
        }
        __syncthreads();
        {                                                                  // thread d: the waves' bases for digit d, in wave order
            uint32_t run = off[tid];
#pragma unroll
            for (int k = 0; k < MT_WAVES; ++k) {
                const uint32_t t = wh[k][tid];
                wh[k][tid] = run;
                run += t;
            }
            off[tid] = run;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < MT_ITEMS; ++r) {
            const bool valid = e0 + 64 * r < end;
            const unsigned d = (unsigned)(v[r] >> shift) & 255u;
            uint64_t same = __ballot(valid);                               // the valid lanes of this wave with my digit
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (d >> b) & 1u;
                const uint64_t bal = __ballot(bit);
                same &= bit ? bal : ~bal;
            }
            const unsigned rank = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
            if (valid) {
                const size_t pos = (size_t)wh[w][d] + rank;
                if (pos < (size_t)n) dst[pos] = v[r];
            }
            __syncthreads();
            if (valid && rank == 0) wh[w][d] += (uint32_t)__popcll(same);
            __syncthreads();
        }
    }
}

// part[c][g] = (positives, group ends) of workgroup g's span of the sorted elements
__global__ __launch_bounds__(MT_THREADS) void mt_part_kernel(const uint64_t* __restrict__ in, long n, long span,
                                                             long long* __restrict__ part) {
    __shared__ int red[2][MT_WAVES];
    const int tid = threadIdx.x, g = blockIdx.x, c = blockIdx.y, G = gridDim.x;
    const uint64_t* src = in + (size_t)c * n;
    const long begin = (long)g * span, end = begin + span < n ? begin + span : n;
    int pos = 0, ends = 0;
    for (long i = begin + tid; i < end; i += MT_THREADS) {
        const uint64_t v = src[i];
        pos += (int)(v & 1ull);
        ends += (i == n - 1) || ((src[i + 1] >> 1) != (v >> 1));
    }
    pos = wave_sum_i(pos);
    ends = wave_sum_i(ends);
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = pos;
        red[1][tid >> 6] = ends;
    }
    __syncthreads();
    if (tid == 0) {
        long long p = 0, e = 0;
        for (int k = 0; k < MT_WAVES; ++k) {
            p += red[0][k];
            e += red[1][k];
        }
        part[((size_t)c * G + g) * 2] = p;
        part[((size_t)c * G + g) * 2 + 1] = e;
    }
}

// in place: part[c][g] -> the sums in front of workgroup g; tot[c] = (P, T); n_thresholds[c] = T
__global__ void mt_part_scan_kernel(long long* __restrict__ part, int G, int C, long long* __restrict__ tot,
                                    long long* __restrict__ n_thresholds) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    long long p = 0, e = 0;
    long long* row = part + (size_t)c * G * 2;
    for (int g = 0; g < G; ++g) {
        const long long tp = row[2 * g], te = row[2 * g + 1];
        row[2 * g] = p;
        row[2 * g + 1] = e;
        p += tp;
        e += te;
    }
    tot[2 * c] = p;
    tot[2 * c + 1] = e;
    n_thresholds[c] = e;
}

// group end i, the k-th of its class: b[c][k] = tp << 32 | (i + 1); thresholds[c][k] = the group's score
__global__ __launch_bounds__(MT_THREADS) void mt_compact_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ b,
                                                                long n, long span, const long long* __restrict__ part,
                                                                float* __restrict__ thresholds) {
    __shared__ unsigned long long sw[MT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = blockIdx.x, c = blockIdx.y, G = gridDim.x;
    const uint64_t* src = in + (size_t)c * n;
    const long begin = (long)g * span, end = begin + span < n ? begin + span : n;
    unsigned long long run_tp = (unsigned long long)part[((size_t)c * G + g) * 2];
    unsigned long long run_k = (unsigned long long)part[((size_t)c * G + g) * 2 + 1];
    for (long cb = begin; cb < end; cb += MT_THREADS) {                    // uniform in the workgroup
        const long i = cb + tid;
        uint64_t v = 0;
        unsigned f = 0, e = 0;
        if (i < end) {
            v = src[i];
            f = (unsigned)(v & 1ull);
            e = (i == n - 1) || ((src[i + 1] >> 1) != (v >> 1));
        }
        unsigned long long x = (unsigned long long)f | ((unsigned long long)e << 32);   // both sums stay below 2^31
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = __shfl_up(x, o, 64);
            if (lane >= o) x += t;
        }
        if (lane == 63) sw[w] = x;
        __syncthreads();
        unsigned long long before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < MT_WAVES; ++k) {
            const unsigned long long t = sw[k];
            if (k < w) before += t;
            total += t;
        }
        x += before;
        if (e) {
            const unsigned long long tp = run_tp + (x & 0xffffffffull), k = run_k + (x >> 32) - 1ull;
            if (k < (unsigned long long)n) {
                b[(size_t)c * n + k] = (tp << 32) | (unsigned long long)(i + 1);
                if (thresholds) thresholds[(size_t)c * n + k] = __uint_as_float(mt_unkey((uint32_t)(v >> 1)));
            }
        }
        run_tp += total & 0xffffffffull;
        run_k += total >> 32;
        __syncthreads();
    }
}

// the curve's count arrays and the workgroup's partial sums (S, A) over its share of the T groups
__global__ __launch_bounds__(MT_THREADS) void mt_integrate_kernel(const uint64_t* __restrict__ b, long n,
                                                                  const long long* __restrict__ tot,
                                                                  long long* __restrict__ tps, long long* __restrict__ fps,
                                                                  long long* __restrict__ partial) {
    __shared__ long long rs[MT_THREADS];
    __shared__ double ra[MT_THREADS];
    const int tid = threadIdx.x, g = blockIdx.x, c = blockIdx.y, G = gridDim.x;
    const long long T = tot[2 * c + 1];
    const long long chunk = (T + G - 1) / G;
    const long long k0 = (long long)g * chunk, k1 = k0 + chunk < T ? k0 + chunk : T;
    const uint64_t* grp = b + (size_t)c * n;
    long long S = 0;
    double A = 0.0;
    for (long long k = k0 + tid; k < k1; k += MT_THREADS) {
        const uint64_t cur = grp[k], prev = k > 0 ? grp[k - 1] : 0ull;
        const long long tp = (long long)(cur >> 32), cnt = (long long)(cur & 0xffffffffull), fp = cnt - tp;
        const long long tpp = (long long)(prev >> 32), cntp = (long long)(prev & 0xffffffffull), fpp = cntp - tpp;
        if (tps) tps[(size_t)c * n + k] = tp;
        if (fps) fps[(size_t)c * n + k] = fp;
        S += (fp - fpp) * (tp + tpp);
        if (tp != tpp) {
            const double pk = (double)tp / (double)cnt, pp = k > 0 ? (double)tpp / (double)cntp : 1.0;
            A += (double)(tp - tpp) * (pk + pp);
        }
    }
    rs[tid] = S;
    ra[tid] = A;
    __syncthreads();
    for (int o = MT_THREADS / 2; o > 0; o >>= 1) {                        // a fixed tree
        if (tid < o) {
            rs[tid] += rs[tid + o];
            ra[tid] += ra[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        partial[((size_t)c * G + g) * 2] = rs[0];
        reinterpret_cast<double*>(partial)[((size_t)c * G + g) * 2 + 1] = ra[0];
    }
}

__global__ void mt_final_kernel(const long long* __restrict__ partial, int G, int C, long n, const long long* __restrict__ tot,
                                double* __restrict__ auroc, double* __restrict__ auprc) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    long long S = 0;
    double A = 0.0;
    for (int g = 0; g < G; ++g) {                                         // index order
        S += partial[((size_t)c * G + g) * 2];
        A += reinterpret_cast<const double*>(partial)[((size_t)c * G + g) * 2 + 1];
    }
    const long long P = tot[2 * c], N = (long long)n - P;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (P == 0) {                         // sklearn: recall is set to one, precision is zero, the appended point (0, 1)
        auroc[c] = nan;
        auprc[c] = 0.5;
    } else {
        auroc[c] = N == 0 ? nan : (double)S / (double)(2 * P * N);
        auprc[c] = A * 0.5 / (double)P;
    }
}

// ---- confusion counts ---------------------------------------------------------------------------------------------------
__global__ void cf_zero_kernel(unsigned long long* counts, int KK, unsigned long long* bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < KK) counts[i] = 0ull;
    if (i == 0) *bad = 0ull;
}

__global__ __launch_bounds__(256) void cf_count_kernel(const long long* __restrict__ yt, const long long* __restrict__ yp, long n,
                                                       int K, unsigned long long* counts, unsigned long long* bad) {
    __shared__ uint32_t cnt[CF_KMAX * CF_KMAX + 1];                       // the last word counts labels outside [0, K)
    const int tid = threadIdx.x, lane = tid & 63, KK = K * K;
    for (int i = tid; i <= CF_KMAX * CF_KMAX; i += 256) cnt[i] = 0u;
    __syncthreads();
    for (long base = (long)blockIdx.x * 256; base < n; base += (long)gridDim.x * 256) {      // uniform in the workgroup
        const long i = base + tid;
        int cell = -1;                                                    // -1: no element
        if (i < n) {
            const long long t = yt[i], p = yp[i];
            cell = (t >= 0 && t < K && p >= 0 && p < K) ? (int)(t * K + p) : CF_KMAX * CF_KMAX;
        }
        const int first = __shfl(cell, 0, 64);
        if (__ballot(cell == first) == ~0ull) {                           // one cell in the whole wave: one add
            if (lane == 0 && first >= 0) atomicAdd(&cnt[first], 64u);
        } else if (cell >= 0) {
            atomicAdd(&cnt[cell], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < KK; i += 256)
        if (cnt[i]) atomicAdd(&counts[i], (unsigned long long)cnt[i]);
    if (tid == 0 && cnt[CF_KMAX * CF_KMAX]) atomicAdd(bad, (unsigned long long)cnt[CF_KMAX * CF_KMAX]);
}

// ---- misclassification density --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mc_kernel(const float* __restrict__ smax, const long long* __restrict__ tru, int C, long HW,
                                                 double* __restrict__ out, unsigned long long* bad) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    int over = 0;
    if (i < HW) {
        const long long t = tru[i];
        double r = 0.0;
        if (t > (long long)C) over = 1;
        else if (t > 0) r = (double)(1.0f - smax[(size_t)(t - 1) * HW + i]);
        out[i] = r;
    }
    over = wave_sum_i(over);
    if ((threadIdx.x & 63) == 0 && over) atomicAdd(bad, (unsigned long long)over);
}

}  // namespace

GNX_EXPORT long gnx_clf_curve_tile(void) { return MT_TILE; }
GNX_EXPORT long gnx_clf_curve_max_groups(void) { return MT_GMAX; }
GNX_EXPORT long gnx_confusion_max_classes(void) { return CF_KMAX; }

GNX_EXPORT long gnx_clf_curve_workspace(long n, int C) {
    if (n <= 0 || C <= 0 || n > MT_NMAX || C > MT_CMAX) return 0;
    return (long)mt_ws(n, C, mt_geo(n).G).total;
}

GNX_EXPORT int gnx_clf_curve(const float* scores, long ld, const long long* y_true, long n, int C, float* thresholds,
                             long long* tps, long long* fps, long long* n_thresholds, double* auroc, double* auprc,
                             long long* bad, void* workspace, hipStream_t stream) {
    if (n <= 0 || C <= 0 || ld < C) return GNX_ERR_BAD_ARG;
    if (!scores || !y_true || !n_thresholds || !auroc || !auprc || !bad || !workspace) return GNX_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return GNX_ERR_BAD_ARG;
    if (n > MT_NMAX || C > MT_CMAX) return GNX_ERR_UNSUPPORTED;
    const MtGeo geo = mt_geo(n);
    const MtWs ws = mt_ws(n, C, geo.G);
    char* base = static_cast<char*>(workspace);
    uint64_t* a = reinterpret_cast<uint64_t*>(base + ws.a);
    uint64_t* b = reinterpret_cast<uint64_t*>(base + ws.b);
    uint32_t* hist = reinterpret_cast<uint32_t*>(base + ws.hist);
    long long* part = reinterpret_cast<long long*>(base + ws.part);
    long long* tot = reinterpret_cast<long long*>(base + ws.tot);
    long long* partial = reinterpret_cast<long long*>(base + ws.partial);
    unsigned long long* badw = reinterpret_cast<unsigned long long*>(bad);
    const dim3 grid((unsigned)geo.G, (unsigned)C);
    const unsigned cblocks = (unsigned)((C + 63) / 64);

    mt_zero_word_kernel<<<1, 64, 0, stream>>>(badw);
    mt_key_kernel<<<(unsigned)((n + MT_THREADS - 1) / MT_THREADS), MT_THREADS, 0, stream>>>(scores, ld, y_true, n, C, a, badw);
    for (int pass = 0; pass < 4; ++pass) {                               // a -> b -> a -> b -> a
        const int shift = 1 + 8 * pass;
        const uint64_t* in = (pass & 1) ? b : a;
        uint64_t* out = (pass & 1) ? a : b;
        mt_hist_kernel<<<grid, MT_THREADS, 0, stream>>>(in, n, geo.span, shift, hist);
        mt_hist_scan_kernel<<<(unsigned)C, MT_RADIX, 0, stream>>>(hist, geo.G);
        mt_scatter_kernel<<<grid, MT_THREADS, 0, stream>>>(in, out, n, geo.span, shift, hist);
    }
    mt_part_kernel<<<grid, MT_THREADS, 0, stream>>>(a, n, geo.span, part);
    mt_part_scan_kernel<<<cblocks, 64, 0, stream>>>(part, geo.G, C, tot, n_thresholds);
    mt_compact_kernel<<<grid, MT_THREADS, 0, stream>>>(a, b, n, geo.span, part, thresholds);
    mt_integrate_kernel<<<grid, MT_THREADS, 0, stream>>>(b, n, tot, tps, fps, partial);
    mt_final_kernel<<<cblocks, 64, 0, stream>>>(partial, geo.G, C, n, tot, auroc, auprc);
    return gnx_launch_status();
}

GNX_EXPORT int gnx_confusion_counts(const long long* y_true, const long long* y_pred, long n, int K, long long* counts,
                                    long long* bad, hipStream_t stream) {
    if (n <= 0 || K <= 0 || !y_true || !y_pred || !counts || !bad) return GNX_ERR_BAD_ARG;
    if (K > CF_KMAX || n > CF_NMAX) return GNX_ERR_UNSUPPORTED;
    const int KK = K * K;
    long blocks = (n + 256L * 16 - 1) / (256L * 16);
    blocks = blocks > CF_BLOCKS ? CF_BLOCKS : blocks;
    unsigned long long* cw = reinterpret_cast<unsigned long long*>(counts);
    unsigned long long* bw = reinterpret_cast<unsigned long long*>(bad);
    cf_zero_kernel<<<(unsigned)((KK + 255) / 256), 256, 0, stream>>>(cw, KK, bw);
    cf_count_kernel<<<(unsigned)blocks, 256, 0, stream>>>(y_true, y_pred, n, K, cw, bw);
    return gnx_launch_status();
}

GNX_EXPORT int gnx_misclass_density(const float* smax, const long long* true_labels, int C, long H, long W, double* out,
                                    long long* bad, hipStream_t stream) {
    if (C <= 0 || H <= 0 || W <= 0 || !smax || !true_labels || !out || !bad) return GNX_ERR_BAD_ARG;
    if (H > (1L << 31) || W > (1L << 31) || H * W > (1L << 38)) return GNX_ERR_UNSUPPORTED;
    const long HW = H * W;
    unsigned long long* bw = reinterpret_cast<unsigned long long*>(bad);
    mt_zero_word_kernel<<<1, 64, 0, stream>>>(bw);
    mc_kernel<<<(unsigned)((HW + 255) / 256), 256, 0, stream>>>(smax, true_labels, C, HW, out, bw);
    return gnx_launch_status();
}

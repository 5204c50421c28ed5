// Hexagonal 7-neighbour convolution for the corrector g (forward, data gradient, weight gradient).
//
// Replaces hexagdly.Conv2d(kernel_size=1, stride=1) as called from
// /root/reference/gridnext/gridnet_models.py:130-147, including the
// rot90/flip sandwich of :178-185 (mode 1 applies the stencil directly on the
// Visium odd-right grid, so no data is moved).
//
// Data layout in HBM: activations are channels-last [B][H][W][C] fp32 (a spot's
// channel vector is contiguous: f writes it, g reads it, the masked CE reads it).
// Parameters keep hexagdly's shapes: kernel0 [O][I][3][1], kernel1 [O][I][2][2],
// bias [O].  Tap t (0..6): t<3 -> kernel0[..][a=t]; t>=3 -> kernel1[..][a][b], a=(t-3)>>1, b=(t-3)&1.
//
// Geometry (P = parity axis, Q = run axis):
//   mode 0 (hexagdly addressing): P = W (column index), Q = H (row index)
//   mode 1 (Visium odd-right)   : P = H (row index),    Q = W (column index)
//   tap a of kernel0      : (dp, dq) = (0, a-1)
//   tap (a,b) of kernel1  : (dp, dq) = (2b-1, (p even ? -1 : 0) + a)
// Roofline: HBM/latency bound (7*I*O MAC per position on a 4992-position grid); see DESIGN.md.
//
// Channel counts: any I, O >= 1.  One launch handles up to 64 x 64 (forward, data gradient) or 32 x 32 (weight gradient)
// channels - the corrector's own shapes (f_dim <= 64 -> 32 -> n_classes) are single launches; wider layers (many classes,
// classify=False feature inputs) are tiled over channel chunks by the entry points, the later input chunks accumulating
// onto the earlier ones' result.
//
// Layers of any radius k (hexagdly.Conv2d(kernel_size = k), a user's own corrector): the second half of this file.
// Cartesian layers (nn.Conv2d, stride 1, zero "same" padding, odd kh x kw - GridNet's corrector,
// gridnext/gridnet_models.py:51-66): the radius-k kernels over a rectangular tap table, at the end of this file.
#include "common.h"

namespace {

struct HexGeom {
    int B, H, W, mode;
    __device__ __forceinline__ void pq(int y, int x, int& p, int& q) const {
        if (mode) { p = y; q = x; } else { p = x; q = y; }
    }
    // flat position index of the tap-t neighbour of (y,x), or -1 if outside the grid
    __device__ __forceinline__ int nbr(int b, int y, int x, int t) const {
        int p, q;
        pq(y, x, p, q);
        int dp, dq;
        if (t < 3) { dp = 0; dq = t - 1; }
        else { const int a = (t - 3) >> 1, bb = (t - 3) & 1; dp = 2 * bb - 1; dq = ((p & 1) ? 0 : -1) + a; }
        const int np = p + dp, nq = q + dq;
        const int ny = mode ? np : nq, nx = mode ? nq : np;
        if (ny < 0 || ny >= H || nx < 0 || nx >= W) return -1;
        return (b * H + ny) * W + nx;
    }
    // position s whose tap-t neighbour is (y,x), or -1 (transpose of nbr)
    __device__ __forceinline__ int src(int b, int y, int x, int t) const {
        int p, q;
        pq(y, x, p, q);
        int sp, sq;
        if (t < 3) { sp = p; sq = q - (t - 1); }
        else {
            const int a = (t - 3) >> 1, bb = (t - 3) & 1;
            sp = p - (2 * bb - 1);
            sq = q - (((sp & 1) ? 0 : -1) + a);
        }
        const int sy = mode ? sp : sq, sx = mode ? sq : sp;
        if (sy < 0 || sy >= H || sx < 0 || sx >= W) return -1;
        return (b * H + sy) * W + sx;
    }
};

__device__ __forceinline__ float load_w(const float* k0, const float* k1, int I, int t, int o, int i) {
    return t < 3 ? k0[(o * I + i) * 3 + t] : k1[(o * I + i) * 4 + (t - 3)];
}

constexpr int POS_PER_BLOCK = 16;      // 312 workgroups on a 78 x 64 grid (64 per block left 178 CUs idle: 38 us per launch)

// y[pos][o] = bias[o] + sum_t sum_i W_t[o][i] * x[nbr_t(pos)][i]
// One (input chunk, output chunk) pair of channels: I, O are the chunk's sizes, i0 / o0 its first channels, IF / OF the
// layer's full channel counts (= the row strides of x, y and of the parameter tensors).
__global__ __launch_bounds__(256) void hexconv_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ k0, const float* __restrict__ k1,
    const float* __restrict__ bias, float* __restrict__ y, HexGeom g, int I, int O, int opad,
    int IF, int OF, int i0, int o0) {
    extern __shared__ __attribute__((aligned(16))) float wl[];   // [7][I][O]
    for (int idx = threadIdx.x; idx < 7 * I * O; idx += blockDim.x) {
        const int o = idx % O, i = (idx / O) % I, t = idx / (O * I);
        wl[idx] = load_w(k0, k1, IF, t, o0 + o, i0 + i);
    }
    __syncthreads();
    const int o = threadIdx.x % opad, pl0 = threadIdx.x / opad, pstep = blockDim.x / opad;
    const int npos = g.B * g.H * g.W;
    const int base = blockIdx.x * POS_PER_BLOCK;
    if (o >= O) return;
    const bool vec = ((I | IF | i0) & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const float bo = bias ? bias[o0 + o] : 0.f;
    for (int pl = pl0; pl < POS_PER_BLOCK; pl += pstep) {
        const int pos = base + pl;
        if (pos >= npos) break;
        const int xx = pos % g.W, yy = (pos / g.W) % g.H, b = pos / (g.W * g.H);
        float acc = i0 == 0 ? bo : y[(size_t)pos * OF + o0 + o];      // later input chunks continue the sum
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            const int n = g.nbr(b, yy, xx, t);
            if (n < 0) continue;
            const float* xr = x + (size_t)n * IF + i0;
            const float* wr = wl + t * I * O + o;
            if (vec) {                                      // 16-B loads of the neighbour's row, same order of the adds
                for (int i = 0; i < I; i += 4) {
                    const float4 xv = *reinterpret_cast<const float4*>(xr + i);
                    acc = fmaf(wr[i * O], xv.x, acc);
                    acc = fmaf(wr[(i + 1) * O], xv.y, acc);
                    acc = fmaf(wr[(i + 2) * O], xv.z, acc);
                    acc = fmaf(wr[(i + 3) * O], xv.w, acc);
                }
            } else {
                for (int i = 0; i < I; ++i) acc = fmaf(wr[i * O], xr[i], acc);
            }
        }
        y[(size_t)pos * OF + o0 + o] = acc;
    }
}

// dx[pos][i] = sum_t sum_o W_t[o][i] * dy[src_t(pos)][o]
__global__ __launch_bounds__(256) void hexconv_bwd_data_kernel(
    const float* __restrict__ dy, const float* __restrict__ k0, const float* __restrict__ k1,
    float* __restrict__ dx, HexGeom g, int I, int O, int ipad, int IF, int OF, int i0, int o0) {
    extern __shared__ __attribute__((aligned(16))) float wl[];   // [7][O][I]
    for (int idx = threadIdx.x; idx < 7 * I * O; idx += blockDim.x) {
        const int i = idx % I, o = (idx / I) % O, t = idx / (O * I);
        wl[idx] = load_w(k0, k1, IF, t, o0 + o, i0 + i);
    }
    __syncthreads();
    const int i = threadIdx.x % ipad, pl0 = threadIdx.x / ipad, pstep = blockDim.x / ipad;
    const int npos = g.B * g.H * g.W;
    const int base = blockIdx.x * POS_PER_BLOCK;
    if (i >= I) return;
    const bool vec = ((O | OF | o0) & 3) == 0 && (reinterpret_cast<uintptr_t>(dy) & 15) == 0;
    for (int pl = pl0; pl < POS_PER_BLOCK; pl += pstep) {
        const int pos = base + pl;
        if (pos >= npos) break;
        const int xx = pos % g.W, yy = (pos / g.W) % g.H, b = pos / (g.W * g.H);
        float acc = o0 == 0 ? 0.f : dx[(size_t)pos * IF + i0 + i];    // later output chunks continue the sum
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            const int s = g.src(b, yy, xx, t);
            if (s < 0) continue;
            const float* dr = dy + (size_t)s * OF + o0;
            const float* wr = wl + t * I * O + i;
            if (vec) {
                for (int o = 0; o < O; o += 4) {
                    const float4 dv = *reinterpret_cast<const float4*>(dr + o);
                    acc = fmaf(wr[o * I], dv.x, acc);
                    acc = fmaf(wr[(o + 1) * I], dv.y, acc);
                    acc = fmaf(wr[(o + 2) * I], dv.z, acc);
                    acc = fmaf(wr[(o + 3) * I], dv.w, acc);
                }
            } else {
                for (int o = 0; o < O; ++o) acc = fmaf(wr[o * I], dr[o], acc);
            }
        }
        dx[(size_t)pos * IF + i0 + i] = acc;
    }
}

// Weight gradient: hexconv_bwd_weight2_kernel below (its first matrix-core form - 64 positions per workgroup, 7 neighbour rows
// of every position staged element by element, a slab per wave - was removed in round 3).
constexpr int HW_POS = 64;         // (workspace sizing keeps the first version's slab count: an upper bound)


// ---- round 2: forward and data gradient on the matrix cores.  The scalar kernels above run 7 * I FMAs per output out of LDS
// (17 us per launch on a 78 x 64 grid - five forward and four data-gradient launches were a sixth of a count-only step).
// Both are, per tap, a [positions x CK] x [CK x CN] product (forward: contraction CK = input channels, data gradient:
// CK = output channels and the neighbour map transposed): a workgroup takes 32 positions x 32 output columns, its four waves
// split the seven taps (0,4 | 1,5 | 2,6 | 3), each wave multiplying with v_mfma_f32_32x32x2_f32 straight from global memory
// - a lane loads 16 B of its position's neighbour row (channels 8 g + 4 h ..) and the four matching weights (L2) - and the
// four partial 32 x 32 tiles are summed through LDS in a fixed order.  No operand staging, one barrier.  NG = CK / 8.
template <int NG, bool BWD>
__global__ __launch_bounds__(256) void hexconv_mfma_kernel(
    const float* __restrict__ in, const float* __restrict__ k0, const float* __restrict__ k1,
    const float* __restrict__ bias, float* __restrict__ out, HexGeom g, int IF, int OF) {
    __shared__ float red[4][16][64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, h = lane >> 5, i = lane & 31;
    const int npos = g.B * g.H * g.W;
    const int base = blockIdx.x * 32, n0 = blockIdx.y * 32;
    const int CN = BWD ? IF : OF, LDI = BWD ? OF : IF, LDO = BWD ? IF : OF;      // output columns; row strides
    const int pos = base + i;
    const int xx = pos % g.W, yy = (pos / g.W) % g.H, b = pos / (g.W * g.H);
    const int col = n0 + i;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const int tap = wave + 4 * tt;
        if (tap >= 7) break;                                   // wave-uniform
        const int nb = pos < npos ? (BWD ? g.src(b, yy, xx, tap) : g.nbr(b, yy, xx, tap)) : -1;
        float4 a[NG];
        float w[NG][4];
#pragma unroll
        for (int q = 0; q < NG; ++q) {
            a[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (nb >= 0) a[q] = *reinterpret_cast<const float4*>(in + (size_t)nb * LDI + 8 * q + 4 * h);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int k = 8 * q + 4 * h + c;               // contraction channel
                w[q][c] = col < CN ? (BWD ? load_w(k0, k1, IF, tap, k, col) : load_w(k0, k1, IF, tap, col, k)) : 0.f;
            }
        }
#pragma unroll
        for (int q = 0; q < NG; ++q) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, w[q][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, w[q][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].z, w[q][2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].w, w[q][3], acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
    __syncthreads();
    const float bo = (!BWD && bias && col < CN) ? bias[col] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = wave + 4 * j;
        const float v = ((red[0][r][lane] + red[1][r][lane]) + red[2][r][lane]) + red[3][r][lane];
        const int p = base + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (p < npos && col < CN) out[(size_t)p * LDO + col] = v + bo;
    }
}

// ---- round 2, second form of the weight gradient: no staging at all.  A workgroup takes 32 positions; wave w owns taps
// w and w + 4 for ALL of them (so the waves' results are disjoint: one slab per workgroup, a quarter of the slab traffic
// and of the reduce) and feeds the MFMAs straight from global memory - lane (h, c): dy[position 2 pp + h][o = c] and
// x[neighbour_t(position)][ch = c], both 128-B coalesced rows.  (The first form staged 64 x 7 neighbour rows element by
// element, a division and a neighbour computation per float: 35 us per launch.)
constexpr int HW2_POS = 32;
// (bx: the block's index in ONE layer's grid - blockIdx.x, or derived from the flat block id of the batched launch)
__device__ __forceinline__ void hexconv_bwd_weight2_body(
    const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ partial,
    const HexGeom& g, int I, int O, int IF, int OF, int i0, int o0, int bx) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, h = lane >> 5, c = lane & 31;
    const int npos = g.B * g.H * g.W;
    const int base = bx * HW2_POS;
    const int ta = wave, tb = wave + 4;                         // tb == 7: this wave has one tap only
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    float bsum = 0.f;
#pragma unroll                                                  // (all 16 position pairs' loads in flight: one round trip, not four)
    for (int pp = 0; pp < HW2_POS / 2; ++pp) {
        const int pos = base + 2 * pp + h;
        float a = 0.f, b0 = 0.f, b1 = 0.f;
        if (pos < npos) {
            const int xx = pos % g.W, yy = (pos / g.W) % g.H, b = pos / (g.W * g.H);
            if (c < O) a = dy[(size_t)pos * OF + o0 + c];
            if (c < I) {
                const int na = g.nbr(b, yy, xx, ta);
                if (na >= 0) b0 = x[(size_t)na * IF + i0 + c];
                if (tb < 7) {
                    const int nb = g.nbr(b, yy, xx, tb);
                    if (nb >= 0) b1 = x[(size_t)nb * IF + i0 + c];
                }
            }
        }
        bsum += a;
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
        if (tb < 7) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
    }
    const int nout = 7 * O * I + O;
    float* dst = partial + (size_t)bx * nout;
    if (c < I) {                                               // D[row = o][col = ch = c]
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = (r & 3) + 8 * (r >> 2) + 4 * h;
            if (o < O) {
                dst[(ta * O + o) * I + c] = acc0[r];
                if (tb < 7) dst[(tb * O + o) * I + c] = acc1[r];
            }
        }
    }
    if (wave == 0) {
        bsum += __shfl_xor(bsum, 32, 64);                      // the two position halves of output channel c
        if (h == 0 && c < O) dst[7 * O * I + c] = bsum;
    }
}
__global__ __launch_bounds__(256) void hexconv_bwd_weight2_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ partial,
    HexGeom g, int I, int O, int IF, int OF, int i0, int o0) {
    hexconv_bwd_weight2_body(x, dy, partial, g, I, O, IF, OF, i0, o0, blockIdx.x);
}

// ---- the weight gradients of SEVERAL hex layers as one launch (gnx_hexconv_bwd_weight_batch): the five layers of the
// corrector g are independent once their output gradients exist, 156 workgroups of 32 positions each, and cost a launch
// (12 us + 8 us of reduce) apiece - a quarter of a count-only training step.  Their grids are laid end to end (entry e owns
// flat block ids [first_block, first_block + nblk)); kernel body, slabs and the fixed-order reduce are the single launches'.
struct HexWEntry {
    const float* x; const float* dy; float* partial; float* dk0; float* dk1; float* dbias;
    HexGeom g;
    int I, O, nblk, first_block, accumulate;
};
constexpr int HEXW_BATCH = 8;
struct HexWBatch { HexWEntry e[HEXW_BATCH]; int n; };
__global__ __launch_bounds__(256) void hexconv_bwd_weight2_batch_kernel(const HexWBatch b) {
    int k = 0;
    while (k + 1 < b.n && (int)blockIdx.x >= b.e[k + 1].first_block) ++k;      // (uniform: at most 8 entries)
    const HexWEntry& e = b.e[k];
    hexconv_bwd_weight2_body(e.x, e.dy, e.partial, e.g, e.I, e.O, e.I, e.O, 0, 0, blockIdx.x - e.first_block);
}

// fixed-order sum of the partial slabs, scattered into hexagdly's parameter layouts (accumulating or not)
__device__ __forceinline__ void hexconv_reduce_weight_body(const float* __restrict__ partial, int nblk, int I, int O,
                                                           float* __restrict__ dk0, float* __restrict__ dk1,
                                                           float* __restrict__ dbias, int accumulate, int IF, int i0, int o0,
                                                           int out) {
    const int nout = 7 * O * I + O;
    if (out >= nout) return;
    // slabs added in index order, their loads issued 16 at a time (a plain loop over ~1000 slabs is one memory round trip
    // per term: 74 us for 29 MB)
    float s = 0.f;
    int b = 0;
    for (; b + 16 <= nblk; b += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = partial[(size_t)(b + u) * nout + out];
#pragma unroll
        for (int u = 0; u < 16; ++u) s += v[u];
    }
    for (; b < nblk; ++b) s += partial[(size_t)b * nout + out];
    float* dst;
    if (out < 7 * O * I) {
        const int i = out % I, o = (out / I) % O, t = out / (O * I);
        const int oi = (o0 + o) * IF + i0 + i;
        dst = t < 3 ? dk0 + oi * 3 + t : dk1 + oi * 4 + (t - 3);
    } else {
        if (!dbias || i0 != 0) return;                  // the bias gradient comes from the first input chunk's launches
        dst = dbias + o0 + (out - 7 * O * I);
    }
    *dst = accumulate ? *dst + s : s;
}
__global__ void hexconv_reduce_weight_kernel(const float* __restrict__ partial, int nblk, int I, int O,
                                             float* __restrict__ dk0, float* __restrict__ dk1,
                                             float* __restrict__ dbias, int accumulate, int IF, int i0, int o0) {
    hexconv_reduce_weight_body(partial, nblk, I, O, dk0, dk1, dbias, accumulate, IF, i0, o0, blockIdx.x * blockDim.x + threadIdx.x);
}
__global__ void hexconv_reduce_weight_batch_kernel(const HexWBatch b) {        // grid (blocks of 64 outputs, entries)
    const HexWEntry& e = b.e[blockIdx.y];
    hexconv_reduce_weight_body(e.partial, e.nblk, e.I, e.O, e.dk0, e.dk1, e.dbias, e.accumulate, e.I, 0, 0,
                               blockIdx.x * blockDim.x + threadIdx.x);
}

int pow2_at_least(int v) { int p = 1; while (p < v) p <<= 1; return p; }

constexpr int HEX_CHUNK = 64;      // channels per launch, forward and data gradient (7 * 64 * 64 weights = 112 KB of LDS)
constexpr int HEX_WCHUNK = 32;     // channels per launch, weight gradient (one 32 x 32 MFMA tile per tap)

// the MFMA forward / data-gradient form takes contraction widths 8, 16, 32, 64 on 16-B aligned rows (other widths:
// the scalar kernels)
bool hex_mfma_ok(int CK, const float* in, long npos) {
    return (CK == 8 || CK == 16 || CK == 32 || CK == 64) && (reinterpret_cast<uintptr_t>(in) & 15) == 0 &&
           npos < (1L << 30);
}

}  // namespace

GNX_EXPORT int gnx_hexconv_fwd(const float* x, const float* kernel0, const float* kernel1, const float* bias,
                               float* y, int B, int H, int W, int I, int O, int mode, hipStream_t stream) {
    if (!x || !kernel0 || !kernel1 || !y || B < 0 || H <= 0 || W <= 0 || I <= 0 || O <= 0) return GNX_ERR_BAD_ARG;
    const long npos = (long)B * H * W;
    if (npos == 0) return GNX_OK;
    HexGeom g{B, H, W, mode};
    if (hex_mfma_ok(I, x, npos)) {
        dim3 grid(gnx_cdiv(npos, 32), gnx_cdiv(O, 32));
        if (I == 8) hexconv_mfma_kernel<1, false><<<grid, 256, 0, stream>>>(x, kernel0, kernel1, bias, y, g, I, O);
        else if (I == 16) hexconv_mfma_kernel<2, false><<<grid, 256, 0, stream>>>(x, kernel0, kernel1, bias, y, g, I, O);
        else if (I == 32) hexconv_mfma_kernel<4, false><<<grid, 256, 0, stream>>>(x, kernel0, kernel1, bias, y, g, I, O);
        else hexconv_mfma_kernel<8, false><<<grid, 256, 0, stream>>>(x, kernel0, kernel1, bias, y, g, I, O);
        return gnx_launch_status();
    }
    for (int o0 = 0; o0 < O; o0 += HEX_CHUNK)
        for (int i0 = 0; i0 < I; i0 += HEX_CHUNK) {         // input chunks in order: chunk k continues chunk k-1's sums
            const int oc = O - o0 < HEX_CHUNK ? O - o0 : HEX_CHUNK, ic = I - i0 < HEX_CHUNK ? I - i0 : HEX_CHUNK;
            hexconv_fwd_kernel<<<gnx_cdiv(npos, POS_PER_BLOCK), 256, 7 * ic * oc * sizeof(float), stream>>>(
                x, kernel0, kernel1, bias, y, g, ic, oc, pow2_at_least(oc), I, O, i0, o0);
        }
    return gnx_launch_status();
}

GNX_EXPORT int gnx_hexconv_bwd_data(const float* dy, const float* kernel0, const float* kernel1, float* dx,
                                    int B, int H, int W, int I, int O, int mode, hipStream_t stream) {
    if (!dy || !kernel0 || !kernel1 || !dx || B < 0 || H <= 0 || W <= 0 || I <= 0 || O <= 0) return GNX_ERR_BAD_ARG;
    const long npos = (long)B * H * W;
    if (npos == 0) return GNX_OK;
    HexGeom g{B, H, W, mode};
    if (hex_mfma_ok(O, dy, npos)) {
        dim3 grid(gnx_cdiv(npos, 32), gnx_cdiv(I, 32));
        if (O == 8) hexconv_mfma_kernel<1, true><<<grid, 256, 0, stream>>>(dy, kernel0, kernel1, nullptr, dx, g, I, O);
        else if (O == 16) hexconv_mfma_kernel<2, true><<<grid, 256, 0, stream>>>(dy, kernel0, kernel1, nullptr, dx, g, I, O);
        else if (O == 32) hexconv_mfma_kernel<4, true><<<grid, 256, 0, stream>>>(dy, kernel0, kernel1, nullptr, dx, g, I, O);
        else hexconv_mfma_kernel<8, true><<<grid, 256, 0, stream>>>(dy, kernel0, kernel1, nullptr, dx, g, I, O);
        return gnx_launch_status();
    }
    for (int i0 = 0; i0 < I; i0 += HEX_CHUNK)
        for (int o0 = 0; o0 < O; o0 += HEX_CHUNK) {
            const int oc = O - o0 < HEX_CHUNK ? O - o0 : HEX_CHUNK, ic = I - i0 < HEX_CHUNK ? I - i0 : HEX_CHUNK;
            hexconv_bwd_data_kernel<<<gnx_cdiv(npos, POS_PER_BLOCK), 256, 7 * ic * oc * sizeof(float), stream>>>(
                dy, kernel0, kernel1, dx, g, ic, oc, pow2_at_least(ic), I, O, i0, o0);
        }
    return gnx_launch_status();
}

// workspace floats needed by gnx_hexconv_bwd_weight
GNX_EXPORT long gnx_hexconv_bwd_weight_workspace(int B, int H, int W, int I, int O) {
    const long npos = (long)B * H * W;
    const long ic = I < HEX_WCHUNK ? I : HEX_WCHUNK, oc = O < HEX_WCHUNK ? O : HEX_WCHUNK;     // one chunk pair at a time
    return 4L * gnx_cdiv(npos, HW_POS) * (7L * oc * ic + oc);                                // one slab per wave
}

GNX_EXPORT int gnx_hexconv_bwd_weight(const float* x, const float* dy, float* dkernel0, float* dkernel1,
                                      float* dbias, float* workspace, int B, int H, int W, int I, int O,
                                      int mode, int accumulate, hipStream_t stream) {
    if (!x || !dy || !dkernel0 || !dkernel1 || !workspace || I <= 0 || O <= 0 || H <= 0 || W <= 0 || B < 0)
        return GNX_ERR_BAD_ARG;
    const long npos = (long)B * H * W;
    const int nblk = gnx_cdiv(npos, HW2_POS);
    HexGeom g{B, H, W, mode};
    // one (input chunk, output chunk) pair after the other on the stream, each through the same workspace
    for (int o0 = 0; o0 < O; o0 += HEX_WCHUNK)
        for (int i0 = 0; i0 < I; i0 += HEX_WCHUNK) {
            const int oc = O - o0 < HEX_WCHUNK ? O - o0 : HEX_WCHUNK, ic = I - i0 < HEX_WCHUNK ? I - i0 : HEX_WCHUNK;
            const int nout = 7 * oc * ic + oc;
            if (nblk > 0) {
                hexconv_bwd_weight2_kernel<<<nblk, 256, 0, stream>>>(x, dy, workspace, g, ic, oc, I, O, i0, o0);
            }
            hexconv_reduce_weight_kernel<<<gnx_cdiv(nout, 64), 64, 0, stream>>>(workspace, nblk, ic, oc, dkernel0,
                                                                                dkernel1, dbias, accumulate, I, i0, o0);
        }
    return gnx_launch_status();
}

// n hex layers' weight gradients as ONE launch plus one batched reduce: exactly gnx_hexconv_bwd_weight for every item, bit for
// bit (same kernel body, slab layout and reduce order).  Layers wider than 32 channels on either side (which the single entry
// point cuts into chunk pairs) or more than 8 items: GNX_ERR_UNSUPPORTED, nothing launched.  `items`: HOST array of
// gnx_hexconv_wgrad_item (include/gridnext_hip.h); each item's workspace: gnx_hexconv_bwd_weight_workspace floats.
GNX_EXPORT int gnx_hexconv_bwd_weight_batch(const void* items_v, int n, hipStream_t stream) {
    const gnx_hexconv_wgrad_item* it = static_cast<const gnx_hexconv_wgrad_item*>(items_v);
    if (!it || n < 0) return GNX_ERR_BAD_ARG;
    if (n == 0) return GNX_OK;
    if (n > HEXW_BATCH) return GNX_ERR_UNSUPPORTED;
    HexWBatch b;
    b.n = n;
    int blocks = 0, max_nout = 0;
    for (int q = 0; q < n; ++q) {
        const gnx_hexconv_wgrad_item& a = it[q];
        if (!a.x || !a.dy || !a.dkernel0 || !a.dkernel1 || !a.workspace || a.I <= 0 || a.O <= 0 || a.H <= 0 || a.W <= 0 || a.B < 0)
            return GNX_ERR_BAD_ARG;
        if (a.I > HEX_WCHUNK || a.O > HEX_WCHUNK) return GNX_ERR_UNSUPPORTED;
        const long npos = (long)a.B * a.H * a.W;
        if (npos <= 0 || npos >= (1L << 30)) return GNX_ERR_UNSUPPORTED;
        HexWEntry& e = b.e[q];
        e.x = a.x; e.dy = a.dy; e.partial = a.workspace; e.dk0 = a.dkernel0; e.dk1 = a.dkernel1; e.dbias = a.dbias;
        e.g = HexGeom{a.B, a.H, a.W, a.mode};
        e.I = a.I; e.O = a.O; e.nblk = gnx_cdiv(npos, HW2_POS); e.first_block = blocks; e.accumulate = a.accumulate;
        blocks += e.nblk;
        const int nout = 7 * a.O * a.I + a.O;
        if (nout > max_nout) max_nout = nout;
    }
    hexconv_bwd_weight2_batch_kernel<<<blocks, 256, 0, stream>>>(b);
    hexconv_reduce_weight_batch_kernel<<<dim3(gnx_cdiv(max_nout, 64), n), 64, 0, stream>>>(b);
    return gnx_launch_status();
}

// ==== radius-k layers: hexagdly.Conv2d(kernel_size = k) for any k in 1..HEXK_KMAX ==========================================
// The size-1 kernels above stay as they are (the reference's corrector); these generalise their structure from the 7-entry
// neighbour table to the T(k) = 1 + 3k(k+1) taps of a radius-k layer.  Parameters in hexagdly's order and shapes:
//   kernel0 [O][I][2k+1][1]          tap a     -> (dp, dq) = (0, a - k)
//   kernel{j} [O][I][2k+1-j][2]      tap (a,b) -> (dp, dq) = ((2b - 1) j, top(j, p) + a),   j = 1..k,
//   top(j, p) = -k + floor(j/2) + (j odd ? p mod 2 : 0)          (P / Q axes as in HexGeom)
// Tap t counts kernel0's taps first, then kernel1's (a, b) row-major, then kernel2's, ...  At k = 1 this is the table above.
// Neighbours outside the grid read zero; the output has the input's size; the bias is added once.
//
//   forward / data gradient, contraction width 8/16/32/64 on 16-B aligned rows: hexk_mfma_kernel - hexconv_mfma_kernel's
//     per-tap [32 positions x CK] x [CK x 32 columns] products on v_mfma_f32_32x32x2_f32, the T taps dealt round-robin to
//     eight waves, the eight partial tiles summed through LDS in wave order.  Operands come straight from global memory as
//     there (the weights of a tap are L2-resident: T x 32 x 32 fp32 is 78 KB at k = 2, 151 KB at k = 3 - staging them
//     whole would take most of a CU's 160 KiB of LDS, so nothing is staged; the LDS holds only the 32 KB of partial tiles);
//   any other width: hexk_scalar_kernel - the scalar kernels' form (one thread per (position, output channel), the chunk's
//     weights in LDS), its channel chunks sized so that T x KC x NC fp32 fit HEXK_LDS;
//   weight gradient: hexk_bwd_weight_kernel writes one slab [T][O][I] + [O] per 64 positions (a workgroup: 8 taps, two per
//     wave, grid.y over tap groups), hexk_reduce_weight_kernel sums the slabs in index order into hexagdly's per-kernel
//     layouts.  No atomics: every result is the same bits on every call.
namespace {

constexpr int HEXK_KMAX = 8;                   // T(8) = 217 taps
constexpr int HEXK_WAVES = 8;                  // waves of the matrix-core forward / data gradient
constexpr int HEXK_LDS = 64 * 1024;            // bytes of staged weights in the scalar kernel (two workgroups per CU)
constexpr int HEXK_WPOS = 64;                  // positions per weight-gradient slab

struct HexKW { const float* k[HEXK_KMAX + 1]; };          // kernel0 .. kernel{k}
struct HexKD { float* k[HEXK_KMAX + 1]; };                // their gradients (NULL: not wanted)

__host__ __device__ __forceinline__ int hexk_taps(int k) { return 1 + 3 * k * (k + 1); }

struct HexTap { int j, dp, dq0, idx, ntap; };  // tensor, P offset, Q offset before the parity term, index in / taps of tensor j

__device__ __forceinline__ HexTap hexk_tap(int k, int t) {
    HexTap r;
    const int n0 = 2 * k + 1;
    if (t < n0) { r.j = 0; r.dp = 0; r.dq0 = t - k; r.idx = t; r.ntap = n0; return r; }
    t -= n0;
    int j = 1;
    while (t >= 2 * (n0 - j)) { t -= 2 * (n0 - j); ++j; }
    const int a = t >> 1, b = t & 1;
    r.j = j; r.dp = (2 * b - 1) * j; r.dq0 = -k + j / 2 + a; r.idx = t; r.ntap = 2 * (n0 - j);
    return r;
}

// flat position of the tap-tp neighbour of (y, x) (BWD: of the position whose tap-tp neighbour is (y, x)), or -1
template <bool BWD>
__device__ __forceinline__ int hexk_link(const HexGeom& g, int b, int y, int x, const HexTap& tp) {
    int p, q;
    g.pq(y, x, p, q);
    int np, nq;
    if (!BWD) { np = p + tp.dp; nq = q + tp.dq0 + ((tp.j & 1) ? (p & 1) : 0); }
    else { np = p - tp.dp; nq = q - tp.dq0 - ((tp.j & 1) ? (np & 1) : 0); }
    const int ny = g.mode ? np : nq, nx = g.mode ? nq : np;
    if (ny < 0 || ny >= g.H || nx < 0 || nx >= g.W) return -1;
    return (b * g.H + ny) * g.W + nx;
}

// The tap geometry is a compile-time policy G of the kernels below (a kernel argument: the grid's sizes B, H, W plus what the
// table needs).  G::WT / G::DT: the weight tensors / their gradients, tensor j laid out [O][I][tensor_taps(j)]; tap(t): tap t of
// the table, with its tensor j, its index idx in it and that tensor's tap count ntap; link<BWD>: the flat position a tap reads.
struct HexTaps : HexGeom {                     // radius-k hexagonal table
    int k;
    using WT = HexKW;
    using DT = HexKD;
    using Tap = HexTap;
    __device__ __forceinline__ int taps() const { return hexk_taps(k); }
    __device__ __forceinline__ int tensors() const { return k + 1; }
    __device__ __forceinline__ int tensor_taps(int j) const { return j ? 2 * (2 * k + 1 - j) : 2 * k + 1; }
    __device__ __forceinline__ Tap tap(int t) const { return hexk_tap(k, t); }
    template <bool BWD>
    __device__ __forceinline__ int link(int b, int y, int x, const Tap& tp) const { return hexk_link<BWD>(*this, b, y, x, tp); }
};

// kh x kw Cartesian table, zero "same" padding: tap t = a kw + b reads (r + a - kh/2, c + b - kw/2); ONE weight tensor
// [O][I][kh][kw] (nn.Conv2d's).  Positions are flat, so a tap is tested against its own row and array: no wrap-around into
// the next row, none into the next array of the batch.
struct GridKW { const float* k[1]; };
struct GridKD { float* k[1]; };
struct GridTap { int j, dr, dc, idx, ntap; };
struct GridTaps {
    int B, H, W, kh, kw;
    using WT = GridKW;
    using DT = GridKD;
    using Tap = GridTap;
    __device__ __forceinline__ int taps() const { return kh * kw; }
    __device__ __forceinline__ int tensors() const { return 1; }
    __device__ __forceinline__ int tensor_taps(int) const { return kh * kw; }
    __device__ __forceinline__ Tap tap(int t) const { return Tap{0, t / kw - kh / 2, t % kw - kw / 2, t, kh * kw}; }
    template <bool BWD>
    __device__ __forceinline__ int link(int b, int y, int x, const Tap& tp) const {
        const int ny = BWD ? y - tp.dr : y + tp.dr, nx = BWD ? x - tp.dc : x + tp.dc;
        if (ny < 0 || ny >= H || nx < 0 || nx >= W) return -1;
        return (b * H + ny) * W + nx;
    }
};

template <class KW, class Tap>
__device__ __forceinline__ float hexk_w(const KW& w, const Tap& tp, int I, int o, int i) {
    return w.k[tp.j][((size_t)o * I + i) * tp.ntap + tp.idx];
}

// out[pos][n] (+)= sum_t sum_c W_t * in[link_t(pos)][c]; forward: c = input channel, n = output channel (+ bias);
// BWD: c = output channel, n = input channel, links transposed.  NG = CK / 8.
template <class G, int NG, bool BWD>
__global__ __launch_bounds__(64 * HEXK_WAVES) void hexk_mfma_kernel(
    const float* __restrict__ in, const typename G::WT w, const float* __restrict__ bias, float* __restrict__ out, G g,
    int I, int O) {
    __shared__ float red[HEXK_WAVES][16][64];
    const int lane = threadIdx.x & 63, h = lane >> 5, i = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int T = g.taps();
    const int npos = g.B * g.H * g.W;
    const int base = blockIdx.x * 32, n0 = blockIdx.y * 32;
    const int CN = BWD ? I : O, LDI = BWD ? O : I, LDO = BWD ? I : O;      // output columns; row strides
    const int pos = base + i;
    const int xx = pos % g.W, yy = (pos / g.W) % g.H, b = pos / (g.W * g.H);
    const int col = n0 + i;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int tap = wave; tap < T; tap += HEXK_WAVES) {
        const typename G::Tap tp = g.tap(tap);
        const int nb = pos < npos ? g.template link<BWD>(b, yy, xx, tp) : -1;
        float4 a[NG];
        float wv[NG][4];
#pragma unroll
        for (int q = 0; q < NG; ++q) {
            a[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (nb >= 0) a[q] = *reinterpret_cast<const float4*>(in + (size_t)nb * LDI + 8 * q + 4 * h);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int kc = 8 * q + 4 * h + c;                 // contraction channel
                wv[q][c] = col < CN ? (BWD ? hexk_w(w, tp, I, kc, col) : hexk_w(w, tp, I, col, kc)) : 0.f;
            }
        }
#pragma unroll
        for (int q = 0; q < NG; ++q) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, wv[q][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, wv[q][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].z, wv[q][2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].w, wv[q][3], acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
    __syncthreads();
    const float bo = (!BWD && bias && col < CN) ? bias[col] : 0.f;
#pragma unroll
    for (int jj = 0; jj < 16 / HEXK_WAVES; ++jj) {
        const int r = wave + HEXK_WAVES * jj;
        float v = red[0][r][lane];
#pragma unroll
        for (int u = 1; u < HEXK_WAVES; ++u) v += red[u][r][lane];
        const int p = base + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (p < npos && col < CN) out[(size_t)p * LDO + col] = v + bo;
    }
}

// Any widths: one (contraction chunk [kc0, kc0 + KC), output chunk [nc0, nc0 + NC)) per launch; KF / NF: the full widths
// (row strides of `in` / `out`).  Later contraction chunks continue the sums of the earlier ones.
template <class G, bool BWD>
__global__ __launch_bounds__(256) void hexk_scalar_kernel(
    const float* __restrict__ in, const typename G::WT w, const float* __restrict__ bias, float* __restrict__ out, G g,
    int KC, int NC, int npad, int KF, int NF, int kc0, int nc0) {
    extern __shared__ __attribute__((aligned(16))) float wl[];   // [T][KC][NC]
    const int T = g.taps(), I = BWD ? NF : KF;
    // staged tensor by tensor in their own [o][i][tap] order (contiguous reads), scattered into the tap-major LDS image
    const int IC = BWD ? NC : KC, OC = BWD ? KC : NC, i0 = BWD ? nc0 : kc0, o0 = BWD ? kc0 : nc0;
    for (int j = 0, t0 = 0; j < g.tensors(); t0 += g.tensor_taps(j), ++j) {
        const int ntap = g.tensor_taps(j);
        for (int e = threadIdx.x; e < OC * IC * ntap; e += blockDim.x) {
            const int idx = e % ntap, i = (e / ntap) % IC, o = e / (ntap * IC);
            const int c = BWD ? o : i, n = BWD ? i : o;
            wl[((t0 + idx) * KC + c) * NC + n] = w.k[j][((size_t)(o0 + o) * I + i0 + i) * ntap + idx];
        }
    }
    __syncthreads();
    const int n = threadIdx.x % npad, pl0 = threadIdx.x / npad, pstep = blockDim.x / npad;
    const int npos = g.B * g.H * g.W;
    const int base = blockIdx.x * POS_PER_BLOCK;
    if (n >= NC) return;
    const bool vec = ((KC | KF | kc0) & 3) == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    const float bo = (!BWD && bias) ? bias[nc0 + n] : 0.f;
    for (int pl = pl0; pl < POS_PER_BLOCK; pl += pstep) {
        const int pos = base + pl;
        if (pos >= npos) break;
        const int xx = pos % g.W, yy = (pos / g.W) % g.H, b = pos / (g.W * g.H);
        float acc = kc0 == 0 ? bo : out[(size_t)pos * NF + nc0 + n];
        for (int t = 0; t < T; ++t) {
            const int s = g.template link<BWD>(b, yy, xx, g.tap(t));
            if (s < 0) continue;
            const float* r = in + (size_t)s * KF + kc0;
            const float* wr = wl + t * KC * NC + n;
            if (vec) {
                for (int c = 0; c < KC; c += 4) {
                    const float4 v = *reinterpret_cast<const float4*>(r + c);
                    acc = fmaf(wr[c * NC], v.x, acc);
                    acc = fmaf(wr[(c + 1) * NC], v.y, acc);
                    acc = fmaf(wr[(c + 2) * NC], v.z, acc);
                    acc = fmaf(wr[(c + 3) * NC], v.w, acc);
                }
            } else {
                for (int c = 0; c < KC; ++c) acc = fmaf(wr[c * NC], r[c], acc);
            }
        }
        out[(size_t)pos * NF + nc0 + n] = acc;
    }
}

// Weight-gradient slab of positions [64 bx, 64 bx + 64) for taps [8 by, 8 by + 8): wave w owns taps 8 by + w and 8 by + w + 4,
// lane (h, c) feeds dy[position 2 pp + h][o = c] and x[link_t(position)][ch = c] to the MFMAs (hexconv_bwd_weight2_body's
// form).  Slab layout: [T][O][I] then the bias gradient [O] (written by the tap group 0).
template <class G>
__global__ __launch_bounds__(256) void hexk_bwd_weight_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ partial, G g,
    int I, int O, int IF, int OF, int i0, int o0) {
    const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int T = g.taps();
    const int npos = g.B * g.H * g.W;
    const int base = blockIdx.x * HEXK_WPOS;
    const int ta = blockIdx.y * 8 + wave, tb = ta + 4;
    const bool has_a = ta < T, has_b = tb < T;
    const typename G::Tap tpa = g.tap(has_a ? ta : 0), tpb = g.tap(has_b ? tb : 0);
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    float bsum = 0.f;
    for (int half = 0; half < HEXK_WPOS / 32; ++half) {
#pragma unroll                                                  // (the 16 position pairs' loads in flight together)
        for (int pp = 0; pp < 16; ++pp) {
            const int pos = base + 32 * half + 2 * pp + h;
            float a = 0.f, b0 = 0.f, b1 = 0.f;
            if (pos < npos) {
                const int xx = pos % g.W, yy = (pos / g.W) % g.H, b = pos / (g.W * g.H);
                if (c < O) a = dy[(size_t)pos * OF + o0 + c];
                if (c < I) {
                    if (has_a) {
                        const int na = g.template link<false>(b, yy, xx, tpa);
                        if (na >= 0) b0 = x[(size_t)na * IF + i0 + c];
                    }
                    if (has_b) {
                        const int nb = g.template link<false>(b, yy, xx, tpb);
                        if (nb >= 0) b1 = x[(size_t)nb * IF + i0 + c];
                    }
                }
            }
            bsum += a;
            if (has_a) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
            if (has_b) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
        }
    }
    float* dst = partial + (size_t)blockIdx.x * ((size_t)T * O * I + O);
    if (c < I) {                                               // D[row = o][col = ch = c]
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = (r & 3) + 8 * (r >> 2) + 4 * h;
            if (o < O) {
                if (has_a) dst[((size_t)ta * O + o) * I + c] = acc0[r];
                if (has_b) dst[((size_t)tb * O + o) * I + c] = acc1[r];
            }
        }
    }
    if (blockIdx.y == 0 && wave == 0) {
        bsum += __shfl_xor(bsum, 32, 64);                      // the two position halves of output channel c
        if (h == 0 && c < O) dst[(size_t)T * O * I + c] = bsum;
    }
}

// fixed-order sum of the slabs into kernel{j} [O][I][..] and the bias (accumulating or not); NULL destinations are skipped
template <class G>
__global__ void hexk_reduce_weight_kernel(const float* __restrict__ partial, int nblk, G g, int I, int O,
                                          const typename G::DT d, float* __restrict__ dbias, int accumulate, int IF, int i0,
                                          int o0) {
    const int T = g.taps();
    const long nout = (long)T * O * I + O;
    const long out = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (out >= nout) return;
    float* dst;
    if (out < (long)T * O * I) {
        const int i = out % I, o = (out / I) % O, t = out / ((long)O * I);
        const typename G::Tap tp = g.tap(t);
        if (!d.k[tp.j]) return;
        dst = d.k[tp.j] + ((size_t)(o0 + o) * IF + i0 + i) * tp.ntap + tp.idx;
    } else {
        if (!dbias || i0 != 0) return;                  // the bias gradient comes from the first input chunk's launches
        dst = dbias + o0 + (out - (long)T * O * I);
    }
    float s = 0.f;
    int b = 0;
    for (; b + 16 <= nblk; b += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = partial[(size_t)(b + u) * nout + out];
#pragma unroll
        for (int u = 0; u < 16; ++u) s += v[u];
    }
    for (; b < nblk; ++b) s += partial[(size_t)b * nout + out];
    *dst = accumulate ? *dst + s : s;
}

// the forward (BWD false: in = x, K = I, N = O) or data gradient (in = dy, K = O, N = I) of a layer of T taps
template <class G, bool BWD>
int hexk_apply(const float* in, const typename G::WT& w, const float* bias, float* out, const G& g, int T, int I, int O,
               hipStream_t stream) {
    const long npos = (long)g.B * g.H * g.W;
    const int K = BWD ? O : I, N = BWD ? I : O;
    if (hex_mfma_ok(K, in, npos)) {
        const dim3 grid(gnx_cdiv(npos, 32), gnx_cdiv(N, 32));
        const int blk = 64 * HEXK_WAVES;
        if (K == 8) hexk_mfma_kernel<G, 1, BWD><<<grid, blk, 0, stream>>>(in, w, bias, out, g, I, O);
        else if (K == 16) hexk_mfma_kernel<G, 2, BWD><<<grid, blk, 0, stream>>>(in, w, bias, out, g, I, O);
        else if (K == 32) hexk_mfma_kernel<G, 4, BWD><<<grid, blk, 0, stream>>>(in, w, bias, out, g, I, O);
        else hexk_mfma_kernel<G, 8, BWD><<<grid, blk, 0, stream>>>(in, w, bias, out, g, I, O);
        return gnx_launch_status();
    }
    const int NC = N < HEX_CHUNK ? N : HEX_CHUNK;
    int KC = HEXK_LDS / (int)(T * NC * sizeof(float));
    KC = KC < 1 ? 1 : (KC > K ? K : KC);
    for (int n0 = 0; n0 < N; n0 += NC)
        for (int c0 = 0; c0 < K; c0 += KC) {             // contraction chunks in order: chunk c continues chunk c-1's sums
            const int nc = N - n0 < NC ? N - n0 : NC, kc = K - c0 < KC ? K - c0 : KC;
            hexk_scalar_kernel<G, BWD><<<gnx_cdiv(npos, POS_PER_BLOCK), 256, T * kc * nc * sizeof(float), stream>>>(
                in, w, bias, out, g, kc, nc, pow2_at_least(nc), K, N, c0, n0);
        }
    return gnx_launch_status();
}

// the weight and bias gradient of a layer of T taps: one (input chunk, output chunk) pair after the other on the stream, each
// through the same workspace
template <class G>
int hexk_weight_grad(const float* x, const float* dy, const typename G::DT& d, float* dbias, float* workspace, const G& g,
                     int T, int I, int O, int accumulate, hipStream_t stream) {
    const int nblk = gnx_cdiv((long)g.B * g.H * g.W, HEXK_WPOS);
    for (int o0 = 0; o0 < O; o0 += HEX_WCHUNK)
        for (int i0 = 0; i0 < I; i0 += HEX_WCHUNK) {
            const int oc = O - o0 < HEX_WCHUNK ? O - o0 : HEX_WCHUNK, ic = I - i0 < HEX_WCHUNK ? I - i0 : HEX_WCHUNK;
            const long nout = (long)T * oc * ic + oc;
            if (nblk > 0)
                hexk_bwd_weight_kernel<G><<<dim3(nblk, gnx_cdiv(T, 8)), 256, 0, stream>>>(x, dy, workspace, g, ic, oc, I, O,
                                                                                           i0, o0);
            hexk_reduce_weight_kernel<G><<<gnx_cdiv(nout, 64), 64, 0, stream>>>(workspace, nblk, g, ic, oc, d, dbias,
                                                                                 accumulate, I, i0, o0);
        }
    return gnx_launch_status();
}

// common argument checks; fills w from the HOST array `kernels` (k + 1 device pointers)
int hexk_check(const float* const* kernels, HexKW& w, int B, int H, int W, int I, int O, int k) {
    if (!kernels || B < 0 || H <= 0 || W <= 0 || I <= 0 || O <= 0 || k < 1) return GNX_ERR_BAD_ARG;
    if (k > HEXK_KMAX) return GNX_ERR_UNSUPPORTED;
    if ((long)B * H * W >= (1L << 30)) return GNX_ERR_UNSUPPORTED;
    for (int j = 0; j <= HEXK_KMAX; ++j) {
        w.k[j] = j <= k ? kernels[j] : nullptr;
        if (j <= k && !w.k[j]) return GNX_ERR_BAD_ARG;
    }
    return GNX_OK;
}

}  // namespace

GNX_EXPORT int gnx_hexconv_k_fwd(const float* x, const float* const* kernels, const float* bias, float* y,
                                 int B, int H, int W, int I, int O, int k, int mode, hipStream_t stream) {
    if (!x || !y) return GNX_ERR_BAD_ARG;
    HexKW w;
    const int rc = hexk_check(kernels, w, B, H, W, I, O, k);
    if (rc != GNX_OK) return rc;
    if ((long)B * H * W == 0) return GNX_OK;
    return hexk_apply<HexTaps, false>(x, w, bias, y, HexTaps{{B, H, W, mode}, k}, hexk_taps(k), I, O, stream);
}

GNX_EXPORT int gnx_hexconv_k_bwd_data(const float* dy, const float* const* kernels, float* dx,
                                      int B, int H, int W, int I, int O, int k, int mode, hipStream_t stream) {
    if (!dy || !dx) return GNX_ERR_BAD_ARG;
    HexKW w;
    const int rc = hexk_check(kernels, w, B, H, W, I, O, k);
    if (rc != GNX_OK) return rc;
    if ((long)B * H * W == 0) return GNX_OK;
    return hexk_apply<HexTaps, true>(dy, w, nullptr, dx, HexTaps{{B, H, W, mode}, k}, hexk_taps(k), I, O, stream);
}

// workspace floats needed by gnx_hexconv_k_bwd_weight: one slab per 64 positions for one 32 x 32 chunk pair
GNX_EXPORT long gnx_hexconv_k_bwd_weight_workspace(int B, int H, int W, int I, int O, int k) {
    if (B < 0 || H <= 0 || W <= 0 || I <= 0 || O <= 0 || k < 1 || k > HEXK_KMAX) return 0;
    const long ic = I < HEX_WCHUNK ? I : HEX_WCHUNK, oc = O < HEX_WCHUNK ? O : HEX_WCHUNK;
    return (long)gnx_cdiv((long)B * H * W, HEXK_WPOS) * (hexk_taps(k) * oc * ic + oc);
}

GNX_EXPORT int gnx_hexconv_k_bwd_weight(const float* x, const float* dy, float* const* dkernels, float* dbias,
                                        float* workspace, int B, int H, int W, int I, int O, int k, int mode,
                                        int accumulate, hipStream_t stream) {
    if (!x || !dy || !dkernels || B < 0 || H <= 0 || W <= 0 || I <= 0 || O <= 0 || k < 1) return GNX_ERR_BAD_ARG;
    if (k > HEXK_KMAX) return GNX_ERR_UNSUPPORTED;
    const long npos = (long)B * H * W;
    if (npos >= (1L << 30)) return GNX_ERR_UNSUPPORTED;
    HexKD d;
    bool any = dbias != nullptr;
    for (int j = 0; j <= HEXK_KMAX; ++j) {
        d.k[j] = j <= k ? dkernels[j] : nullptr;
        any = any || d.k[j];
    }
    if (!any) return GNX_OK;                             // no gradient wanted: nothing written
    if (npos > 0 && !workspace) return GNX_ERR_BAD_ARG;
    return hexk_weight_grad(x, dy, d, dbias, workspace, HexTaps{{B, H, W, mode}, k}, hexk_taps(k), I, O, accumulate, stream);
}

// ==== Cartesian layers: nn.Conv2d(I, O, (kh, kw), stride 1, zero "same" padding), odd kh, kw ================================
// The kernels above over GridTaps: forward, data gradient and slab + fixed-order-reduce weight gradient of the Cartesian
// corrector's layers on the same channels-last grids.  weight [O][I][kh][kw] is the table's single tensor as it stands.
namespace {

constexpr int GRIDCONV_TMAX = 217;             // kh kw at most the taps of the widest hex table (T(HEXK_KMAX))

int gridconv_check(int B, int H, int W, int I, int O, int kh, int kw) {
    if (B < 0 || H <= 0 || W <= 0 || I <= 0 || O <= 0 || kh < 1 || kw < 1 || !(kh & 1) || !(kw & 1)) return GNX_ERR_BAD_ARG;
    if ((long)kh * kw > GRIDCONV_TMAX) return GNX_ERR_UNSUPPORTED;
    if ((long)B * H * W >= (1L << 30)) return GNX_ERR_UNSUPPORTED;
    return GNX_OK;
}

}  // namespace

GNX_EXPORT int gnx_gridconv_fwd(const float* x, const float* weight, const float* bias, float* y,
                                int B, int H, int W, int I, int O, int kh, int kw, hipStream_t stream) {
    if (!x || !weight || !y) return GNX_ERR_BAD_ARG;
    const int rc = gridconv_check(B, H, W, I, O, kh, kw);
    if (rc != GNX_OK) return rc;
    if ((long)B * H * W == 0) return GNX_OK;
    return hexk_apply<GridTaps, false>(x, GridKW{{weight}}, bias, y, GridTaps{B, H, W, kh, kw}, kh * kw, I, O, stream);
}

GNX_EXPORT int gnx_gridconv_bwd_data(const float* dy, const float* weight, float* dx,
                                     int B, int H, int W, int I, int O, int kh, int kw, hipStream_t stream) {
    if (!dy || !weight || !dx) return GNX_ERR_BAD_ARG;
    const int rc = gridconv_check(B, H, W, I, O, kh, kw);
    if (rc != GNX_OK) return rc;
    if ((long)B * H * W == 0) return GNX_OK;
    return hexk_apply<GridTaps, true>(dy, GridKW{{weight}}, nullptr, dx, GridTaps{B, H, W, kh, kw}, kh * kw, I, O, stream);
}

// workspace floats needed by gnx_gridconv_bwd_weight: one slab per 64 positions for one 32 x 32 chunk pair
GNX_EXPORT long gnx_gridconv_bwd_weight_workspace(int B, int H, int W, int I, int O, int kh, int kw) {
    if (gridconv_check(B, H, W, I, O, kh, kw) != GNX_OK) return 0;
    const long ic = I < HEX_WCHUNK ? I : HEX_WCHUNK, oc = O < HEX_WCHUNK ? O : HEX_WCHUNK;
    return (long)gnx_cdiv((long)B * H * W, HEXK_WPOS) * ((long)kh * kw * oc * ic + oc);
}

GNX_EXPORT int gnx_gridconv_bwd_weight(const float* x, const float* dy, float* dweight, float* dbias, float* workspace,
                                       int B, int H, int W, int I, int O, int kh, int kw, int accumulate,
                                       hipStream_t stream) {
    if (!x || !dy) return GNX_ERR_BAD_ARG;
    const int rc = gridconv_check(B, H, W, I, O, kh, kw);
    if (rc != GNX_OK) return rc;
    if (!dweight && !dbias) return GNX_OK;               // no gradient wanted: nothing written
    if ((long)B * H * W > 0 && !workspace) return GNX_ERR_BAD_ARG;
    return hexk_weight_grad(x, dy, GridKD{{dweight}}, dbias, workspace, GridTaps{B, H, W, kh, kw}, kh * kw, I, O, accumulate,
                            stream);
}

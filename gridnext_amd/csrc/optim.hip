// Multi-tensor Adam / AdamW step for fp32 parameters: every tensor of a parameter group in one table-driven launch.
//
// Replaces the `optimizer.step()` calls of /root/reference/gridnext/training.py (:67 train_spotwise, :167-170 train_gridwise:
// torch.optim.Adam walks the group's tensors on the host).  Per element, torch's order (rounded as its multi-tensor step):
//   g  = grad + weight_decay * p              (classic L2)     |  decoupled (AdamW):  p *= 1 - lr * weight_decay ; g = grad
//   m += (g - m) * (1 - beta1)
//   v  = beta2 * v + (1 - beta2) * g * g
//   p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)          bc1 = 1 - beta1^t, bc2 = 1 - beta2^t, t = step + 1
//
// Two launches per table of up to GNX_ADAM_TABLE tensors:
//   adam_prologue_kernel  one block, one lane per tensor: increments the tensor's float32 step count ON THE DEVICE and writes
//                         lr/bc1 and sqrt(bc2), computed in double, to coef[2*i], coef[2*i + 1].  The element kernel never
//                         touches a counter, so no block reads a counter that another block of its launch writes.
//   adam_elements_kernel  one block per chunk of GNX_ADAM_CHUNK elements of one tensor.  The table (five pointers and numel per
//                         tensor, and the first chunk of every tensor) IS the kernel argument: nothing is copied to the device,
//                         nothing is staged, and the call is legal inside a stream capture.  A replay of a captured call is
//                         therefore valid only while the addresses it was captured with stand.
// Alignment: chunks are cut at multiples of GNX_ADAM_CHUNK elements from the tensor's start, so every chunk of a tensor has
// the parameter pointer's misalignment.  Up to three head elements bring p to a 16-byte boundary, the body moves 16 B per
// lane, up to three tail elements follow.  grad, m and v take 16-byte accesses when they share p's misalignment and four
// 4-byte accesses per lane otherwise (a `.grad` that is a view into a flat all-reduce buffer sits at any element offset).
// Every element goes through the one function adam_element(), built from explicitly rounded operations only (no
// contraction is left to the compiler), so its result bits do not depend on the path, the chunking or the launch's other
// tensors.  Only ordinary vector stores.  Neither kernel uses scratch: the element kernel reads the table with scalar loads,
// the prologue's per-lane `tab.step[i]` is a per-lane load from the argument segment (kernel-resource-usage: scratch 0).
#include "common.h"

#define GNX_ADAM_TABLE 64      // tensors per launch: 64 * 48 B + 65 * 4 B of table stay below the 4 KiB kernel-argument limit
#define GNX_ADAM_CHUNK 4096    // elements per block: 256 lanes x 4 vectors of 4

namespace {

struct AdamTable {
    float* p[GNX_ADAM_TABLE];
    const float* g[GNX_ADAM_TABLE];
    float* m[GNX_ADAM_TABLE];
    float* v[GNX_ADAM_TABLE];
    float* step[GNX_ADAM_TABLE];
    long numel[GNX_ADAM_TABLE];
    int first[GNX_ADAM_TABLE + 1];   // first[i] = chunks before tensor i; first[n] = grid size
    int n;
};

struct AdamHyper {
    float omb1, beta2, omb2, eps, wd, decay;   // 1 - beta1, beta2, 1 - beta2, eps, L2 factor (0 when decoupled), 1 - lr * wd (AdamW)
    int decoupled;
};

__global__ __launch_bounds__(GNX_ADAM_TABLE) void adam_prologue_kernel(const AdamTable tab, float* __restrict__ coef,
                                                                        double lr, double beta1, double beta2) {
    const int i = threadIdx.x;
    if (i >= tab.n) return;
    const float t = *tab.step[i] + 1.0f;          // float32 on the device, as torch's `step_t += 1`
    *tab.step[i] = t;
    const double bc1 = 1.0 - pow(beta1, (double)t);
    const double bc2 = 1.0 - pow(beta2, (double)t);
    coef[2 * i] = (float)(lr / bc1);
    coef[2 * i + 1] = (float)sqrt(bc2);
}

// (sqrtf, not __fsqrt_rn: HIP maps the latter to the approximate native square root; sqrtf and `/` are correctly rounded under
//  hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt.  With these the step is torch's multi-tensor step bit for bit.)
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const AdamHyper& h, float step_size,
                                             float bc2_sqrt) {
    if (h.decoupled) p = __fmul_rn(p, h.decay);
    if (h.wd != 0.f) g = __fmaf_rn(h.wd, p, g);                    // (wd = 0 when decoupled)
    m = __fmaf_rn(__fsub_rn(g, m), h.omb1, m);
    v = __fmaf_rn(h.omb2, __fmul_rn(g, g), __fmul_rn(h.beta2, v));   // torch's addcmul: value * (g * g)
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(v), bc2_sqrt), h.eps);
    p = __fmaf_rn(-step_size, __fdiv_rn(m, denom), p);
}

__device__ __forceinline__ f32x4 load4(const float* a, bool vec) {
    if (vec) return *reinterpret_cast<const f32x4*>(a);
    f32x4 r;
    r.x = a[0]; r.y = a[1]; r.z = a[2]; r.w = a[3];
    return r;
}

__device__ __forceinline__ void store4(float* a, f32x4 r, bool vec) {
    if (vec) {
        *reinterpret_cast<f32x4*>(a) = r;
    } else {
        a[0] = r.x; a[1] = r.y; a[2] = r.z; a[3] = r.w;
    }
}

__global__ __launch_bounds__(256) void adam_elements_kernel(const AdamTable tab, const float* __restrict__ coef,
                                                            const AdamHyper h) {
    // the tensor of this block: the last i with first[i] <= blockIdx.x (tensors without elements own no chunk)
    int lo = 0, hi = tab.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab.first[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
    }
    const int ti = lo;
    const long off = (long)((int)blockIdx.x - tab.first[ti]) * GNX_ADAM_CHUNK;
    const long rest = tab.numel[ti] - off;
    const int len = rest < GNX_ADAM_CHUNK ? (int)rest : GNX_ADAM_CHUNK;
    float* p = tab.p[ti] + off;
    const float* g = tab.g[ti] + off;
    float* m = tab.m[ti] + off;
    float* v = tab.v[ti] + off;
    const float step_size = coef[2 * ti], bc2_sqrt = coef[2 * ti + 1];

    const unsigned mis = (unsigned)((uintptr_t)p & 15u);
    int head = (int)(((16u - mis) & 15u) >> 2);                     // elements in front of p's first 16-byte boundary
    if (head > len) head = len;
    const int nvec = (len - head) >> 2;
    const int tail0 = head + 4 * nvec;                              // tail elements: [tail0, len)
    const bool gv = ((uintptr_t)g & 15u) == mis, mv = ((uintptr_t)m & 15u) == mis, vv = ((uintptr_t)v & 15u) == mis;

    for (int i = threadIdx.x; i < nvec; i += 256) {
        const int e = head + 4 * i;
        f32x4 P = *reinterpret_cast<const f32x4*>(p + e);
        const f32x4 G = load4(g + e, gv);
        f32x4 M = load4(m + e, mv), V = load4(v + e, vv);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = P[j], mj = M[j], vj = V[j];
            adam_element(pj, G[j], mj, vj, h, step_size, bc2_sqrt);
            P[j] = pj; M[j] = mj; V[j] = vj;
        }
        *reinterpret_cast<f32x4*>(p + e) = P;
        store4(m + e, M, mv);
        store4(v + e, V, vv);
    }
    // head: lanes 0..head-1 of the first wave; tail: lanes 0..2 of the second wave
    int e = -1;
    if ((int)threadIdx.x < head) e = threadIdx.x;
    else if (threadIdx.x >= 64 && tail0 + (int)threadIdx.x - 64 < len) e = tail0 + (int)threadIdx.x - 64;
    if (e >= 0) {
        float P = p[e], M = m[e], V = v[e];
        adam_element(P, g[e], M, V, h, step_size, bc2_sqrt);
        p[e] = P;
        m[e] = M;
        v[e] = V;
    }
}

}  // namespace

// tensors one launch holds (a longer list is split into ceil(n / this) launch pairs by gnx_adam_step itself)
GNX_EXPORT long gnx_adam_table_tensors() { return GNX_ADAM_TABLE; }
// elements per chunk (= per block)
GNX_EXPORT long gnx_adam_chunk() { return GNX_ADAM_CHUNK; }

// One Adam (decoupled = 0) or AdamW (decoupled = 1) step over n fp32 tensors.  p, grad, m, v, step: HOST arrays of n device
// pointers (step: one float32 count per tensor, incremented on the device); numel: host array of n element counts (0 is
// legal: the count still advances); coef: 2 * n device floats of workspace.  The pointers are packed into the launches'
// kernel arguments: the host arrays are free once the call returns.  Hyperparameters by value, every call.
GNX_EXPORT int gnx_adam_step(float* const* p, const float* const* grad, float* const* m, float* const* v, float* const* step,
                             const long* numel, int n, float* coef, double lr, double beta1, double beta2, double eps,
                             double weight_decay, int decoupled, hipStream_t stream) {
    if (n < 0 || (n > 0 && (!p || !grad || !m || !v || !step || !numel || !coef))) return GNX_ERR_BAD_ARG;
    for (int i = 0; i < n; ++i) {
        if (!step[i] || numel[i] < 0) return GNX_ERR_BAD_ARG;
        if (numel[i] > 0 && (!p[i] || !grad[i] || !m[i] || !v[i])) return GNX_ERR_BAD_ARG;
        if (((uintptr_t)p[i] | (uintptr_t)grad[i] | (uintptr_t)m[i] | (uintptr_t)v[i] | (uintptr_t)step[i]) & 3u)
            return GNX_ERR_BAD_ARG;
    }
    AdamHyper h;
    h.omb1 = (float)(1.0 - beta1);
    h.beta2 = (float)beta2;
    h.omb2 = (float)(1.0 - beta2);
    h.eps = (float)eps;
    h.wd = decoupled ? 0.f : (float)weight_decay;
    h.decay = (float)(1.0 - lr * weight_decay);
    h.decoupled = (decoupled && weight_decay != 0.0) ? 1 : 0;
    for (int base = 0; base < n;) {
        AdamTable tab = {};
        int k = 0;
        long chunks = 0;
        // (a table also closes before its chunk count would pass what `first` and a grid dimension hold)
        while (base + k < n && k < GNX_ADAM_TABLE) {
            const long c = (numel[base + k] + GNX_ADAM_CHUNK - 1) / GNX_ADAM_CHUNK;
            if (c > 0x7fffffffL) return GNX_ERR_UNSUPPORTED;
            if (k > 0 && chunks + c > 0x7fffffffL) break;
            tab.p[k] = p[base + k];
            tab.g[k] = grad[base + k];
            tab.m[k] = m[base + k];
            tab.v[k] = v[base + k];
            tab.step[k] = step[base + k];
            tab.numel[k] = numel[base + k];
            tab.first[k] = (int)chunks;
            chunks += c;
            ++k;
        }
        tab.first[k] = (int)chunks;
        tab.n = k;
        adam_prologue_kernel<<<1, GNX_ADAM_TABLE, 0, stream>>>(tab, coef + 2L * base, lr, beta1, beta2);
        if (chunks > 0)
            adam_elements_kernel<<<(unsigned)chunks, 256, 0, stream>>>(tab, coef + 2L * base, h);
        base += k;
    }
    return gnx_launch_status();
}

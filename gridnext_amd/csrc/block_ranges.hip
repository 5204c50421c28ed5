// The eval layers of one dense block for two disjoint row ranges of the same block buffer, one range per stream: host code over
// the launchers of conv1x1.hip and conv3x3.hip, no kernel of its own (include/gridnext_hip.h: gnx_dense_block_ranges).
//
// Every kernel of the 8 x 8 and 4 x 4 maps is persistent and holds its workgroup slots to the end of its launch, so its last,
// partial round of tiles leaves most CUs empty.  Spots are independent in eval mode: while range 0 is at a layer's conv2, range 1
// can be at its conv1, and a launch on the other stream gets CUs exactly when the first one enters that partial round.  The same
// kernels run on the same rows with the same tile boundaries as in one range, so no bit of the result changes.
#include "common.h"

#include <mutex>

namespace {

constexpr int BR_MAX_DEVICES = 64;
struct BrSide {
    hipStream_t stream;
    hipEvent_t fork, join;
    bool ready;
};
BrSide br_side[BR_MAX_DEVICES];     // one side stream and one event pair per device, created at first use and kept
std::mutex br_mutex;                // one call at a time enqueues through them: a fork's record and its wait stay a pair

// the current device's side stream (the caller holds br_mutex)
int br_side_stream(BrSide** out) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= BR_MAX_DEVICES) return GNX_ERR_LAUNCH;
    BrSide& s = br_side[dev];
    if (!s.ready) {
        hipStream_t st = nullptr;
        hipEvent_t fork = nullptr, join = nullptr;
        // non-blocking: ordered against the caller's stream by the two events alone, whichever stream that is
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return GNX_ERR_LAUNCH;
        if (hipEventCreateWithFlags(&fork, hipEventDisableTiming) != hipSuccess) {
            (void)hipStreamDestroy(st);
            return GNX_ERR_LAUNCH;
        }
        if (hipEventCreateWithFlags(&join, hipEventDisableTiming) != hipSuccess) {
            (void)hipEventDestroy(fork);
            (void)hipStreamDestroy(st);
            return GNX_ERR_LAUNCH;
        }
        s.stream = st;
        s.fork = fork;
        s.join = join;
        s.ready = true;
    }
    *out = &s;
    return GNX_OK;
}

struct BrArgs {
    float* buf;
    long ld;
    float* bott;
    int S, mid, growth;
};

// the kernel forms of one layer over `rows` rows starting at row `r0`: conv1's GNX_C1_* code and conv2's GNX_C3_* code (the
// Winograd form where the layer has W2u and the launcher takes the shape, else the direct one); a negative GNX_ERR_* in either
void br_layer_forms(const BrArgs& a, const gnx_dense_layer_item& it, long r0, long rows, int* f1, int* f2) {
    const float* A = a.buf + r0 * a.ld;
    const float* B = a.bott + r0 * (long)a.mid;
    *f1 = gnx_conv1x1_form(A, a.ld, it.W1, B, a.mid, rows, a.mid, it.cin, it.scale1, it.shift1, 0, 0, it.scale2, it.shift2,
                           nullptr, nullptr, nullptr);
    *f2 = GNX_ERR_UNSUPPORTED;
    if (it.W2u) *f2 = gnx_conv3x3_winograd_form(B, a.mid, it.W2u, A + it.cin, a.ld, rows, a.growth, a.mid, a.S, nullptr);
    if (*f2 == GNX_ERR_UNSUPPORTED)
        *f2 = gnx_conv3x3_form(B, a.mid, it.W2r, A + it.cin, a.ld, rows, a.growth, a.mid, a.S, nullptr, nullptr, nullptr);
}

// What a call does, decided in ONE place: gnx_dense_block_ranges acts on it, gnx_dense_block_ranges_form returns it.
// A GNX_BR_* code, or the GNX_ERR_* the call returns before it launches anything.
int br_plan(const BrArgs& a, long M, long M0, const gnx_dense_layer_item* items, int n, hipStream_t stream) {
    if (!a.buf || !a.bott || !items || n < 0 || M < 0 || M0 < 0 || M0 > M || a.S <= 0 || a.mid <= 0 || a.growth <= 0 ||
        a.ld <= 0 || M % ((long)a.S * a.S) != 0)
        return GNX_ERR_BAD_ARG;
    bool wino = false;
    for (int i = 0; i < n; ++i) {
        const gnx_dense_layer_item& it = items[i];
        if (!it.W1 || !it.W2r || !it.scale1 || !it.shift1 || !it.scale2 || !it.shift2 || it.cin <= 0 ||
            (long)it.cin + a.growth > a.ld)
            return GNX_ERR_BAD_ARG;
        wino = wino || it.W2u;
    }
    const long M1 = M - M0, spot = (long)a.S * a.S;
    if (M0 == 0 || M1 == 0 || n == 0) return GNX_BR_ONE;            // an empty range: nothing is launched for it
    if (M0 % 128 != 0 || M1 % 128 != 0 || M0 % spot != 0 || (wino && M0 % 256 != 0)) return GNX_BR_ONE;
    for (int i = 0; i < n; ++i) {                                   // both ranges on the kernels all M rows would run
        int w1, w2, p1, p2, q1, q2;
        br_layer_forms(a, items[i], 0, M, &w1, &w2);
        br_layer_forms(a, items[i], 0, M0, &p1, &p2);
        br_layer_forms(a, items[i], M0, M1, &q1, &q2);
        if (w1 < 0 || w2 < 0 || p1 != w1 || q1 != w1 || p2 != w2 || q2 != w2) return GNX_BR_ONE;
    }
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &status) != hipSuccess) return GNX_ERR_LAUNCH;
    return status == hipStreamCaptureStatusNone ? GNX_BR_TWO : GNX_BR_SERIAL;
}

// one layer over rows [r0, r0 + rows) on `stream`; the bottleneck rows are the range's own
int br_layer(const BrArgs& a, const gnx_dense_layer_item& it, long r0, long rows, hipStream_t stream) {
    float* A = a.buf + r0 * a.ld;
    float* B = a.bott + r0 * (long)a.mid;
    int rc = gnx_conv1x1_bnrelu_act(A, a.ld, it.W1, B, a.mid, rows, a.mid, it.cin, it.scale1, it.shift1, it.scale2, it.shift2,
                                    stream);
    if (rc != GNX_OK) return rc;
    if (it.W2u) {
        rc = gnx_conv3x3_winograd(B, a.mid, it.W2u, A + it.cin, a.ld, rows, a.growth, a.mid, a.S, stream);
        if (rc != GNX_ERR_UNSUPPORTED) return rc;
    }
    return gnx_conv3x3_bnrelu(B, a.mid, it.W2r, A + it.cin, a.ld, rows, a.growth, a.mid, a.S, nullptr, nullptr, stream);
}

}  // namespace

GNX_EXPORT int gnx_dense_block_ranges_form(const float* buf, long ld, const float* bott, long M, long M0, int S, int mid,
                                           int growth, const void* layers, int n_layers, hipStream_t stream) {
    const BrArgs a = {const_cast<float*>(buf), ld, const_cast<float*>(bott), S, mid, growth};
    return br_plan(a, M, M0, static_cast<const gnx_dense_layer_item*>(layers), n_layers, stream);
}

GNX_EXPORT int gnx_dense_block_ranges(float* buf, long ld, float* bott, long M, long M0, int S, int mid, int growth,
                                      const void* layers, int n_layers, hipStream_t stream) {
    const BrArgs a = {buf, ld, bott, S, mid, growth};
    const gnx_dense_layer_item* items = static_cast<const gnx_dense_layer_item*>(layers);
    std::lock_guard<std::mutex> lock(br_mutex);
    const int plan = br_plan(a, M, M0, items, n_layers, stream);
    if (plan < 0) return plan;
    if (M == 0) return GNX_OK;
    if (plan == GNX_BR_ONE || plan == GNX_BR_SERIAL) {
        const long starts[3] = {0, plan == GNX_BR_ONE ? M : M0, M};
        for (int r = 0; r < 2; ++r)
            for (int i = 0; i < n_layers && starts[r + 1] > starts[r]; ++i) {
                const int rc = br_layer(a, items[i], starts[r], starts[r + 1] - starts[r], stream);
                if (rc != GNX_OK) return rc;
            }
        return GNX_OK;
    }
    BrSide* side = nullptr;
    int rc = br_side_stream(&side);
    if (rc != GNX_OK) return rc;
    // fork: the side stream starts after everything the caller's stream holds so far (the block's input columns)
    if (hipEventRecord(side->fork, stream) != hipSuccess || hipStreamWaitEvent(side->stream, side->fork, 0) != hipSuccess)
        return GNX_ERR_LAUNCH;
    for (int i = 0; i < n_layers && rc == GNX_OK; ++i) {
        rc = br_layer(a, items[i], 0, M0, stream);
        if (rc == GNX_OK) rc = br_layer(a, items[i], M0, M - M0, side->stream);
    }
    // join, also after an error (it launches nothing): the caller's stream goes on after whatever the side stream was given
    if (hipEventRecord(side->join, side->stream) != hipSuccess || hipStreamWaitEvent(stream, side->join, 0) != hipSuccess)
        return rc != GNX_OK ? rc : GNX_ERR_LAUNCH;
    return rc;
}

// Linear power-of-two weight quantizers lin / lin+.
// Reference: LinearPowerOfTwoQuantizer.forward / LinearPowerOfTwoPlusQuantizer.forward,
// utils/quantizers.py:59-136, with quantize_per_filter (:8-16).  Per input channel c
// (dim 1 of the 4-D weight [d0, d1, d2, d3]):
//   delta = (max_c - min_c) / (2^bits - 1);  q = qpf(w, delta) / delta
//   num_iters x: delta = 2 ** round(log2(sum(q w) / sum(q q)))   (lin+: of sqrt(8/9) x that)
//                q = qpf(w, delta) / delta
//   out = q * delta
// qpf(x, d) = d * clamp(round(x / d), -(2^(bits-1) - 1), 2^(bits-1) - 1), all fp32.
//
// One workgroup per channel.  A channel's d0*d2*d3 elements (<= 576 for ResNet, <= 960
// for MobileNet's pointwise convs) stay in VGPRs across every pass: one HBM read and one
// write per element, the rest is ALU plus two block reductions per iteration.  The sums
// are fp64 in a fixed order (deterministic; the reference sums fp32 in an unspecified
// order and only the power-of-two snap consumes them).  The snap is torch's own fp32
// round(log2) decision, tabulated per binade (po2q_log2_table.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "po2q_internal.h"
#include "po2q_lin_dev.h"

namespace po2q {

namespace {

// NTH threads per channel; REG: the channel's elements fit in VGPRs (<= 16 NTH)
template <int NTH, bool REG>
__global__ __launch_bounds__(NTH) void quantize_lin_kernel(const float* __restrict__ w, float* __restrict__ out,
                                                                   int d0, int d1, int rs, int bits, int num_iters,
                                                                   int plus) {
    const int c = blockIdx.x;
    const int m = d0 * rs;
    const float lim = (float)((1 << (bits - 1)) - 1);
    auto addr = [&](int i) { return ((int64_t)(i / rs) * d1 + c) * rs + i % rs; };
    float xr[REG ? kLinMaxPer : 1];
    const float delta = lin_channel_delta<NTH, REG>(w, d0, d1, rs, c, bits, num_iters, plus, xr);
    // ---- out = (qpf(w, delta) / delta) * delta
    if constexpr (REG) {
#pragma unroll
        for (int u = 0; u < kLinMaxPer; ++u) {
            const int i = threadIdx.x + u * NTH;
            if (i < m) out[addr(i)] = lin_value(xr[u], delta, lim);
        }
    } else {
        for (int i = threadIdx.x; i < m; i += NTH) {
            const int64_t a = addr(i);
            out[a] = lin_value(w[a], delta, lim);
        }
    }
}

// Phase 1 of the lin conv modes' weight pack: the step of every (tensor, input channel) of a batch
// of weight tensors in one launch, one workgroup per channel, delta[c] into the tensor's workspace.
// blk0 is the prefix table that maps blockIdx.x to its job (block b serves channel b - blk0 of the
// last job with blk0 <= b).  Same body as quantize_lin_kernel: the same bits.
struct LinJob {
    const float* w;
    float* delta;
    int d0, d1, rs, bits, num_iters, plus, blk0, pad;
};
constexpr int kLinBatch = 84;  // 84 x 48-byte jobs + the count: under the 4 KB kernel-argument limit
struct LinBatch {
    LinJob job[kLinBatch];
    int n;
};
static_assert(sizeof(LinBatch) <= 4096, "lin_delta_batch_kernel's arguments must fit the 4 KB kernel-argument limit");

template <int NTH, bool REG>
__global__ __launch_bounds__(NTH) void lin_delta_batch_kernel(LinBatch B) {
    int j = 0;
    while (j + 1 < B.n && (int)blockIdx.x >= B.job[j + 1].blk0) ++j;  // block-uniform
    const LinJob& J = B.job[j];
    const int c = (int)blockIdx.x - J.blk0;
    if (c >= J.d1) return;  // block-uniform (never taken: the grid is the sum of the d1)
    float xr[REG ? kLinMaxPer : 1];
    const float delta = lin_channel_delta<NTH, REG>(J.w, J.d0, J.d1, J.rs, c, J.bits, J.num_iters, J.plus, xr);
    if (threadIdx.x == 0) J.delta[c] = delta;
}

// thread-count class of a channel of m elements: launch_quantize_lin's choice, so the fixed-order
// sums (and with them the step) are the plain quantizer's
int lin_class(int m) { return m <= 256 * kLinMaxPer ? 0 : (m <= 1024 * kLinMaxPer ? 1 : 2); }

}  // namespace

hipError_t launch_lin_delta_batch(int n, const LinReq* reqs, hipStream_t s) {
    for (int cls = 0; cls < 3; ++cls) {
        LinBatch B;
        B.n = 0;
        int blocks = 0;
        auto flush = [&]() -> hipError_t {
            if (B.n == 0) return hipSuccess;
            if (cls == 0)
                hipLaunchKernelGGL((lin_delta_batch_kernel<256, true>), dim3((unsigned)blocks), dim3(256), 0, s, B);
            else if (cls == 1)
                hipLaunchKernelGGL((lin_delta_batch_kernel<1024, true>), dim3((unsigned)blocks), dim3(1024), 0, s, B);
            else
                hipLaunchKernelGGL((lin_delta_batch_kernel<1024, false>), dim3((unsigned)blocks), dim3(1024), 0, s, B);
            B.n = 0;
            blocks = 0;
            return hipGetLastError();
        };
        for (int i = 0; i < n; ++i) {
            const LinReq& r = reqs[i];
            if (lin_class(r.d0 * r.rs) != cls) continue;
            B.job[B.n++] = LinJob{r.w, r.delta, r.d0, r.d1, r.rs, r.bits, r.num_iters, r.plus, blocks, 0};
            blocks += r.d1;
            if (B.n == kLinBatch) {
                const hipError_t e = flush();
                if (e != hipSuccess) return e;
            }
        }
        const hipError_t e = flush();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_quantize_lin(const float* w, float* out, int d0, int d1, int rs, int bits, int num_iters, int plus,
                               hipStream_t s) {
    const int m = d0 * rs;  // elements per channel
#define PO2Q_LIN(nth, reg)                                                                                    \
    hipLaunchKernelGGL((quantize_lin_kernel<nth, reg>), dim3((unsigned)d1), dim3(nth), 0, s, w, out, d0, d1, rs, \
                       bits, num_iters, plus)
    if (m <= 256 * kLinMaxPer)
        PO2Q_LIN(256, true);
    else if (m <= 1024 * kLinMaxPer)  // e.g. depthwise [960, 1, 3, 3]: one channel of 8640
        PO2Q_LIN(1024, true);
    else
        PO2Q_LIN(1024, false);
#undef PO2Q_LIN
    return hipGetLastError();
}

}  // namespace po2q

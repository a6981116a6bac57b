// Device helpers of the bf16 PO2 / PO2+ quantizer, shared by the stand-alone quantizer
// (po2q_quant_dtypes.hip) and the bf16 conv's quantize-and-pack launch (po2q_conv_b16.hip): one
// body, so the conv's Q(w) is what po2q_quantize_bf16 returns, bit for bit.  Not part of the C ABI.
//
// Reference: utils/quantizers.py:19-56 on a bf16 tensor, i.e. torch's bf16 arithmetic: every op
// computed in fp32 and rounded to bf16.  The exponent decision is a table measured from the
// reference itself (po2q_thresholds_dtypes.h), one entry per bf16 value below 1.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "po2q_thresholds_dtypes.h"

namespace po2q {

// torch's float -> bf16 conversion (c10::BFloat16 round_to_nearest_even; NaN -> 0x7fc0)
__device__ __forceinline__ uint16_t bf16_rne(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)0x7fc0u;
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ float bf16_to_f(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

// torch.sign
template <typename F>
__device__ __forceinline__ F sgn(F v) {
    return v > F(0) ? F(1) : (v < F(0) ? F(-1) : F(0));
}

__device__ __forceinline__ int clampi(int d, int lo, int hi) { return d < lo ? lo : (d > hi ? hi : d); }

// Q(w) of one bf16 weight wb for the tensor's scale sb = max|w| (bf16 bit patterns); mode 0 po2,
// 1 po2+ (the table row); [lo, hi] the exponent clamp window.
__device__ __forceinline__ uint16_t quant_bf16(uint16_t wb, uint16_t sb, int mode, int lo, int hi) {
    const float w = bf16_to_f(wb), scale = bf16_to_f(sb);
    const uint16_t ab = bf16_rne(w / scale);  // bf16 division: fp32 then round (:24)
    const uint32_t b = ab & 0x7fffu;           // |.| (:25)
    if (b > 0x7f80u) return (uint16_t)0x7fc0u;  // NaN
    int d;
    if (b == 0u) {
        d = lo;
    } else if (b < 0x3f80u) {
        const int k = (b >= 0x0080u) ? (int)(b >> 7) - 127 : (31 - (int)__clz(b)) - 133;
        d = k + (int)po2q_bf16_dec[mode][b] - 1;
    } else if (b == 0x3f80u) {
        d = 0;
    } else {
        d = hi;
    }
    const int e = clampi(d, lo, hi);
    const uint16_t lq = bf16_rne(ldexpf(1.0f, e));          // 2**q in bf16
    const uint16_t ls = bf16_rne(bf16_to_f(lq) * sgn(w));   // * sign: exact
    return bf16_rne(bf16_to_f(ls) * scale);                 // * scale: fp32 product, rounded
}

}  // namespace po2q

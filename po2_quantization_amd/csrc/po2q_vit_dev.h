// Helpers shared by the three fused fp32 transformer kernels: the attention core (po2q_mhsa.hip), LayerNorm + MLP +
// residual (po2q_ffn.hip) and LayerNorm + Linear + residual (po2q_lnlin.hip).  Not part of the C ABI.  Each file
// keeps its own work split, staging and tuning constants; what the kernels have in common is here, once.
//
// Layout.  All three run v_mfma_f32_16x16x4_f32 transposed on tiles of 16 tokens: lane = 16 g + (lane & 15), the
// lane's token is lane & 15 of the tile and its part of a [M, width] row is one dwordx4 per 16-wide tile t,
// row[16 t + 4 g .. + 3].  That is the B operand of the four k-steps k = 16 t + 4 g + r, r = 0..3 (the reduction order
// is free), and it is also how a 16x16 accumulator comes out: Y^T[16 t + 4 g + r][tok].  So a row is loaded
// (load_tokens), normalised (layer_norm), multiplied (mfma4) and stored (store_quad) in one register layout.  A
// token's values sit in the four lanes that share lane & 15: quad_sum / quad_max reduce over them.
// Only the last tile of a row can be ragged: tail_ok says the lane's dwordx4 of it is inside the row
// (16 (T - 1) + 4 g < width; width % 4 == 0 keeps every dwordx4 whole).  What lies outside reads as zeros.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>

namespace po2q {

// ------------------------------------------------------------------------------------------ host --
template <int N, class F>
hipError_t call_with_tiles(F& fn) {
    return fn(std::integral_constant<int, N>());
}

template <class F, int... I>
hipError_t dispatch_tiles(int n, F& fn, std::integer_sequence<int, I...>) {
    using Fn = hipError_t (*)(F&);
    static constexpr Fn table[] = {&call_with_tiles<I + 1, F>...};
    return table[n - 1](fn);
}

// fn(std::integral_constant<int, n>()) for a runtime tile count 1 <= n <= Max: the kernels are templates of it
template <int Max, class F>
hipError_t dispatch_tiles(int n, F fn) {
    return dispatch_tiles(n, fn, std::make_integer_sequence<int, Max>());
}

// One launch of 256-thread blocks.  A grid that does not fit is an error; more than 64 KB of LDS is asked for first.
template <class K, class... Args>
hipError_t launch_blocks(K kern, int64_t grid_x, int64_t grid_y, size_t lds_bytes, hipStream_t s, Args... args) {
    if (grid_x > INT32_MAX || grid_y > 65535) return hipErrorInvalidConfiguration;
    if (lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)grid_x, (unsigned)grid_y), dim3(256), lds_bytes, s, args...);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------- device --
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr float kLog2e = 1.44269504088896341f;

__device__ __forceinline__ f32x4 ld4(const float* p, bool ok) {
    return ok ? *reinterpret_cast<const f32x4*>(p) : f32x4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ float quad_sum(float v) {  // over the four lanes that share lane & 15
    v += __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}

__device__ __forceinline__ float quad_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16));
    return fmaxf(v, __shfl_xor(v, 32));
}

// acc += A B over the four k-steps of one dwordx4 pair
__device__ __forceinline__ void mfma4(f32x4& acc, f32x4 a4, f32x4 b4) {
#pragma unroll
    for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[r], b4[r], acc, 0, 0, 0);
}

// xv[t] = x[tok][16 t + 4 g .. + 3], zeros past width and for a token >= M
template <int T>
__device__ __forceinline__ void load_tokens(f32x4 (&xv)[T], const float* x, int M, int width, int64_t tok, int g,
                                            bool tail_ok) {
    const float* xr = x + (size_t)tok * width + 4 * g;
#pragma unroll
    for (int t = 0; t < T; ++t) xv[t] = ld4(xr + 16 * t, tok < M && (t < T - 1 || tail_ok));
}

// xv <- LN(xv) in place, zeros past width kept (a token >= M becomes ln_b: finite, and never stored).  The mean and
// then the centred variance take two lane exchanges each; the statistics divide by width.
template <int T>
__device__ __forceinline__ void layer_norm(f32x4 (&xv)[T], const float* ln_w, const float* ln_b, int width, float eps,
                                           int g, bool tail_ok) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t) s += (xv[t][0] + xv[t][1]) + (xv[t][2] + xv[t][3]);
    const float mean = quad_sum(s) / (float)width;
    float ss = 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float d = (t < T - 1 || tail_ok) ? xv[t][r] - mean : 0.f;
            xv[t][r] = d;
            ss = fmaf(d, d, ss);
        }
    }
    const float rstd = rsqrtf(quad_sum(ss) / (float)width + eps);
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const bool ok = t < T - 1 || tail_ok;  // past width: d = 0, w = b = 0
        const f32x4 w = ld4(ln_w + 16 * t + 4 * g, ok), b = ld4(ln_b + 16 * t + 4 * g, ok);
#pragma unroll
        for (int r = 0; r < 4; ++r) xv[t][r] = fmaf(xv[t][r] * rstd, w[r], b[r]);
    }
}

// out[tok][col .. + 3] = (y + bias[col .. + 3]) + residual[tok][col .. + 3], y = Y^T[col .. + 3][tok]; col = 16 t + 4 g.
// bias and residual (an [M, width] tensor) may be null.
__device__ __forceinline__ void store_quad(float* out, f32x4 y, int64_t tok, int M, int col, int width,
                                           const float* bias, const float* residual) {
    if (tok < M && col < width) {
        if (bias) y += *reinterpret_cast<const f32x4*>(bias + col);
        const size_t at = (size_t)tok * width + col;
        if (residual) y += *reinterpret_cast<const f32x4*>(residual + at);
        *reinterpret_cast<f32x4*>(out + at) = y;
    }
}

}  // namespace po2q

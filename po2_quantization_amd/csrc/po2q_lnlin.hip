// Fused fp32 LayerNorm + Linear + residual (po2q_ln_linear_f32):
//     out[m, :] = [residual[m, :] +] (LN(x[m, :]) or x[m, :]) W^T [+ bias]
// the two halves of Attention in models/mobile_vit.py around the attention core: to_qkv(norm(x)) (LN, no bias, no
// residual) and x + to_out(core) (no LN, bias, residual), each in one launch.  x [M, in_dim]; W [out_dim, in_dim] as
// nn.Linear.weight stores it; out, residual [M, out_dim].  LayerNorm, bias and residual are each optional.
//
// v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation), transposed as in po2q_ffn.hip, on a tile of 16
// tokens and a tile of 16 outputs (g = lane >> 4, TK = ceil(in_dim / 16) in-tiles):
//   * Y^T[16 out x 16 tok] = W[out tile, :] X^T: A = W[out = lane & 15][k], B = X[tok = lane & 15][k]; k-step (t, r)
//     takes k = 16 t + 4 g + r, so the lane's part of its token is x[tok][16 t + 4 g .. + 3], one dwordx4 per
//     in-tile, and its part of W is W[out][16 t + 4 g .. + 3].
//   * the accumulator Y^T[16 ot + 4 g + r][tok], r = 0..3, is one dwordx4 of out[tok][16 ot + 4 g .. + 3]; bias and
//     residual are read in that layout.
//   * LayerNorm in registers: a token's values sit in the four lanes that share lane & 15; the mean and then the
//     centred variance take two lane exchanges each (xor 16, xor 32).  The statistics divide by in_dim.
//   * partial tiles (in_dim or out_dim no multiple of 16, tokens >= M) run on zero operands; tokens >= M and
//     outputs >= out_dim are not stored.  in_dim % 4 == 0 and out_dim % 4 == 0 keep every dwordx4 whole.
// Work split (the weights are small: 55 KB at most in the model):
//   weight resident (lnlin_resident_kernel, many tokens)  a block of 4 waves stages its rows of W into LDS once,
//       with coalesced dwordx4 loads, and keeps them; after that one barrier the waves never meet again.  Each wave
//       grid-strides over 16-token tiles: it normalises the tile, fetches its next tile's x, runs the out-tiles in
//       groups of kGroup against the resident rows (one ds_read_b128 per 4 MFMAs) and stores.  The LDS row pitch is
//       an odd multiple of 4 floats (in_dim + 4, or in_dim if it is one), so the 16 lanes of a ds_read_b128 (rows
//       lane & 15, same g) cover the 64 banks once.  Rows that do not fit kLdsBytes are split over gridDim.y in
//       chunks of the largest multiple of 16 rows that fits; each chunk's blocks normalise the tokens again.
//   out split (lnlin_split_kernel, few tokens)  a block is ONE token tile; its 4 waves take the out-tiles
//       ot = wave (mod 4) with the W operands straight from global memory / L2.  No LDS, no barrier; all four waves
//       normalise the same 16 tokens.
#include <utility>

#include "po2q.h"
#include "po2q_internal.h"

namespace po2q {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxTK = PO2Q_LNLIN_MAX_IN / 16;  // in-tiles of the widest supported in_dim
constexpr int kGroup = 4;                       // out-tiles a wave runs at once: kGroup accumulators, one x operand
constexpr int kLdsBytes = 64 * 1024;            // resident rows per block: the model's 57 KB fit, two blocks share a CU
constexpr int kGridCap = 512;                   // resident blocks in x: two per CU on 256 CUs
// PO2Q_LNLIN_AUTO: the out-split kernel up to this many tokens.  LN + to_qkv, resident / out split in us on an MI355X:
// 8.4 / 7.0 at 8,192 x 96 -> 96, 8.9 / 11.8 at 16,384 (profiles/lnlin_ab_sweep.jsonl); the same side wins at 120 and 144.
constexpr int kSplitMaxM = 8192;

constexpr int w_pitch(int in_dim) { return (in_dim / 4) % 2 ? in_dim : in_dim + 4; }

__device__ __forceinline__ f32x4 ld4(const float* p, bool ok) {
    return ok ? *reinterpret_cast<const f32x4*>(p) : f32x4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ float quad_sum(float v) {  // over the four lanes that share lane & 15
    v += __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}

// xv[t] = x[tok][16 t + 4 g .. + 3], zeros past in_dim and for a token >= M.  Only the last in-tile can be ragged
// (tail_ok: the lane's part of it is inside in_dim).
template <int TK>
__device__ __forceinline__ void load_x(f32x4 (&xv)[TK], const LnLinArgs& a, int64_t tok, int g, bool tail_ok) {
    const float* xr = a.x + (size_t)tok * a.in_dim + 4 * g;
#pragma unroll
    for (int t = 0; t < TK; ++t) xv[t] = ld4(xr + 16 * t, tok < a.M && (t < TK - 1 || tail_ok));
}

// xv <- LN(xv) in place, zeros past in_dim kept (a token >= M becomes ln_b: finite, and never stored)
template <int TK>
__device__ __forceinline__ void layer_norm(f32x4 (&xv)[TK], const LnLinArgs& a, int g, bool tail_ok) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < TK; ++t) s += (xv[t][0] + xv[t][1]) + (xv[t][2] + xv[t][3]);
    const float mean = quad_sum(s) / (float)a.in_dim;
    float ss = 0.f;
#pragma unroll
    for (int t = 0; t < TK; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float d = (t < TK - 1 || tail_ok) ? xv[t][r] - mean : 0.f;
            xv[t][r] = d;
            ss = fmaf(d, d, ss);
        }
    }
    const float rstd = rsqrtf(quad_sum(ss) / (float)a.in_dim + a.eps);
#pragma unroll
    for (int t = 0; t < TK; ++t) {
        const bool ok = t < TK - 1 || tail_ok;  // past in_dim: d = 0, w = b = 0
        const f32x4 w = ld4(a.ln_w + 16 * t + 4 * g, ok), b = ld4(a.ln_b + 16 * t + 4 * g, ok);
#pragma unroll
        for (int r = 0; r < 4; ++r) xv[t][r] = fmaf(xv[t][r] * rstd, w[r], b[r]);
    }
}

// out[tok][o0 .. + 3] = residual + (y + bias), y = Y^T[o0 .. + 3][tok]; o0 = 16 ot + 4 g
__device__ __forceinline__ void store_quad(const LnLinArgs& a, f32x4 y, int64_t tok, int o0) {
    if (tok < a.M && o0 < a.out_dim) {
        if (a.bias) y += *reinterpret_cast<const f32x4*>(a.bias + o0);
        const size_t at = (size_t)tok * a.out_dim + o0;
        if (a.residual) y += *reinterpret_cast<const f32x4*>(a.residual + at);
        *reinterpret_cast<f32x4*>(a.out + at) = y;
    }
}

// N <= kGroup out-tiles from ot0 on against one token tile.  wl: the lane's LDS address of chunk row lane & 15,
// column 4 g; row0: the chunk's first output.
template <int TK, int N>
__device__ __forceinline__ void out_group(const f32x4 (&xv)[TK], const LnLinArgs& a, const float* wl, int pitch,
                                          int ot0, int row0, int64_t tok, int g, bool tail_ok) {
    f32x4 acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TK; ++t) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            // the ragged in-tile's columns past in_dim are not staged: zero operands there
            const f32x4 w = ld4(wl + (size_t)16 * (ot0 + j) * pitch + 16 * t, t < TK - 1 || tail_ok);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[r], xv[t][r], acc[j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) store_quad(a, acc[j], tok, row0 + 16 * (ot0 + j) + 4 * g);
}

template <int TK>
__global__ __launch_bounds__(256) void lnlin_resident_kernel(const LnLinArgs a, const int chunk_rows) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // the chunk's rows of W, 16-row padded, at `pitch`
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
    const int pitch = w_pitch(a.in_dim), kq = a.in_dim >> 2;  // dwordx4 per row
    const int row0 = blockIdx.y * chunk_rows;
    const int rows = min(chunk_rows, a.out_dim - row0), n_ot = (rows + 15) >> 4;
    const bool tail_ok = 16 * (TK - 1) + 4 * g < a.in_dim;

    const int64_t ntiles = ((int64_t)a.M + 15) >> 4, stride = (int64_t)gridDim.x * 4;
    int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    f32x4 cur[TK], nxt[TK];
    load_x<TK>(cur, a, tile * 16 + l15, g, tail_ok);

    // rows past out_dim in the last out-tile are staged as zeros
    for (int i = threadIdx.x; i < 16 * n_ot * kq; i += 256) {
        const int r = i / kq, q = i - r * kq;
        *reinterpret_cast<f32x4*>(lds + r * pitch + 4 * q) =
            ld4(a.w + (size_t)(row0 + r) * a.in_dim + 4 * q, r < rows);
    }
    __syncthreads();  // the only barrier: the rows stay for the block's lifetime

    const float* wl = lds + l15 * pitch + 4 * g;
    for (; tile < ntiles; tile += stride) {
        if (a.ln_w) layer_norm<TK>(cur, a, g, tail_ok);
        load_x<TK>(nxt, a, (tile + stride) * 16 + l15, g, tail_ok);  // past the last tile: tokens >= M, no load
        const int64_t tok = tile * 16 + l15;
        int ot0 = 0;
        for (; ot0 + kGroup <= n_ot; ot0 += kGroup)
            out_group<TK, kGroup>(cur, a, wl, pitch, ot0, row0, tok, g, tail_ok);
        switch (n_ot - ot0) {
            case 1: out_group<TK, 1>(cur, a, wl, pitch, ot0, row0, tok, g, tail_ok); break;
            case 2: out_group<TK, 2>(cur, a, wl, pitch, ot0, row0, tok, g, tail_ok); break;
            case 3: out_group<TK, 3>(cur, a, wl, pitch, ot0, row0, tok, g, tail_ok); break;
            default: break;
        }
#pragma unroll
        for (int t = 0; t < TK; ++t) cur[t] = nxt[t];
    }
}

template <int TK>
__global__ __launch_bounds__(256) void lnlin_split_kernel(const LnLinArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
    const int n_ot = (a.out_dim + 15) >> 4;
    const bool tail_ok = 16 * (TK - 1) + 4 * g < a.in_dim;
    const int64_t tok = (int64_t)blockIdx.x * 16 + l15;
    f32x4 xv[TK];
    load_x<TK>(xv, a, tok, g, tail_ok);
    if (a.ln_w) layer_norm<TK>(xv, a, g, tail_ok);
    for (int ot = wave; ot < n_ot; ot += 4) {
        const int o = 16 * ot + l15;  // the lane's row of W
        const float* wr = a.w + (size_t)o * a.in_dim + 4 * g;
        f32x4 w[TK];
#pragma unroll
        for (int t = 0; t < TK; ++t) w[t] = ld4(wr + 16 * t, o < a.out_dim && (t < TK - 1 || tail_ok));
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < TK; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][r], xv[t][r], acc, 0, 0, 0);
        store_quad(a, acc, tok, 16 * ot + 4 * g);
    }
}

template <int TK>
hipError_t launch_tk(const LnLinArgs& a, int kernel, hipStream_t s) {
    const int64_t tiles = ((int64_t)a.M + 15) / 16;
    if (kernel == PO2Q_LNLIN_OUT_SPLIT) {
        if (tiles > INT32_MAX) return hipErrorInvalidConfiguration;
        hipLaunchKernelGGL(lnlin_split_kernel<TK>, dim3((unsigned)tiles), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    const int pitch = w_pitch(a.in_dim), padded = (a.out_dim + 15) / 16 * 16;
    const int chunk_rows = std::min(padded, kLdsBytes / (pitch * (int)sizeof(float)) / 16 * 16);  // >= 16 by MAX_IN
    const int64_t chunks = (a.out_dim + chunk_rows - 1) / chunk_rows;
    if (chunks > 65535) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)std::min<int64_t>((tiles + 3) / 4, kGridCap), (unsigned)chunks);
    hipLaunchKernelGGL(lnlin_resident_kernel<TK>, grid, dim3(256), (size_t)chunk_rows * pitch * sizeof(float), s, a,
                       chunk_rows);
    return hipGetLastError();
}

template <int... I>
hipError_t launch_in_tiles(int TK, const LnLinArgs& a, int kernel, hipStream_t s, std::integer_sequence<int, I...>) {
    using Fn = hipError_t (*)(const LnLinArgs&, int, hipStream_t);
    static constexpr Fn table[] = {&launch_tk<I + 1>...};
    return table[TK - 1](a, kernel, s);
}

}  // namespace

hipError_t launch_ln_linear(const LnLinArgs& a, int kernel, hipStream_t s) {
    if (kernel == PO2Q_LNLIN_AUTO) kernel = a.M <= kSplitMaxM ? PO2Q_LNLIN_OUT_SPLIT : PO2Q_LNLIN_RESIDENT;
    return launch_in_tiles((a.in_dim + 15) / 16, a, kernel, s, std::make_integer_sequence<int, kMaxTK>());
}

}  // namespace po2q

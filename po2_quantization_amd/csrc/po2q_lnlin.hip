// Fused fp32 LayerNorm + Linear + residual (po2q_ln_linear_f32):
//     out[m, :] = [residual[m, :] +] (LN(x[m, :]) or x[m, :]) W^T [+ bias]
// the two halves of Attention in models/mobile_vit.py around the attention core: to_qkv(norm(x)) (LN, no bias, no
// residual) and x + to_out(core) (no LN, bias, residual), each in one launch.  x [M, in_dim]; W [out_dim, in_dim] as
// nn.Linear.weight stores it; out, residual [M, out_dim].  LayerNorm, bias and residual are each optional.
//
// v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation), transposed (po2q_vit_dev.h), on a tile of 16
// tokens and a tile of 16 outputs (g = lane >> 4, TK = ceil(in_dim / 16) in-tiles):
//   * Y^T[16 out x 16 tok] = W[out tile, :] X^T: A = W[out = lane & 15][k], B = X[tok = lane & 15][k]; k-step (t, r)
//     takes k = 16 t + 4 g + r, so the lane's part of its token is x[tok][16 t + 4 g .. + 3], one dwordx4 per
//     in-tile, and its part of W is W[out][16 t + 4 g .. + 3].
//   * the accumulator Y^T[16 ot + 4 g + r][tok], r = 0..3, is one dwordx4 of out[tok][16 ot + 4 g .. + 3]; bias and
//     residual are read in that layout.
//   * the row load, the in-register LayerNorm (statistics over in_dim) and the store are the shared ones of
//     po2q_vit_dev.h.
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
#include <algorithm>

#include "po2q.h"
#include "po2q_internal.h"
#include "po2q_vit_dev.h"

namespace po2q {

namespace {

constexpr int kMaxTK = PO2Q_LNLIN_MAX_IN / 16;  // in-tiles of the widest supported in_dim
constexpr int kGroup = 4;                       // out-tiles a wave runs at once: kGroup accumulators, one x operand
constexpr int kLdsBytes = 64 * 1024;            // resident rows per block: the model's 57 KB fit, two blocks share a CU
constexpr int kGridCap = 512;                   // resident blocks in x: two per CU on 256 CUs
// PO2Q_LNLIN_AUTO: the out-split kernel up to this many tokens.  LN + to_qkv, resident / out split in us on an MI355X:
// 8.4 / 7.0 at 8,192 x 96 -> 96, 8.9 / 11.8 at 16,384 (profiles/lnlin_ab_sweep.jsonl); the same side wins at 120 and 144.
constexpr int kSplitMaxM = 8192;

constexpr int w_pitch(int in_dim) { return (in_dim / 4) % 2 ? in_dim : in_dim + 4; }

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
            mfma4(acc[j], ld4(wl + (size_t)16 * (ot0 + j) * pitch + 16 * t, t < TK - 1 || tail_ok), xv[t]);
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j)
        store_quad(a.out, acc[j], tok, a.M, row0 + 16 * (ot0 + j) + 4 * g, a.out_dim, a.bias, a.residual);
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
    load_tokens<TK>(cur, a.x, a.M, a.in_dim, tile * 16 + l15, g, tail_ok);

    // rows past out_dim in the last out-tile are staged as zeros
    for (int i = threadIdx.x; i < 16 * n_ot * kq; i += 256) {
        const int r = i / kq, q = i - r * kq;
        *reinterpret_cast<f32x4*>(lds + r * pitch + 4 * q) =
            ld4(a.w + (size_t)(row0 + r) * a.in_dim + 4 * q, r < rows);
    }
    __syncthreads();  // the only barrier: the rows stay for the block's lifetime

    const float* wl = lds + l15 * pitch + 4 * g;
    for (; tile < ntiles; tile += stride) {
        if (a.ln_w) layer_norm<TK>(cur, a.ln_w, a.ln_b, a.in_dim, a.eps, g, tail_ok);
        // past the last tile: tokens >= M, no load
        load_tokens<TK>(nxt, a.x, a.M, a.in_dim, (tile + stride) * 16 + l15, g, tail_ok);
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
    load_tokens<TK>(xv, a.x, a.M, a.in_dim, tok, g, tail_ok);
    if (a.ln_w) layer_norm<TK>(xv, a.ln_w, a.ln_b, a.in_dim, a.eps, g, tail_ok);
    for (int ot = wave; ot < n_ot; ot += 4) {
        const int o = 16 * ot + l15;  // the lane's row of W
        const float* wr = a.w + (size_t)o * a.in_dim + 4 * g;
        f32x4 w[TK];
#pragma unroll
        for (int t = 0; t < TK; ++t) w[t] = ld4(wr + 16 * t, o < a.out_dim && (t < TK - 1 || tail_ok));
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < TK; ++t) mfma4(acc, w[t], xv[t]);
        store_quad(a.out, acc, tok, a.M, 16 * ot + 4 * g, a.out_dim, a.bias, a.residual);
    }
}

}  // namespace

hipError_t launch_ln_linear(const LnLinArgs& a, int kernel, hipStream_t s) {
    if (kernel == PO2Q_LNLIN_AUTO) kernel = a.M <= kSplitMaxM ? PO2Q_LNLIN_OUT_SPLIT : PO2Q_LNLIN_RESIDENT;
    const int64_t tiles = ((int64_t)a.M + 15) / 16;
    const int pitch = w_pitch(a.in_dim), padded = (a.out_dim + 15) / 16 * 16;
    const int chunk_rows = std::min(padded, kLdsBytes / (pitch * (int)sizeof(float)) / 16 * 16);  // >= 16 by MAX_IN
    return dispatch_tiles<kMaxTK>((a.in_dim + 15) / 16, [&](auto in_tiles) {
        constexpr int TK = decltype(in_tiles)::value;
        if (kernel == PO2Q_LNLIN_OUT_SPLIT) return launch_blocks(lnlin_split_kernel<TK>, tiles, 1, 0, s, a);
        return launch_blocks(lnlin_resident_kernel<TK>, std::min<int64_t>((tiles + 3) / 4, kGridCap),
                             (a.out_dim + chunk_rows - 1) / chunk_rows, (size_t)chunk_rows * pitch * sizeof(float), s,
                             a, chunk_rows);
    });
}

}  // namespace po2q

// Fused fp32 transformer MLP (po2q_ffn_f32): out = x + W2 SiLU(W1 LN(x) + b1) + b2 per token, the FeedForward of a
// MobileViT transformer layer and the add around it (models/mobile_vit.py FeedForward, Transformer.forward) in one
// launch.  x, out [M, dim]; w1 [hidden, dim] and w2 [dim, hidden] as nn.Linear.weight stores them.  The
// [M, hidden] activations never reach memory.
//
// Everything runs on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation), transposed, on a tile of 16
// tokens and a chunk of 16 hidden units (g = lane >> 4, T = ceil(dim / 16) dim tiles):
//   * H^T[16 hid x 16 tok] = W1[chunk, :] LN(x)^T: A = W1[hid = lane & 15][k], B = LN(x)[tok = lane & 15][k].  The
//     reduction order is free, so k-step (t, r) takes k = 16 t + 4 g + r: the lane's part of its token is
//     x[tok][16 t + 4 g .. + 3], one dwordx4 per dim tile, and its part of W1 is W1[hid][16 t + 4 g .. + 3].
//   * the accumulator is the next operand.  After + b1 and SiLU the lane holds H^T[4 g + r][tok], r = 0..3: the B
//     operand of k-step r of Y^T[16 dim x 16 tok] += W2[dim tile, chunk] H^T once that k-step's A operand is
//     W2[d = lane & 15][hid = 4 g + r] -- the lane's dwordx4 W2[d][16 c + 4 g .. + 3].  The hidden tile goes from
//     one GEMM to the next in the lane's own registers: no LDS round trip, no shuffle.
//   * Y^T[16 t + 4 g + r][tok] is the layout x was loaded in: bias, residual and one dwordx4 store per dim tile.
//   * the row load, the in-register LayerNorm and the store are the shared ones of po2q_vit_dev.h.
//   * SiLU(h) = h * v_rcp_f32(1 + v_exp_f32(-h log2 e)): h -> -inf gives h * 0 = -0, h -> +inf gives h.
//   * partial tiles (dim or hidden no multiple of 16, tokens >= M) run on zero operands; tokens >= M and dims
//     >= dim are not stored.  dim % 4 == 0 and hidden % 4 == 0 keep every dwordx4 whole.
// Work split:
//   token tiles (ffn_tiles_kernel, many tokens)  a block is 4 waves, a wave owns TW = 2 token tiles (1 above
//       dim 144) with all their Y^T accumulators in registers; the block streams the hidden dimension in chunks of
//       16, staging W1[chunk, :] and W2[:, chunk] through LDS once per block, double-buffered: the next chunk is
//       fetched into registers before the current chunk's MFMAs and written to the other buffer after them, one
//       barrier per chunk.  LDS rows: W1 16 T + 4 floats, W2 20 floats -- both pitches are odd multiples of 4
//       floats, so the 16 lanes of a dwordx4 read (rows lane & 15, same g) cover the 64 banks once.
//   hidden split (ffn_split_kernel, few tokens)  a block is ONE token tile; its 4 waves take the hidden chunks
//       c = wave (mod 4) with operands straight from global memory (each weight is read once per block), the four
//       partial Y^T are summed through LDS in wave order and each wave finishes the dim tiles t = wave (mod 4).
#include "po2q.h"
#include "po2q_internal.h"
#include "po2q_vit_dev.h"

namespace po2q {

namespace {

constexpr int kMaxT = PO2Q_FFN_MAX_DIM / 16;  // dim tiles of the widest supported dim
constexpr int kP2 = 20;                       // LDS floats per W2 row (16 used)
constexpr int kSplitMaxM = 16384;             // PO2Q_FFN_AUTO: the hidden-split kernel up to this many tokens

constexpr int tiles_per_wave(int T) { return T <= 9 ? 2 : 1; }
constexpr int w1_pitch(int T) { return 16 * T + 4; }
constexpr int lds_buf_floats(int T) { return 16 * w1_pitch(T) + 16 * T * kP2; }  // one chunk: W1 rows, then W2 rows

// One chunk of 16 hidden units for the wave's TW token tiles.  w1op(t) / w2op(t) give the lane's A operands:
// W1[16 c + (lane & 15)][16 t + 4 g .. + 3] and W2[16 t + (lane & 15)][16 c + 4 g .. + 3]; b1v = b1[16 c + 4 g .. + 3].
// The k-steps of the TW token tiles are interleaved (independent accumulators back to back), so this is not mfma4:
// one tile after the other costs the TW = 2 instances 4 more VGPRs.
template <int T, int TW, class W1Op, class W2Op>
__device__ __forceinline__ void hidden_chunk(const f32x4 (&xn)[TW][T], f32x4 (&acc)[TW][T], f32x4 b1v, W1Op w1op,
                                             W2Op w2op) {
    f32x4 h[TW];
#pragma unroll
    for (int u = 0; u < TW; ++u) h[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const f32x4 w = w1op(t);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int u = 0; u < TW; ++u) h[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[r], xn[u][t][r], h[u], 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < TW; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = h[u][r] + b1v[r];
            h[u][r] = p * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-kLog2e * p));
        }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const f32x4 w = w2op(t);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int u = 0; u < TW; ++u)
                acc[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[r], h[u][r], acc[u][t], 0, 0, 0);
    }
}

template <int T, int TW>
__global__ __launch_bounds__(256) void ffn_tiles_kernel(const FfnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // 2 x [W1: 16 rows of P1 | W2: 16 T rows of kP2]
    constexpr int P1 = w1_pitch(T), W1F = 16 * P1, BUF = lds_buf_floats(T);
    constexpr int NV = 64 * T;          // dwordx4 per operand and chunk: W1 16 rows x 4 T, W2 16 T rows x 4
    constexpr int PER = (T + 1) / 2;    // dwordx4 a thread stages per chunk (2 NV / 256, rounded up)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
    const int nch = (a.hidden + 15) >> 4;
    __builtin_assume(a.x != nullptr && a.b2 != nullptr);  // checked by the C entry: store_quad branches on neither
    const bool tail_ok = 16 * (T - 1) + 4 * g < a.dim;

    f32x4 pre[PER];
    auto fetch = [&](int c) {  // chunk c's weights into registers, zeros outside [hidden, dim]
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = threadIdx.x + 256 * j;
            if (i < NV) {
                const int hid = 16 * c + i / (4 * T), k = 4 * (i % (4 * T));
                pre[j] = ld4(a.w1 + (size_t)hid * a.dim + k, hid < a.hidden && k < a.dim);
            } else {
                const int d = (i - NV) >> 2, hid = 16 * c + 4 * (i & 3);
                pre[j] = ld4(a.w2 + (size_t)d * a.hidden + hid, i < 2 * NV && d < a.dim && hid < a.hidden);
            }
        }
    };
    auto commit = [&](float* buf) {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = threadIdx.x + 256 * j;
            if (i < NV)
                *reinterpret_cast<f32x4*>(buf + (i / (4 * T)) * P1 + 4 * (i % (4 * T))) = pre[j];
            else if (i < 2 * NV)
                *reinterpret_cast<f32x4*>(buf + W1F + ((i - NV) >> 2) * kP2 + 4 * (i & 3)) = pre[j];
        }
    };

    fetch(0);
    const int64_t tok0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * TW) + l15;
    const bool active = tok0 - l15 < a.M;  // wave-uniform; an idle wave still stages and meets the barriers
    f32x4 xn[TW][T], acc[TW][T];
#pragma unroll
    for (int u = 0; u < TW; ++u) {
        if (active) {
            load_tokens<T>(xn[u], a.x, a.M, a.dim, tok0 + 16 * u, g, tail_ok);
            layer_norm<T>(xn[u], a.ln_w, a.ln_b, a.dim, a.eps, g, tail_ok);
        }
#pragma unroll
        for (int t = 0; t < T; ++t) acc[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    commit(lds);
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        float* buf = lds + (c & 1) * BUF;
        if (c + 1 < nch) fetch(c + 1);
        if (active) {
            const float* w1l = buf + l15 * P1 + 4 * g;
            const float* w2l = buf + W1F + l15 * kP2 + 4 * g;
            hidden_chunk<T, TW>(
                xn, acc, ld4(a.b1 + 16 * c + 4 * g, 16 * c + 4 * g < a.hidden),
                [&](int t) { return *reinterpret_cast<const f32x4*>(w1l + 16 * t); },
                [&](int t) { return *reinterpret_cast<const f32x4*>(w2l + 16 * t * kP2); });
        }
        if (c + 1 < nch) commit(lds + ((c + 1) & 1) * BUF);  // its last readers passed the barrier of chunk c - 1
        __syncthreads();
    }
    if (!active) return;
    const float* res = a.residual ? a.x : nullptr;
#pragma unroll
    for (int u = 0; u < TW; ++u)
#pragma unroll
        for (int t = 0; t < T; ++t) store_quad(a.out, acc[u][t], tok0 + 16 * u, a.M, 16 * t + 4 * g, a.dim, a.b2, res);
}

template <int T>
__global__ __launch_bounds__(256) void ffn_split_kernel(const FfnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // the waves' partial Y^T: [4][T][64] dwordx4
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
    const int nch = (a.hidden + 15) >> 4;
    __builtin_assume(a.x != nullptr && a.b2 != nullptr);  // checked by the C entry: store_quad branches on neither
    const bool tail_ok = 16 * (T - 1) + 4 * g < a.dim;
    const int64_t tok = (int64_t)blockIdx.x * 16 + l15;
    f32x4 xn[1][T], acc[1][T];
    load_tokens<T>(xn[0], a.x, a.M, a.dim, tok, g, tail_ok);
    layer_norm<T>(xn[0], a.ln_w, a.ln_b, a.dim, a.eps, g, tail_ok);
#pragma unroll
    for (int t = 0; t < T; ++t) acc[0][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = wave; c < nch; c += 4) {
        const int hid = 16 * c + l15, hq = 16 * c + 4 * g;  // the lane's W1 row, and its four W2 columns
        const float* w1r = a.w1 + (size_t)hid * a.dim + 4 * g;
        const float* w2r = a.w2 + (size_t)l15 * a.hidden + hq;
        hidden_chunk<T, 1>(
            xn, acc, ld4(a.b1 + hq, hq < a.hidden),
            [&](int t) { return ld4(w1r + 16 * t, hid < a.hidden && (t < T - 1 || tail_ok)); },
            [&](int t) { return ld4(w2r + (size_t)16 * t * a.hidden, 16 * t + l15 < a.dim && hq < a.hidden); });
    }
    f32x4* part = reinterpret_cast<f32x4*>(lds);
#pragma unroll
    for (int t = 0; t < T; ++t) part[(wave * T + t) * 64 + lane] = acc[0][t];
    __syncthreads();
    for (int t = wave; t < T; t += 4) {
        f32x4 y = part[t * 64 + lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) y += part[(w * T + t) * 64 + lane];
        store_quad(a.out, y, tok, a.M, 16 * t + 4 * g, a.dim, a.b2, a.residual ? a.x : nullptr);
    }
}

}  // namespace

hipError_t launch_ffn(const FfnArgs& a, int kernel, hipStream_t s) {
    if (kernel == PO2Q_FFN_AUTO) kernel = a.M <= kSplitMaxM ? PO2Q_FFN_HIDDEN_SPLIT : PO2Q_FFN_TOKEN_TILES;
    return dispatch_tiles<kMaxT>((a.dim + 15) / 16, [&](auto tiles) {
        constexpr int T = decltype(tiles)::value, TW = tiles_per_wave(T);
        if (kernel == PO2Q_FFN_HIDDEN_SPLIT)
            return launch_blocks(ffn_split_kernel<T>, ((int64_t)a.M + 15) / 16, 1, (size_t)4 * T * 64 * sizeof(f32x4),
                                 s, a);
        return launch_blocks(ffn_tiles_kernel<T, TW>, ((int64_t)a.M + 64 * TW - 1) / (64 * TW), 1,
                             2 * lds_buf_floats(T) * sizeof(float), s, a);
    });
}

}  // namespace po2q

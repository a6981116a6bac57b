// Fused fp32 multi-head self-attention core (po2q_mhsa_f32): out = softmax(scale * q k^T) v per (sequence, head)
// straight from the [S, N, 3 H D] tensor the qkv projection writes into the [S, N, H D] tensor the output
// projection reads, H = 4 heads of D = 8 (the reference's MobileViT Transformer(dim, depth, 4, 8, ...),
// models/mobile_vit.py:68-98).  No score or probability ever reaches memory.
//
// One wave = one head x one tile of 16 queries, streaming over the key tiles with a running max
// (online softmax) on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation):
//   * transposed scores.  S^T = K_tile Q^T: A = K[key = lane & 15][d = g + 4 s], B = Q[query = lane & 15][d = g + 4 s]
//     (g = lane >> 4, s = 0, 1: two MFMAs).  The lane then holds the scores of ONE query (lane & 15) against keys
//     4 g + r, r = 0..3, so max, exp and the rescale are per-lane work.
//   * the accumulator is the next operand.  For O^T += V^T P^T the B operand of k-step j is P^T[key slot g][query]:
//     the lane's own register j, if k-step j's A operand is V[key = 4 g + j][d = lane & 15] -- four MFMAs per key
//     tile, no probability goes through LDS or a shuffle.
//   * the denominator rides along.  Rows 8..15 of O^T are spare: row 8 of the V operand is 1.0, so O^T[8][query]
//     accumulates sum_j p_j in the same MFMAs (and is rescaled with the rest).
//   * the running max of a query must agree in the four lanes that share lane & 15: one quad_max (po2q_vit_dev.h,
//     two lane exchanges) per group of up to four key tiles.
//   * scale * log2(e) is folded into Q once per wave; p = v_exp_f32(s - m).  Keys >= N are set to -inf before the
//     max (p exactly 0, and every group holds a real key, so the max is finite); their K / V operands are zeros.
//     N == 1 gives p = 1.0, denominator 1.0 and out == v bit for bit.
// Work split:
//   N <= 16  a block's 4 waves are the 4 heads of one sequence; the operands come straight from global memory
//            (the block reads whole 384-byte token rows), no LDS, no barrier.
//   N > 16   a block's 4 waves are query tiles of one (sequence, head); that head's K and V are staged once into
//            LDS (rows of 12 floats: the A-operand reads of both are bank-conflict free; V's carry the 1.0 of the
//            denominator row, so the V operand is a plain LDS read) and each wave runs up to
//            kTilesPerWave query tiles against them.  More than kLdsKeys keys are staged in chunks, the waves
//            carrying their running state across chunks.
#include <algorithm>

#include "po2q_internal.h"
#include "po2q_vit_dev.h"

namespace po2q {

namespace {

constexpr int kHeads = 4, kDim = 8;
constexpr int kRow = 3 * kHeads * kDim;  // floats per token row of qkv: [q | k | v]
constexpr int kOutRow = kHeads * kDim;
constexpr int kLdsRow = 12;              // LDS floats per key (8 used): bank = 12 key + d is conflict free
constexpr int kLdsKeys = 512;            // keys per LDS chunk (K + V: 48 KiB + 16 bytes)
constexpr int kTilesPerWave = 4;         // query tiles a wave of the N > 16 kernel runs
constexpr int kGroup = 4;                // key tiles per running-max exchange

struct Running {
    float m;   // running max of the query's scores (log2 domain); the same in the 4 lanes of a query
    f32x4 o;   // O^T[d = 4 g + r][query]: g 0, 1 the output, g 2 r 0 the denominator
};

// One group of nt <= kGroup key tiles, first key key0 (a multiple of 16).  kop(t, s) / vop(t, j) give the lane's
// A operands of tile t: K[16 t + (lane & 15)][g + 4 s] and V'[16 t + 4 g + j][lane & 15] (V' = [v | 1 | 0..]).
template <class KOp, class VOp>
__device__ __forceinline__ void key_group(Running& st, float q0, float q1, int key0, int nt, int N, int g, KOp kop,
                                          VOp vop) {
    f32x4 sc[kGroup];
    float cmax = -INFINITY;
#pragma unroll
    for (int u = 0; u < kGroup; ++u) {
        if (u < nt) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            s = __builtin_amdgcn_mfma_f32_16x16x4f32(kop(u, 0), q0, s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_16x16x4f32(kop(u, 1), q1, s, 0, 0, 0);
            if (key0 + 16 * (u + 1) > N) {  // the ragged last tile (wave-uniform)
                const int key = key0 + 16 * u + 4 * g;
#pragma unroll
                for (int r = 0; r < 4; ++r) s[r] = key + r < N ? s[r] : -INFINITY;
            }
            cmax = fmaxf(fmaxf(cmax, fmaxf(s[0], s[1])), fmaxf(s[2], s[3]));
            sc[u] = s;
        }
    }
    const float m = fmaxf(st.m, quad_max(cmax));
    const float alpha = __builtin_amdgcn_exp2f(st.m - m);  // first group: exp2(-inf) = 0 on O^T = 0
    st.m = m;
#pragma unroll
    for (int r = 0; r < 4; ++r) st.o[r] *= alpha;
#pragma unroll
    for (int u = 0; u < kGroup; ++u) {
        if (u < nt) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                st.o = __builtin_amdgcn_mfma_f32_16x16x4f32(vop(u, j), __builtin_amdgcn_exp2f(sc[u][j] - m), st.o, 0, 0,
                                                            0);
        }
    }
}

// out[s, query, 8 h + 4 g .. + 3] = O^T[4 g .. + 3][query] / denominator, lanes g = 0, 1 of real queries
__device__ __forceinline__ void store_tile(const Running& st, float* __restrict__ out, size_t seq_row0, int query, int N,
                                           int h, int lane) {
    const float den = __shfl(st.o[0], 32 + (lane & 15));
    const int g = lane >> 4;
    if (g < 2 && query < N) {
        const f32x4 v = {st.o[0] / den, st.o[1] / den, st.o[2] / den, st.o[3] / den};  // IEEE division: exact for
                                                                                         // uniform p (N c / N = c)
        *reinterpret_cast<f32x4*>(out + (seq_row0 + query) * kOutRow + kDim * h + 4 * g) = v;
    }
}

// N <= 16: block = sequence, wave = head, one query tile, one key tile, operands from global memory
__global__ __launch_bounds__(256) void mhsa_heads_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N,
                                                         float qscale) {
    const int lane = threadIdx.x & 63, h = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
    const size_t row0 = (size_t)blockIdx.x * N;
    const float* base = qkv + row0 * kRow + kDim * h;
    float q[2], k[2], v[4];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        q[s] = l15 < N ? base[(size_t)l15 * kRow + g + 4 * s] * qscale : 0.f;
        k[s] = l15 < N ? base[(size_t)l15 * kRow + kOutRow + g + 4 * s] : 0.f;
    }
    const float fill = l15 == kDim ? 1.f : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int key = 4 * g + j;
        v[j] = l15 < kDim ? (key < N ? base[(size_t)key * kRow + 2 * kOutRow + l15] : 0.f) : fill;
    }
    Running st;
    st.m = -INFINITY;
    st.o = f32x4{0.f, 0.f, 0.f, 0.f};
    key_group(st, q[0], q[1], 0, 1, N, g, [&](int, int s) { return k[s]; }, [&](int, int j) { return v[j]; });
    store_tile(st, out, row0, l15, N, h, lane);
}

// N > 16: block = (sequence, head) x 16 query tiles, wave = up to kTilesPerWave query tiles, K / V through LDS
__global__ __launch_bounds__(256) void mhsa_tiles_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N,
                                                         float qscale, int lds_keys, int qblocks) {
    extern __shared__ float lds[];
    float* kl = lds;                                // [lds_keys][kLdsRow]: k0..k7
    float* vl = lds + (size_t)lds_keys * kLdsRow;  // [lds_keys][kLdsRow] + 4: v0..v7, 1, 0, 0, 0 -- rows 0..11 of the
    // V operand as they are; its rows 12..15 read the next key's v0..v3 (past the last key: the 4 spare floats), which
    // only reach rows 12..15 of O^T, registers of lanes g = 3 that nothing reads
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
    const int sh = blockIdx.x / qblocks;  // (sequence, head); the block's 16 query tiles: blockIdx.x % qblocks
    const int h = sh & (kHeads - 1);
    const size_t row0 = (size_t)(sh >> 2) * N;
    const float* base = qkv + row0 * kRow + kDim * h;
    const int ntiles = (N + 15) >> 4;
    const int tile0 = (blockIdx.x - sh * qblocks) * (4 * kTilesPerWave);
    const int iters = min(kTilesPerWave, (ntiles - tile0 + 3) >> 2);
    const int nchunks = (N + lds_keys - 1) / lds_keys;
    const int kofs = l15 * kLdsRow + g, vofs = 4 * g * kLdsRow + l15;

    for (int it = 0; it < iters; ++it) {
        const int tile = tile0 + 4 * it + wave;
        const bool active = tile < ntiles;  // wave-uniform
        const int query = 16 * tile + l15;
        float q0 = 0.f, q1 = 0.f;
        if (active && query < N) {
            q0 = base[(size_t)query * kRow + g] * qscale;
            q1 = base[(size_t)query * kRow + g + 4] * qscale;
        }
        Running st;
        st.m = -INFINITY;
        st.o = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < nchunks; ++c) {
            const int ckey0 = c * lds_keys;
            const int ckeys = min(lds_keys, ((N - ckey0 + 15) >> 4) << 4);  // whole tiles; keys >= N are zeros
            if (nchunks > 1 || it == 0) {  // block-uniform: a single chunk is staged once for every query tile
                __syncthreads();
                for (int i = threadIdx.x; i < 4 * ckeys; i += 256) {
                    const int key = i >> 2, part = i & 3;  // part: K lo, K hi, V lo, V hi
                    f32x4 val = {0.f, 0.f, 0.f, 0.f};
                    if (ckey0 + key < N)
                        val = *reinterpret_cast<const f32x4*>(base + (size_t)(ckey0 + key) * kRow +
                                                              kOutRow * (1 + (part >> 1)) + 4 * (part & 1));
                    *reinterpret_cast<f32x4*>((part >> 1 ? vl : kl) + key * kLdsRow + 4 * (part & 1)) = val;
                    if (part == 3) *reinterpret_cast<f32x4*>(vl + key * kLdsRow + 8) = f32x4{1.f, 0.f, 0.f, 0.f};
                }
                __syncthreads();
            }
            if (!active) continue;
            const int ctiles = ckeys >> 4;
            for (int t0 = 0; t0 < ctiles; t0 += kGroup) {
                const float* kt = kl + 16 * t0 * kLdsRow + kofs;
                const float* vt = vl + 16 * t0 * kLdsRow + vofs;
                key_group(
                    st, q0, q1, ckey0 + 16 * t0, min(kGroup, ctiles - t0), N, g,
                    [&](int u, int s) { return kt[16 * u * kLdsRow + 4 * s]; },
                    [&](int u, int j) { return vt[(16 * u + j) * kLdsRow]; });
            }
        }
        if (active) store_tile(st, out, row0, query, N, h, lane);
    }
}

}  // namespace

bool mhsa_supported(int heads, int dim_head) { return heads == kHeads && dim_head == kDim; }

hipError_t launch_mhsa(const float* qkv, float* out, int S, int N, float scale, hipStream_t s) {
    const float qscale = scale * kLog2e;  // p = 2^(qscale q.k - m)
    if (N <= 16) return launch_blocks(mhsa_heads_kernel, S, 1, 0, s, qkv, out, N, qscale);
    const int ntiles = (N + 15) / 16;
    const int lds_keys = std::min(kLdsKeys, 16 * ntiles);
    const size_t lds_bytes = ((size_t)2 * lds_keys * kLdsRow + 4) * sizeof(float);  // + 4: see the kernel's V rows
    const int qblocks = (ntiles + 4 * kTilesPerWave - 1) / (4 * kTilesPerWave);
    return launch_blocks(mhsa_tiles_kernel, (int64_t)S * kHeads * qblocks, 1, lds_bytes, s, qkv, out, N, qscale,
                         lds_keys, qblocks);
}

}  // namespace po2q

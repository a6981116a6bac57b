// bf16 quantized conv forward on single-pass bf16 MFMA (po2q_qconv2d_bf16).
//
// Reference: QuantizedConv2d.forward (models/quantized_conv.py:32-38) with every tensor bf16:
//   F.conv2d(x, quantize_fn.apply(w, bits), bias, stride, padding, dilation, groups).
//
// Why one MFMA pass is exact: a bf16 weight quantized in bf16 is Q(w) = bf16(+-2^e * max|w|),
// itself a bf16 number, and a bf16 activation already is the MFMA operand.  So
// v_mfma_f32_16x16x32_bf16 forms every product x * Q(w) exactly (8 x 8 significand bits) and
// accumulates in fp32; y = bf16_rne(acc + bias).  No scale factor, no hi/mid/lo split: one MFMA
// per k-step where the fp32 entry's bf16x3 kernels issue three, and half the bytes in and out.
// Exact while every nonzero |x| and |Q(w)| is a normal bf16 (the matrix unit may flush subnormals).
//
// groups == 1: conv_bf16x1, a tile implicit GEMM in the mould of conv_bf16x3 (po2q_conv_x3.hip):
//   one 256-thread block per (image, 16*NT output channels, TP x TQ output pixels);
//   per input-channel chunk of CC channels:
//     x halo tile  HBM bf16 NCHW -> LDS, one plane [halo pixel][CC] bf16 (x_addr of po2q_x3_dev.h);
//                  pixels outside the image and channels >= C are written as zeros;
//     weights      B fragments packed by pack_b16 into the workspace -> LDS;
//   GEMM: M = pixels (NJ groups of 16 per wave), N = output channels (NT tiles), k = (tap, channel)
//         tap-major, 32 per MFMA; padded taps read a zeroed 16-byte slot, never a real pixel.
//   Epilogue: a lane's 4 consecutive pixels of one channel -> bf16 RNE -> one 8-byte store when the
//   run lies in one output row and its address is 8-byte aligned, else 2-byte stores.
//   Staging and 2-byte elements: a row start is only 2-byte aligned when W is odd, a channel plane
//   only when H*W is odd, and a dword taking two pixels could straddle a row end.  The dword path
//   (two pixels of 8 channels per item) is therefore taken only when W is even and x is 4-byte
//   aligned: every row and plane then starts on a dword, pairs start at even columns and a pair is
//   inside the row or outside it as a whole.  Every other shape stages with 2-byte loads.
// groups == C == K, R, S <= 5: conv_dw_b16, one output per thread, fp32 FMAs in tap order, padded
//   taps skipped.
//
// Fused epilogue (po2q_qconv2d_fused_bf16): both kernels carry a template flag EPI.  The EPI = false
// instances are the kernels above, unchanged; the EPI = true instances apply, on the fp32
// accumulator and before the single rounding to bf16,
//   v = acc + bias[k];  v = v * ps[k] + pb[k];  v += residual[n, k, p, q];  y = bf16_rne(act(v)).
// ps / pb are loaded once per (nt, lane & 15) beside the bias.  The residual is read with the y
// store's own index arithmetic: one 8-byte load where the lane's 4 pixels go out as one 8-byte
// store and the residual address is 8-byte aligned too (tested per lane), else 2-byte loads under
// the guard of the 2-byte stores, so no element outside [N, K, P, Q] is read.  The activation is
// dispatched once per block (with_act).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <vector>

#include "po2q_epi.h"
#include "po2q_internal.h"
#include "po2q_quant_b16_dev.h"
#include "po2q_x3_dev.h"

namespace po2q {

namespace {

struct B16Args {
    int N, C, H, W, K, P, Q, sh, sw, ph, pw, dh, dw, R, S;
    int TP, TQ, tilesP, tilesQ, kblocks, nchunks, HH, WW, ksteps, taps;
    int w_off;    // LDS byte offset of the weight fragments
    int tap_off;  // LDS byte offset of the tap offset table
    int pair;     // dword staging (W even, x 4-byte aligned)
    int vec;      // 8-byte epilogue stores possible (TQ % 4 == 0)
};

// (a & 0xffff) | (b << 16): the low bf16 halves of a (low) and b (high) as one dword
__device__ __forceinline__ uint32_t pk_lo16(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x05040100u); }

// The fused epilogue on a lane's 4 values: v * sk + tk (when aff), + residual (when has), activation
template <int ACT>
__device__ __forceinline__ void b16_epi4(float (&v)[4], bool aff, float sk, float tk, bool has,
                                         const float (&rv)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (aff) v[i] = v[i] * sk + tk;
        if (has) v[i] += rv[i];
        v[i] = epi_act_ct<ACT>(v[i]);
    }
}

// (the largest fused instance is held to the 3 waves per SIMD its plain twin runs at)
template <int CC, int NT, int NJ, bool EPI>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(EPI && NT * NJ == 16 ? 3 : 1))) void conv_bf16x1(const uint16_t* __restrict__ x,
                                                        const uint4* __restrict__ wpk,
                                                        const uint16_t* __restrict__ bias,
                                                        uint16_t* __restrict__ y, B16Args a, B16Epi e) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int OCT = CC / 8;  // channel octets per tap
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int o = lane >> 4;
    const int npix = a.TP * a.TQ;
    const int hw_halo = a.HH * a.WW;
    const int zero_off = hw_halo * (2 * CC);  // 16 zero bytes after the halo pixels
    const int64_t HWi = (int64_t)a.H * a.W;

    int v = blockIdx.x;
    const int tiles = a.tilesP * a.tilesQ;
    const int tile = v % tiles;
    v /= tiles;
    const int kb = v % a.kblocks;
    const int n = v / a.kblocks;
    const int p0 = (tile / a.tilesQ) * a.TP, q0 = (tile % a.tilesQ) * a.TQ;
    const int h0 = p0 * a.sh - a.ph, w0 = q0 * a.sw - a.pw;

    int* tapt = reinterpret_cast<int*>(lds + a.tap_off);
    for (int t = tid; t < a.taps; t += kThreads) {
        const int r = t / a.S, s = t - r * a.S;
        tapt[t] = r * a.dh * a.WW + s * a.dw;
    }
    if (tid == 0) *reinterpret_cast<uint4*>(lds + zero_off) = make_uint4(0u, 0u, 0u, 0u);

    // halo pixel of this lane's pixel in each group (tile-linear, row-major)
    int hp0[NJ];
#pragma unroll
    for (int g = 0; g < NJ; ++g) {
        int slot = (wave * NJ + g) * 16 + (lane & 15);
        if (slot >= npix) slot = 0;
        const int pl = slot / a.TQ, ql = slot - pl * a.TQ;
        hp0[g] = pl * a.sh * a.WW + ql * a.sw;
    }

    floatx4 acc[NJ][NT];
#pragma unroll
    for (int g = 0; g < NJ; ++g)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[g][t] = floatx4{0.f, 0.f, 0.f, 0.f};

    uint4* wl = reinterpret_cast<uint4*>(lds + a.w_off);
    const int kfr = a.ksteps * NT * 64;  // weight fragments (uint4) per chunk

    for (int chunk = 0; chunk < a.nchunks; ++chunk) {
        __syncthreads();  // the previous chunk's MFMAs are done with LDS
        // ---- x halo tile of this chunk -> LDS (zeros outside the image and past C)
        const uint16_t* xn = x + ((int64_t)n * a.C + chunk * CC) * HWi;
        const int crem = a.C - chunk * CC;  // channels left from this chunk's first
        if (a.pair) {
            const int WP = a.WW / 2 + 1;  // dword columns covering the halo row from an even column
            const int wa = w0 & ~1;
            const int per_oc = a.HH * WP;
            for (int it = tid; it < OCT * per_oc; it += kThreads) {
                const int oc = it / per_oc, r = it - oc * per_oc;
                const int hh = r / WP, m = r - hh * WP;
                const int h = h0 + hh, w = wa + 2 * m;
                // w is even and W is even: the pair (w, w + 1) is inside the row or outside it as a whole
                const bool in = ((unsigned)h < (unsigned)a.H) && ((unsigned)w < (unsigned)a.W);
                const uint16_t* px = xn + (int64_t)(oc * 8) * HWi + (int64_t)h * a.W + w;
                uint32_t d[8];
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    d[j] = (in && oc * 8 + j < crem) ? *reinterpret_cast<const uint32_t*>(px + j * HWi) : 0u;
                const int ww0 = w - w0;  // halo column of the pair's first pixel (-1 .. WW)
                const int hpr = hh * a.WW;
                if ((unsigned)ww0 < (unsigned)a.WW)
                    *reinterpret_cast<uint4*>(lds + x_addr<CC>(hpr + ww0, oc)) =
                        make_uint4(pk_lo16(d[0], d[1]), pk_lo16(d[2], d[3]), pk_lo16(d[4], d[5]), pk_lo16(d[6], d[7]));
                if ((unsigned)(ww0 + 1) < (unsigned)a.WW)
                    *reinterpret_cast<uint4*>(lds + x_addr<CC>(hpr + ww0 + 1, oc)) =
                        make_uint4(pk_hi16(d[0], d[1]), pk_hi16(d[2], d[3]), pk_hi16(d[4], d[5]), pk_hi16(d[6], d[7]));
            }
        } else {
            for (int it = tid; it < OCT * hw_halo; it += kThreads) {
                const int oc = it / hw_halo, hp = it - oc * hw_halo;
                const int hh = hp / a.WW, ww = hp - hh * a.WW;
                const int h = h0 + hh, w = w0 + ww;
                const bool in = ((unsigned)h < (unsigned)a.H) && ((unsigned)w < (unsigned)a.W);
                const uint16_t* px = xn + (int64_t)(oc * 8) * HWi + (int64_t)h * a.W + w;
                uint32_t d[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) d[j] = (in && oc * 8 + j < crem) ? (uint32_t)px[j * HWi] : 0u;
                *reinterpret_cast<uint4*>(lds + x_addr<CC>(hp, oc)) =
                    make_uint4(d[0] | (d[1] << 16), d[2] | (d[3] << 16), d[4] | (d[5] << 16), d[6] | (d[7] << 16));
            }
        }
        // ---- this (k-block, chunk)'s weight fragments -> LDS
        const uint4* wc = wpk + ((int64_t)kb * a.nchunks + chunk) * kfr;
        for (int e = tid; e < kfr; e += kThreads) wl[e] = wc[e];
        __syncthreads();

        // ---- MFMAs over this chunk: k = (tap, channel), 32 per step
        for (int ks = 0; ks < a.ksteps; ++ks) {
            const int oi = ks * 4 + o;
            const int t = oi / OCT, coct = oi % OCT;
            const bool pad = t >= a.taps;
            const int toff = pad ? 0 : tapt[t];
            bf16x8 bw[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bw[nt] = __builtin_bit_cast(bf16x8, wl[(ks * NT + nt) * 64 + lane]);
#pragma unroll
            for (int g = 0; g < NJ; ++g) {
                const int ad = pad ? zero_off : x_addr<CC>(hp0[g] + toff, coct);
                const bf16x8 a0 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds + ad));
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[g][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, bw[nt], acc[g][nt], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: D[row = pixel 4*(lane>>4)+i][col = channel lane&15]
    const int64_t PQ = (int64_t)a.P * a.Q;
    if constexpr (!EPI) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int k = kb * 16 * NT + nt * 16 + (lane & 15);
            if (k >= a.K) continue;  // channels past K are not stored
            const float bk = bias ? bf16_to_f(bias[k]) : 0.0f;
            uint16_t* yk = y + ((int64_t)n * a.K + k) * PQ;
#pragma unroll
            for (int g = 0; g < NJ; ++g) {
                const int i0 = (wave * NJ + g) * 16 + 4 * o;
                if (i0 >= npix) continue;
                uint32_t r[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] = bf16_rne(acc[g][nt][i] + bk);
                const int pl = i0 / a.TQ, ql = i0 - pl * a.TQ;
                const int pp = p0 + pl, qq = q0 + ql;
                uint16_t* yp = yk + (int64_t)pp * a.Q + qq;
                if (a.vec && pp < a.P && qq + 3 < a.Q && (reinterpret_cast<uintptr_t>(yp) & 7u) == 0) {
                    *reinterpret_cast<uint2*>(yp) = make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int idx = i0 + i;
                        const int pli = idx / a.TQ, qli = idx - pli * a.TQ;
                        const int ppi = p0 + pli, qqi = q0 + qli;
                        if (idx < npix && ppi < a.P && qqi < a.Q) yk[(int64_t)ppi * a.Q + qqi] = (uint16_t)r[i];
                    }
                }
            }
        }
    } else {
        // the same stores with the fused epilogue in front of the one rounding; the activation is
        // dispatched once per block (with_act), never per value.
        // Loads are kept apart from the stores.  On gfx9 one counter (vmcnt) covers loads and stores, and
        // behind the divergent store branches the compiler can only wait for all of them: a load between
        // two stores would drain the stores first.  So the per-channel bias / scale / shift of all NT
        // tiles are loaded, and waited for, before the first store, and a tile's residual values for
        // all its NJ pixel groups are requested together (packed, two bf16 per register) and waited for
        // once: no wait is left between stores without a residual, one per tile with one.
        constexpr int kWaitVm0 = 0x0F70;  // s_waitcnt vmcnt(0) alone (expcnt 7, lgkmcnt 15: not waited)
        const bool aff = e.ps || e.pb;
        float bk[NT], sk[NT], tk[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int k = min(kb * 16 * NT + nt * 16 + (lane & 15), a.K - 1);  // lanes past K load, never store
            bk[nt] = bias ? bf16_to_f(bias[k]) : 0.0f;
            sk[nt] = e.ps ? e.ps[k] : 1.0f;
            tk[nt] = e.pb ? e.pb[k] : 0.0f;
        }
        __builtin_amdgcn_s_waitcnt(kWaitVm0);
        with_act(e.act, [&](auto act_c) {
            constexpr int ACT = decltype(act_c)::value;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int k = kb * 16 * NT + nt * 16 + (lane & 15);
                if (k >= a.K) continue;  // channels past K are not stored
                const uint16_t* rk = e.res ? e.res + ((int64_t)n * a.K + k) * PQ : nullptr;
                uint16_t* yk = y + ((int64_t)n * a.K + k) * PQ;
                // (the 8-byte load and the packed 2-byte loads land in registers of their own, OR-ed after
                // the wait: one register for both would make the compiler wait inside each branch)
                uint2 rq[NJ];
                uint32_t rp[NJ][2];
                if (rk) {
#pragma unroll
                    for (int g = 0; g < NJ; ++g) {
                        rp[g][0] = rp[g][1] = 0u;
                        rq[g] = make_uint2(0u, 0u);
                        const int i0 = (wave * NJ + g) * 16 + 4 * o;
                        if (i0 >= npix) continue;
                        const int pl = i0 / a.TQ, ql = i0 - pl * a.TQ;
                        const int pp = p0 + pl, qq = q0 + ql;
                        const int64_t off = (int64_t)pp * a.Q + qq;
                        const bool vst =
                            a.vec && pp < a.P && qq + 3 < a.Q && (reinterpret_cast<uintptr_t>(yk + off) & 7u) == 0;
                        // the residual with the store's index arithmetic: 8 bytes at once only where y
                        // goes out so and this lane's residual address is 8-byte aligned as well
                        if (vst && (reinterpret_cast<uintptr_t>(rk + off) & 7u) == 0) {
                            rq[g] = *reinterpret_cast<const uint2*>(rk + off);
                        } else {
                            uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const int idx = i0 + i;
                                const int pli = idx / a.TQ, qli = idx - pli * a.TQ;
                                const int ppi = p0 + pli, qqi = q0 + qli;
                                if (idx < npix && ppi < a.P && qqi < a.Q) d[i] = rk[(int64_t)ppi * a.Q + qqi];
                            }
                            rp[g][0] = d[0] | (d[1] << 16);
                            rp[g][1] = d[2] | (d[3] << 16);
                        }
                    }
                    __builtin_amdgcn_s_waitcnt(kWaitVm0);
                }
#pragma unroll
                for (int g = 0; g < NJ; ++g) {
                    const int i0 = (wave * NJ + g) * 16 + 4 * o;
                    if (i0 >= npix) continue;
                    float v[4], rv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = acc[g][nt][i] + bk[nt];
                    if (rk) {
                        const uint32_t d0 = rq[g].x | rp[g][0], d1 = rq[g].y | rp[g][1];
                        rv[0] = __uint_as_float(d0 << 16);
                        rv[1] = __uint_as_float(d0 & 0xffff0000u);
                        rv[2] = __uint_as_float(d1 << 16);
                        rv[3] = __uint_as_float(d1 & 0xffff0000u);
                    }
                    b16_epi4<ACT>(v, aff, sk[nt], tk[nt], rk != nullptr, rv);
                    uint32_t r[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) r[i] = bf16_rne(v[i]);  // the one rounding
                    const int pl = i0 / a.TQ, ql = i0 - pl * a.TQ;
                    const int pp = p0 + pl, qq = q0 + ql;
                    uint16_t* yp = yk + (int64_t)pp * a.Q + qq;
                    if (a.vec && pp < a.P && qq + 3 < a.Q && (reinterpret_cast<uintptr_t>(yp) & 7u) == 0) {
                        *reinterpret_cast<uint2*>(yp) = make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int idx = i0 + i;
                            const int pli = idx / a.TQ, qli = idx - pli * a.TQ;
                            const int ppi = p0 + pli, qqi = q0 + qli;
                            if (idx < npix && ppi < a.P && qqi < a.Q) yk[(int64_t)ppi * a.Q + qqi] = (uint16_t)r[i];
                        }
                    }
                }
            }
        });
    }
}

// Depthwise: one output per thread, fp32 FMAs in tap order (r, then s), padded taps skipped.
struct DwB16Args {
    int C, H, W, P, Q, R, S, sh, sw, ph, pw, dh, dw;
    int64_t total;  // N * C * P * Q
};

template <bool EPI, int ACT>
__device__ __forceinline__ void dw_b16_body(const uint16_t* __restrict__ x, const uint16_t* __restrict__ qw,
                                            const uint16_t* __restrict__ bias, uint16_t* __restrict__ y,
                                            const DwB16Args& a, const B16Epi& e) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    const int64_t PQ = (int64_t)a.P * a.Q, HW = (int64_t)a.H * a.W;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.total; i += stride) {
        const int64_t nc = i / PQ;
        const int pq = (int)(i - nc * PQ);
        const int p = pq / a.Q, q = pq - p * a.Q;
        const int c = (int)(nc % a.C);
        const uint16_t* xc = x + nc * HW;
        const uint16_t* wc = qw + (int64_t)c * a.R * a.S;
        float acc = 0.0f;
        for (int r = 0; r < a.R; ++r) {
            const int h = p * a.sh - a.ph + r * a.dh;
            if ((unsigned)h >= (unsigned)a.H) continue;
            for (int s = 0; s < a.S; ++s) {
                const int w = q * a.sw - a.pw + s * a.dw;
                if ((unsigned)w >= (unsigned)a.W) continue;
                acc = fmaf(bf16_to_f(xc[(int64_t)h * a.W + w]), bf16_to_f(wc[r * a.S + s]), acc);
            }
        }
        float v = acc + (bias ? bf16_to_f(bias[c]) : 0.0f);
        if constexpr (EPI) {
            if (e.ps || e.pb) v = v * (e.ps ? e.ps[c] : 1.0f) + (e.pb ? e.pb[c] : 0.0f);
            if (e.res) v += bf16_to_f(e.res[i]);  // laid out like y: the store's own index
            v = epi_act_ct<ACT>(v);
        }
        y[i] = bf16_rne(v);
    }
}

template <bool EPI>
__global__ __launch_bounds__(kThreads) void conv_dw_b16(const uint16_t* __restrict__ x,
                                                        const uint16_t* __restrict__ qw,
                                                        const uint16_t* __restrict__ bias,
                                                        uint16_t* __restrict__ y, DwB16Args a, B16Epi e) {
    if constexpr (EPI)
        with_act(e.act, [&](auto act_c) { dw_b16_body<true, decltype(act_c)::value>(x, qw, bias, y, a, e); });
    else
        dw_b16_body<false, 0>(x, qw, bias, y, a, e);
}

// ---- weight staging: max|w| partials, then quantize + pack ---------------------------------
// Each step is one __device__ body with two callers: the kernel of one weight tensor (b16_run) and
// the batched kernel (b16_pack_batch: blockIdx.y = weight tensor).  `block` of `nblocks` is the
// block's place among the blocks working on this tensor.
constexpr int kB16Parts = 256;  // at most one partial per thread of the pack kernel's fold

__device__ __forceinline__ void absmax_b16_body(const uint16_t* __restrict__ w, int64_t n,
                                                uint32_t* __restrict__ partial, int block, int nblocks,
                                                uint32_t* red) {
    uint32_t m = 0u;  // sign-cleared bit patterns order as NaN > inf > finite, as torch.max propagates NaN
    const int64_t stride = (int64_t)nblocks * kThreads;
    for (int64_t i = (int64_t)block * kThreads + threadIdx.x; i < n; i += stride) m = max(m, (uint32_t)(w[i] & 0x7fffu));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) partial[block] = max(max(red[0], red[1]), max(red[2], red[3]));
}

__global__ __launch_bounds__(kThreads) void absmax_b16(const uint16_t* __restrict__ w, int64_t n,
                                                       uint32_t* __restrict__ partial) {
    __shared__ uint32_t red[kThreads / 64];
    absmax_b16_body(w, n, partial, (int)blockIdx.x, (int)gridDim.x, red);
}

struct PackB16Args {
    int C, K, taps, CC, NT, ksteps, nchunks, kblocks;
    int dense;       // 1: MFMA B fragments [kb][chunk][ks][nt][lane][8]; 0: plain copy [n];
                     // 2: the row kernels' fragments [kb][tap row][ks][nt][lane][8] (3x3, C = CC: a k-step's
                     //    octets run over one tap row's 3 columns, channel-minor; po2q_conv_b16r.hip: kblocks 1,
                     //    po2q_conv_b16rk.hip: NT 1 and one k-block per 16-channel tile, C = 64 without padding)
    int64_t n;       // weight elements
    int64_t nfrag;   // dense: uint4 fragments
    int quant, mode, lo, hi;  // quant 0: the weight as given (mode none)
    int nparts;
};

__device__ __forceinline__ void pack_b16_body(const uint16_t* __restrict__ w, const uint32_t* __restrict__ partial,
                                              uint16_t* __restrict__ out, const PackB16Args& a, int block,
                                              int nblocks, uint32_t* red) {
    uint16_t sb = 0;
    if (a.quant) {  // fold the partials: the scale max|w| as a bf16
        uint32_t m = ((int)threadIdx.x < a.nparts) ? partial[threadIdx.x] : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        sb = (uint16_t)max(max(red[0], red[1]), max(red[2], red[3]));
    }
    const int64_t stride = (int64_t)nblocks * kThreads;
    if (!a.dense) {
        for (int64_t i = (int64_t)block * kThreads + threadIdx.x; i < a.n; i += stride)
            out[i] = a.quant ? quant_bf16(w[i], sb, a.mode, a.lo, a.hi) : w[i];
        return;
    }
    const int oct = a.CC / 8;
    for (int64_t e = (int64_t)block * kThreads + threadIdx.x; e < a.nfrag; e += stride) {
        const int lane = (int)(e & 63);
        int64_t r = e >> 6;
        const int nt = (int)(r % a.NT);
        r /= a.NT;
        const int ks = (int)(r % a.ksteps);
        r /= a.ksteps;
        const int chunk = (int)(r % a.nchunks);
        const int kb = (int)(r / a.nchunks);
        const int oi = ks * 4 + (lane >> 4);
        int t = oi / oct;
        const int oc = oi % oct;
        if (a.dense == 2) t = t < 3 ? chunk * 3 + t : a.taps;  // `chunk` counts the tap row here; column 3 is padding
        const int k = kb * 16 * a.NT + nt * 16 + (lane & 15);
        const int c0 = (a.dense == 2 ? 0 : chunk * a.CC) + oc * 8;
        uint32_t q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            uint16_t val = 0;  // padded taps, channels past C / K: zero
            if (t < a.taps && k < a.K && c0 + j < a.C) {
                const uint16_t wv = w[((int64_t)k * a.C + c0 + j) * a.taps + t];
                val = a.quant ? quant_bf16(wv, sb, a.mode, a.lo, a.hi) : wv;
            }
            q[j] = val;
        }
        reinterpret_cast<uint4*>(out)[e] =
            make_uint4(q[0] | (q[1] << 16), q[2] | (q[3] << 16), q[4] | (q[5] << 16), q[6] | (q[7] << 16));
    }
}

__global__ __launch_bounds__(kThreads) void pack_b16(const uint16_t* __restrict__ w,
                                                     const uint32_t* __restrict__ partial,
                                                     uint16_t* __restrict__ out, PackB16Args a) {
    __shared__ uint32_t red[kThreads / 64];
    pack_b16_body(w, partial, out, a, (int)blockIdx.x, (int)gridDim.x, red);
}

// Up to kB16Batch weight tensors in one launch of each step (blockIdx.y = tensor): the two or
// three launches per layer of a forward become 2 * ceil(n / kB16Batch) in front of it.  A job
// is what b16_run hands its own two kernels; jobs of one launch differ freely in geometry, bits,
// fsr and mode.  A mode-none job (quant 0) has no max|w| step.  Blocks past a job's own grid
// (nparts / nb, the grids of the single-tensor launches) exit at once.
struct B16PackJob {
    const uint16_t* w;  // 2-byte aligned only
    uint32_t* partial;
    uint16_t* out;
    PackB16Args a;
    int nb;  // pack blocks
};
constexpr int kB16Batch = 36;  // 36 x 104-byte jobs: 3.7 KB of kernel arguments (the limit is 4 KB)
struct B16PackBatch {
    B16PackJob job[kB16Batch];
};
static_assert(sizeof(B16PackBatch) <= 4096, "the batched bf16 pack kernels' arguments must fit the 4 KB kernel-argument limit");

__global__ __launch_bounds__(kThreads) void absmax_b16_batch(B16PackBatch B) {
    const B16PackJob& j = B.job[blockIdx.y];
    if (!j.a.quant || (int)blockIdx.x >= j.a.nparts) return;  // block-uniform
    __shared__ uint32_t red[kThreads / 64];
    absmax_b16_body(j.w, j.a.n, j.partial, (int)blockIdx.x, j.a.nparts, red);
}

__global__ __launch_bounds__(kThreads) void pack_b16_batch(B16PackBatch B) {
    const B16PackJob& j = B.job[blockIdx.y];
    if ((int)blockIdx.x >= j.nb) return;  // block-uniform
    __shared__ uint32_t red[kThreads / 64];
    pack_b16_body(j.w, j.partial, j.out, j.a, (int)blockIdx.x, j.nb, red);
}

int cdiv(int a, int b) { return (a + b - 1) / b; }

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

int b16_parts(int64_t n) { return (int)std::min<int64_t>(kB16Parts, std::max<int64_t>(1, (n + 2047) / 2048)); }

template <int CC, int NT, int NJ>
hipError_t launch_b16_t(const ConvPlan& p, const B16Args& a, const uint16_t* x, const uint16_t* packed,
                        const uint16_t* bias, uint16_t* y, const B16Epi& e, hipStream_t s) {
    // the plain entry (and a fused call with nothing to fuse) runs the EPI = false instance
    if (e.any())
        hipLaunchKernelGGL((conv_bf16x1<CC, NT, NJ, true>), dim3((unsigned)p.blocks), dim3(kThreads), p.lds_bytes, s,
                           x, reinterpret_cast<const uint4*>(packed), bias, y, a, e);
    else
        hipLaunchKernelGGL((conv_bf16x1<CC, NT, NJ, false>), dim3((unsigned)p.blocks), dim3(kThreads), p.lds_bytes, s,
                           x, reinterpret_cast<const uint4*>(packed), bias, y, a, e);
    return hipGetLastError();
}

template <int CC, int NT>
hipError_t launch_b16_nj(const ConvPlan& p, const B16Args& a, const uint16_t* x, const uint16_t* packed,
                         const uint16_t* bias, uint16_t* y, const B16Epi& e, hipStream_t s) {
    switch (p.NJ) {
        case 1: return launch_b16_t<CC, NT, 1>(p, a, x, packed, bias, y, e, s);
        case 2: return launch_b16_t<CC, NT, 2>(p, a, x, packed, bias, y, e, s);
        case 4: return launch_b16_t<CC, NT, 4>(p, a, x, packed, bias, y, e, s);
        default: return hipErrorInvalidValue;
    }
}

template <int CC>
hipError_t launch_b16_nt(const ConvPlan& p, const B16Args& a, const uint16_t* x, const uint16_t* packed,
                         const uint16_t* bias, uint16_t* y, const B16Epi& e, hipStream_t s) {
    switch (p.NT) {
        case 1: return launch_b16_nj<CC, 1>(p, a, x, packed, bias, y, e, s);
        case 2: return launch_b16_nj<CC, 2>(p, a, x, packed, bias, y, e, s);
        case 4: return launch_b16_nj<CC, 4>(p, a, x, packed, bias, y, e, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

// ------------------------------------------------------------------ planning --
// Heuristic only: the tile with the least launched-pixel waste and halo re-read that fits LDS.
int b16_plan(ConvPlan& p) {
    p.taps = p.R * p.S;
    p.vrx = 0; p.PS = 0; p.MI = 0; p.pd = 0; p.nts = 0; p.fp = 0; p.SB = 0; p.plane = 0;
    p.dma_d0 = p.dma_nck = p.dma_ni = p.dma_nw = p.dma_waves = p.dma_ov = 0;
    if (p.groups != 1) {
        if (!(p.groups == p.C && p.K == p.C)) {
            set_error("po2q: the bf16 conv takes groups == 1 or depthwise (groups == C == K) layers, got groups = " +
                      std::to_string(p.groups));
            return 2;
        }
        if (p.R > 5 || p.S > 5) {
            set_error("po2q: the bf16 depthwise conv takes kernels up to 5x5");
            return 2;
        }
        p.kind = KIND_DW_BF16;
        p.CC = p.NT = p.NJ = 1;
        p.TP = p.TQ = p.tilesP = p.tilesQ = p.kblocks = p.nchunks = 1;
        p.HH = p.WW = p.WWp = 0;
        p.steps = 0;
        p.lds_bytes = 0;
        const int64_t total = (int64_t)p.N * p.C * p.P * p.Q;
        p.blocks = std::min<int64_t>((total + kThreads - 1) / kThreads, 1 << 20);
        p.packed_floats = ((int64_t)p.K * p.taps * 2 + 3) / 4;  // Q(w) [C][R*S] bf16
        return 0;
    }
    if (b16_rowsk_plan(p)) return 0;  // opt-in (po2q_bf16_set_rowsk_kernels) and eligible
    if (b16_rows_plan(p)) return 0;   // opt-in (po2q_bf16_set_row_kernels) and eligible
    p.kind = KIND_BF16X1;
    p.CC = (p.taps == 1 && p.C > 16) ? 32 : 16;
    const int OCT = p.CC / 8;
    p.steps = cdiv(p.taps * OCT, 4);
    p.NT = p.K <= 16 ? 1 : (p.K <= 32 ? 2 : 4);
    while (p.NT > 1 && p.steps * p.NT * 1024 > 24 * 1024) p.NT >>= 1;
    p.kblocks = cdiv(p.K, 16 * p.NT);
    p.nchunks = cdiv(p.C, p.CC);
    const size_t wbytes = (size_t)p.steps * p.NT * 1024 + (size_t)p.taps * sizeof(int);
    double best = 1e30;
    bool found = false;
    ConvPlan bp = p;
    const int njs[] = {1, 2, 4};
    for (int nj : njs) {
        const int px = 64 * nj;
        for (int tq = 1; tq <= px; ++tq) {
            if (px % tq) continue;
            const int tp = px / tq;
            const int64_t HH = (int64_t)(tp - 1) * p.sh + (int64_t)(p.R - 1) * p.dh + 1;
            const int64_t WW = (int64_t)(tq - 1) * p.sw + (int64_t)(p.S - 1) * p.dw + 1;
            const int64_t xb = HH * WW * 2 * p.CC + 16;
            if (xb + (int64_t)wbytes > 64 * 1024) continue;
            const size_t lds = (size_t)xb + wbytes;
            const int tP = cdiv(p.P, tp), tQ = cdiv(p.Q, tq);
            const double waste = (double)tP * tQ * px / ((double)p.P * p.Q);
            const double halo = (double)tP * tQ * HH * WW / ((double)p.P * p.Q * p.sh * p.sw);
            const int bpc = std::min<int>(8, (int)((160 * 1024) / lds));
            double cost = waste + 0.35 * (halo - 1.0);
            if (bpc * 4 < 8) cost += 0.15 * (8 - bpc * 4) / 4.0;
            if (tq % 4) cost += 0.1;  // 2-byte epilogue stores
            // short row segments coalesce badly in both directions (measured: 16 -> 16 @224 518 us at
            // 16x16, 418 us at 8x32; 64 -> 64 @56 247 us at 8x8, 153 us at 8x32)
            if (tq < 32 && tq < p.Q) cost += 0.6 * (32 - tq) / 32.0;
            cost += 0.02 * (8.0 / nj);
            const double blocks = (double)p.N * p.kblocks * tP * tQ;
            if (blocks > INT_MAX) continue;
            if (blocks < 1024) cost += 0.5 * (1024 - blocks) / 1024;
            if (cost < best) {
                best = cost;
                found = true;
                bp = p;
                bp.NJ = nj; bp.TP = tp; bp.TQ = tq; bp.tilesP = tP; bp.tilesQ = tQ;
                bp.HH = (int)HH; bp.WW = (int)WW; bp.WWp = (int)WW;
                bp.lds_bytes = lds;
                bp.blocks = (int64_t)blocks;
            }
        }
    }
    if (!found) {
        set_error("po2q: conv tile does not fit in LDS (kernel too large)");
        return 1;
    }
    p = bp;
    // packed bf16 fragments [kb][chunk][ks][nt][lane][8] -> 4-byte words
    p.packed_floats = (int64_t)p.kblocks * p.nchunks * p.steps * p.NT * 64 * 4;
    return 0;
}

// Workspace: [max|w| partials, 256 B aligned][packed weight]
size_t b16_workspace_bytes(const ConvPlan& p) {
    return align256((size_t)kB16Parts * sizeof(uint32_t)) + align256((size_t)p.packed_floats * 4);
}

void b16_describe(const ConvPlan& p, char* buf, size_t len) {
    if (p.kind == KIND_BF16_ROWSK)
        b16_rowsk_describe(p, buf, len);
    else if (p.kind == KIND_BF16_ROWS)
        b16_rows_describe(p, buf, len);
    else if (p.kind == KIND_DW_BF16)
        snprintf(buf, len, "kind=dw_bf16 taps=%dx%d blocks=%lld", p.R, p.S, (long long)p.blocks);
    else
        snprintf(buf, len,
                 "kind=bf16x1 CC=%d NT=%d NJ=%d tile=%dx%d tiles=%dx%d halo=%dx%d chunks=%d kblocks=%d ksteps=%d "
                 "lds=%zu blocks=%lld",
                 p.CC, p.NT, p.NJ, p.TP, p.TQ, p.tilesP, p.tilesQ, p.HH, p.WW, p.nchunks, p.kblocks, p.steps,
                 p.lds_bytes, (long long)p.blocks);
}

namespace {

uint16_t* b16_packed_ptr(void* workspace) {
    return reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(workspace) + align256((size_t)kB16Parts * sizeof(uint32_t)));
}

// what the quantize + pack of one weight tensor is told: the plan's fragment layout and the window
PackB16Args b16_pack_args(const ConvPlan& p, int bits, int fsr, int mode) {
    const int64_t nw = (int64_t)p.K * p.Cg * p.taps;
    PackB16Args pa;
    pa.C = p.Cg; pa.K = p.K; pa.taps = p.taps; pa.CC = p.CC; pa.NT = p.NT; pa.ksteps = p.steps;
    pa.nchunks = p.nchunks; pa.kblocks = p.kblocks;
    const bool rows = p.kind == KIND_BF16_ROWS || p.kind == KIND_BF16_ROWSK;
    pa.dense = p.kind == KIND_BF16X1 ? 1 : (rows ? 2 : 0);
    if (pa.dense == 2) pa.nchunks = 3;  // the fragment index's chunk field is the tap row
    if (p.kind == KIND_BF16_ROWSK) {    // [channel tile][tap row][k-step][lane][8]: the k-block field is the tile
        pa.NT = 1;
        pa.kblocks = p.NT;
    }
    pa.n = nw;
    pa.nfrag = pa.dense ? p.packed_floats / 4 : 0;
    pa.quant = mode != 0 ? 1 : 0;
    pa.mode = mode - 1;
    pa.lo = pa.quant ? fsr - (1 << (bits - 1)) : 0;
    pa.hi = fsr - 1;
    pa.nparts = b16_parts(nw);
    return pa;
}

int b16_pack_blocks(const PackB16Args& pa) {
    const int64_t units = pa.dense ? pa.nfrag : pa.n;
    return (int)std::min<int64_t>(1024, std::max<int64_t>(1, (units + kThreads - 1) / kThreads));
}

}  // namespace

hipError_t b16_pack_batch(int n, const B16PackReq* reqs, hipStream_t s) {
    for (int i0 = 0; i0 < n; i0 += kB16Batch) {
        B16PackBatch B;
        const int m = std::min(kB16Batch, n - i0);
        int nbmax = 1, npmax = 0;
        for (int i = 0; i < m; ++i) {
            const B16PackReq& r = reqs[i0 + i];
            B16PackJob& j = B.job[i];
            j.w = r.w;
            j.partial = reinterpret_cast<uint32_t*>(r.workspace);
            j.out = b16_packed_ptr(r.workspace);
            j.a = b16_pack_args(*r.plan, r.bits, r.fsr, r.mode);
            j.nb = b16_pack_blocks(j.a);
            nbmax = std::max(nbmax, j.nb);
            if (j.a.quant) npmax = std::max(npmax, j.a.nparts);
        }
        if (npmax > 0) {  // a group of mode-none jobs alone has no max|w| launch
            hipLaunchKernelGGL(absmax_b16_batch, dim3((unsigned)npmax, (unsigned)m), dim3(kThreads), 0, s, B);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(pack_b16_batch, dim3((unsigned)nbmax, (unsigned)m), dim3(kThreads), 0, s, B);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t b16_run(const ConvPlan& p, const uint16_t* x, const uint16_t* w, const uint16_t* bias, uint16_t* y, int bits,
                   int fsr, int mode, void* workspace, hipStream_t s, const B16Epi& epi) {
    uint32_t* partial = reinterpret_cast<uint32_t*>(workspace);
    const PackB16Args pa = b16_pack_args(p, bits, fsr, mode);
    if (pa.quant) {
        hipLaunchKernelGGL(absmax_b16, dim3(pa.nparts), dim3(kThreads), 0, s, w, pa.n, partial);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(pack_b16, dim3(b16_pack_blocks(pa)), dim3(kThreads), 0, s, w, partial, b16_packed_ptr(workspace),
                       pa);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return b16_run_packed(p, x, bias, y, workspace, s, epi);
}

// The conv alone, from a workspace b16_run's pack launches or b16_pack_batch filled
hipError_t b16_run_packed(const ConvPlan& p, const uint16_t* x, const uint16_t* bias, uint16_t* y,
                          const void* workspace, hipStream_t s, const B16Epi& epi) {
    const uint16_t* packed = b16_packed_ptr(const_cast<void*>(workspace));
    if (p.kind == KIND_BF16_ROWSK) return b16_rowsk_launch(p, x, packed, bias, y, s, epi);
    if (p.kind == KIND_BF16_ROWS) return b16_rows_launch(p, x, packed, bias, y, s, epi);
    if (p.kind == KIND_DW_BF16) {
        DwB16Args d;
        d.C = p.C; d.H = p.H; d.W = p.W; d.P = p.P; d.Q = p.Q; d.R = p.R; d.S = p.S;
        d.sh = p.sh; d.sw = p.sw; d.ph = p.ph; d.pw = p.pw; d.dh = p.dh; d.dw = p.dw;
        d.total = (int64_t)p.N * p.C * p.P * p.Q;
        if (epi.any())
            hipLaunchKernelGGL(conv_dw_b16<true>, dim3((unsigned)p.blocks), dim3(kThreads), 0, s, x, packed, bias, y, d,
                               epi);
        else
            hipLaunchKernelGGL(conv_dw_b16<false>, dim3((unsigned)p.blocks), dim3(kThreads), 0, s, x, packed, bias, y,
                               d, epi);
        return hipGetLastError();
    }
    B16Args a;
    a.N = p.N; a.C = p.C; a.H = p.H; a.W = p.W; a.K = p.K; a.P = p.P; a.Q = p.Q;
    a.sh = p.sh; a.sw = p.sw; a.ph = p.ph; a.pw = p.pw; a.dh = p.dh; a.dw = p.dw; a.R = p.R; a.S = p.S;
    a.TP = p.TP; a.TQ = p.TQ; a.tilesP = p.tilesP; a.tilesQ = p.tilesQ; a.kblocks = p.kblocks;
    a.nchunks = p.nchunks; a.HH = p.HH; a.WW = p.WW; a.ksteps = p.steps; a.taps = p.taps;
    a.w_off = p.HH * p.WW * 2 * p.CC + 16;
    a.tap_off = a.w_off + p.steps * p.NT * 1024;
    a.pair = (p.W % 2 == 0 && (reinterpret_cast<uintptr_t>(x) & 3u) == 0) ? 1 : 0;
    a.vec = (p.TQ % 4 == 0) ? 1 : 0;
    if (p.CC == 16) return launch_b16_nt<16>(p, a, x, packed, bias, y, epi, s);
    return launch_b16_nt<32>(p, a, x, packed, bias, y, epi, s);
}

}  // namespace po2q

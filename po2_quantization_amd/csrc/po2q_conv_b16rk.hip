// Row-streaming bf16 conv for 3x3 / stride 1 / pad 1 layers with C = K = 64 (KIND_BF16_ROWSK; opt-in:
// po2q_bf16_set_rowsk_kernels / PO2Q_B16_ROWSK, off by default and independent of the C = 16 / 32
// row kernel's switch).
//
// Arithmetic: conv_bf16x1's (po2q_conv_b16.hip), as for conv_b16_rows (po2q_conv_b16r.hip): Q(w) from
// the shared quant_bf16 body through pack_b16, one v_mfma_f32_16x16x32_bf16 per k-step, fp32
// accumulation, y = bf16_rne(acc + bias) (plain) or the po2q_epi.h epilogue on the fp32 accumulator
// followed by the one rounding (EPI).  Only the accumulation order differs.
//
// Walk: conv_b16_rows with conv_rowsk's split of the output channels over the waves.
//   * one 256-thread block owns (image, band of RB output rows) across the whole width (W <= 64);
//   * wave w owns the output channels 16w .. 16w + 15.  Its B fragments, 3 tap rows x 6 k-steps
//     (a tap row is 3 taps x 64 channels = 6 x 32: no k-step is padded, so there is no zero slot),
//     are 72 VGPRs and stay resident for the whole kernel;
//   * every wave computes all ceil(W / 16) pixel groups of a row (GW = 1, 2 or 4 group slots; a slot
//     past the last group is idle), three rotating accumulator sets per group (rows h - 1, h, h + 1);
//   * halo rows p0 - 1 .. p0 + RB go HBM [64][W] bf16 -> registers (8 channels x 2 pixels per thread:
//     8 octets x W / 2 pairs <= 256 items, one per thread) -> one of two LDS planes [W + 2][64] bf16
//     (x_addr<64> of po2q_x3_dev.h).  The two halo columns of both planes are written once, as zeros.
//     A halo row outside the image is skipped: not loaded, not multiplied, so padding never meets a
//     weight (no 0 * inf);
//   * the loads of row j + 1 are issued before row j multiplies and land in LDS after it, one barrier
//     per row;
//   * k-step ks = (tap column s = ks / 2, channel half ks % 2): lane octet o reads channel octet
//     4 * (ks % 2) + o of plane column q + s.  The swizzle of x_addr<64> touches the low two octet
//     bits only, so the second half's address is the first's + 64 bytes: three addresses per group.
//     Each A fragment is read by all four waves (6 ds_read_b128 per group and halo row against 18
//     MFMAs: DESIGN.md has the count);
//   * a finished row leaves through a wave-private LDS transpose [16][16 * GW] bf16 (+ 16 B pitch) as
//     16-byte pieces; a piece that is not 16-byte aligned or crosses the row end goes out as 4-byte
//     stores (W even), or 2-byte stores when y is only 2-byte aligned.  The ragged last group is masked
//     here; its lanes read a clamped column;
//   * x is staged with dword loads only when it is 4-byte aligned, else with 2-byte loads;
//   * the residual (EPI) comes in the way y goes out, backwards.
// Plain C++ loads and stores and __syncthreads() only: no inline assembly, no hand-written waits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>

#include "po2q_epi.h"
#include "po2q_internal.h"
#include "po2q_quant_b16_dev.h"
#include "po2q_x3_dev.h"

namespace po2q {

namespace {

constexpr int kKC = 64;                // C = K
constexpr int kKWaves = kThreads / 64;  // = channel tiles of 16
constexpr int kKWmax = 64;             // 4 group slots x 16 columns
constexpr int kKRing = 2;              // LDS planes
constexpr int kKSteps = 6;             // k-steps per tap row: 3 taps x 64 channels / 32
constexpr int kKOct = kKC / 8;

static_assert(kKWaves * 16 == kKC, "one 16-channel tile per wave");
static_assert(kKOct * (kKWmax / 2) <= kThreads, "one staging item per thread");

// bytes per channel of a wave's transpose tile: GW groups of 16 bf16, + 16 (as in po2q_conv_b16r.hip)
constexpr int rowsk_tpitch(int GW) { return GW * 32 + 16; }
int rowsk_plane(int W) { return (W + 2) * 2 * kKC; }

struct B16RKArgs {
    int N, H, W;
    int RB, bands, ngroups;
    int plane;  // bytes per LDS plane
    int pair;   // dword staging: x is 4-byte aligned (W is even)
};

__device__ __forceinline__ uint32_t kpk_lo16(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x05040100u); }

template <int GW, bool EPI>
__global__ __launch_bounds__(kThreads) void conv_b16_rowsk(const uint16_t* __restrict__ x,
                                                           const uint4* __restrict__ wpk,
                                                           const uint16_t* __restrict__ bias,
                                                           uint16_t* __restrict__ y, B16RKArgs a, B16Epi e) {
    static_assert(GW == 1 || GW == 2 || GW == 4, "group slots per wave");
    constexpr int C = kKC, KS = kKSteps, OCT = kKOct;
    constexpr int TP = rowsk_tpitch(GW);
    constexpr int CH = GW * 2;                 // 16-byte pieces per channel of the transpose tile
    constexpr int NPI = (16 * CH + 63) / 64;   // pieces per lane
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int o = lane >> 4;
    const int W = a.W, H = a.H;
    const int64_t HW = (int64_t)H * W;
    const int k0 = wave * 16;  // this wave's first output channel

    const int band = (int)(blockIdx.x % (unsigned)a.bands);
    const int n = (int)(blockIdx.x / (unsigned)a.bands);
    const int p0 = band * a.RB;
    const int rbe = min(a.RB, H - p0);
    const int nrows = rbe + 2;  // halo rows p0 - 1 .. p0 + rbe

    unsigned char* tile = lds + kKRing * a.plane + wave * (16 * TP);

    // ---- zeros, once: halo columns 0 and W + 1 of every plane
    if (tid < kKRing * 2 * OCT) {
        const int pl = tid / (2 * OCT), r = tid - pl * (2 * OCT);
        *reinterpret_cast<uint4*>(lds + pl * a.plane + x_addr<C>(r < OCT ? 0 : W + 1, r % OCT)) =
            make_uint4(0u, 0u, 0u, 0u);
    }

    // ---- B fragments of this wave's channel tile [tap row][k-step], resident
    bf16x8 bw[3][KS];
    {
        const uint4* wt = wpk + wave * (3 * KS * 64) + lane;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) bw[r][ks] = __builtin_bit_cast(bf16x8, wt[(r * KS + ks) * 64]);
    }

    // ---- A fragment addresses inside a plane (channel half 0; half 1 is + 64 bytes): plane column =
    // image column + 1
    int aoff[GW][3];
#pragma unroll
    for (int g = 0; g < GW; ++g) {
        const int q = min(g * 16 + (lane & 15), W - 1);  // ragged / idle groups: a column inside
#pragma unroll
        for (int s = 0; s < 3; ++s) aoff[g][s] = x_addr<C>(q + s, o);
    }

    // ---- staging item: (channel octet, pixel pair) -> 8 dwords from HBM, two 16-byte LDS writes
    const int W2 = W >> 1;
    const bool sv = tid < OCT * W2;
    const int soc = sv ? tid / W2 : 0, sm = sv ? tid - soc * W2 : 0;
    const int64_t sg = (int64_t)(soc * 8) * HW + 2 * sm;
    const int sl0 = x_addr<C>(2 * sm + 1, soc), sl1 = x_addr<C>(2 * sm + 2, soc);
    const uint16_t* xn = x + (int64_t)n * C * HW;
    uint32_t d[8];
    auto load_row = [&](int h) __attribute__((always_inline)) {
        if (!sv) return;
        const uint16_t* px = xn + (int64_t)h * W + sg;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint16_t* pj = px + j * HW;
            d[j] = a.pair ? *reinterpret_cast<const uint32_t*>(pj) : ((uint32_t)pj[0] | ((uint32_t)pj[1] << 16));
        }
    };
    auto write_row = [&](int pl) __attribute__((always_inline)) {
        if (!sv) return;
        unsigned char* pb = lds + pl * a.plane;
        *reinterpret_cast<uint4*>(pb + sl0) =
            make_uint4(kpk_lo16(d[0], d[1]), kpk_lo16(d[2], d[3]), kpk_lo16(d[4], d[5]), kpk_lo16(d[6], d[7]));
        *reinterpret_cast<uint4*>(pb + sl1) =
            make_uint4(pk_hi16(d[0], d[1]), pk_hi16(d[2], d[3]), pk_hi16(d[4], d[5]), pk_hi16(d[6], d[7]));
    };

    // ---- per-lane epilogue parameters: channel k0 + (lane & 15)
    const int kl = k0 + (lane & 15);
    const float bk = bias ? bf16_to_f(bias[kl]) : 0.0f;
    const float sk = (EPI && e.ps) ? e.ps[kl] : 1.0f;
    const float tk = (EPI && e.pb) ? e.pb[kl] : 0.0f;
    const bool aff = EPI && (e.ps || e.pb);

    // acc[g][slot]: slot 0 = output row h - 1, 1 = row h, 2 = row h + 1 of the halo row h at hand
    floatx4 acc[GW][3];
#pragma unroll
    for (int g = 0; g < GW; ++g)
#pragma unroll
        for (int sl = 0; sl < 3; ++sl) acc[g][sl] = floatx4{0.f, 0.f, 0.f, 0.f};

    // The residual of an output row takes the stores' way backwards (po2q_conv_b16r.hip): 16-byte pieces
    // HBM -> registers, requested before the row's last MFMAs, -> the wave's transpose tile.  A piece
    // is read 16 bytes at once only where it lies inside the row and this lane's address is 16-byte
    // aligned, else as 4-byte pairs (4-byte aligned; W even) or 2-byte elements inside the row; what
    // lies past the row end stays zero.
    uint4 rres[EPI ? NPI : 1];
    auto load_res = [&](int p) __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < NPI; ++it) {
            const int el = it * 64 + lane;
            const int k = el / CH, j = el % CH;
            const int qq = j * 8;
            uint32_t t[4] = {0u, 0u, 0u, 0u};
            if (el < 16 * CH && qq < W) {
                const uint16_t* rp = e.res + (((int64_t)n * C + k0 + k) * H + p) * W + qq;
                if (qq + 7 < W && (reinterpret_cast<uintptr_t>(rp) & 15u) == 0) {
                    const uint4 r4 = *reinterpret_cast<const uint4*>(rp);
                    t[0] = r4.x; t[1] = r4.y; t[2] = r4.z; t[3] = r4.w;
                } else if ((reinterpret_cast<uintptr_t>(rp) & 3u) == 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (qq + 2 * i < W) t[i] = reinterpret_cast<const uint32_t*>(rp)[i];
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (qq + i < W) t[i >> 1] |= (uint32_t)rp[i] << (16 * (i & 1));
                }
            }
            rres[EPI ? it : 0] = make_uint4(t[0], t[1], t[2], t[3]);
        }
    };

    // one finished output row: epilogue, rounding, transpose, stores
    auto store_row = [&](int p, auto act_c) __attribute__((always_inline)) {
        constexpr int ACT = decltype(act_c)::value;
        if constexpr (EPI) {
            if (e.res) {
#pragma unroll
                for (int it = 0; it < NPI; ++it) {
                    const int el = it * 64 + lane;
                    if (el < 16 * CH) *reinterpret_cast<uint4*>(tile + (el / CH) * TP + (el % CH) * 16) = rres[it];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
#pragma unroll
        for (int g = 0; g < GW; ++g) {
            if (g >= a.ngroups) continue;  // block-uniform
            unsigned char* tp = tile + (lane & 15) * TP + (g * 16 + 4 * o) * 2;
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = acc[g][0][i] + bk;
            if constexpr (EPI) {
                float rv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (e.res) {  // the lane's 4 residual values, from the tile (the result goes back in place)
                    const uint2 rq = *reinterpret_cast<const uint2*>(tp);
                    rv[0] = __uint_as_float(rq.x << 16);
                    rv[1] = __uint_as_float(rq.x & 0xffff0000u);
                    rv[2] = __uint_as_float(rq.y << 16);
                    rv[3] = __uint_as_float(rq.y & 0xffff0000u);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (aff) v[i] = v[i] * sk + tk;
                    if (e.res) v[i] += rv[i];
                    v[i] = epi_act_ct<ACT>(v[i]);
                }
            }
            uint32_t r[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = bf16_rne(v[i]);  // the one rounding
            *reinterpret_cast<uint2*>(tp) = make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
        }
        // the tile is this wave's own: LDS executes a wave's accesses in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int it = 0; it < NPI; ++it) {
            const int el = it * 64 + lane;
            const int k = el / CH, j = el % CH;
            const int qq = j * 8;
            if (el >= 16 * CH || qq >= W) continue;  // (GW = 1: 32 pieces;) idle groups, pieces past the row end
            const uint4 t4 = *reinterpret_cast<const uint4*>(tile + k * TP + j * 16);
            uint16_t* yp = y + (((int64_t)n * C + k0 + k) * H + p) * W + qq;
            const uint32_t t[4] = {t4.x, t4.y, t4.z, t4.w};
            if (qq + 7 < W && (reinterpret_cast<uintptr_t>(yp) & 15u) == 0) {
                *reinterpret_cast<uint4*>(yp) = t4;
            } else if ((reinterpret_cast<uintptr_t>(yp) & 3u) == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (qq + 2 * i < W) reinterpret_cast<uint32_t*>(yp)[i] = t[i];  // W, qq even: a whole pair
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (qq + i < W) yp[i] = (uint16_t)(t[i >> 1] >> (16 * (i & 1)));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };

    auto body = [&](auto act_c) __attribute__((always_inline)) {
        // ---- prologue: the first halo row (p0 - 1; outside the image for the first band)
        if (p0 >= 1) {
            load_row(p0 - 1);
            write_row(0);
        }
        __syncthreads();
        for (int hr = 0; hr < nrows; ++hr) {
            const int h = p0 - 1 + hr;
            const bool in = h >= 0 && h < H;               // block-uniform
            const bool inn = hr + 1 < nrows && h + 1 < H;  // the next halo row is wanted and inside
            if (inn) load_row(h + 1);
            if constexpr (EPI) {
                if (e.res && hr >= 2) load_res(p0 + hr - 2);  // block-uniform
            }
            if (in) {
                const unsigned char* pb = lds + (hr & 1) * a.plane;
#pragma unroll
                for (int g = 0; g < GW; ++g) {
                    if (g >= a.ngroups) continue;  // block-uniform
                    bf16x8 af[KS];
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        af[ks] = __builtin_bit_cast(
                            bf16x8, *reinterpret_cast<const uint4*>(pb + aoff[g][ks >> 1] + (ks & 1) * 64));
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int ks = 0; ks < KS; ++ks)
                            acc[g][2 - r] =
                                __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], bw[r][ks], acc[g][2 - r], 0, 0, 0);
                }
            }
            if (inn) write_row((hr + 1) & 1);
            if (hr >= 2) store_row(p0 + hr - 2, act_c);
#pragma unroll
            for (int g = 0; g < GW; ++g) {
                acc[g][0] = acc[g][1];
                acc[g][1] = acc[g][2];
                acc[g][2] = floatx4{0.f, 0.f, 0.f, 0.f};
            }
            __syncthreads();  // plane (hr + 1) & 1 is written, plane hr & 1 is read
        }
    };
    if constexpr (EPI)
        with_act(e.act, body);
    else
        body(std::integral_constant<int, 0>{});
}

template <int GW>
hipError_t launch_rowsk_t(const ConvPlan& p, const B16RKArgs& a, const uint16_t* x, const uint16_t* packed,
                          const uint16_t* bias, uint16_t* y, const B16Epi& e, hipStream_t s) {
    if (e.any())
        hipLaunchKernelGGL((conv_b16_rowsk<GW, true>), dim3((unsigned)p.blocks), dim3(kThreads), p.lds_bytes, s, x,
                           reinterpret_cast<const uint4*>(packed), bias, y, a, e);
    else
        hipLaunchKernelGGL((conv_b16_rowsk<GW, false>), dim3((unsigned)p.blocks), dim3(kThreads), p.lds_bytes, s, x,
                           reinterpret_cast<const uint4*>(packed), bias, y, a, e);
    return hipGetLastError();
}

// the switch: process-wide, PO2Q_B16_ROWSK gives the initial value (read once)
std::atomic<int>& rowsk_switch() {
    static std::atomic<int> v([] {
        const char* s = getenv("PO2Q_B16_ROWSK");
        return (s && atoi(s) != 0) ? 1 : 0;
    }());
    return v;
}

}  // namespace

int b16_rowsk_get() { return rowsk_switch().load(); }
int b16_rowsk_set(int on) { return rowsk_switch().exchange(on ? 1 : 0); }

int b16_rowsk_wmax() { return kKWmax; }

// Eligibility is a function of the geometry alone; the plan is taken only with the switch on.
bool b16_rowsk_plan(ConvPlan& p) {
    if (!b16_rowsk_get()) return false;
    if (p.groups != 1 || p.R != 3 || p.S != 3) return false;
    if (p.sh != 1 || p.sw != 1 || p.ph != 1 || p.pw != 1 || p.dh != 1 || p.dw != 1) return false;
    if (p.C != kKC || p.K != kKC) return false;
    if (p.W % 2 != 0 || p.W > kKWmax) return false;
    const int ngroups = (p.W + 15) / 16;
    const int GW = ngroups <= 1 ? 1 : (ngroups <= 2 ? 2 : 4);
    // RB: b16_rows_plan's rule
    int RB = 16;
    while (RB > 4 && (int64_t)p.N * ((p.P + RB - 1) / RB) < 1024) RB >>= 1;
    const int bands = (p.P + RB - 1) / RB;
    const int64_t blocks = (int64_t)p.N * bands;
    if (blocks > INT32_MAX) return false;
    p.kind = KIND_BF16_ROWSK;
    p.CC = kKC;
    p.NT = kKWaves;  // channel tiles, one per wave
    p.NJ = GW;
    p.TP = RB; p.TQ = p.W; p.tilesP = bands; p.tilesQ = ngroups;
    p.kblocks = 1; p.nchunks = 1;
    p.HH = RB + 2; p.WW = p.WWp = p.W + 2;
    p.steps = kKSteps;
    p.pd = kKRing;
    p.lds_bytes = (size_t)kKRing * rowsk_plane(p.W) + (size_t)kKWaves * 16 * rowsk_tpitch(GW);
    p.blocks = blocks;
    // packed bf16 fragments [channel tile][tap row][k-step][lane][8] -> 4-byte words
    p.packed_floats = (int64_t)p.NT * 3 * p.steps * 64 * 4;
    return true;
}

void b16_rowsk_describe(const ConvPlan& p, char* buf, size_t len) {
    snprintf(buf, len, "kind=bf16_rowsk C=%d RB=%d bands=%d groups=%d GW=%d ring=%d lds=%zu blocks=%lld", p.C, p.TP,
             p.tilesP, p.tilesQ, p.NJ, p.pd, p.lds_bytes, (long long)p.blocks);
}

hipError_t b16_rowsk_launch(const ConvPlan& p, const uint16_t* x, const uint16_t* packed, const uint16_t* bias,
                            uint16_t* y, hipStream_t s, const B16Epi& e) {
    B16RKArgs a;
    a.N = p.N; a.H = p.H; a.W = p.W;
    a.RB = p.TP; a.bands = p.tilesP; a.ngroups = p.tilesQ;
    a.plane = rowsk_plane(p.W);
    a.pair = (reinterpret_cast<uintptr_t>(x) & 3u) == 0 ? 1 : 0;
    switch (p.NJ) {
        case 1: return launch_rowsk_t<1>(p, a, x, packed, bias, y, e, s);
        case 2: return launch_rowsk_t<2>(p, a, x, packed, bias, y, e, s);
        case 4: return launch_rowsk_t<4>(p, a, x, packed, bias, y, e, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace po2q

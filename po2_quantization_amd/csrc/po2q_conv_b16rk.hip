// Row-streaming bf16 conv for 3x3 / stride 1 / pad 1 layers with C = K = 64 (KIND_BF16_ROWSK; opt-in:
// po2q_bf16_set_rowsk_kernels / PO2Q_B16_ROWSK, off by default and independent of the C = 16 / 32
// row kernel's switch).
//
// Arithmetic: conv_bf16x1's (po2q_conv_b16.hip), as for conv_b16_rows (po2q_conv_b16r.hip); only the
// accumulation order differs.
//
// Walk: conv_b16_rows with conv_rowsk's split of the output channels over the waves; staging, stores
// and the residual path are po2q_b16_rows_dev.h's and are described there.
//   * one 256-thread block owns (image, band of RB output rows) across the whole width (W <= 64);
//   * wave w owns the output channels 16w .. 16w + 15.  Its B fragments, 3 tap rows x 6 k-steps
//     (a tap row is 3 taps x 64 channels = 6 x 32: no k-step is padded, so there is no zero slot),
//     are 72 VGPRs and stay resident for the whole kernel;
//   * every wave computes all ceil(W / 16) pixel groups of a row (GW = 1, 2 or 4 group slots; a slot
//     past the last group is idle), three rotating accumulator sets per group (rows h - 1, h, h + 1);
//   * halo rows p0 - 1 .. p0 + RB: 8 octets x W / 2 pairs <= 256 staging items, one per thread, into
//     one of two LDS planes [W + 2][64] bf16; one barrier per row;
//   * k-step ks = (tap column s = ks / 2, channel half ks % 2): lane octet o reads channel octet
//     4 * (ks % 2) + o of plane column q + s.  The swizzle of x_addr<64> touches the low two octet
//     bits only, so the second half's address is the first's + 64 bytes: three addresses per group.
//     Each A fragment is read by all four waves (6 ds_read_b128 per group and halo row against 18
//     MFMAs: DESIGN.md has the count);
//   * a finished row leaves through the wave's tile [16][16 * GW], from column 0.
// Plain C++ loads and stores and __syncthreads() only: no inline assembly, no hand-written waits.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>

#include "po2q_b16_rows_dev.h"

namespace po2q {

namespace {

constexpr int kKC = 64;                     // C = K
constexpr int kKWmax = 64;                  // 4 group slots x 16 columns
constexpr int kKRing = 2;                   // LDS planes
constexpr int kKSteps = b16_rows_ks(kKC);   // k-steps per tap row: 3 taps x 64 channels / 32

static_assert(kB16RowWaves * 16 == kKC, "one 16-channel tile per wave");
static_assert(kKC / 8 * (kKWmax / 2) <= kThreads, "one staging item per thread");

template <int GW, bool EPI>
__global__ __launch_bounds__(kThreads) void conv_b16_rowsk(const uint16_t* __restrict__ x,
                                                           const uint4* __restrict__ wpk,
                                                           const uint16_t* __restrict__ bias,
                                                           uint16_t* __restrict__ y, B16RowArgs a, B16Epi e) {
    static_assert(GW == 1 || GW == 2 || GW == 4, "group slots per wave");
    constexpr int C = kKC, KS = kKSteps;
    constexpr int TP = b16_rows_tpitch(GW);
    constexpr int CH = GW * 2;  // 16-byte pieces per channel of the transpose tile
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

    zero_planes<C, false>(lds, kKRing, a.plane, W, 0, tid);

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

    // ---- staging item
    const int W2 = W >> 1;
    B16Stage st;
    st.v = tid < C / 8 * W2;
    const int soc = st.v ? tid / W2 : 0, sm = st.v ? tid - soc * W2 : 0;
    st.g = (int64_t)(soc * 8) * HW + 2 * sm;
    st.l0 = x_addr<C>(2 * sm + 1, soc);
    st.l1 = x_addr<C>(2 * sm + 2, soc);
    const uint16_t* xn = x + (int64_t)n * C * HW;
    uint32_t d[8];
    auto load_row = [&](int h) __attribute__((always_inline)) { stage_load(st, xn + (int64_t)h * W, HW, a.pair, d); };
    auto write_row = [&](int pl) __attribute__((always_inline)) { stage_write(st, lds + pl * a.plane, d); };

    // ---- per-lane epilogue parameters: channel k0 + (lane & 15)
    const int kl = k0 + (lane & 15);
    const float bk = bias ? bf16_to_f(bias[kl]) : 0.0f;
    const float sk = (EPI && e.ps) ? e.ps[kl] : 1.0f;
    const float tk = (EPI && e.pb) ? e.pb[kl] : 0.0f;
    const bool aff = EPI && (e.ps || e.pb);
    const bool hres = EPI && e.res;

    // acc[g][slot]: slot 0 = output row h - 1, 1 = row h, 2 = row h + 1 of the halo row h at hand
    floatx4 acc[GW][3];
#pragma unroll
    for (int g = 0; g < GW; ++g)
#pragma unroll
        for (int sl = 0; sl < 3; ++sl) acc[g][sl] = floatx4{0.f, 0.f, 0.f, 0.f};

    uint4 rres[pieces_per_lane(16, CH)];  // the residual pieces of the row to finish next

    // one finished output row: epilogue, rounding, transpose, stores
    auto store_row = [&](int p, auto act_c) __attribute__((always_inline)) {
        constexpr int ACT = decltype(act_c)::value;
        if (hres) {
            tile_fill<16, CH, TP>(tile, rres, lane);
            tile_fence();
        }
#pragma unroll
        for (int g = 0; g < GW; ++g) {
            if (g >= a.ngroups) continue;  // block-uniform
            finish4_inplace<ACT>(tile + (lane & 15) * TP + (g * 16 + 4 * o) * 2, acc[g][0], bk, aff, sk, tk, hres);
        }
        tile_fence();
        tile_drain<16, CH, TP>(tile, y, (int64_t)n * C, k0, H, W, p, 0, lane);
        tile_fence<false>();
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
            if (hres && hr >= 2) res_load<16, CH>(rres, e.res, (int64_t)n * C, k0, H, W, p0 + hr - 2, 0, lane);  // block-uniform
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
            rotate_acc(acc);
            __syncthreads();  // plane (hr + 1) & 1 is written, plane hr & 1 is read
        }
    };
    if constexpr (EPI)
        with_act(e.act, body);
    else
        body(std::integral_constant<int, 0>{});
}

template <int GW>
hipError_t launch_rowsk_t(const ConvPlan& p, const B16RowArgs& a, const uint16_t* x, const uint16_t* packed,
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
    static std::atomic<int> v(env_switch("PO2Q_B16_ROWSK"));
    return v;
}

}  // namespace

int b16_rowsk_get() { return rowsk_switch().load(); }
int b16_rowsk_set(int on) { return rowsk_switch().exchange(on ? 1 : 0); }

int b16_rowsk_wmax() { return kKWmax; }

// Eligibility is a function of the geometry alone; the plan is taken only with the switch on.
bool b16_rowsk_plan(ConvPlan& p) {
    if (!b16_rowsk_get() || !b16_rows_geom_ok(p)) return false;
    if (p.C != kKC || p.K != kKC || p.W > kKWmax) return false;
    return fill_rows_plan(p, KIND_BF16_ROWSK, kKRing, kKRing, 2, 0);
}

void b16_rowsk_describe(const ConvPlan& p, char* buf, size_t len) {
    snprintf(buf, len, "kind=bf16_rowsk C=%d RB=%d bands=%d groups=%d GW=%d ring=%d lds=%zu blocks=%lld", p.C, p.TP,
             p.tilesP, p.tilesQ, p.NJ, p.pd, p.lds_bytes, (long long)p.blocks);
}

hipError_t b16_rowsk_launch(const ConvPlan& p, const uint16_t* x, const uint16_t* packed, const uint16_t* bias,
                            uint16_t* y, hipStream_t s, const B16Epi& e) {
    const B16RowArgs a = b16_row_args(p, x);
    switch (p.NJ) {
        case 1: return launch_rowsk_t<1>(p, a, x, packed, bias, y, e, s);
        case 2: return launch_rowsk_t<2>(p, a, x, packed, bias, y, e, s);
        case 4: return launch_rowsk_t<4>(p, a, x, packed, bias, y, e, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace po2q

// Row-streaming bf16 conv for 3x3 / stride 1 / pad 1 layers with C = K = 16 or 32 (KIND_BF16_ROWS;
// opt-in: po2q_bf16_set_row_kernels / PO2Q_B16_ROWS, off by default).
//
// Arithmetic: conv_bf16x1's (po2q_conv_b16.hip).  Q(w) comes from the shared quant_bf16 body through
// pack_b16, every product x * Q(w) is formed exactly by v_mfma_f32_16x16x32_bf16, accumulation is
// fp32, there is no scale factor, and y = bf16_rne(acc + bias) (plain) or the po2q_epi.h epilogue on
// the fp32 accumulator followed by the one rounding (EPI).  Only the accumulation order differs.
//
// Walk (after conv_rowsf / conv_rows of the fp32 entry); staging, zero slot, stores and the residual
// path are po2q_b16_rows_dev.h's and are described there:
//   * one 256-thread block owns (image, band of RB output rows) across the whole width; its 16-column
//     pixel groups are dealt to the 4 waves, GW consecutive groups each (GW = 1, 2 or 4);
//   * the block walks the halo rows p0 - 1 .. p0 + RB, C / 16 staging items per thread and row;
//   * two planes: the loads of row j + 1 are issued before row j multiplies and land in LDS after it,
//     one barrier per row.  (A three-deep ring wants a second register set per thread; the blocks are
//     small enough that 2 - 6 of them share a CU, which is what hides the load latency.)
//   * a halo row's A fragments are read once per group and multiplied with the B fragments of all
//     three tap rows into three rotating accumulator sets (rows h - 1, h, h + 1).  k = (tap column s,
//     channel): C = 16 has the k-steps (s0 | s1) and (s2 | zero), C = 32 one per tap column;
//   * B fragments stay in VGPRs for the whole kernel (24 registers at C = 16, 72 at C = 32);
//   * a finished output row leaves through the wave's tile [C][GW * 16]; the residual (EPI) of a row
//     is requested ahead of the row's last MFMAs.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>

#include "po2q_b16_rows_dev.h"

namespace po2q {

namespace {

constexpr int kRWmax = 256;  // 4 waves x 4 groups x 16 columns
constexpr int kRRing = 2;    // LDS planes

template <int C, int GW, bool EPI>
__global__ __launch_bounds__(kThreads) void conv_b16_rows(const uint16_t* __restrict__ x,
                                                          const uint4* __restrict__ wpk,
                                                          const uint16_t* __restrict__ bias,
                                                          uint16_t* __restrict__ y, B16RowArgs a, B16Epi e) {
    static_assert(C == 16 || C == 32, "C = K = 16 or 32");
    static_assert(GW == 1 || GW == 2 || GW == 4, "groups per wave");
    constexpr int NT = C / 16, KS = b16_rows_ks(C), OCT = C / 8;
    constexpr int NI = C / 16;  // staging items per thread: OCT * Wmax / 2 / kThreads
    constexpr int TP = b16_rows_tpitch(GW);
    constexpr int CH = GW * 2;  // 16-byte pieces per channel of the transpose tile
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int o = lane >> 4;
    const int W = a.W, H = a.H;
    const int64_t HW = (int64_t)H * W;

    const int band = (int)(blockIdx.x % (unsigned)a.bands);
    const int n = (int)(blockIdx.x / (unsigned)a.bands);
    const int p0 = band * a.RB;
    const int rbe = min(a.RB, H - p0);
    const int nrows = rbe + 2;  // halo rows p0 - 1 .. p0 + rbe

    unsigned char* tile = lds + kRRing * a.plane + wave * (C * TP);
    const int zero_off = (W + 2) * 2 * C;

    zero_planes<C, true>(lds, kRRing, a.plane, W, zero_off, tid);

    // ---- B fragments [tap row][k-step][nt], resident
    bf16x8 bw[3][KS][NT];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bw[r][ks][nt] = __builtin_bit_cast(bf16x8, wpk[((r * KS + ks) * NT + nt) * 64 + lane]);

    // ---- A fragment addresses inside a plane: plane column = image column + 1
    int aoff[GW][KS];
#pragma unroll
    for (int g = 0; g < GW; ++g) {
        const int q = min((wave * GW + g) * 16 + (lane & 15), W - 1);  // ragged / idle groups: a column inside
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) aoff[g][ks] = frag_off<C>(q, ks, o, zero_off);
    }

    // ---- staging items
    const int W2 = W >> 1;
    B16Stage st[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int it = tid + i * kThreads;
        st[i].v = it < OCT * W2;
        const int oc = st[i].v ? it / W2 : 0, m = st[i].v ? it - oc * W2 : 0;
        st[i].g = (int64_t)(oc * 8) * HW + 2 * m;
        st[i].l0 = x_addr<C>(2 * m + 1, oc);
        st[i].l1 = x_addr<C>(2 * m + 2, oc);
    }
    const uint16_t* xn = x + (int64_t)n * C * HW;
    uint32_t d[NI][8];
    auto load_row = [&](int h) __attribute__((always_inline)) {
        const uint16_t* xr = xn + (int64_t)h * W;
#pragma unroll
        for (int i = 0; i < NI; ++i) stage_load(st[i], xr, HW, a.pair, d[i]);
    };
    auto write_row = [&](int pl) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NI; ++i) stage_write(st[i], lds + pl * a.plane, d[i]);
    };

    // ---- per-lane epilogue parameters: channel nt * 16 + (lane & 15) < C
    float bk[NT], sk[NT], tk[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int k = nt * 16 + (lane & 15);
        bk[nt] = bias ? bf16_to_f(bias[k]) : 0.0f;
        sk[nt] = (EPI && e.ps) ? e.ps[k] : 1.0f;
        tk[nt] = (EPI && e.pb) ? e.pb[k] : 0.0f;
    }
    const bool aff = EPI && (e.ps || e.pb);
    const bool hres = EPI && e.res;

    // acc[g][slot]: slot 0 = output row h - 1, 1 = row h, 2 = row h + 1 of the halo row h at hand
    floatx4 acc[GW][3][NT];
#pragma unroll
    for (int g = 0; g < GW; ++g)
#pragma unroll
        for (int sl = 0; sl < 3; ++sl)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[g][sl][nt] = floatx4{0.f, 0.f, 0.f, 0.f};

    uint4 rres[pieces_per_lane(C, CH)];  // the residual pieces of the row to finish next

    // one finished output row: epilogue, rounding, transpose, stores
    auto store_row = [&](int p, auto act_c) __attribute__((always_inline)) {
        constexpr int ACT = decltype(act_c)::value;
        if (hres) {
            tile_fill<C, CH, TP>(tile, rres, lane);
            tile_fence();
        }
#pragma unroll
        for (int g = 0; g < GW; ++g) {
            if ((wave * GW + g) >= a.ngroups) continue;  // wave-uniform
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int k = nt * 16 + (lane & 15);
                finish4_inplace<ACT>(tile + k * TP + (g * 16 + 4 * o) * 2, acc[g][0][nt], bk[nt], aff, sk[nt], tk[nt], hres);
            }
        }
        tile_fence();
        tile_drain<C, CH, TP>(tile, y, (int64_t)n * C, 0, H, W, p, wave * (GW * 16), lane);
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
            const bool in = h >= 0 && h < H;                 // block-uniform
            const bool inn = hr + 1 < nrows && h + 1 < H;    // the next halo row is wanted and inside
            if (inn) load_row(h + 1);
            if (hres && hr >= 2)  // block-uniform
                res_load<C, CH>(rres, e.res, (int64_t)n * C, 0, H, W, p0 + hr - 2, wave * (GW * 16), lane);
            if (in) {
                const unsigned char* pb = lds + (hr & 1) * a.plane;
#pragma unroll
                for (int g = 0; g < GW; ++g) {
                    if ((wave * GW + g) >= a.ngroups) continue;  // wave-uniform
                    bf16x8 af[KS];
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        af[ks] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(pb + aoff[g][ks]));
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                            for (int nt = 0; nt < NT; ++nt)
                                acc[g][2 - r][nt] =
                                    __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], bw[r][ks][nt], acc[g][2 - r][nt], 0, 0, 0);
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

template <int C, int GW>
hipError_t launch_rows_t(const ConvPlan& p, const B16RowArgs& a, const uint16_t* x, const uint16_t* packed,
                         const uint16_t* bias, uint16_t* y, const B16Epi& e, hipStream_t s) {
    if (e.any())
        hipLaunchKernelGGL((conv_b16_rows<C, GW, true>), dim3((unsigned)p.blocks), dim3(kThreads), p.lds_bytes, s, x,
                           reinterpret_cast<const uint4*>(packed), bias, y, a, e);
    else
        hipLaunchKernelGGL((conv_b16_rows<C, GW, false>), dim3((unsigned)p.blocks), dim3(kThreads), p.lds_bytes, s, x,
                           reinterpret_cast<const uint4*>(packed), bias, y, a, e);
    return hipGetLastError();
}

template <int C>
hipError_t launch_rows_gw(const ConvPlan& p, const B16RowArgs& a, const uint16_t* x, const uint16_t* packed,
                          const uint16_t* bias, uint16_t* y, const B16Epi& e, hipStream_t s) {
    switch (p.NJ) {
        case 1: return launch_rows_t<C, 1>(p, a, x, packed, bias, y, e, s);
        case 2: return launch_rows_t<C, 2>(p, a, x, packed, bias, y, e, s);
        case 4: return launch_rows_t<C, 4>(p, a, x, packed, bias, y, e, s);
        default: return hipErrorInvalidValue;
    }
}

// the switch: process-wide, PO2Q_B16_ROWS gives the initial value (read once)
std::atomic<int>& rows_switch() {
    static std::atomic<int> v(env_switch("PO2Q_B16_ROWS"));
    return v;
}

}  // namespace

int b16_rows_get() { return rows_switch().load(); }
int b16_rows_set(int on) { return rows_switch().exchange(on ? 1 : 0); }

int b16_rows_wmax() { return kRWmax; }

// Eligibility is a function of the geometry alone; the plan is taken only with the switch on.
bool b16_rows_plan(ConvPlan& p) {
    if (!b16_rows_get() || !b16_rows_geom_ok(p)) return false;
    if (p.C != p.K || (p.C != 16 && p.C != 32) || p.W > kRWmax) return false;
    return fill_rows_plan(p, KIND_BF16_ROWS, kRRing, kRRing, 2, 0);
}

void b16_rows_describe(const ConvPlan& p, char* buf, size_t len) {
    snprintf(buf, len, "kind=bf16_rows C=%d RB=%d bands=%d groups=%d ring=%d lds=%zu blocks=%lld", p.C, p.TP, p.tilesP,
             p.tilesQ, p.pd, p.lds_bytes, (long long)p.blocks);
}

hipError_t b16_rows_launch(const ConvPlan& p, const uint16_t* x, const uint16_t* packed, const uint16_t* bias,
                           uint16_t* y, hipStream_t s, const B16Epi& e) {
    const B16RowArgs a = b16_row_args(p, x);
    if (p.C == 16) return launch_rows_gw<16>(p, a, x, packed, bias, y, e, s);
    return launch_rows_gw<32>(p, a, x, packed, bias, y, e, s);
}

}  // namespace po2q

// Row-streaming bf16 conv for 3x3 / stride 1 / pad 1 layers with C = K = 16 or 32 (KIND_BF16_ROWS;
// opt-in: po2q_bf16_set_row_kernels / PO2Q_B16_ROWS, off by default).
//
// Arithmetic: conv_bf16x1's (po2q_conv_b16.hip).  Q(w) comes from the shared quant_bf16 body through
// pack_b16, every product x * Q(w) is formed exactly by v_mfma_f32_16x16x32_bf16, accumulation is
// fp32, there is no scale factor, and y = bf16_rne(acc + bias) (plain) or the po2q_epi.h epilogue on
// the fp32 accumulator followed by the one rounding (EPI).  Only the accumulation order differs.
//
// Walk (after conv_rowsf / conv_rows of the fp32 entry):
//   * one 256-thread block owns (image, band of RB output rows) across the whole width; its 16-column
//     pixel groups are dealt to the 4 waves, GW consecutive groups each (GW = 1, 2 or 4);
//   * the block walks the halo rows p0 - 1 .. p0 + RB.  A halo row inside the image goes
//     HBM [C][W] bf16 -> registers (8 channels x 2 pixels per thread and item, whole-row dword runs
//     per channel) -> one LDS plane [W + 2 halo columns][C] bf16 (x_addr of po2q_x3_dev.h).  The two
//     halo columns and the plane's 16-byte zero slot are written once, as zeros.  A halo row outside
//     the image is skipped: not loaded, not multiplied;
//   * two planes: the loads of row j + 1 are issued before row j multiplies and land in LDS after it,
//     one barrier per row.  (A three-deep ring wants a second register set per thread; the blocks are
//     small enough that 2 - 6 of them share a CU, which is what hides the load latency.)
//   * a halo row's A fragments are read once per group and multiplied with the B fragments of all
//     three tap rows into three rotating accumulator sets (rows h - 1, h, h + 1).  k = (tap column s,
//     channel): C = 16 has the k-steps (s0 | s1) and (s2 | zero), C = 32 one per tap column.  The
//     padded half of (s2 | zero) reads the plane's zero slot on the A side as well: 0 * inf cannot
//     appear from padding;
//   * B fragments stay in VGPRs for the whole kernel (24 registers at C = 16, 72 at C = 32);
//   * a finished output row is transposed through a wave-private LDS tile [C][GW * 16] bf16 and
//     stored as 16-byte pieces: one store instruction covers 128-byte runs of 8 channels (GW = 4).
//     A piece that is not 16-byte aligned, or that crosses the row end, goes out as 4-byte stores
//     (W is even: a pixel pair is inside the row or outside it as a whole) or, when y is only
//     2-byte aligned, as 2-byte stores.  The ragged last group is masked here, at the store; its lanes
//     read a clamped column, never one outside the plane.
//   * x is staged with dword loads only when it is 4-byte aligned (a.pair), else with 2-byte loads;
//   * the residual (EPI) comes in the way y goes out: 16-byte pieces into registers ahead of the row's
//     last MFMAs, through the wave's tile to the lanes; 16 bytes at once only where the lane's address
//     is 16-byte aligned (tested per lane), else 4-byte pairs or 2-byte elements with the same bits.
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

constexpr int kRWaves = kThreads / 64;
constexpr int kRWmax = 256;  // 4 waves x 4 groups x 16 columns
constexpr int kRRing = 2;    // LDS planes

constexpr int rows_ks(int C) { return C == 16 ? 2 : 3; }
// bytes per channel of a wave's transpose tile: GW groups of 16 bf16, + 16 so that the 16 channels
// of an 8-byte write instruction fall into distinct banks
constexpr int rows_tpitch(int GW) { return GW * 32 + 16; }
int rows_plane(int C, int W) { return (W + 2) * 2 * C + 16; }  // + the zero slot

struct B16RArgs {
    int N, H, W;
    int RB, bands, ngroups;
    int plane;  // bytes per LDS plane (zero slot included)
    int pair;   // dword staging: x is 4-byte aligned (W is even)
};

__device__ __forceinline__ uint32_t rpk_lo16(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x05040100u); }

template <int C, int GW, bool EPI>
__global__ __launch_bounds__(kThreads) void conv_b16_rows(const uint16_t* __restrict__ x,
                                                          const uint4* __restrict__ wpk,
                                                          const uint16_t* __restrict__ bias,
                                                          uint16_t* __restrict__ y, B16RArgs a, B16Epi e) {
    static_assert(C == 16 || C == 32, "C = K = 16 or 32");
    static_assert(GW == 1 || GW == 2 || GW == 4, "groups per wave");
    constexpr int NT = C / 16, KS = rows_ks(C), OCT = C / 8;
    constexpr int NI = C / 16;  // staging items per thread: OCT * Wmax / 2 / kThreads
    constexpr int TP = rows_tpitch(GW);
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

    // ---- zeros, once: halo columns 0 and W + 1 and the zero slot of every plane
    if (tid < kRRing * (2 * OCT + 1)) {
        const int pl = tid / (2 * OCT + 1), r = tid - pl * (2 * OCT + 1);
        const int off = r == 2 * OCT ? zero_off : x_addr<C>(r < OCT ? 0 : W + 1, r % OCT);
        *reinterpret_cast<uint4*>(lds + pl * a.plane + off) = make_uint4(0u, 0u, 0u, 0u);
    }

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
        for (int ks = 0; ks < KS; ++ks) {
            if constexpr (C == 16)
                aoff[g][ks] = ks == 0 ? x_addr<16>(q + (o >> 1), o & 1) : (o < 2 ? x_addr<16>(q + 2, o) : zero_off);
            else
                aoff[g][ks] = x_addr<32>(q + ks, o);
        }
    }

    // ---- staging items: (channel octet, pixel pair) -> 8 dwords from HBM, two 16-byte LDS writes
    const int W2 = W >> 1;
    bool sv[NI];
    int64_t sg[NI];
    int sl0[NI], sl1[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int it = tid + i * kThreads;
        sv[i] = it < OCT * W2;
        const int oc = sv[i] ? it / W2 : 0, m = sv[i] ? it - oc * W2 : 0;
        sg[i] = (int64_t)(oc * 8) * HW + 2 * m;
        sl0[i] = x_addr<C>(2 * m + 1, oc);
        sl1[i] = x_addr<C>(2 * m + 2, oc);
    }
    const uint16_t* xn = x + (int64_t)n * C * HW;
    uint32_t d[NI][8];
    auto load_row = [&](int h) __attribute__((always_inline)) {
        const uint16_t* xr = xn + (int64_t)h * W;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (!sv[i]) continue;
            const uint16_t* px = xr + sg[i];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint16_t* pj = px + j * HW;
                d[i][j] = a.pair ? *reinterpret_cast<const uint32_t*>(pj) : ((uint32_t)pj[0] | ((uint32_t)pj[1] << 16));
            }
        }
    };
    auto write_row = [&](int pl) __attribute__((always_inline)) {
        unsigned char* pb = lds + pl * a.plane;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (!sv[i]) continue;
            *reinterpret_cast<uint4*>(pb + sl0[i]) = make_uint4(rpk_lo16(d[i][0], d[i][1]), rpk_lo16(d[i][2], d[i][3]),
                                                                rpk_lo16(d[i][4], d[i][5]), rpk_lo16(d[i][6], d[i][7]));
            *reinterpret_cast<uint4*>(pb + sl1[i]) = make_uint4(pk_hi16(d[i][0], d[i][1]), pk_hi16(d[i][2], d[i][3]),
                                                                pk_hi16(d[i][4], d[i][5]), pk_hi16(d[i][6], d[i][7]));
        }
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

    // acc[g][slot]: slot 0 = output row h - 1, 1 = row h, 2 = row h + 1 of the halo row h at hand
    floatx4 acc[GW][3][NT];
#pragma unroll
    for (int g = 0; g < GW; ++g)
#pragma unroll
        for (int sl = 0; sl < 3; ++sl)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[g][sl][nt] = floatx4{0.f, 0.f, 0.f, 0.f};

    // The residual of an output row takes the stores' way backwards: 16-byte pieces (128-byte runs per
    // channel) HBM -> registers, requested before the row's last MFMAs, -> the wave's transpose tile, from
    // where each lane picks its 4 pixels.  A piece is read 16 bytes at once only where it lies inside the
    // row and this lane's address is 16-byte aligned, else as 4-byte pairs (4-byte aligned; W even) or
    // 2-byte elements inside the row; what lies past the row end stays zero.
    constexpr int NPI = (C * CH + 63) / 64;  // pieces per lane
    uint4 rres[EPI ? NPI : 1];
    auto load_res = [&](int p) __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < NPI; ++it) {
            const int el = it * 64 + lane;
            const int k = el / CH, j = el % CH;
            const int qq = wave * (GW * 16) + j * 8;
            uint32_t t[4] = {0u, 0u, 0u, 0u};
            if (el < C * CH && qq < W) {
                const uint16_t* rp = e.res + (((int64_t)n * C + k) * H + p) * W + qq;
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
                    if (el < C * CH) *reinterpret_cast<uint4*>(tile + (el / CH) * TP + (el % CH) * 16) = rres[it];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
#pragma unroll
        for (int g = 0; g < GW; ++g) {
            if ((wave * GW + g) >= a.ngroups) continue;  // wave-uniform
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int k = nt * 16 + (lane & 15);
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = acc[g][0][nt][i] + bk[nt];
                if constexpr (EPI) {
                    float rv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (e.res) {  // the lane's 4 residual values, from the tile (the result goes back in place)
                        const uint2 rq = *reinterpret_cast<const uint2*>(tile + k * TP + (g * 16 + 4 * o) * 2);
                        rv[0] = __uint_as_float(rq.x << 16);
                        rv[1] = __uint_as_float(rq.x & 0xffff0000u);
                        rv[2] = __uint_as_float(rq.y << 16);
                        rv[3] = __uint_as_float(rq.y & 0xffff0000u);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (aff) v[i] = v[i] * sk[nt] + tk[nt];
                        if (e.res) v[i] += rv[i];
                        v[i] = epi_act_ct<ACT>(v[i]);
                    }
                }
                uint32_t r[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] = bf16_rne(v[i]);  // the one rounding
                *reinterpret_cast<uint2*>(tile + k * TP + (g * 16 + 4 * o) * 2) =
                    make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
            }
        }
        // the tile is this wave's own: LDS executes a wave's accesses in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int it = 0; it < (C * CH + 63) / 64; ++it) {
            const int el = it * 64 + lane;
            const int k = el / CH, j = el % CH;
            const int qq = wave * (GW * 16) + j * 8;
            if (el >= C * CH || qq >= W) continue;  // (C = 16, GW = 1: 32 pieces;) idle groups, pieces past the row end
            const uint4 t4 = *reinterpret_cast<const uint4*>(tile + k * TP + j * 16);
            uint16_t* yp = y + (((int64_t)n * C + k) * H + p) * W + qq;
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
            const bool in = h >= 0 && h < H;                 // block-uniform
            const bool inn = hr + 1 < nrows && h + 1 < H;    // the next halo row is wanted and inside
            if (inn) load_row(h + 1);
            if constexpr (EPI) {
                if (e.res && hr >= 2) load_res(p0 + hr - 2);  // block-uniform
            }
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
#pragma unroll
            for (int g = 0; g < GW; ++g)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    acc[g][0][nt] = acc[g][1][nt];
                    acc[g][1][nt] = acc[g][2][nt];
                    acc[g][2][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
                }
            __syncthreads();  // plane (hr + 1) & 1 is written, plane hr & 1 is read
        }
    };
    if constexpr (EPI)
        with_act(e.act, body);
    else
        body(std::integral_constant<int, 0>{});
}

template <int C, int GW>
hipError_t launch_rows_t(const ConvPlan& p, const B16RArgs& a, const uint16_t* x, const uint16_t* packed,
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
hipError_t launch_rows_gw(const ConvPlan& p, const B16RArgs& a, const uint16_t* x, const uint16_t* packed,
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
    static std::atomic<int> v([] {
        const char* s = getenv("PO2Q_B16_ROWS");
        return (s && atoi(s) != 0) ? 1 : 0;
    }());
    return v;
}

}  // namespace

int b16_rows_get() { return rows_switch().load(); }
int b16_rows_set(int on) { return rows_switch().exchange(on ? 1 : 0); }

int b16_rows_wmax() { return kRWmax; }

// Eligibility is a function of the geometry alone; the plan is taken only with the switch on.
bool b16_rows_plan(ConvPlan& p) {
    if (!b16_rows_get()) return false;
    if (p.groups != 1 || p.R != 3 || p.S != 3) return false;
    if (p.sh != 1 || p.sw != 1 || p.ph != 1 || p.pw != 1 || p.dh != 1 || p.dw != 1) return false;
    if (p.C != p.K || (p.C != 16 && p.C != 32)) return false;
    if (p.W % 2 != 0 || p.W > kRWmax) return false;
    const int ngroups = (p.W + 15) / 16;
    const int gpw = (ngroups + kRWaves - 1) / kRWaves;
    const int GW = gpw <= 1 ? 1 : (gpw <= 2 ? 2 : 4);
    // RB: 16 rows re-read 2 halo rows in 18; halved while the grid would leave CUs without a block
    int RB = 16;
    while (RB > 4 && (int64_t)p.N * ((p.P + RB - 1) / RB) < 1024) RB >>= 1;
    const int bands = (p.P + RB - 1) / RB;
    const int64_t blocks = (int64_t)p.N * bands;
    if (blocks > INT32_MAX) return false;
    p.kind = KIND_BF16_ROWS;
    p.CC = p.C;
    p.NT = p.C / 16;
    p.NJ = GW;
    p.TP = RB; p.TQ = p.W; p.tilesP = bands; p.tilesQ = ngroups;
    p.kblocks = 1; p.nchunks = 1;
    p.HH = RB + 2; p.WW = p.WWp = p.W + 2;
    p.steps = rows_ks(p.C);
    p.pd = kRRing;
    p.lds_bytes = (size_t)kRRing * rows_plane(p.C, p.W) + (size_t)kRWaves * p.C * rows_tpitch(GW);
    p.blocks = blocks;
    // packed bf16 fragments [tap row][k-step][nt][lane][8] -> 4-byte words
    p.packed_floats = (int64_t)3 * p.steps * p.NT * 64 * 4;
    return true;
}

void b16_rows_describe(const ConvPlan& p, char* buf, size_t len) {
    snprintf(buf, len, "kind=bf16_rows C=%d RB=%d bands=%d groups=%d ring=%d lds=%zu blocks=%lld", p.C, p.TP, p.tilesP,
             p.tilesQ, p.pd, p.lds_bytes, (long long)p.blocks);
}

hipError_t b16_rows_launch(const ConvPlan& p, const uint16_t* x, const uint16_t* packed, const uint16_t* bias,
                           uint16_t* y, hipStream_t s, const B16Epi& e) {
    B16RArgs a;
    a.N = p.N; a.H = p.H; a.W = p.W;
    a.RB = p.TP; a.bands = p.tilesP; a.ngroups = p.tilesQ;
    a.plane = rows_plane(p.C, p.W);
    a.pair = (reinterpret_cast<uintptr_t>(x) & 3u) == 0 ? 1 : 0;
    if (p.C == 16) return launch_rows_gw<16>(p, a, x, packed, bias, y, e, s);
    return launch_rows_gw<32>(p, a, x, packed, bias, y, e, s);
}

}  // namespace po2q

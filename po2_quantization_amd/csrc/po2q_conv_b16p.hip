// bf16 BasicBlock conv pair for C = 16 and C = 32 (po2q_qconv2d_pair_bf16): both 3x3 / stride 1 / pad 1
// convs of an identity block in one launch, the intermediate kept in LDS.
//
// Arithmetic: two po2q_qconv2d_fused_bf16 calls with residual = x, up to the accumulation order.
//   mid = bf16_rne(act1((acc1 + bias1) * ps1 + pb1))                 acc1 = sum of the exact products x * Q(w1)
//   y   = bf16_rne(act2((acc2 + bias2) * ps2 + pb2 + x (add_x)))     acc2 = sum of the exact products mid * Q(w2)
// Q(w) comes from the shared quant_bf16 body through pack_b16 (row layout [tap row][k-step][nt][lane][8]),
// one v_mfma_f32_16x16x32_bf16 per k-step, fp32 accumulation, one rounding per value.
//
// Walk: conv_b16_rows' (po2q_conv_b16r.hip) with the fp32 pairs' role split.
//   * one 512-thread block owns (image, band of RB output rows) across the whole width.  Waves 0 - 3 are
//     conv-1 waves, waves 4 - 7 conv-2 waves: one of each role on every SIMD.  Within a role the 16-column
//     pixel groups are dealt as in conv_b16_rows, GW consecutive groups per wave;
//   * rows are counted from the band's first x row: row index j is image row p0 - 2 + j.  Step t:
//       conv-1 waves  request x row t + 1 from HBM, multiply x row t (LDS x plane t & 3) with the three tap
//                     rows into three rotating accumulator sets, finish mid row t - 1 (epilogue 1, rounding)
//                     and write it to mid plane (t - 1) & 1, then write x row t + 1 to x plane (t + 1) & 3;
//       conv-2 waves  multiply mid row t - 2 (mid plane t & 1) with the three tap rows, finish y row t - 3
//                     (epilogue 2, the residual values held in registers since step t - 1), store it through
//                     the wave's transpose tile, then pick the residual of y row t - 2 out of x plane
//                     (t - 2) & 3 into registers;
//       one __syncthreads().
//     An x row is written at step j - 1, multiplied at step j and last read (residual) at step j + 2: four
//     planes.  A mid row is written at step j + 1 and read at step j + 2: two planes.  x is read from HBM
//     once, mid never leaves the CU;
//   * conv 1 runs transposed: A = weights, B = x (the fragment layouts of the 16x16x32 MFMA are symmetric, so
//     the row kernels' pack and plane addressing serve as they are).  A lane ends with 4 consecutive channels
//     of one pixel: one 8-byte write into the mid plane [W + 2][C], which has the x planes' layout (x_addr),
//     so conv 2 reads its A fragments exactly as conv_b16_rows reads x;
//   * rows outside the image are skipped: an x row is not loaded and not multiplied, a mid row is not computed
//     and not multiplied (conv 2 pads with zeros, never with act1(pb1)).  The planes' halo columns and zero
//     slots are written once, as zeros; conv-1 lanes past the row end write nothing;
//   * a band computes the mid rows p0 - 1 and p0 + RB it shares with its neighbours itself; tap rows whose
//     output row the band does not want are skipped (wave-uniform);
//   * stores: conv_b16_rows' (16-byte pieces, 4-byte and 2-byte fallbacks by alignment); x staging with dword
//     loads only when x is 4-byte aligned.
// LDS: 6 planes of (W + 2) * 2C + 16 bytes, 4 tiles of C * (32 GW + 16) bytes and conv 1's 12 C bytes of
// epilogue parameters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>

#include "po2q_epi.h"
#include "po2q_internal.h"
#include "po2q_quant_b16_dev.h"
#include "po2q_x3_dev.h"

namespace po2q {

namespace {

constexpr int kPThreads = 512;   // 4 conv-1 waves + 4 conv-2 waves
constexpr int kPRole = 4;        // waves per role
constexpr int kPXRing = 4, kPMRing = 2;

constexpr int pair_ks(int C) { return C == 16 ? 2 : 3; }
constexpr int pair_tpitch(int GW) { return GW * 32 + 16; }
int pair_plane(int C, int W) { return (W + 2) * 2 * C + 16; }  // + the zero slot
int pair_wmax(int C) { return C == 16 ? 256 : 128; }           // one staging item per conv-1 thread

struct B16PArgs {
    int H, W;
    int RB, bands, ngroups;
    int plane;  // bytes per LDS plane (zero slot included)
    int pair;   // dword staging: x is 4-byte aligned (W is even)
    int add_x, act1, act2;
    const uint16_t *b1, *b2;
    const float *ps1, *pb1, *ps2, *pb2;
};

__device__ __forceinline__ uint32_t ppk_lo16(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x05040100u); }

template <int C, int GW>
__global__ __launch_bounds__(kPThreads) void conv_b16_pair(const uint16_t* __restrict__ x,
                                                           const uint4* __restrict__ wpk1,
                                                           const uint4* __restrict__ wpk2,
                                                           uint16_t* __restrict__ y, B16PArgs a) {
    static_assert(C == 16 || C == 32, "C = 16 or 32");
    static_assert(GW == 1 || GW == 2 || GW == 4, "groups per wave");
    constexpr int NT = C / 16, KS = pair_ks(C), OCT = C / 8;
    constexpr int TP = pair_tpitch(GW);
    constexpr int CH = GW * 2;  // 16-byte pieces per channel of the transpose tile
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool conv2 = wave >= kPRole;  // wave-uniform
    const int rw = wave & (kPRole - 1);
    const int o = lane >> 4;
    const int W = a.W, H = a.H, PL = a.plane;
    const int64_t HW = (int64_t)H * W;

    const int band = (int)(blockIdx.x % (unsigned)a.bands);
    const int n = (int)(blockIdx.x / (unsigned)a.bands);
    const int p0 = band * a.RB;
    const int rbe = min(a.RB, H - p0);
    const int nsteps = rbe + 5;

    unsigned char* xpl = lds;                  // x ring
    unsigned char* mpl = lds + kPXRing * PL;   // mid ring
    unsigned char* tile = lds + (kPXRing + kPMRing) * PL + rw * (C * TP);  // conv-2 waves
    const int zero_off = (W + 2) * 2 * C;

    // ---- zeros, once: halo columns 0 and W + 1 and the zero slot of every plane
    if (tid < (kPXRing + kPMRing) * (2 * OCT + 1)) {
        const int pl = tid / (2 * OCT + 1), r = tid - pl * (2 * OCT + 1);
        const int off = r == 2 * OCT ? zero_off : x_addr<C>(r < OCT ? 0 : W + 1, r % OCT);
        *reinterpret_cast<uint4*>(lds + pl * PL + off) = make_uint4(0u, 0u, 0u, 0u);
    }

    // ---- this role's weight fragments [tap row][k-step][nt], resident
    const uint4* wpk = conv2 ? wpk2 : wpk1;
    bf16x8 bw[3][KS][NT];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bw[r][ks][nt] = __builtin_bit_cast(bf16x8, wpk[((r * KS + ks) * NT + nt) * 64 + lane]);

    // ---- pixel fragment addresses inside a plane (x and mid alike): plane column = image column + 1
    int aoff[GW][KS];
#pragma unroll
    for (int g = 0; g < GW; ++g) {
        const int q = min((rw * GW + g) * 16 + (lane & 15), W - 1);  // ragged / idle groups: a column inside
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if constexpr (C == 16)
                aoff[g][ks] = ks == 0 ? x_addr<16>(q + (o >> 1), o & 1) : (o < 2 ? x_addr<16>(q + 2, o) : zero_off);
            else
                aoff[g][ks] = x_addr<32>(q + ks, o);
        }
    }

    // ---- staging (conv-1 waves): one (channel octet, pixel pair) item per thread
    const int W2 = W >> 1;
    const bool sv = !conv2 && tid < OCT * W2;
    const int soc = sv ? tid / W2 : 0, sm = sv ? tid - soc * W2 : 0;
    const int64_t sg = (int64_t)(soc * 8) * HW + 2 * sm;
    const int sl0 = x_addr<C>(2 * sm + 1, soc), sl1 = x_addr<C>(2 * sm + 2, soc);
    const uint16_t* xn = x + (int64_t)n * C * HW;
    uint32_t d[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
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
        unsigned char* pb = xpl + pl * PL;
        *reinterpret_cast<uint4*>(pb + sl0) =
            make_uint4(ppk_lo16(d[0], d[1]), ppk_lo16(d[2], d[3]), ppk_lo16(d[4], d[5]), ppk_lo16(d[6], d[7]));
        *reinterpret_cast<uint4*>(pb + sl1) =
            make_uint4(pk_hi16(d[0], d[1]), pk_hi16(d[2], d[3]), pk_hi16(d[4], d[5]), pk_hi16(d[6], d[7]));
    };

    // ---- epilogue parameters.  conv 1 (transposed: a lane has the channels nt * 16 + 4 * o + i) reads its
    // 4 * NT triples from an LDS table [bias | scale | shift][C] when a mid row is finished; conv 2 (channel
    // nt * 16 + (lane & 15)) keeps its NT triples in registers
    float* ept = reinterpret_cast<float*>(lds + (kPXRing + kPMRing) * PL + kPRole * (C * TP));
    if (tid < C) {
        ept[tid] = a.b1 ? bf16_to_f(a.b1[tid]) : 0.0f;
        ept[C + tid] = a.ps1 ? a.ps1[tid] : 1.0f;
        ept[2 * C + tid] = a.pb1 ? a.pb1[tid] : 0.0f;
    }
    const bool aff = conv2 ? (a.ps2 || a.pb2) : (a.ps1 || a.pb1);
    const int act = conv2 ? a.act2 : a.act1;
    float eb[NT], es[NT], et[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int k = nt * 16 + (lane & 15);
        eb[nt] = a.b2 ? bf16_to_f(a.b2[k]) : 0.0f;
        es[nt] = a.ps2 ? a.ps2[k] : 1.0f;
        et[nt] = a.pb2 ? a.pb2[k] : 0.0f;
    }

    // acc[g][slot]: slot 0 = output row r - 1, 1 = row r, 2 = row r + 1 of the input row r at hand
    floatx4 acc[GW][3][NT];
#pragma unroll
    for (int g = 0; g < GW; ++g)
#pragma unroll
        for (int sl = 0; sl < 3; ++sl)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[g][sl][nt] = floatx4{0.f, 0.f, 0.f, 0.f};

    // the input row in plane `pb` times the tap rows whose output row r + 1 - tap lies in [lo, hi]
    auto mul_row = [&](auto second, const unsigned char* pb, int r, int lo, int hi) __attribute__((always_inline)) {
        constexpr bool kSecond = decltype(second)::value;  // conv 2: A = pixels, B = weights; conv 1 transposed
#pragma unroll
        for (int g = 0; g < GW; ++g) {
            if ((rw * GW + g) >= a.ngroups) continue;  // wave-uniform
            bf16x8 pf[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                pf[ks] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(pb + aoff[g][ks]));
#pragma unroll
            for (int tr = 0; tr < 3; ++tr) {
                const int orow = r + 1 - tr;
                if (orow < lo || orow > hi) continue;  // block-uniform
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[g][2 - tr][nt] =
                            kSecond ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[ks], bw[tr][ks][nt], acc[g][2 - tr][nt], 0, 0, 0)
                                    : __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[tr][ks][nt], pf[ks], acc[g][2 - tr][nt], 0, 0, 0);
            }
        }
    };

    // conv 1: a finished mid row -> epilogue 1, rounding, one 8-byte write per lane and channel tile
    auto emit_mid = [&](int pl) __attribute__((always_inline)) {
        unsigned char* pm = mpl + pl * PL;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float4 b4 = *reinterpret_cast<const float4*>(ept + nt * 16 + 4 * o);
            const float4 s4 = *reinterpret_cast<const float4*>(ept + C + nt * 16 + 4 * o);
            const float4 t4 = *reinterpret_cast<const float4*>(ept + 2 * C + nt * 16 + 4 * o);
            const float b[4] = {b4.x, b4.y, b4.z, b4.w}, sc[4] = {s4.x, s4.y, s4.z, s4.w}, sh[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int g = 0; g < GW; ++g) {
                if ((rw * GW + g) >= a.ngroups) continue;  // wave-uniform
                const int q = (rw * GW + g) * 16 + (lane & 15);
                uint32_t r[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float v = acc[g][0][nt][i] + b[i];
                    if (aff) v = v * sc[i] + sh[i];
                    r[i] = bf16_rne(epi_act(v, act));
                }
                if (q < W)
                    *reinterpret_cast<uint2*>(pm + x_addr<C>(q + 1, nt * 2 + (o >> 1)) + (o & 1) * 8) =
                        make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
            }
        }
    };

    // conv 2: the lane's residual values (channel nt * 16 + (lane & 15), pixels 4 * o + i of each group) out
    // of a resident x plane, two bf16 per register
    uint32_t rres[GW][NT][2];
#pragma unroll
    for (int g = 0; g < GW; ++g)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) rres[g][nt][0] = rres[g][nt][1] = 0u;
    auto load_res = [&](int pl) __attribute__((always_inline)) {
        const unsigned char* px = xpl + pl * PL;
#pragma unroll
        for (int g = 0; g < GW; ++g) {
            if ((rw * GW + g) >= a.ngroups) continue;  // wave-uniform
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int k = nt * 16 + (lane & 15);
                uint32_t t[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int q = min((rw * GW + g) * 16 + 4 * o + i, W - 1);  // past the row end: masked at the store
                    t[i] = *reinterpret_cast<const uint16_t*>(px + x_addr<C>(q + 1, k >> 3) + (k & 7) * 2);
                }
                rres[g][nt][0] = t[0] | (t[1] << 16);
                rres[g][nt][1] = t[2] | (t[3] << 16);
            }
        }
    };

    // conv 2: one finished output row: epilogue 2, rounding, transpose, stores
    auto store_row = [&](int p) __attribute__((always_inline)) {
#pragma unroll
        for (int g = 0; g < GW; ++g) {
            if ((rw * GW + g) >= a.ngroups) continue;  // wave-uniform
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int k = nt * 16 + (lane & 15);
                const float rv[4] = {__uint_as_float(rres[g][nt][0] << 16), __uint_as_float(rres[g][nt][0] & 0xffff0000u),
                                     __uint_as_float(rres[g][nt][1] << 16), __uint_as_float(rres[g][nt][1] & 0xffff0000u)};
                uint32_t r[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float v = acc[g][0][nt][i] + eb[nt];
                    if (aff) v = v * es[nt] + et[nt];
                    if (a.add_x) v += rv[i];
                    r[i] = bf16_rne(epi_act(v, act));  // the one rounding
                }
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
            const int qq = rw * (GW * 16) + j * 8;
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

    // ---- prologue: the band's first x row (index 0 = image row p0 - 2; outside for the first band)
    if (p0 >= 2) {
        load_row(p0 - 2);
        write_row(0);
    }
    __syncthreads();
    for (int t = 0; t < nsteps; ++t) {
        if (!conv2) {
            const int h = p0 - 2 + t;  // the x row at hand
            const bool in = h >= 0 && h < H && t <= rbe + 3;                 // block-uniform
            const bool inn = t + 1 <= rbe + 3 && h + 1 >= 0 && h + 1 < H;    // the next x row is wanted and inside
            if (inn) load_row(h + 1);
            if (in) mul_row(std::false_type{}, xpl + (t & 3) * PL, h, max(p0 - 1, 0), min(p0 + rbe, H - 1));
            // mid row h - 1 is complete: wanted by the band (p0 - 1 .. p0 + rbe) and inside the image
            if (t >= 2 && t <= rbe + 3 && h - 1 >= 0 && h - 1 < H) emit_mid((t - 1) & 1);
            if (inn) write_row((t + 1) & 3);
        } else if (t >= 3) {
            const int m = p0 - 4 + t;  // the mid row at hand (p0 - 1 .. p0 + rbe)
            if (m >= 0 && m < H) mul_row(std::true_type{}, mpl + (t & 1) * PL, m, p0, p0 + rbe - 1);
            if (t >= 5) store_row(m - 1);
            if (a.add_x && m >= p0 && m < p0 + rbe) load_res((t - 2) & 3);  // y row m goes out in the next step
        }
#pragma unroll
        for (int g = 0; g < GW; ++g)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                acc[g][0][nt] = acc[g][1][nt];
                acc[g][1][nt] = acc[g][2][nt];
                acc[g][2][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
            }
        __syncthreads();  // x plane (t + 1) & 3 and mid plane (t - 1) & 1 are written, the others read
    }
}

template <int C, int GW>
hipError_t launch_pair_t(const B16PairPlan& p, const B16PArgs& a, const uint16_t* x, const uint16_t* pk1,
                         const uint16_t* pk2, uint16_t* y, hipStream_t s) {
    hipLaunchKernelGGL((conv_b16_pair<C, GW>), dim3((unsigned)p.blocks), dim3(kPThreads), p.lds_bytes, s, x,
                       reinterpret_cast<const uint4*>(pk1), reinterpret_cast<const uint4*>(pk2), y, a);
    return hipGetLastError();
}

size_t pair_align256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace

// Eligibility is a function of the geometry alone: C in {16, 32}, W even and <= 256 (C = 16) / 128 (C = 32).
int b16_pair_plan(B16PairPlan& p, int64_t N, int64_t C, int64_t H, int64_t W) {
    // the geometry of either conv, and the plan the batched pack reads (the row kernels' fragment layout)
    ConvPlan& c = p.conv;
    if (!plan_geometry(c, N, C, H, W, C, 3, 3, 1, 1, 1, 1, 1, 1, 1)) return 1;
    if (C != 16 && C != 32) {
        set_error("po2q: the bf16 conv pair takes C = 16 or C = 32, got C = " + std::to_string(C));
        return 2;
    }
    if (W % 2 != 0 || W > pair_wmax((int)C)) {
        set_error("po2q: the bf16 conv pair takes an even W up to " + std::to_string(pair_wmax((int)C)) + " at C = " +
                  std::to_string(C) + ", got W = " + std::to_string(W));
        return 2;
    }
    const int ngroups = (c.W + 15) / 16;
    const int gpw = (ngroups + kPRole - 1) / kPRole;
    const int GW = gpw <= 1 ? 1 : (gpw <= 2 ? 2 : 4);
    // RB: conv_b16_rows' rule (16 rows, halved while the grid would leave CUs without a block)
    int RB = 16;
    while (RB > 4 && (int64_t)c.N * ((c.H + RB - 1) / RB) < 1024) RB >>= 1;
    const int bands = (c.H + RB - 1) / RB;
    const int64_t blocks = (int64_t)c.N * bands;
    if (blocks > INT32_MAX) {
        set_error("po2q: the bf16 conv pair: too many blocks");
        return 2;
    }
    c.taps = 9;
    c.vrx = 0; c.PS = 0; c.MI = 0; c.nts = 0; c.fp = 0; c.SB = 0; c.plane = 0;
    c.dma_d0 = c.dma_nck = c.dma_ni = c.dma_nw = c.dma_waves = c.dma_ov = 0;
    c.kind = KIND_BF16_ROWS;
    c.CC = c.C;
    c.NT = c.C / 16;
    c.NJ = GW;
    c.TP = RB; c.TQ = c.W; c.tilesP = bands; c.tilesQ = ngroups;
    c.kblocks = 1; c.nchunks = 1;
    c.HH = RB + 4; c.WW = c.WWp = c.W + 2;
    c.steps = pair_ks(c.C);
    c.pd = kPXRing;
    c.packed_floats = (int64_t)3 * c.steps * c.NT * 64 * 4;
    p.GW = GW; p.RB = RB; p.bands = bands; p.ngroups = ngroups;
    p.lds_bytes = (size_t)(kPXRing + kPMRing) * pair_plane(c.C, c.W) + (size_t)kPRole * c.C * pair_tpitch(GW) +
                  (size_t)3 * c.C * sizeof(float);
    p.blocks = blocks;
    c.lds_bytes = p.lds_bytes;
    c.blocks = blocks;
    return 0;
}

// Workspace: [conv 1: max|w| partials, packed weight][conv 2: the same], each as b16_workspace_bytes lays it out
size_t b16_pair_workspace_bytes(const B16PairPlan& p) { return 2 * pair_align256(b16_workspace_bytes(p.conv)); }

void b16_pair_describe(const B16PairPlan& p, char* buf, size_t len) {
    snprintf(buf, len, "kind=bf16_pair C=%d RB=%d bands=%d groups=%d GW=%d lds=%zu blocks=%lld", p.conv.C, p.RB, p.bands,
             p.ngroups, p.GW, p.lds_bytes, (long long)p.blocks);
}

hipError_t b16_pair_run(const B16PairPlan& p, const uint16_t* x, const uint16_t* w1, const uint16_t* w2, uint16_t* y,
                        int bits, int fsr, int mode, const uint16_t* bias1, const uint16_t* bias2, const B16Epi& e1,
                        const B16Epi& e2, int add_x, void* workspace, hipStream_t s) {
    // both weights through the batched pack: one max|w| launch (quantized modes) and one pack launch
    char* ws = reinterpret_cast<char*>(workspace);
    const size_t half = pair_align256(b16_workspace_bytes(p.conv));
    const B16PackReq reqs[2] = {{&p.conv, w1, ws, bits, fsr, mode}, {&p.conv, w2, ws + half, bits, fsr, mode}};
    const hipError_t pe = b16_pack_batch(2, reqs, s);
    if (pe != hipSuccess) return pe;
    const size_t poff = pair_align256((size_t)256 * sizeof(uint32_t));  // b16_workspace_bytes' partials block
    B16PArgs a;
    a.H = p.conv.H; a.W = p.conv.W;
    a.RB = p.RB; a.bands = p.bands; a.ngroups = p.ngroups;
    a.plane = pair_plane(p.conv.C, p.conv.W);
    a.pair = (reinterpret_cast<uintptr_t>(x) & 3u) == 0 ? 1 : 0;
    a.add_x = add_x ? 1 : 0; a.act1 = e1.act; a.act2 = e2.act;
    a.b1 = bias1; a.b2 = bias2;
    a.ps1 = e1.ps; a.pb1 = e1.pb; a.ps2 = e2.ps; a.pb2 = e2.pb;
    const uint16_t* pk1 = reinterpret_cast<const uint16_t*>(ws + poff);
    const uint16_t* pk2 = reinterpret_cast<const uint16_t*>(ws + half + poff);
    if (p.conv.C == 16) {
        switch (p.GW) {
            case 1: return launch_pair_t<16, 1>(p, a, x, pk1, pk2, y, s);
            case 2: return launch_pair_t<16, 2>(p, a, x, pk1, pk2, y, s);
            case 4: return launch_pair_t<16, 4>(p, a, x, pk1, pk2, y, s);
            default: return hipErrorInvalidValue;
        }
    }
    switch (p.GW) {
        case 1: return launch_pair_t<32, 1>(p, a, x, pk1, pk2, y, s);
        case 2: return launch_pair_t<32, 2>(p, a, x, pk1, pk2, y, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace po2q

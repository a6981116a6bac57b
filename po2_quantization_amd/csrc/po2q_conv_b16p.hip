// bf16 BasicBlock conv pair for C = 16 and C = 32 (po2q_qconv2d_pair_bf16): both 3x3 / stride 1 / pad 1
// convs of an identity block in one launch, the intermediate kept in LDS.
//
// Arithmetic: two po2q_qconv2d_fused_bf16 calls with residual = x, up to the accumulation order.
//   mid = bf16_rne(act1((acc1 + bias1) * ps1 + pb1))                 acc1 = sum of the exact products x * Q(w1)
//   y   = bf16_rne(act2((acc2 + bias2) * ps2 + pb2 + x (add_x)))     acc2 = sum of the exact products mid * Q(w2)
// Q(w) comes from the shared quant_bf16 body through pack_b16 (row layout [tap row][k-step][nt][lane][8]),
// one v_mfma_f32_16x16x32_bf16 per k-step, fp32 accumulation, one rounding per value.
//
// Walk: conv_b16_rows' (po2q_conv_b16r.hip) with the fp32 pairs' role split; staging, zero slot and stores are
// po2q_b16_rows_dev.h's and are described there.
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
//   * the residual is x itself and never comes from HBM a second time: a lane picks it out of the x ring.
// LDS: 6 planes of (W + 2) * 2C + 16 bytes, 4 tiles of C * (32 GW + 16) bytes and conv 1's 12 C bytes of
// epilogue parameters.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

#include "po2q_b16_rows_dev.h"

namespace po2q {

namespace {

constexpr int kPThreads = 512;        // 4 conv-1 waves + 4 conv-2 waves
constexpr int kPRole = kB16RowWaves;  // waves per role
constexpr int kPXRing = 4, kPMRing = 2;

int pair_wmax(int C) { return C == 16 ? 256 : 128; }  // one staging item per conv-1 thread

struct B16PArgs {
    int H, W;
    int RB, bands, ngroups;
    int plane;  // bytes per LDS plane (zero slot included)
    int pair;   // dword staging: x is 4-byte aligned (W is even)
    int add_x, act1, act2;
    const uint16_t *b1, *b2;
    const float *ps1, *pb1, *ps2, *pb2;
};

template <int C, int GW>
__global__ __launch_bounds__(kPThreads) void conv_b16_pair(const uint16_t* __restrict__ x,
                                                           const uint4* __restrict__ wpk1,
                                                           const uint4* __restrict__ wpk2,
                                                           uint16_t* __restrict__ y, B16PArgs a) {
    static_assert(C == 16 || C == 32, "C = 16 or 32");
    static_assert(GW == 1 || GW == 2 || GW == 4, "groups per wave");
    constexpr int NT = C / 16, KS = b16_rows_ks(C);
    constexpr int TP = b16_rows_tpitch(GW);
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

    zero_planes<C, true>(lds, kPXRing + kPMRing, PL, W, zero_off, tid);

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
        for (int ks = 0; ks < KS; ++ks) aoff[g][ks] = frag_off<C>(q, ks, o, zero_off);
    }

    // ---- staging (conv-1 waves): one (channel octet, pixel pair) item per thread
    const int W2 = W >> 1;
    B16Stage st;
    st.v = !conv2 && tid < C / 8 * W2;
    const int soc = st.v ? tid / W2 : 0, sm = st.v ? tid - soc * W2 : 0;
    st.g = (int64_t)(soc * 8) * HW + 2 * sm;
    st.l0 = x_addr<C>(2 * sm + 1, soc);
    st.l1 = x_addr<C>(2 * sm + 2, soc);
    const uint16_t* xn = x + (int64_t)n * C * HW;
    uint32_t d[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    auto load_row = [&](int h) __attribute__((always_inline)) { stage_load(st, xn + (int64_t)h * W, HW, a.pair, d); };
    auto write_row = [&](int pl) __attribute__((always_inline)) { stage_write(st, xpl + pl * PL, d); };

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
                *reinterpret_cast<uint2*>(tile + k * TP + (g * 16 + 4 * o) * 2) =
                    finish4(acc[g][0][nt], eb[nt], aff, es[nt], et[nt], a.add_x, rres[g][nt][0], rres[g][nt][1], act);
            }
        }
        tile_fence();
        // the drain loop stays here: through tile_drain's for_pieces it measured 1.5 % slower on <16, 4> and 1 % on
        // <32, 2> (profiles/bf16_rows_helpers_bisect.jsonl, arm "tile_drain")
#pragma unroll
        for (int it = 0; it < pieces_per_lane(C, CH); ++it) {
            const int el = it * 64 + lane;
            const int k = el / CH, j = el % CH;
            const int qq = rw * (GW * 16) + j * 8;
            if (el >= C * CH || qq >= W) continue;  // (C = 16, GW = 1: 32 pieces;) idle groups, pieces past the row end
            const uint4 t4 = *reinterpret_cast<const uint4*>(tile + k * TP + j * 16);
            store_piece(y + (((int64_t)n * C + k) * H + p) * W + qq, t4, qq, W);
        }
        tile_fence<false>();
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
        rotate_acc(acc);
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
    c.taps = 9;
    c.vrx = 0; c.PS = 0; c.MI = 0; c.nts = 0; c.fp = 0; c.SB = 0; c.plane = 0;
    c.dma_d0 = c.dma_nck = c.dma_ni = c.dma_nw = c.dma_waves = c.dma_ov = 0;
    // 4 x planes + 2 mid planes, conv 1's epilogue table behind the tiles; a band reads 2 x rows either side
    if (!fill_rows_plan(c, KIND_BF16_ROWS, kPXRing, kPXRing + kPMRing, 4, (size_t)3 * c.C * sizeof(float))) {
        set_error("po2q: the bf16 conv pair: too many blocks");
        return 2;
    }
    p.GW = c.NJ; p.RB = c.TP; p.bands = c.tilesP; p.ngroups = c.tilesQ;
    p.lds_bytes = c.lds_bytes;
    p.blocks = c.blocks;
    return 0;
}

// Workspace: [conv 1: max|w| partials, packed weight][conv 2: the same], each as b16_workspace_bytes lays it out
// (a multiple of 256 bytes, so the second half is aligned as the first)
size_t b16_pair_workspace_bytes(const B16PairPlan& p) { return 2 * b16_workspace_bytes(p.conv); }

void b16_pair_describe(const B16PairPlan& p, char* buf, size_t len) {
    snprintf(buf, len, "kind=bf16_pair C=%d RB=%d bands=%d groups=%d GW=%d lds=%zu blocks=%lld", p.conv.C, p.RB, p.bands,
             p.ngroups, p.GW, p.lds_bytes, (long long)p.blocks);
}

hipError_t b16_pair_run(const B16PairPlan& p, const uint16_t* x, const uint16_t* w1, const uint16_t* w2, uint16_t* y,
                        int bits, int fsr, int mode, const uint16_t* bias1, const uint16_t* bias2, const B16Epi& e1,
                        const B16Epi& e2, int add_x, void* workspace, hipStream_t s) {
    // both weights through the batched pack: one max|w| launch (quantized modes) and one pack launch
    char* ws = reinterpret_cast<char*>(workspace);
    const size_t half = b16_workspace_bytes(p.conv);
    const B16PackReq reqs[2] = {{&p.conv, w1, ws, bits, fsr, mode}, {&p.conv, w2, ws + half, bits, fsr, mode}};
    const hipError_t pe = b16_pack_batch(2, reqs, s);
    if (pe != hipSuccess) return pe;
    const size_t poff = b16_packed_offset();
    B16PArgs a;
    a.H = p.conv.H; a.W = p.conv.W;
    a.RB = p.RB; a.bands = p.bands; a.ngroups = p.ngroups;
    a.plane = b16_rows_plane(p.conv.C, p.conv.W);
    a.pair = b16_dword_aligned(x);
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

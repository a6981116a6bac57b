// The stage-3 conv pair (C = 64 -> 64 -> 64, 3x3 / stride 1 / pad 1, 32 < W <= 64) as one launch:
//   y = Q(w2) * (Q(w1) * x)         (plain form: scale * acc, + bias where given)
// two consecutive QuantizedConv2d.forward calls (reference models/quantized_conv.py:32-38) of a
// ResNet56 stage-3 run, the intermediate activation kept on chip.  conv_pairw's role split
// (po2q_conv_pairw.hip) with conv_rowsk<64>'s waves over the output channels (po2q_conv_rowsk.hip):
//   * a block owns (image, segment of rows) and full rows (64 padded columns: 4 groups of 16, 3 when
//     W <= 48); 8 waves = role x output-channel tile.  Waves 0-3 ("B") run conv 1 for channels
//     16t .. 16t+15, waves 4-7 ("A") conv 2 for the same tile; wave t and t + 4 share a SIMD and run in
//     opposite phases (A's MFMAs beside B's epilogue / split, B's MFMAs beside A's stores);
//   * each wave keeps its conv's 18 B fragments (72 VGPRs) for the kernel's lifetime, loaded from the
//     fragments launch_pack_bf16x3_batch wrote (conv_rowsk's pack layout): no weight staging here;
//   * B, per step: LDS-DMA its 16 channels of an x row into a 2-slot raw ring, the exact split of the
//     NEXT row's 16 channels into the double-buffered hi / mid / lo x planes, conv 1's MFMAs of this row
//     (transposed: A = weights, so a lane ends with 4 consecutive channels of one pixel) on three
//     rotating accumulator sets, every A fragment feeding the three tap rows; one step later epilogue 1
//     goes through the exact split straight into a 2-slot intermediate plane ring -- zeros for rows
//     outside the image and columns >= W (conv 2's padding), recomputed rows at a segment's halo;
//   * A, per step: conv 2's MFMAs from that ring, epilogue 2 and the stores, two groups' values
//     exchanged by one row_ror:8 DPP move each so a store covers whole 128-byte runs;
//   * one s_barrier per step, the same count in both roles through the fill and drain steps;
//   * PIPE (the default): B issues that vector work in slices between its own MFMAs (mfmas_pipe), so both
//     waves of a SIMD offer the matrix pipe MFMAs for the whole step; without it (PO2Q_PAIR64_PIPE=0) all
//     of it comes in front of the MFMAs.  Same values either way.
// Per accumulator the order is conv_rowsk's (tap row, then k-step, then plane) and the epilogue its
// expression: the output equals two conv_rowsk launches bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>

#include "../../include/po2q.h"
#include "po2q_internal.h"
#include "po2q_rows_dev.h"
#include "po2q_x3_dev.h"

namespace po2q {

namespace {
constexpr int kP6C = 64;                        // channels (C = K)
constexpr int kP6Wp = 64;                       // padded row width: 4 groups of 16 columns
constexpr int kP6PL = (kP6Wp + 2) * 2 * kP6C;   // one bf16 plane row: [66 px][64 ch] (columns -1 .. 64)
constexpr int kP6Set = 3 * kP6PL;               // hi / mid / lo
constexpr int kP6Raw = kP6C * kP6Wp * 4;        // a raw x slot: [64 ch][64 px] fp32
constexpr int kP6RPB = kP6Wp * 4;               // raw row pitch
constexpr int kP6PD = 2;                        // raw ring slots
constexpr int kP6KS = 6;                        // k-steps per tap row: 2 chunks of 32 channels x 3 taps
constexpr int kP6Lds = kP6PD * kP6Raw + 2 * kP6Set + 2 * kP6Set;
constexpr int kP6PackBytes = 3 * kP6KS * 4 * 64 * 16;  // one conv's packed fragments

// byte offset of channel octet oc of padded pixel P (column P - 1) in a plane: 128 bytes per pixel,
// octets XOR-swizzled by the pixel (conv_rowsk's k_addr<64>)
__device__ __forceinline__ int p6_addr(int P, int oc) { return P * 128 + ((oc ^ (P & 7)) << 4); }

// f(integral_constant<int, 0>), ..., f(integral_constant<int, N - 1>) in order
template <class F, int... R>
__device__ __forceinline__ void p6_unroll(F&& f, std::integer_sequence<int, R...>) {
    (f(std::integral_constant<int, R>{}), ...);
}
}  // namespace

struct Pair64Args {
    int N, H, W;
    int RB, nseg, items, remap;
    const uint4* wp1;  // packed B fragments [r][ks][nt][lane] of conv 1 / conv 2
    const uint4* wp2;
    const float* s1;   // the convs' max|w| multipliers
    const float* s2;
    const float* b1;   // conv biases (NULL: none)
    const float* b2;
};

// NG: 16-column groups per row (4, or 3 when W <= 48: a group wholly past W issues no MFMAs);
// NTS bit 0: non-temporal stores, bit 1: non-temporal x loads.
// PIPE: the conv-1 waves issue their vector work (x DMAs, epilogue 1, the split of the next row) in
// slices between their own MFMAs instead of in front of them; same values, same order per accumulator.
template <int NG, int NTS, bool PIPE>
__global__ __launch_bounds__(512, 1) void conv_pair64(const float* __restrict__ x, float* __restrict__ y,
                                                      Pair64Args a) {
    static_assert(NG == 3 || NG == 4, "column groups");
    constexpr int C = kP6C, KS = kP6KS, PL = kP6PL, SET = kP6Set, RPB = kP6RPB;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool roleA = wave >= 4;  // wave-uniform: conv 2 (A) or conv 1 (B)
    const int t = wave & 3;        // output-channel tile
    unsigned char* raw = lds;                    // 2 x [64][64] fp32
    unsigned char* xp = raw + kP6PD * kP6Raw;    // 2 x 3 planes: x
    // (then 2 x 3 planes: the intermediate)

    int blk = blockIdx.x;
    if (a.remap) blk = (blk & 7) * (int)(gridDim.x >> 3) + (blk >> 3);
    if (blk >= a.items) return;  // block-uniform
    const int seg = blk % a.nseg;
    const int n = blk / a.nseg;
    const int p0 = seg * a.RB;
    const int rbe = min(a.RB, a.H - p0);
    const int nx = rbe + 4;  // x rows p0-2 .. p0+rbe+1
    const int n1 = rbe + 2;  // intermediate rows p0-1 .. p0+rbe
    // epilogue 1 of a step runs in the NEXT step, so conv 2 takes intermediate row j - 4 at step j and
    // output row p0 + o completes at step o + 6
    const int nsteps = nx + 2;
    const int HW = a.H * a.W;

    // ---- this wave's conv: B fragments bw[r][ks = chunk * 3 + s], scale, bias
    bf16x8 bw[3][KS];
    {
        const uint4* wp = roleA ? a.wp2 : a.wp1;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) bw[r][ks] = __builtin_bit_cast(bf16x8, wp[((r * KS + ks) * 4 + t) * 64 + lane]);
    }
    float scale = *(roleA ? a.s2 : a.s1);
    // B (transposed): lane = pixel lane & 15, channels 16t + 4 (lane >> 4) + e; A: channel 16t + (lane & 15)
    float bk[4];
    {
        const float* b = roleA ? a.b2 : a.b1;
#pragma unroll
        for (int e = 0; e < 4; ++e) bk[e] = b ? b[roleA ? 16 * t + (lane & 15) : 16 * t + 4 * (lane >> 4) + e] : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("s_waitcnt vmcnt(0)" : "+v"(bw[r][ks]));
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(scale), "+v"(bk[0]), "+v"(bk[1]), "+v"(bk[2]), "+v"(bk[3]));

    // the plane sets start as zeros: the padding columns -1 and 64 of both, every intermediate row
    // conv 2 reads before epilogue 1 has written it, the columns of a group NG == 3 leaves out
    for (int e = tid; e < (4 * SET) / 16; e += 512) reinterpret_cast<uint4*>(xp)[e] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();

    // ---- B: x DMA, instruction i, lane l -> channel 16t + 4i + (l >> 4), columns 4 (l & 15) .. + 3 at
    // raw[c][col] (columns >= W load out of range: zeros)
    const __amdgpu_buffer_rsrc_t rs = rows_rsrc(x + (int64_t)n * C * HW, C * HW * 4);
    uint32_t vi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = 16 * t + 4 * i + (lane >> 4), q = 4 * (lane & 15);
        vi[i] = q < a.W ? ((uint32_t)c * (uint32_t)HW + (uint32_t)q) * 4u : 0x7fffffffu;
    }
    const uint32_t raw_lds = (uint32_t)(uintptr_t)raw;
    auto load_x1 = [&](int sl, int jn, int i) __attribute__((always_inline)) {  // DMA instruction i of a row
        const int h = p0 - 2 + jn;
        const bool hok = jn < nx && h >= 0 && h < a.H;
        const uint32_t roff = (uint32_t)(hok ? h : 0) * (uint32_t)a.W * 4u;
        const uint32_t base = raw_lds + (uint32_t)(sl * kP6Raw) + (uint32_t)(16 * t) * (uint32_t)RPB;
        rows_dma16<(NTS & 2) != 0>(rs, (hok && vi[i] != 0x7fffffffu) ? vi[i] + roff : 0x7fffffffu, 0u,
                                   base + (uint32_t)i * 1024u);
    };
    auto load_x = [&](int sl, int jn) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) load_x1(sl, jn, i);
    };
    // LDS addresses: one per-lane base VGPR per access pattern, opaque to the compiler, + compile-time
    // offsets that fit the instructions' 16-bit immediates (the regions past 64 KiB otherwise cost an
    // address VGPR per access, hoisted out of the loop and spilled)
    // ---- B: the exact split of this wave's 16 channels of a raw row: lane = column, octets 2t, 2t + 1
    int xwb[2] = {p6_addr(lane + 1, 2 * t) + kP6PD * kP6Raw, p6_addr(lane + 1, 2 * t + 1) + kP6PD * kP6Raw};
    asm volatile("" : "+v"(xwb[0]), "+v"(xwb[1]));
    auto split_rd = [&](const unsigned char* rw, int o, uint32_t (&b8)[8]) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            b8[e] = *reinterpret_cast<const uint32_t*>(rw + (16 * t + 8 * o + e) * RPB + lane * 4);
    };
    auto split_wr = [&](int o, int pb, const uint32_t (&b8)[8]) __attribute__((always_inline)) {
        uint4 hi, mid, lo;
        split3(b8, hi, mid, lo);
        unsigned char* pw = lds + (xwb[o] + pb);
        *reinterpret_cast<uint4*>(pw) = hi;
        *reinterpret_cast<uint4*>(pw + PL) = mid;
        *reinterpret_cast<uint4*>(pw + 2 * PL) = lo;
    };
    auto split_x = [&](const unsigned char* rw, int pb) __attribute__((always_inline)) {
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            uint32_t b8[8];
            split_rd(rw, o, b8);
            split_wr(o, pb, b8);
        }
    };

    // A-fragment addresses (one b128 each), the same in the x planes and the intermediate planes: k-step
    // ks = chunk * 3 + s of group grp reads pixel 16 grp + p + s, octet 4 chunk + g -- the swizzle depends
    // on the pixel's low 3 bits only, so a group is a constant 2 KiB apart
    int foff[KS];
    {
        const int p = lane & 15, g = lane >> 4;
        const int region = kP6PD * kP6Raw + (roleA ? 2 * SET : 0);  // B reads the x planes, A the intermediate
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            foff[ks] = p6_addr(p + ks % 3, 4 * (ks / 3) + g) + region;
            asm volatile("" : "+v"(foff[ks]));
        }
    }
    // epilogue 1: pixel 16 grp + p + 1, channels 16t + 4g .. + 3 (a group is 2 KiB apart here too)
    int ywb = p6_addr((lane & 15) + 1, 2 * t + (lane >> 5)) + 8 * ((lane >> 4) & 1) + kP6PD * kP6Raw + 2 * SET;
    asm volatile("" : "+v"(ywb));

    floatx4 acc[3][NG];
#pragma unroll
    for (int sl = 0; sl < 3; ++sl)
#pragma unroll
        for (int grp = 0; grp < NG; ++grp) acc[sl][grp] = floatx4{0.f, 0.f, 0.f, 0.f};

    // The MFMAs of one split row: row j feeds output row j (tap row 0), j - 1 (1) and j - 2 (2) in the
    // accumulator slots SL of step S.  TR (B, conv 1): transposed.  Per accumulator the MFMAs come k-step
    // outer, plane inner, as in conv_rowsk (there the tap rows are the middle loop, here the innermost:
    // different accumulators, so each one sees the same sequence).
    auto mfmas = [&](auto S_, auto TR_, int pb) __attribute__((always_inline)) {
        constexpr int S = decltype(S_)::value;
        constexpr bool TR = decltype(TR_)::value;
        constexpr int SL[3] = {(S + 1) % 3, S, (S + 2) % 3};
        // stage st = (ks, plane): NG fragment reads, each feeding the three tap rows; the reads of stage
        // st + 1 go out before the 3 NG MFMAs of stage st (two fragment sets: 8 NG VGPRs)
        bf16x8 af[2][NG];
        auto ldf = [&](bf16x8 (&f)[NG], int st) __attribute__((always_inline)) {
#pragma unroll
            for (int grp = 0; grp < NG; ++grp)
                f[grp] = __builtin_bit_cast(
                    bf16x8, *reinterpret_cast<const uint4*>(lds + (foff[st / 3] + (pb + (st % 3) * PL + grp * (16 * 128)))));
        };
        ldf(af[0], 0);
#pragma unroll
        for (int st = 0; st < 3 * KS; ++st) {
            if (st + 1 < 3 * KS) ldf(af[(st + 1) & 1], st + 1);
            const int ks = st / 3;
#pragma unroll
            for (int rr = 0; rr < 3; ++rr)
#pragma unroll
                for (int grp = 0; grp < NG; ++grp)
                    acc[SL[rr]][grp] =
                        TR ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[rr][ks], af[st & 1][grp], acc[SL[rr]][grp], 0, 0, 0)
                           : __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[st & 1][grp], bw[rr][ks], acc[SL[rr]][grp], 0, 0, 0);
            // keeps the scheduler from hoisting later stages' reads (it spilled to hold them)
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // The same MFMAs (conv 1, transposed) with the step's vector slices between them: pre(st) runs in
    // front of stage st's fragment reads (the DMA issues: their lgkmcnt(0) then finds no read in flight
    // but the ones the stage's MFMAs wait for anyway), hook(3 st + rr) after the NG MFMAs of tap row rr.
    // One scheduling region per tap row keeps the emitted order.
    auto mfmas_pipe = [&](auto S_, int pb, auto&& pre, auto&& hook) __attribute__((always_inline)) {
        constexpr int S = decltype(S_)::value;
        constexpr int SL[3] = {(S + 1) % 3, S, (S + 2) % 3};
        bf16x8 af[2][NG];
        auto ldf = [&](bf16x8 (&f)[NG], int st) __attribute__((always_inline)) {
#pragma unroll
            for (int grp = 0; grp < NG; ++grp)
                f[grp] = __builtin_bit_cast(
                    bf16x8, *reinterpret_cast<const uint4*>(lds + (foff[st / 3] + (pb + (st % 3) * PL + grp * (16 * 128)))));
        };
        ldf(af[0], 0);
        auto stage = [&](auto ST_) __attribute__((always_inline)) {
            constexpr int st = decltype(ST_)::value;
            constexpr int ks = st / 3;
            pre(ST_);
            if constexpr (st + 1 < 3 * KS) ldf(af[(st + 1) & 1], st + 1);
            __builtin_amdgcn_sched_barrier(0);
            auto row = [&](auto RR_) __attribute__((always_inline)) {
                constexpr int rr = decltype(RR_)::value;
#pragma unroll
                for (int grp = 0; grp < NG; ++grp)
                    acc[SL[rr]][grp] =
                        __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[rr][ks], af[st & 1][grp], acc[SL[rr]][grp], 0, 0, 0);
                hook(std::integral_constant<int, 3 * st + rr>{});
                __builtin_amdgcn_sched_barrier(0);
            };
            p6_unroll(row, std::make_integer_sequence<int, 3>{});
        };
        p6_unroll(stage, std::make_integer_sequence<int, 3 * KS>{});
    };

    // B: conv 1's completed accumulator slot, held until the next step's epilogue 1
    floatx4 pend[NG];
#pragma unroll
    for (int grp = 0; grp < NG; ++grp) pend[grp] = floatx4{0.f, 0.f, 0.f, 0.f};

    // ---- B, step j: refill the raw slot of row j with row j + 2, epilogue 1 of intermediate row j - 3
    // (pend, completed at step j - 1) into ring slot (j + 1) & 1, the split of x row j + 1 into the other
    // x plane set, conv 1 on row j (split in step j - 1)
    auto stepB = [&](auto S_, int j) __attribute__((always_inline)) {
        constexpr int S6 = decltype(S_)::value;
        constexpr int S = S6 % 3;
        constexpr int D = (S + 2) % 3;    // the accumulator slot that completes
        constexpr int B2 = S6 & 1;        // x plane set of row j, raw slot of rows j and j + 2
        // everyone's reads of the sets written below have retired; row j's planes are published
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        const int i1 = j - 3;
        const int r1 = p0 - 1 + i1;
        const bool irow = i1 >= 0 && i1 < n1 && r1 >= 0 && r1 < a.H;
        unsigned char* yw = lds + (ywb + (1 - B2) * SET);
        auto epi1 = [&](int grp) __attribute__((always_inline)) {
            const int q = 16 * grp + (lane & 15);  // lane: pixel q, channels 16t + 4g .. + 3
            const bool okq = irow && q < a.W;
            uint32_t b4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = pend[grp][e] * scale + bk[e];
                b4[e] = okq ? __float_as_uint(v) : 0u;  // conv 2's zero padding
            }
            uint2 h2, m2, l2;
            split4p(b4, h2, m2, l2);
            unsigned char* yg = yw + grp * (16 * 128);
            *reinterpret_cast<uint2*>(yg) = h2;
            *reinterpret_cast<uint2*>(yg + PL) = m2;
            *reinterpret_cast<uint2*>(yg + 2 * PL) = l2;
        };
        // x rows outside the image / segment are zeros: their MFMAs would add exact zeros
        const int hx = p0 - 2 + j;
        const bool xrow = j < nx && hx >= 0 && hx < a.H;
        if constexpr (!PIPE) {
            load_x(B2, j + 2);
#pragma unroll
            for (int grp = 0; grp < NG; ++grp) epi1(grp);
            rows_wait<4>();  // this wave's DMAs of row j + 1 have landed (row j + 2's may fly)
            split_x(raw + (1 - B2) * kP6Raw, (1 - B2) * SET);
            if (xrow) mfmas(std::integral_constant<int, S>{}, std::true_type{}, B2 * SET);
        } else {
            // the same work as slices: DMA i in front of stage i; epilogue-1 tile v after MFMA slot 2 v + 1;
            // then (all four DMAs issued) the counted wait and the raw reads of octet 0, its split two slots
            // later, and the same for octet 1.  Nothing here touches what this step's MFMAs (either role's)
            // read: the ring slot and the plane set written are the ones read in the NEXT step.
            uint32_t b8[8];
            const unsigned char* rw = raw + (1 - B2) * kP6Raw;
            auto pre = [&](auto ST_) __attribute__((always_inline)) {
                constexpr int st = decltype(ST_)::value;
                if constexpr (st < 4) load_x1(B2, j + 2, st);
            };
            auto hook = [&](auto K_) __attribute__((always_inline)) {
                constexpr int K = decltype(K_)::value;
                if constexpr (K % 2 == 1 && K / 2 < NG) epi1(K / 2);
                if constexpr (K == 10) {
                    rows_wait<4>();  // this wave's DMAs of row j + 1 have landed (row j + 2's may fly)
                    split_rd(rw, 0, b8);
                }
                if constexpr (K == 12) split_wr(0, (1 - B2) * SET, b8);
                if constexpr (K == 13) split_rd(rw, 1, b8);
                if constexpr (K == 15) split_wr(1, (1 - B2) * SET, b8);
            };
            static_assert(2 * (NG - 1) + 1 < 10, "epilogue-1 tiles come before the split");
            if (xrow) {
                mfmas_pipe(std::integral_constant<int, S>{}, B2 * SET, pre, hook);
            } else {  // no MFMAs to hide under: the slices in the same order
                p6_unroll(pre, std::make_integer_sequence<int, 4>{});
                p6_unroll(hook, std::make_integer_sequence<int, 16>{});
            }
        }
#pragma unroll
        for (int grp = 0; grp < NG; ++grp) {
            pend[grp] = acc[D][grp];
            acc[D][grp] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
    };

    const __amdgpu_buffer_rsrc_t ry = rows_rsrc(y + (int64_t)n * C * HW, C * HW * 4);

    // ---- A, step j: conv 2 on intermediate row j - 4 (ring slot j & 1), then epilogue 2 of output row
    // j - 6: lane L holds pixels 4g .. 4g + 3 of each group for channel 16t + (L & 15); one row_ror:8 DPP
    // move per value gives store a channels 0-7 and store b channels 8-15 of the tile over two groups
    auto stepA = [&](auto S_, int j) __attribute__((always_inline)) {
        constexpr int S6 = decltype(S_)::value;
        constexpr int S = S6 % 3;
        constexpr int D = (S + 2) % 3;
        constexpr int YR = S6 & 1;
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // + B's epilogue-1 writes
        {
            // intermediate rows outside the image / segment were written as zeros: skipped
            const int i2 = j - 4, r2 = p0 - 1 + i2;
            if (i2 >= 0 && i2 < n1 && r2 >= 0 && r2 < a.H)
                mfmas(std::integral_constant<int, S>{}, std::false_type{}, YR * SET);
        }
        const int o = j - 6;
        const bool orow = o >= 0 && o < rbe;
        const int g = lane >> 4;
        const uint32_t ca = (uint32_t)(16 * t) + (uint32_t)(lane & 7), cb = ca + 8u;
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            floatx4 vv[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int grp = 2 * pr + h;
                if (grp < NG) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) vv[h][e] = acc[D][grp][e] * scale + bk[0];
                    acc[D][grp] = floatx4{0.f, 0.f, 0.f, 0.f};
                } else {
                    vv[h] = floatx4{0.f, 0.f, 0.f, 0.f};
                }
            }
            floatx4 sa, sb;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sa[e] = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(vv[0][e]), __float_as_int(vv[1][e]),
                                                                   0x128, 0xf, 0xc, false));
                sb[e] = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(vv[1][e]), __float_as_int(vv[0][e]),
                                                                   0x128, 0xf, 0x3, false));
            }
            const int qs = 32 * pr + ((lane & 8) ? 16 : 0) + 4 * g;
            const bool ok = orow && qs < a.W;
            const uint32_t rowoff = (uint32_t)(orow ? p0 + o : 0) * (uint32_t)a.W + (uint32_t)qs;
            rows_store<(NTS & 1) != 0>(ry, ok ? (ca * (uint32_t)HW + rowoff) * 4u : 0x7fffffffu, sa);
            rows_store<(NTS & 1) != 0>(ry, ok ? (cb * (uint32_t)HW + rowoff) * 4u : 0x7fffffffu, sb);
        }
    };

    if (roleA) {
        for (int j = 0; j < nsteps; j += 6) {
            stepA(std::integral_constant<int, 0>{}, j);
            stepA(std::integral_constant<int, 1>{}, j + 1);
            stepA(std::integral_constant<int, 2>{}, j + 2);
            if (j + 3 >= nsteps) break;
            stepA(std::integral_constant<int, 3>{}, j + 3);
            stepA(std::integral_constant<int, 4>{}, j + 4);
            stepA(std::integral_constant<int, 5>{}, j + 5);
        }
    } else {
        // rows 0 and 1 in flight, row 0 split: step 0's barrier publishes its planes
        load_x(0, 0);
        load_x(1, 1);
        rows_wait<4>();
        split_x(raw, 0);
        for (int j = 0; j < nsteps; j += 6) {
            stepB(std::integral_constant<int, 0>{}, j);
            stepB(std::integral_constant<int, 1>{}, j + 1);
            stepB(std::integral_constant<int, 2>{}, j + 2);
            if (j + 3 >= nsteps) break;
            stepB(std::integral_constant<int, 3>{}, j + 3);
            stepB(std::integral_constant<int, 4>{}, j + 4);
            stepB(std::integral_constant<int, 5>{}, j + 5);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // trailing DMAs / stores land before the wave ends
}

// ------------------------------------------------------------------- host side --
bool pair64_enabled() {
    const char* e = getenv("PO2Q_PAIR64");
    return !(e && e[0] == '0');
}

bool pair64_geom_ok(int64_t N, int64_t C, int64_t H, int64_t W) {
    return C == kP6C && W > 32 && W <= kP6Wp && W % 4 == 0 && N > 0 && H > 0 && C * H * W * 4 < (1LL << 31) &&
           N * H <= INT_MAX / 2;
}

size_t pair64_pack_bytes() { return (size_t)kP6PackBytes; }

hipError_t pair64_launch(const float* x, float* y, int64_t N, int64_t H, int64_t W, const uint16_t* packed1,
                         const float* scale1, const uint16_t* packed2, const float* scale2, const float* bias1,
                         const float* bias2, hipStream_t s) {
    if (!pair64_geom_ok(N, kP6C, H, W)) return hipErrorInvalidValue;
    // one block per CU at bs 256; fewer images: segments of at least 8 rows (the halo rows of a segment
    // are recomputed).  PO2Q_PAIR64_NSEG forces the segment count (test knob)
    int64_t nseg = std::max<int64_t>(1, (256 + N - 1) / N);
    nseg = std::min<int64_t>(nseg, std::max<int64_t>(1, H / 8));
    if (const char* e = getenv("PO2Q_PAIR64_NSEG")) nseg = std::min<int64_t>(std::max(1, atoi(e)), H);
    Pair64Args a;
    a.N = (int)N; a.H = (int)H; a.W = (int)W;
    a.RB = (int)((H + nseg - 1) / nseg);
    a.nseg = (int)((H + a.RB - 1) / a.RB);
    const int64_t items = N * a.nseg;
    if (items > INT_MAX / 2) return hipErrorInvalidValue;
    const int blocks = (int)((items + 7) / 8 * 8);
    a.items = (int)items;
    a.remap = 1;
    a.wp1 = reinterpret_cast<const uint4*>(packed1);
    a.wp2 = reinterpret_cast<const uint4*>(packed2);
    a.s1 = scale1; a.s2 = scale2;
    a.b1 = bias1; a.b2 = bias2;
    // temporal x loads and y stores: inside a stage-3 run a pair's 205 MB output is the next launch's
    // input and partly still in the Infinity Cache (17 layers at bs 256: 2.33 ms against 2.39 with the
    // non-temporal policy conv_pairw uses, 5 of 5 interleaved rounds, profiles/pair64_ab.jsonl).
    // PO2Q_PAIR64_NTS=3: non-temporal (A/B knob)
    int nts = 0;
    if (const char* e = getenv("PO2Q_PAIR64_NTS")) nts = atoi(e) == 0 ? 0 : 3;
    // PO2Q_PAIR64_PIPE=0: the conv-1 waves' vector work in front of their MFMAs (the earlier schedule;
    // A/B knob and the in-build bitwise reference); on by default
    bool pipe = true;
    if (const char* e = getenv("PO2Q_PAIR64_PIPE")) pipe = e[0] != '0';
    const dim3 grid((unsigned)blocks), block(512);
#define PO2Q_P6(g, t, p)                                                                         \
    if ((W <= 48 ? 3 : 4) == g && nts == t && pipe == p) {                                       \
        hipLaunchKernelGGL((conv_pair64<g, t, p>), grid, block, (size_t)kP6Lds, s, x, y, a);     \
        return hipGetLastError();                                                                \
    }
    PO2Q_P6(4, 0, true) PO2Q_P6(3, 0, true) PO2Q_P6(4, 3, true) PO2Q_P6(3, 3, true)
    PO2Q_P6(4, 0, false) PO2Q_P6(3, 0, false) PO2Q_P6(4, 3, false) PO2Q_P6(3, 3, false)
#undef PO2Q_P6
    return hipErrorInvalidValue;
}

// The pack geometry of one conv (conv_rowsk's layout [r][ks = chunk * 3 + s][nt][lane][8]).
ConvPlan pair64_pack_plan(int64_t N, int64_t H, int64_t W) {
    ConvPlan p{};
    p.N = (int)N; p.C = kP6C; p.H = (int)H; p.W = (int)W; p.K = kP6C;
    p.R = p.S = 3; p.sh = p.sw = 1; p.ph = p.pw = 1; p.dh = p.dw = 1; p.groups = 1;
    p.P = p.H; p.Q = p.W; p.Cg = p.C; p.Kg = p.K;
    p.kind = KIND_BF16X3_ROWS;
    p.vrx = 1;
    p.CC = 32;
    p.nchunks = 2;
    p.steps = kP6KS;
    p.NT = 4;
    p.taps = 9;
    p.packed_floats = kP6PackBytes / 4;
    return p;
}

namespace {
// po2q_qconv2d_pair_f32 has no workspace argument: the two packs of a direct call live in a scratch
// buffer per (device, stream), allocated at the first call and kept (calls on one stream are ordered,
// so reusing it is safe; 145 KiB each)
constexpr size_t kP6Scratch = 256 + 2 * ((kP6PackBytes + 255) / 256 * 256);
char* pair64_scratch(hipStream_t s) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, char*> pool;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    auto it = pool.find({dev, s});
    if (it != pool.end()) return it->second;
    void* p = nullptr;
    if (hipMalloc(&p, kP6Scratch) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    pool[{dev, s}] = reinterpret_cast<char*>(p);
    return reinterpret_cast<char*>(p);
}
}  // namespace

int pair64_entry(const float* x, const float* w1, const float* w2, float* y, int64_t N, int64_t H, int64_t W,
                 int bits, int fsr, int mode, const float* bias1, const float* bias2, bool plain, void* stream) {
    if (mode != PO2Q_MODE_PO2 && mode != PO2Q_MODE_PO2_PLUS) {
        set_error("po2q: pair: mode must be po2 or po2+");
        return PO2Q_ERR_INVALID;
    }
    if (bits < 1 || bits > 16) {
        set_error("po2q: bits must be in [1, 16]");
        return PO2Q_ERR_INVALID;
    }
    const long lo = (long)fsr - (1L << (bits - 1)), hi = (long)fsr - 1;
    if (lo < -126 || hi > 127) {
        set_error("po2q: pair: the exponent window leaves the bf16 range");
        return PO2Q_ERR_INVALID;
    }
    if (!pair64_geom_ok(N, kP6C, H, W)) {
        set_error("po2q: pair: 64 channels take 32 < W <= 64 with W % 4 == 0 (ResNet56 stage 3 at 56 x 56)");
        return PO2Q_ERR_INVALID;
    }
    if (!plain) {
        set_error("po2q: pair: 64 channels take the plain form only (biases; no BN affine, activation or residual): "
                  "run the two layers with po2q_qconv2d_fused_f32");
        return PO2Q_ERR_UNSUPPORTED;
    }
    if (!x || !w1 || !w2 || !y) {
        set_error("po2q: null pointer");
        return PO2Q_ERR_INVALID;
    }
    if (x == y) {
        set_error("po2q: pair: y must not alias x or the residual");
        return PO2Q_ERR_INVALID;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = pair64_scratch(s);
    if (!ws) {
        set_error("po2q: pair: no device memory for the weight packs (the first 64-channel call on a stream "
                  "allocates them: make it outside a graph capture)");
        return PO2Q_ERR_HIP;
    }
    const ConvPlan plan = pair64_pack_plan(N, H, W);
    const size_t pb = (kP6PackBytes + 255) / 256 * 256;
    const ConvPlan* plans[2] = {&plan, &plan};
    const float* ws_[2] = {w1, w2};
    uint16_t* packed[2] = {reinterpret_cast<uint16_t*>(ws + 256), reinterpret_cast<uint16_t*>(ws + 256 + pb)};
    float* scales[2] = {reinterpret_cast<float*>(ws), reinterpret_cast<float*>(ws) + 1};
    hipError_t he = launch_pack_bf16x3_batch(2, plans, ws_, packed, scales, bits, fsr, mode, s);
    if (he != hipSuccess) {
        set_error(std::string("po2q: pair weight pack launch: ") + hipGetErrorString(he));
        return PO2Q_ERR_HIP;
    }
    he = pair64_launch(x, y, N, H, W, packed[0], scales[0], packed[1], scales[1], bias1, bias2, s);
    if (he != hipSuccess) {
        set_error(std::string("po2q: pair launch: ") + hipGetErrorString(he));
        return PO2Q_ERR_HIP;
    }
    return PO2Q_OK;
}

}  // namespace po2q

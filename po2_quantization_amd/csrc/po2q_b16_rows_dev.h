// Helpers shared by the three bf16 row-streaming kernels: conv_b16_rows (po2q_conv_b16r.hip, C = K in
// {16, 32}), conv_b16_rowsk (po2q_conv_b16rk.hip, C = K = 64) and conv_b16_pair (po2q_conv_b16p.hip, the
// BasicBlock pair).  Not part of the C ABI.  Each kernel keeps its own walk (row loop, ring indices, barriers,
// wave-to-work mapping); what the walks have in common is here, once, so a change to the staging, store or
// residual path is made here and reaches all three.
//
// Staging.  An image row goes HBM [C][W] bf16 -> registers -> one LDS plane [W + 2 halo columns][C] bf16
// (x_addr of po2q_x3_dev.h; plane column = image column + 1).  A staging item is (channel octet, pixel pair):
// 8 dwords from HBM, one per channel (whole-row dword runs per channel over the threads), and two 16-byte LDS
// writes, one per pixel.  x is read with dword loads only when it is 4-byte aligned (W is even, so then every
// pair is), else with 2-byte loads.  The loads of a row are issued before the row before it multiplies and
// land in LDS after it.
//
// Zeros.  The two halo columns of every plane are written once, as zeros.  At C = 16 the second k-step
// (s2 | zero) is half padding, and the padded half reads the plane's 16-byte zero slot (behind the last
// column) on the pixel side as well as zero weights: 0 * inf cannot appear from padding.  C = 32 carries the
// slot too (one plane layout for both); C = 64 has no padded k-step and no slot.  A halo row outside the image
// is never loaded and never multiplied.
//
// Stores.  A finished output row is rounded once (finish4 / finish4_inplace), transposed through a wave-private
// LDS tile [channels][GW * 16 columns] bf16 (pitch + 16 bytes: the 16 channels of an 8-byte write instruction fall
// into distinct banks) and leaves as 16-byte pieces, 128-byte runs per channel at GW = 4.  The piece ladder:
// a piece inside the row whose address is 16-byte aligned (tested per lane) is one 16-byte access; else it
// goes as 4-byte pairs when 4-byte aligned (W and the piece's column are even: a pair is inside the row or
// outside it as a whole), else as 2-byte elements; either is masked at the row end.  The ragged last group is
// masked only here; its lanes computed a clamped column, never one outside the plane.
//
// Residual.  It comes in the way y goes out, backwards: pieces HBM -> registers by the same ladder (res_load,
// requested ahead of the row's last MFMAs; what lies past the row end stays zero) -> the wave's tile
// (tile_fill) -> each lane picks its 4 values, and its result goes back in place.
// The tile is its wave's own and LDS executes a wave's accesses in order, so a wavefront fence is all the
// ordering it needs (tile_fence).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "po2q_epi.h"
#include "po2q_internal.h"
#include "po2q_quant_b16_dev.h"
#include "po2q_x3_dev.h"

namespace po2q {

// ------------------------------------------------------------------------------------------ host --
constexpr int kB16RowWaves = 4;  // waves the 16-column groups (C = 16 / 32) or the channel tiles (C = 64) go over

// k-steps per tap row: C = 16 (s0 | s1) (s2 | zero), C = 32 one per tap column, C = 64 two
constexpr int b16_rows_ks(int C) { return C == 16 ? 2 : (C == 32 ? 3 : 6); }
// bytes per channel of a wave's transpose tile
constexpr int b16_rows_tpitch(int GW) { return GW * 32 + 16; }
// bytes per LDS plane, the zero slot included where there is one
constexpr int b16_rows_plane(int C, int W) { return (W + 2) * 2 * C + (C == 64 ? 0 : 16); }
// group slots per wave for `g` groups to compute
constexpr int b16_rows_gw(int g) { return g <= 1 ? 1 : (g <= 2 ? 2 : 4); }

// RB: 16 rows re-read 2 halo rows in 18; halved while the grid would leave CUs without a block
inline int b16_rows_rb(int64_t N, int P) {
    int RB = 16;
    while (RB > 4 && N * ((P + RB - 1) / RB) < 1024) RB >>= 1;
    return RB;
}

// what every kernel here takes: 3x3, stride 1, pad 1, dilation 1, groups 1, W even
inline bool b16_rows_geom_ok(const ConvPlan& p) {
    return p.groups == 1 && p.R == 3 && p.S == 3 && p.sh == 1 && p.sw == 1 && p.ph == 1 && p.pw == 1 && p.dh == 1 &&
           p.dw == 1 && p.W % 2 == 0;
}

// The plan of an eligible geometry: rows per band, bands, groups, group slots per wave, the pack's size
// ([tap row][k-step][nt][lane][8], per channel tile at C = 64) and the LDS budget of `planes` planes (`ring`
// of them x planes: pd), 4 tiles and `lds_extra` bytes; a band reads `halo` rows beyond its own.  KIND_BF16_ROWSK
// gives every wave all the groups of a row and a 16-channel tile, else the groups are dealt over the waves.
// False: too many blocks.
inline bool fill_rows_plan(ConvPlan& p, int kind, int ring, int planes, int halo, size_t lds_extra) {
    const bool dealt = kind != KIND_BF16_ROWSK;
    const int ngroups = (p.W + 15) / 16;
    const int GW = b16_rows_gw(dealt ? (ngroups + kB16RowWaves - 1) / kB16RowWaves : ngroups);
    const int RB = b16_rows_rb(p.N, p.P);
    const int bands = (p.P + RB - 1) / RB;
    const int64_t blocks = (int64_t)p.N * bands;
    if (blocks > INT32_MAX) return false;
    p.kind = kind;
    p.CC = p.C;
    p.NT = p.C / 16;
    p.NJ = GW;
    p.TP = RB; p.TQ = p.W; p.tilesP = bands; p.tilesQ = ngroups;
    p.kblocks = 1; p.nchunks = 1;
    p.HH = RB + halo; p.WW = p.WWp = p.W + 2;
    p.steps = b16_rows_ks(p.C);
    p.pd = ring;
    p.lds_bytes = (size_t)planes * b16_rows_plane(p.C, p.W) +
                  (size_t)kB16RowWaves * (dealt ? p.C : 16) * b16_rows_tpitch(GW) + lds_extra;
    p.blocks = blocks;
    p.packed_floats = (int64_t)3 * p.steps * p.NT * 64 * 4;  // 4-byte words
    return true;
}

// kernel arguments of conv_b16_rows and conv_b16_rowsk
struct B16RowArgs {
    int N, H, W;
    int RB, bands, ngroups;
    int plane;  // bytes per LDS plane
    int pair;   // dword staging: x is 4-byte aligned (W is even)
};

inline int b16_dword_aligned(const void* x) { return (reinterpret_cast<uintptr_t>(x) & 3u) == 0 ? 1 : 0; }

inline B16RowArgs b16_row_args(const ConvPlan& p, const uint16_t* x) {
    B16RowArgs a;
    a.N = p.N; a.H = p.H; a.W = p.W;
    a.RB = p.TP; a.bands = p.tilesP; a.ngroups = p.tilesQ;
    a.plane = b16_rows_plane(p.C, p.W);
    a.pair = b16_dword_aligned(x);
    return a;
}

// initial value of a process-wide switch: `name` in the environment, non-zero = on
inline int env_switch(const char* name) {
    const char* s = getenv(name);
    return (s && atoi(s) != 0) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------- device --
// One staging item: (channel octet oc, pixel pair m) of a row.  Each kernel decodes its own items (item index ->
// oc, m -> these fields): the decode as a shared function changed the C = 16 instances' register allocation and
// measured 5 % slower on conv_b16_rows<16, 2, EPI> (profiles/bf16_rows_helpers_bisect.jsonl, arm "decode").
struct B16Stage {
    bool v;      // the thread has this item
    int64_t g;   // element offset of its first channel's pair inside the image row's [C][H][W] slab
    int l0, l1;  // LDS byte offsets of its two pixels inside a plane
};

// xr: the image's row ([C] rows HW apart)
__device__ __forceinline__ void stage_load(const B16Stage& s, const uint16_t* xr, int64_t HW, int pair, uint32_t (&d)[8]) {
    if (!s.v) return;
    const uint16_t* px = xr + s.g;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint16_t* pj = px + j * HW;
        d[j] = pair ? *reinterpret_cast<const uint32_t*>(pj) : ((uint32_t)pj[0] | ((uint32_t)pj[1] << 16));
    }
}

__device__ __forceinline__ void stage_write(const B16Stage& s, unsigned char* plane, const uint32_t (&d)[8]) {
    if (!s.v) return;
    *reinterpret_cast<uint4*>(plane + s.l0) =
        make_uint4(pk_lo16(d[0], d[1]), pk_lo16(d[2], d[3]), pk_lo16(d[4], d[5]), pk_lo16(d[6], d[7]));
    *reinterpret_cast<uint4*>(plane + s.l1) =
        make_uint4(pk_hi16(d[0], d[1]), pk_hi16(d[2], d[3]), pk_hi16(d[4], d[5]), pk_hi16(d[6], d[7]));
}

// Zeros, once: halo columns 0 and W + 1 of `nplanes` planes `plane` bytes apart, and (ZS) their zero slots at
// byte `zero_off` of the plane.
template <int C, bool ZS>
__device__ __forceinline__ void zero_planes(unsigned char* lds, int nplanes, int plane, int W, int zero_off, int tid) {
    constexpr int OCT = C / 8, PER = 2 * OCT + (ZS ? 1 : 0);
    if (tid < nplanes * PER) {
        const int pl = tid / PER, r = tid - pl * PER;
        if constexpr (ZS) {
            const int off = r == 2 * OCT ? zero_off : x_addr<C>(r < OCT ? 0 : W + 1, r % OCT);
            *reinterpret_cast<uint4*>(lds + pl * plane + off) = make_uint4(0u, 0u, 0u, 0u);
        } else {
            *reinterpret_cast<uint4*>(lds + pl * plane + x_addr<C>(r < OCT ? 0 : W + 1, r % OCT)) =
                make_uint4(0u, 0u, 0u, 0u);
        }
    }
}

// Pixel fragment address inside a plane, C = 16 / 32: k-step ks of the group whose lane column is q (clamped
// into the row by the caller: ragged and idle groups read a column inside), lane octet o.
template <int C>
__device__ __forceinline__ int frag_off(int q, int ks, int o, int zero_off) {
    static_assert(C == 16 || C == 32, "C = 16 or 32");
    if constexpr (C == 16)
        return ks == 0 ? x_addr<16>(q + (o >> 1), o & 1) : (o < 2 ? x_addr<16>(q + 2, o) : zero_off);
    else
        return x_addr<32>(q + ks, o);
}

// The piece ladder, the only two copies of it.  p: the piece's first element, at column qq < W of its row.
__device__ __forceinline__ uint4 load_piece(const uint16_t* p, int qq, int W) {
    uint32_t t[4] = {0u, 0u, 0u, 0u};
    if (qq + 7 < W && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        const uint4 r4 = *reinterpret_cast<const uint4*>(p);
        t[0] = r4.x; t[1] = r4.y; t[2] = r4.z; t[3] = r4.w;
    } else if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (qq + 2 * i < W) t[i] = reinterpret_cast<const uint32_t*>(p)[i];
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (qq + i < W) t[i >> 1] |= (uint32_t)p[i] << (16 * (i & 1));
    }
    return make_uint4(t[0], t[1], t[2], t[3]);
}

__device__ __forceinline__ void store_piece(uint16_t* p, uint4 t4, int qq, int W) {
    const uint32_t t[4] = {t4.x, t4.y, t4.z, t4.w};
    if (qq + 7 < W && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        *reinterpret_cast<uint4*>(p) = t4;
    } else if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (qq + 2 * i < W) reinterpret_cast<uint32_t*>(p)[i] = t[i];  // W, qq even: a whole pair
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (qq + i < W) p[i] = (uint16_t)(t[i >> 1] >> (16 * (i & 1)));
    }
}

// The lane's 16-byte pieces of a wave's tile of NC channels x CH pieces, the tile's first column being q0:
// f(it, live, channel, piece of the channel, the piece's column).  (NC * CH = 32 at 16 channels and GW = 1: half
// the lanes have no live piece.)
constexpr int pieces_per_lane(int NC, int CH) { return (NC * CH + 63) / 64; }

template <int NC, int CH, class F>
__device__ __forceinline__ void for_pieces(int lane, int q0, F&& f) {
#pragma unroll
    for (int it = 0; it < pieces_per_lane(NC, CH); ++it) {
        const int el = it * 64 + lane;
        const int k = el / CH, j = el % CH;
        const int qq = q0 + j * 8;
        f(it, el < NC * CH, k, j, qq);
    }
}

// Row p of the tile's channels k0 .. k0 + NC - 1 of image n (nc = n * C) from column q0 on: HBM -> registers,
// registers -> tile, tile -> HBM.  Idle groups and pieces past the row end are skipped.
template <int NC, int CH>
__device__ __forceinline__ void res_load(uint4 (&r)[pieces_per_lane(NC, CH)], const uint16_t* res, int64_t nc, int k0,
                                         int H, int W, int p, int q0, int lane) {
    for_pieces<NC, CH>(lane, q0, [&](int it, bool live, int k, int, int qq) {
        uint4 t = make_uint4(0u, 0u, 0u, 0u);
        if (live && qq < W) t = load_piece(res + ((nc + k0 + k) * H + p) * W + qq, qq, W);
        r[it] = t;
    });
}

template <int NC, int CH, int TP>
__device__ __forceinline__ void tile_fill(unsigned char* tile, const uint4 (&r)[pieces_per_lane(NC, CH)], int lane) {
    for_pieces<NC, CH>(lane, 0, [&](int it, bool live, int k, int j, int) {
        if (live) *reinterpret_cast<uint4*>(tile + k * TP + j * 16) = r[it];
    });
}

template <int NC, int CH, int TP>
__device__ __forceinline__ void tile_drain(const unsigned char* tile, uint16_t* y, int64_t nc, int k0, int H, int W,
                                           int p, int q0, int lane) {
    for_pieces<NC, CH>(lane, q0, [&](int, bool live, int k, int j, int qq) {
        if (!live || qq >= W) return;
        const uint4 t4 = *reinterpret_cast<const uint4*>(tile + k * TP + j * 16);
        store_piece(y + ((nc + k0 + k) * H + p) * W + qq, t4, qq, W);
    });
}

// Orders a wave's accesses to its own tile: what it wrote is visible to its reads behind the fence (ACQ), and
// (always) its reads are done before it writes the tile again.
template <bool ACQ = true>
__device__ __forceinline__ void tile_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if constexpr (ACQ) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// two packed bf16 pairs -> 4 fp32 values
__device__ __forceinline__ void unpack_bf16x4(uint32_t lo, uint32_t hi, float (&v)[4]) {
    v[0] = __uint_as_float(lo << 16);
    v[1] = __uint_as_float(lo & 0xffff0000u);
    v[2] = __uint_as_float(hi << 16);
    v[3] = __uint_as_float(hi & 0xffff0000u);
}

// A lane's four values of one channel: y = bf16_rne(act((acc + b) * s + t + residual)), the affine map and the
// residual where asked for, the one rounding, packed as the tile takes them.  Two forms: the row kernels have
// the activation as a compile-time constant (one kernel body per activation) and the residual in the tile slot
// `tp` the result goes back to; the pair has a run-time activation and the residual in two registers.
template <int ACT>
__device__ __forceinline__ void finish4_inplace(unsigned char* tp, floatx4 acc, float b, bool aff, float s, float t,
                                                bool res) {
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = acc[i] + b;
    float rv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (res) {
        const uint2 rq = *reinterpret_cast<const uint2*>(tp);
        unpack_bf16x4(rq.x, rq.y, rv);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (aff) v[i] = v[i] * s + t;
        if (res) v[i] += rv[i];
        v[i] = epi_act_ct<ACT>(v[i]);
    }
    uint32_t r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = bf16_rne(v[i]);
    *reinterpret_cast<uint2*>(tp) = make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
}

__device__ __forceinline__ uint2 finish4(floatx4 acc, float b, bool aff, float s, float t, bool res, uint32_t r0,
                                         uint32_t r1, int act) {
    float rv[4];
    unpack_bf16x4(r0, r1, rv);
    uint32_t r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float v = acc[i] + b;
        if (aff) v = v * s + t;
        if (res) v += rv[i];
        r[i] = bf16_rne(epi_act(v, act));
    }
    return make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
}

// The three accumulator sets of a group move up one output row: slot 0 <- 1 <- 2 <- zeros.
__device__ __forceinline__ void rotate_acc(floatx4 (&a)[3]) {
    a[0] = a[1];
    a[1] = a[2];
    a[2] = floatx4{0.f, 0.f, 0.f, 0.f};
}
template <int GW>
__device__ __forceinline__ void rotate_acc(floatx4 (&acc)[GW][3]) {
#pragma unroll
    for (int g = 0; g < GW; ++g) rotate_acc(acc[g]);
}
template <int GW, int NT>
__device__ __forceinline__ void rotate_acc(floatx4 (&acc)[GW][3][NT]) {
#pragma unroll
    for (int g = 0; g < GW; ++g)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            acc[g][0][nt] = acc[g][1][nt];
            acc[g][1][nt] = acc[g][2][nt];
            acc[g][2][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
}

}  // namespace po2q

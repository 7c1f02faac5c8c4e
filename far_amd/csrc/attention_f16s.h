// The split-fp16 softmax-attention recipe K22 (full_attention_f16s.hip, full_attention_bwd_f16s.hip: head dims 16 / 32, masks, key
// split) and K23 (vit_attention_f16s.hip, vit_attention_bwd_f16s.hip: head dim 64, strided operands) share.  Each file's header says
// what is its own (layout, LDS and register budget, masks, split); the numerically delicate steps are here, once:
//   operands a value x enters a matrix product as the fp16 pair hi = fp16(x 2^e), lo = fp16(x 2^e - hi) (split8); a product of two such
//            operands is hi.hi + hi.lo + lo.hi on 32x32x16 f16 MFMAs with fp32 accumulation (score_tile).  A value beyond
//            65504 / 2^e, or a non-finite one, is out of range (out_of_range): the launch ORs the overflow flag.
//   owned | walked  a workgroup owns 32 rows per wave (a lane ONE row: its operands are the B side of score_tile, in registers) and
//            walks the other axis in tiles staged through LDS: row-major planes for score_tile, and the transpose in the k-order of
//            the accumulator registers (tplane_row) for the product that consumes p or ds straight from those registers.
//   forward  online softmax in the log2 domain (RowState).  The row reference R = ceil(running maximum) is an INTEGER, so a change
//            rescales the running sum and the output accumulators by an exact power of two; p = 2^(x - R + P_EXP_FWD): one exponential
//            per score.  A tile's terms are summed on their own and join the row sum with Kahan compensation.
//   backward p = 2^(x - lse2) from the row statistic lse2 = R - P_EXP_FWD + log2(row sum) the training forward saved; g and ds are
//            scaled by per-image powers of two read from device memory (image_exponents), the results scaled back exactly.
// Every kernel is built with -ffp-contract=off and is deterministic: the order of the operations below is part of the contract.
#pragma once
#include "common.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr float NEG_HUGE = -1.0e30f;
constexpr int ROW_REF0 = -(1 << 24);     // row reference before the first tile
constexpr float LSE_NONE = 1.0e30f;      // row statistic of a row without softmax (padded query / no valid key / past the end): p = 2^(x - 1e30) = 0
constexpr int P_EXP_FWD = 15;            // p is formed as 2^(x - R + 15): its fp16 lo part stays normal down to p = 2^-18 max
constexpr int P_EXP_BWD = 14;            // p in [0, 1] enters the dv product as p 2^14
constexpr int G_EXP = 12;                // max |g| 2^ge in [2^12, 2^13)

__device__ __forceinline__ void split8(const float (&x)[8], float pre, f16x8& hi, f16x8& lo) {
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
        f16x2 h2, l2;
        split2(f32x2{x[e], x[e + 1]} * f32x2{pre, pre}, h2, l2);
        hi[e] = h2.x; hi[e + 1] = h2.y;
        lo[e] = l2.x; lo[e + 1] = l2.y;
    }
}

__device__ __forceinline__ f16x8 round8(const float (&x)[8], float pre) {
    f16x8 y;
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = (_Float16)(x[e] * pre);
    return y;
}

__device__ __forceinline__ void load8(const float* p, float (&x)[8]) {
    const float4 u = *reinterpret_cast<const float4*>(p);
    const float4 w = *reinterpret_cast<const float4*>(p + 4);
    x[0] = u.x; x[1] = u.y; x[2] = u.z; x[3] = u.w; x[4] = w.x; x[5] = w.y; x[6] = w.z; x[7] = w.w;
}

__device__ __forceinline__ bool out_of_range(const float (&x)[8], float pre) {
    bool bad = false;
#pragma unroll
    for (int e = 0; e < 8; ++e) bad |= !(fabsf(x[e]) * pre <= 65504.0f);
    return bad;
}

// The walked row at element e of 16-byte slot g of a transposed plane whose tile starts at row j0.  g = 4 ct + 2 u + h is the slot
// that half-wave h reads for MFMA (ct, u); its A operand there is accumulator registers 8 u .. 8 u + 7 of score block ct, which hold
// rows 32 ct + mfma32_row(8 u + e, h) = 32 ct + 16 u + 4 h + (e < 4 ? e : e + 4): the plane is written in that order.
__device__ __forceinline__ int tplane_row(int j0, int g, int e) {
    return j0 + (32 * (g >> 2) + 16 * ((g >> 1) & 1) + 4 * (g & 1)) + (e < 4 ? e : e + 4);
}

// acc[ct] += A[32 ct + l31] . b over the QS k-steps of the contraction: all ct hi.hi, then all hi.lo, then all lo.hi.  A: the row-major
// hi plane at `a_hi`, its lo plane LO bytes behind it, OFF(row, 16-byte slot) the swizzled offset; b: this lane's owned row.
// Three products keep this loop written out, because the call moved hipcc's register allocation there (each says so): K22's
// forward scores, K22-backward's dp and K23-backward's scores.  A change here is a change there.
template <int (*OFF)(int, int), int LO, int NCT, int QS>
__device__ __forceinline__ void score_tile(f32x16 (&acc)[NCT], const unsigned char* a_hi, int l31, int h, const f16x8 (&bh)[QS],
                                           const f16x8 (&bl)[QS]) {
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        f16x8 ch[NCT], cl[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int off = OFF(32 * ct + l31, 2 * s + h);
            ch[ct] = *reinterpret_cast<const f16x8*>(a_hi + off);
            cl[ct] = *reinterpret_cast<const f16x8*>(a_hi + LO + off);
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch[ct], bh[s], acc[ct], 0, 0, 0);
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch[ct], bl[s], acc[ct], 0, 0, 0);
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl[ct], bh[s], acc[ct], 0, 0, 0);
    }
}

// The exponent that takes a value held against the row reference `from` to the reference `to` >= from: 2^-200 flushes every fp32
// to zero already.
__device__ __forceinline__ int rescale_exp(int from, int to) {
    const int d = from - to;                               // <= 0
    return d < -200 ? -200 : d;
}

// The forward's state of one query row (a lane owns one; lanes l and l + 32 share the row and hold half of its keys each).
struct RowState {
    int R = ROW_REF0;                      // integer row reference, equal in lanes l and l + 32
    float sum = 0.f, comp = 0.f;           // this half-wave's share of the row sum (Kahan-compensated per tile)

    // The reference after a tile whose maximum (log2 domain) is tm: ceil of the running maximum, agreed between the two half-waves
    __device__ __forceinline__ int next_ref(float tm) const {
        int Rn = (int)ceilf(fminf(fmaxf(tm, -1.0e6f), 1.0e6f));
        Rn = Rn > R ? Rn : R;
        const int Ro = __shfl_xor(Rn, 32, 64);
        return Rn > Ro ? Rn : Ro;
    }
    // Moves the row to the reference Rn -> the exponent the caller applies to the row's output accumulators
    __device__ __forceinline__ int rescale(int Rn) {
        const int d = rescale_exp(R, Rn);
        sum = ldexpf(sum, d);
        comp = ldexpf(comp, d);
        R = Rn;
        return d;
    }
    // t: the tile's terms summed on their own, added with Kahan compensation (emm_bilinear_f16s.hip: rowstat_update)
    __device__ __forceinline__ void add_tile(float t) {
        const float y = t - comp;
        const float ns = sum + y;
        comp = (ns - sum) - y;
        sum = ns;
    }
    // after the last tile: the row's sum, both halves (they carry the same reference R)
    __device__ __forceinline__ float total() {
        sum -= comp;
        return sum + shfl_xor_f(sum, 32);
    }
};

// The image's two exponents from the bits k_prep left: g 2^ge has its maximum in [2^12, 2^13); with |v| 2^act_exp < 2^ev,
// |ds| <= 2 D max|g 2^ge| max|v 2^act_exp| < 2^(14 + log2 D + ev), so ds 2^eds < 2^15.  A non-finite maximum (flagged by k_prep)
// and an all-zero image get harmless exponents.
template <int LOG2_D>
__device__ __forceinline__ void image_exponents(const unsigned* scal, int n, int act_exp, int& ge, int& eds) {
    const unsigned gb = scal[2 * n], vb = scal[2 * n + 1];
    ge = G_EXP - ((int)(gb >> 23) - 127);
    const int ev = (int)(vb >> 23) - 127 + 1 + act_exp;
    eds = 1 - LOG2_D - ev;
    if (gb >= 0x7f800000u) ge = 0;
    if (vb >= 0x7f800000u) eds = 0;
    ge = ge < -100 ? -100 : (ge > 100 ? 100 : ge);
    eds = eds < -60 ? -60 : (eds > 60 ? 60 : eds);
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// How a launch is cut: `own` rows in blocks of 128 and `walk` rows in tiles of 64 (small: one wave per block, 32 and 32); the walked
// axis is split when an image alone would start fewer than 64 workgroups.  A function of (L, S, H) only, never of N.  `small` is the
// caller's: the forward walks keys only and passes S <= 32, the backward walks both axes with one kernel form and passes
// L <= 32 && S <= 32.
struct SplitPlan {
    int nI, ntile, nsplit, tps;
};
inline SplitPlan split_plan(int own, int walk, int H, bool small) {
    SplitPlan p;
    const int rows = small ? 32 : 128, kt = small ? 32 : 64;
    p.nI = (own + rows - 1) / rows;
    p.ntile = (walk + kt - 1) / kt;
    int ns = 1;
    const long wg = (long)H * p.nI;
    if (!small && wg < 64 && p.ntile >= 8) {
        ns = (int)(64 / wg);
        if (ns > p.ntile / 4) ns = p.ntile / 4;
        if (ns > 8) ns = 8;
        if (ns < 1) ns = 1;
    }
    p.tps = (p.ntile + ns - 1) / ns;
    p.nsplit = (p.ntile + p.tps - 1) / p.tps;        // no empty split
    return p;
}

}  // namespace

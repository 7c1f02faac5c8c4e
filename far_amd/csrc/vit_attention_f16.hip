// K23 on plain fp16 operands: the head-dim-64 softmax self-attention core of the 8-Point-ViT's Blocks with ONE fp16 value per operand.
//
// The operator, the addressing, the launch geometry and the softmax are vit_attention_f16s.hip's (read its header first, then
// attention_f16s.h); this is its 16-bit-operand sibling for ViTEss.set_precision (narrower than the reference -- never the parity
// configuration).  What differs:
//   operands every q / k / v value enters as the single value fp16(x 2^act_exp): no lo planes, one 32x32x16 MFMA per k-step where
//            K23 spends three (hi.hi + hi.lo + lo.hi), for the scores and for P V: 16 MFMAs per 64-key tile and wave instead of 48.
//   softmax  unchanged and in fp32: RowState in the log2 domain with the integer row reference and the power-of-two rescale,
//            p = 2^(x - R + P_EXP_FWD) with one exp2 per score, the tile sum of the UNROUNDED p joined with Kahan compensation, keys
//            past S selected to p = 0.  Only the P V operand is rounded, once: fp16(p) (round8).  With the scores exact products of
//            the rounded operands in fp32, the output's distance from the softmax of the rounded operands is that one rounding:
//            <= 2^-11 max|v| (+ fp32 accumulation).
//   stage    k as [key][64] rows and v^T as [64][keys] rows, one plane each: 2 x 8 KB = 16 KB per 64-key tile, two stages = 32 KB --
//            half of K23's, with its row_off swizzle.  The tile stays at 64 keys and the workgroup at 32 rows per wave, two
//            workgroups per CU as K23: the next tile's 32 fp32 values per thread, the score block and the two output blocks are
//            what fills the registers, not the operand planes -- asking hipcc for three workgroups per CU made it spill 66
//            registers per thread, and a 128-key tile doubles the staged values.  DESIGN 4 (K23 on plain fp16) has the measurement.
// Ordinary global loads into registers one tile ahead, __syncthreads(), vector stores; no LDS-DMA, no workspace, no float atomics.
// The launch geometry is a function of (L, H) and the image index only: an image's bits do not depend on its batch, and the result is
// the same from run to run.  Inference only: the backward (vit_attention_bwd_f16s.hip) stays a split-fp16 kernel.
// Range: |x| 2^act_exp <= 65504 for every q / k / v value that takes part, flagged as in K23.
#include "attention_f16s.h"
#include <type_traits>

namespace {

constexpr int D = 64;                    // head dim
constexpr int KT = 64, NCT = KT / 32;    // keys per tile, 32-key score blocks per tile
constexpr int WAVES = 4, NT = 64 * WAVES, ROWS = 32 * WAVES;
constexpr int QS = D / 16;               // k-steps of the score contraction
constexpr int NOB = D / 32;              // 32-wide output blocks
constexpr int PLANE = KT * D * 2;        // bytes of one plane (k, v^T): 8 KB
constexpr int STAGE = 2 * PLANE;         // 16 KB
constexpr int KCH = KT * (D / 8) / NT;   // k chunks (8 channels of one key) per thread: 2
constexpr int VCH = D * (KT / 8) / NT;   // v^T items (8 keys of one channel) per thread: 2
static_assert(KT * (D / 8) % NT == 0 && D * (KT / 8) % NT == 0, "staging items divide over the threads");

// 16-byte slot c of the 128-byte row `row` (a key's 64 channels, or a channel's 64 keys): K23's swizzle
__device__ __forceinline__ int row_off(int row, int c) { return row * 128 + ((c ^ ((row >> 1) & 7)) * 16); }

struct Args {
    const float *q, *k, *v;
    float* out;
    int* overflow;
    long q_img, q_head, q_row, kv_img, kv_head, kv_row;     // strides in floats
    int Z, L, S, H, nI;
    float pre, c1, out_mul;
};

// One key tile on its way from global memory to LDS: fp32 in registers while the previous tile is computed.
struct Staged {
    float kx[KCH][8];
    float vx[VCH][8];

    __device__ __forceinline__ void load(const Args& a, const float* kb, const float* vb, int jt, int tid) {
        const int j0 = jt * KT;
#pragma unroll
        for (int ci = 0; ci < KCH; ++ci) {
            const int c = tid + ci * NT;
            const int key = c >> 3, sl = c & 7;
            const int j = j0 + key;
#pragma unroll
            for (int e = 0; e < 8; ++e) kx[ci][e] = 0.f;
            if (j < a.S) load8(kb + (size_t)j * a.kv_row + sl * 8, kx[ci]);
        }
#pragma unroll
        for (int ci = 0; ci < VCH; ++ci) {
            const int c = tid + ci * NT;
            const int d = c & 63, g = c >> 6;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int j = tplane_row(j0, g, e);
                vx[ci][e] = j < a.S ? vb[(size_t)j * a.kv_row + d] : 0.f;
            }
        }
    }

    // -> true when a staged value is beyond fp16's range (checked by the workgroups of row block 0 only: `check`)
    __device__ __forceinline__ bool store(unsigned char* st, float pre, int tid, bool check) {
        bool bad = false;
#pragma unroll
        for (int ci = 0; ci < KCH; ++ci) {
            const int c = tid + ci * NT;
            if (check) bad |= out_of_range(kx[ci], pre);
            *reinterpret_cast<f16x8*>(st + row_off(c >> 3, c & 7)) = round8(kx[ci], pre);
        }
#pragma unroll
        for (int ci = 0; ci < VCH; ++ci) {
            const int c = tid + ci * NT;
            if (check) bad |= out_of_range(vx[ci], pre);
            *reinterpret_cast<f16x8*>(st + PLANE + row_off(c & 63, c >> 6)) = round8(vx[ci], pre);
        }
        return bad;
    }
};

__global__ __launch_bounds__(NT, 2) void k_vit_attention_f16(Args a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_all[2 * STAGE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    int z, Ib;                             // block -> (image-head z, row block Ib)
    tile_coords_of(blockIdx.x, a.nI, a.Z * a.H, z, Ib);
    const int n = z / a.H, hh = z - n * a.H;
    const int i0 = Ib * ROWS + 32 * wave;
    const int irow = i0 + l31;
    const bool qok = irow < a.L;
    bool bad = false;

    // ---- this lane's query row: channels 16 s + 8 h .. + 7 (the B operand of the score MFMAs)
    f16x8 qf[QS];
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (qok) load8(a.q + (size_t)n * a.q_img + (size_t)hh * a.q_head + (size_t)irow * a.q_row + 16 * s + 8 * h, x);
        bad |= out_of_range(x, a.pre);
        qf[s] = round8(x, a.pre);
    }

    f32x16 tacc[NOB];
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
        for (int r = 0; r < 16; ++r) tacc[ob][r] = 0.f;
    RowState row;

    const float* const kb = a.k + (size_t)n * a.kv_img + (size_t)hh * a.kv_head;
    const float* const vb = a.v + (size_t)n * a.kv_img + (size_t)hh * a.kv_head;
    const int ntile = (a.S + KT - 1) / KT;
    const bool check = Ib == 0;
    Staged st;
    st.load(a, kb, vb, 0, tid);
    bad |= st.store(lds_all, a.pre, tid, check);
    __syncthreads();
    for (int jt = 0; jt < ntile; ++jt) {
        // tile jt is in stage jt & 1; the other stage was last read before the barrier that ended the previous iteration:
        // tile jt + 1 goes there once its loads (issued now, in flight during the MFMAs) have arrived
        const unsigned char* const lds = lds_all + (jt & 1) * STAGE;
        const unsigned char* const ldv = lds + PLANE;
        const bool more = jt + 1 < ntile;
        if (more) st.load(a, kb, vb, jt + 1, tid);

        // ---- scores: acc[ct][r] = k[32 ct + mfma32_row(r, h)] . q[l31], one MFMA per (score block, k-step)
        f32x16 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            f16x8 kf[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) kf[ct] = *reinterpret_cast<const f16x8*>(lds + row_off(32 * ct + l31, 2 * s + h));
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[ct], qf[s], acc[ct], 0, 0, 0);
        }
        // validity of this lane's keys: accumulator register r of score block ct is key 32 ct + mfma32_row(r, h) of the tile
        const int nvalid = a.S - jt * KT;                                                  // >= 1
        const bool ragged = nvalid < KT;                                                   // workgroup-uniform: the last tile only
        auto key_ok = [&](int ct, int r) { return 32 * ct + mfma32_row(r, h) < nvalid; };

        // ---- row reference from the tile's maximum (log2 domain)
        float tm = NEG_HUGE;
        if (ragged) {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) tm = fmaxf(tm, key_ok(ct, r) ? acc[ct][r] : NEG_HUGE);
        } else {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) tm = fmaxf(tm, acc[ct][r]);
        }
        tm *= a.c1;                                                                        // c1 > 0
        const int Rn = row.next_ref(tm);
        if (__any(Rn != row.R)) {                                                          // rare after the first tiles
            const int d = row.rescale(Rn);
#pragma unroll
            for (int r = 0; r < 16; ++r) {                                                 // register r: query mfma32_row(r, h)
                const int dr = __shfl(d, mfma32_row(r, h), 64);
#pragma unroll
                for (int ob = 0; ob < NOB; ++ob) tacc[ob][r] = ldexpf(tacc[ob][r], dr);
            }
        }
        const float nR = (float)(P_EXP_FWD - row.R);
        float t = 0.f;
        auto pv_tile = [&](auto ragged_c) {
            constexpr bool RAGGED = decltype(ragged_c)::value;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    float p[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int r = 8 * u + e;
                        p[e] = __builtin_amdgcn_exp2f(fmaf(acc[ct][r], a.c1, nR));
                        if (RAGGED) p[e] = key_ok(ct, r) ? p[e] : 0.f;                     // selected out, whatever the score was
                        t += p[e];                                                         // the sum takes the unrounded p
                    }
                    const f16x8 pf = round8(p, 1.0f);                                      // p <= 2^15: the one rounding of P V
#pragma unroll
                    for (int ob = 0; ob < NOB; ++ob) {
                        const f16x8 vf = *reinterpret_cast<const f16x8*>(ldv + row_off(32 * ob + l31, 4 * ct + 2 * u + h));
                        tacc[ob] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pf, vf, tacc[ob], 0, 0, 0);
                    }
                }
            }
        };
        if (ragged) pv_tile(std::true_type{});
        else pv_tile(std::false_type{});
        row.add_tile(t);

        if (more) bad |= st.store(lds_all + ((jt + 1) & 1) * STAGE, a.pre, tid, check);
        __syncthreads();
    }
    const float rsum = row.total();
    if (a.overflow && __any(bad) && lane == 0) atomicOr(a.overflow, 1);

    // ---- store: the lane holds channels l31 and 32 + l31 of queries i0 + mfma32_row(r, h); the row's sum sits in lane (row)
    const float den = (qok && rsum > 0.f) ? rsum : 0.f;
    float* const ob0 = a.out + (size_t)n * a.L * a.H * D + (size_t)hh * D + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rr = mfma32_row(r, h);
        const float dr = __shfl(den, rr, 64);
        const int i = i0 + rr;
        if (i < a.L) {
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob) ob0[(size_t)i * a.H * D + 32 * ob] = dr > 0.f ? tacc[ob][r] / dr * a.out_mul : 0.f;
        }
    }
}

}  // namespace

extern "C" {

// far_vit_attention_f16s on plain fp16 operands (one fp16 value per q / k / v element and per probability; fp32 softmax and
// accumulation): the same arguments, checks and return codes.  Narrower than the reference; inference only.
int far_vit_attention_f16(const float* q, const float* k, const float* v, int Z, int L, int S, int H, int D, long q_img, long q_head,
                          long q_row, long kv_img, long kv_head, long kv_row, int act_exp, float* out, int* overflow,
                          hipStream_t stream) {
    far_clear_errors();
    if (Z == 0) return FAR_OK;
    if (!q || !k || !v || !out || Z < 0 || L <= 0 || S <= 0 || H <= 0 || D != 64 || act_exp < -24 || act_exp > 8) return FAR_EINVAL;
    if (((q_img | q_head | q_row | kv_img | kv_head | kv_row) & 3) || q_img < 0 || q_head < 0 || q_row < 64 || kv_img < 0 || kv_head < 0 ||
        kv_row < 64)
        return FAR_EINVAL;
    if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) || ((uintptr_t)out & 3)) return FAR_EINVAL;
    Args a;
    a.q = q; a.k = k; a.v = v; a.out = out; a.overflow = overflow;
    a.q_img = q_img; a.q_head = q_head; a.q_row = q_row; a.kv_img = kv_img; a.kv_head = kv_head; a.kv_row = kv_row;
    a.Z = Z; a.L = L; a.S = S; a.H = H;
    a.nI = (L + ROWS - 1) / ROWS;
    const long blocks = (long)Z * H * a.nI;
    if (blocks > 0x7fffffffL || (long)Z * H > 0x7fffffffL) return FAR_EINVAL;
    a.pre = ldexpf(1.0f, act_exp);
    a.c1 = ldexpf(1.44269504088896341f / 8.0f, -2 * act_exp);                  // scores -> log2 domain, 1 / sqrt(64)
    a.out_mul = ldexpf(1.0f, -act_exp);
    hipLaunchKernelGGL(k_vit_attention_f16, dim3((unsigned)blocks), dim3(NT), 0, stream, a);
    return far_check_launch();
}

}  // extern "C"

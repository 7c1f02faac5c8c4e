// K23 backward: the gradients of the 8-Point-ViT's head-dim-64 softmax attention core (vit_attention_f16s.hip) on the f16 matrix cores.
//
// Per (image n, head h), c = 1 / 8, with the training forward's saved row statistic lse2_i = log2 sum_j 2^(c log2(e) q_i.k_j):
//   p_ij = 2^(x_ij - lse2_i)      delta_i = g_i.o_i      dv_j = sum_i p_ij g_i      dp_ij = g_i.v_j      ds_ij = p_ij (dp_ij - delta_i)
//   dq_i = c sum_j ds_ij k_j                            dk_j = c sum_i ds_ij q_i
// The backward recipe of attention_f16s.h (read its header first) in K22-backward's shape (full_attention_bwd_f16s.hip; that file stays
// a head-dim-16/32 kernel -- one 32 x 32 output block per wave, a 32-row transposed plane).  Three launches, no (L, S)-sized tensor:
//   k_prep   delta (Z, H, L) from g and the saved output (16 lanes x float4 per head, a fixed tree), the per-image max |g| and max |v| as
//            integer atomicMax on the float bits -- order-independent; one per workgroup of 32 tokens --, and the range guard of q, k, v, g.
//   k_bwd<KEYS = false>  dq: a workgroup owns 128 query rows (a lane ONE query) and walks the keys in tiles of 64.
//   k_bwd<KEYS = true>   dk, dv: a workgroup owns 128 keys (a lane ONE key) and walks the queries in tiles of 64; dk and dv come from
//            the same recomputed tile.
// Precision (both kernels, as K22-backward): scores and dp are hi.hi + hi.lo + lo.hi split-fp16 32x32x16 MFMAs around the forward's
// activation exponent; ds and p go from the accumulator registers into the output MFMAs as plain fp16 A operands against the
// transposed hi plane of k (dq), q (dk) and g (dv).  g is multiplied by 2^ge (the image's max |g| lands in [2^12, 2^13)), ds by 2^eds
// chosen from max |v| so that |ds| <= 2 D max|g| max|v| stays below 2^15: both exponents are read from device memory (no host
// synchronisation) and are per IMAGE; the results are scaled back by exact powers of two.
// What differs at D = 64:
//   scores, dp  four k-steps per 32 walked rows (x 3 for the split).
//   outputs     two 32-wide blocks per product: dq two accumulator blocks; dk and dv two each.
//   rows        128 bytes, row-major and transposed alike: K23's row_off swizzle (slot c of row r at c ^ ((r >> 1) & 7)).
//   layout      q, k, v and dq, dk, dv are addressed by (image, head, row) strides in floats like the forward: one (Z, N, 3 H 64) qkv
//               projection is read in place and one (Z, N, 3 H 64) gradient buffer written in place.  g, out: (Z, L, H 64) contiguous.
// Budget (MI355X: 160 KiB LDS per CU, 512 unified VGPR / AGPR entries per lane at one wave per SIMD):
//   walked tile 64 rows: four 8 KB row-major planes (A1, A2; hi, lo) + one (dq) or two (dk / dv) 8 KB transposed planes + 512 B of
//            row statistics (dk / dv) = 40 | 48.5 KB per stage.  TWO stages (the next tile's fp32 loads are in flight during the
//            MFMAs and land in the other stage: one barrier per tile) = 80 | 97 KB: one workgroup per CU for dk / dv, two for dq.
//   registers   owned B operands 64 (q | k and g | v, hi and lo, 4 k-steps x 4), score + dp accumulators 64, outputs 32 (dq) | 64
//            (dk, dv), the tile in flight 48 | 64: ~210 (dq) | ~260 + addresses (dk / dv).  The key-owning kernel is therefore built for
//            one wave per SIMD (512 entries, nothing spills), the query-owning one for two (256 entries: hipcc spills four registers,
//            20 bytes of scratch per lane, and two workgroups of 80 KB share a CU).  A 128-row walked tile would double the
//            stage to 97 KB x 2 and the accumulators to 128: it does not fit next to the outputs; a 32-row tile halves the MFMA work
//            per barrier.  64 it is, as in the forward.
// The walked axis is not split (the forward does not split either); launch geometry depends on (L, S, H) and the image index only.
// No float atomics, no data handed between the workgroups of one launch, bit-identical from run to run.  No masks (K23 has none).
#include "attention_f16s.h"

namespace {

constexpr int D = 64;
constexpr int KT = 64, NCT = KT / 32;    // walked rows per tile, 32-row score blocks per tile
constexpr int WAVES = 4, NT = 64 * WAVES, ROWS = 32 * WAVES;
constexpr int QS = D / 16;               // k-steps of the score / dp contraction
constexpr int NOB = D / 32;              // 32-wide output blocks
constexpr int PLANE = KT * D * 2;        // bytes of one plane, row-major [walked row][64] or transposed [channel][64 walked rows]: 8 KB
constexpr int OFF_A2 = 2 * PLANE, OFF_T1 = 4 * PLANE, OFF_T2 = 5 * PLANE;
constexpr int KCH = KT * (D / 8) / NT;   // row-major chunks (8 channels of one row) per thread and operand: 2
constexpr int VCH = D * (KT / 8) / NT;   // transposed items (8 rows of one channel) per thread and operand: 2
static_assert(KT * (D / 8) % NT == 0 && D * (KT / 8) % NT == 0, "staging items divide over the threads");

template <bool KEYS>
struct Lds {
    static constexpr int OFF_ST = OFF_T1 + (KEYS ? 2 : 1) * PLANE;     // KEYS: lse2[KT], delta[KT] floats
    static constexpr int STAGE = OFF_ST + (KEYS ? KT * 8 : 0);
};

// 16-byte slot c of the 128-byte row `row`
__device__ __forceinline__ int row_off(int row, int c) { return row * 128 + ((c ^ ((row >> 1) & 7)) * 16); }

struct Args {
    const float *q, *k, *v, *g, *out, *lse;
    float *dq, *dk, *dv;
    unsigned* scal;        // [Z][2]: bits of max |g|, max |v| of the image
    float* delta;          // [Z H][L]
    int* overflow;
    long q_img, q_head, q_row, kv_img, kv_head, kv_row;             // strides in floats
    long dq_img, dq_head, dq_row, dkv_img, dkv_head, dkv_row;
    int Z, L, S, H, nI, act_exp;
    float pre, c1, c;
};

// ---- delta, the per-image maxima and the range guard.  A workgroup takes PREP_TOK consecutive tokens of ONE image and one side (query
// rows: g, out, q; key rows: k, v), a wave a quarter of them; 16 lanes x float4 are one head's 64 channels, so a wave covers four heads
// per pass.  delta: the lane's four products in a fixed order, then a fixed 16-lane tree.  One atomicMax per workgroup.
constexpr int PREP_TOK = 32;

__device__ __forceinline__ bool prep_scan(const float4 x, float pre, unsigned* mx) {
    const float v[4] = {x.x, x.y, x.z, x.w};
    bool bad = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float ax = fabsf(v[e]);
        bad |= !(ax * pre <= 65504.0f);
        if (mx) {
            const unsigned b = __float_as_uint(ax);
            *mx = b > *mx ? b : *mx;
        }
    }
    return bad;
}

__global__ __launch_bounds__(256) void k_prep(Args a) {
    __shared__ unsigned smx[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nbq = (a.L + PREP_TOK - 1) / PREP_TOK, nbk = (a.S + PREP_TOK - 1) / PREP_TOK, per = nbq + nbk;
    const int n = blockIdx.x / per, b = blockIdx.x - n * per;
    const bool qside = b < nbq;
    const int T = qside ? a.L : a.S;
    const int t0 = (qside ? b : b - nbq) * PREP_TOK + wave * (PREP_TOK / 4);
    const int hl = lane >> 4, cl = (lane & 15) * 4;
    unsigned mx = 0;
    bool bad = false;
    for (int t = t0; t < t0 + PREP_TOK / 4 && t < T; ++t) {                    // wave-uniform bounds
        for (int h0 = 0; h0 < a.H; h0 += 4) {
            const int hh = h0 + hl;
            const bool on = hh < a.H;
            if (qside) {
                float pr = 0.f;
                if (on) {
                    const size_t o = (((size_t)n * a.L + t) * a.H + hh) * D + cl;
                    const float4 gv = *reinterpret_cast<const float4*>(a.g + o);
                    const float4 ov = *reinterpret_cast<const float4*>(a.out + o);
                    const float4 qv = *reinterpret_cast<const float4*>(a.q + (size_t)n * a.q_img + (size_t)hh * a.q_head + (size_t)t * a.q_row + cl);
                    pr = (gv.x * ov.x + gv.y * ov.y) + (gv.z * ov.z + gv.w * ov.w);
                    bad |= prep_scan(gv, 0.f, &mx);                            // g: every finite value is in range (inf 0 and NaN fail)
                    bad |= prep_scan(qv, a.pre, nullptr);
                }
                for (int m = 1; m < 16; m <<= 1) pr += shfl_xor_f(pr, m);      // the 64 channels of the head: a fixed tree
                if (on && (lane & 15) == 0) a.delta[((size_t)n * a.H + hh) * a.L + t] = pr;
            } else if (on) {
                const size_t o = (size_t)n * a.kv_img + (size_t)hh * a.kv_head + (size_t)t * a.kv_row + cl;
                bad |= prep_scan(*reinterpret_cast<const float4*>(a.v + o), a.pre, &mx);
                bad |= prep_scan(*reinterpret_cast<const float4*>(a.k + o), a.pre, nullptr);
            }
        }
    }
    for (int m = 1; m < 64; m <<= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)mx, m, 64);
        mx = o > mx ? o : mx;
    }
    if (lane == 0) smx[wave] = mx;
    if (a.overflow && __any(bad) && lane == 0) atomicOr(a.overflow, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned m = smx[0];
        for (int w = 1; w < 4; ++w) m = smx[w] > m ? smx[w] : m;
        if (m) atomicMax(a.scal + 2 * n + (qside ? 0 : 1), m);
    }
}

// One walked tile on its way from global memory to LDS: fp32 in registers while the previous tile is computed.
// b1 / b2: the first (k | q) and the second (v | g) operand of this (image, head), r1 / r2 their row strides in floats.
template <bool KEYS>
struct Staged {
    float a1[KCH][8], a2[KCH][8];
    float t1[VCH][8], t2[KEYS ? VCH : 1][8];
    float st_lse, st_delta;    // KEYS, thread t < KT: the statistics of query t of the tile

    __device__ __forceinline__ void load(const float* b1, long r1, const float* b2, long r2, const float* lse, const float* delta, int Wn,
                                         int jt, int tid) {
        const int j0 = jt * KT;
#pragma unroll
        for (int ci = 0; ci < KCH; ++ci) {
            const int c = tid + ci * NT;
            const int row = c >> 3, sl = c & 7;
            const int j = j0 + row;
#pragma unroll
            for (int e = 0; e < 8; ++e) a1[ci][e] = a2[ci][e] = 0.f;
            if (j < Wn) {
                load8(b1 + (size_t)j * r1 + sl * 8, a1[ci]);
                load8(b2 + (size_t)j * r2 + sl * 8, a2[ci]);
            }
        }
#pragma unroll
        for (int ci = 0; ci < VCH; ++ci) {
            const int c = tid + ci * NT;
            const int d = c & 63, g = c >> 6;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int j = tplane_row(j0, g, e);
                const bool ok = j < Wn;
                t1[ci][e] = ok ? b1[(size_t)j * r1 + d] : 0.f;
                if constexpr (KEYS) t2[ci][e] = ok ? b2[(size_t)j * r2 + d] : 0.f;
            }
        }
        if (KEYS) {
            const int j = j0 + tid;
            const bool valid = tid < KT && j < Wn;
            st_lse = valid ? lse[j] : LSE_NONE;
            st_delta = valid ? delta[j] : 0.f;
        }
    }

    // pre1 / pre2: the power of two of the first (k | q) and the second (v | g) operand; dexp: delta's exponent
    __device__ __forceinline__ void store(unsigned char* st, float pre1, float pre2, int dexp, int tid) {
#pragma unroll
        for (int ci = 0; ci < KCH; ++ci) {
            const int c = tid + ci * NT;
            f16x8 hi, lo;
            const int off = row_off(c >> 3, c & 7);
            split8(a1[ci], pre1, hi, lo);
            *reinterpret_cast<f16x8*>(st + off) = hi;
            *reinterpret_cast<f16x8*>(st + PLANE + off) = lo;
            split8(a2[ci], pre2, hi, lo);
            *reinterpret_cast<f16x8*>(st + OFF_A2 + off) = hi;
            *reinterpret_cast<f16x8*>(st + OFF_A2 + PLANE + off) = lo;
        }
#pragma unroll
        for (int ci = 0; ci < VCH; ++ci) {
            const int c = tid + ci * NT;
            const int off = row_off(c & 63, c >> 6);
            *reinterpret_cast<f16x8*>(st + OFF_T1 + off) = round8(t1[ci], pre1);
            if constexpr (KEYS) *reinterpret_cast<f16x8*>(st + OFF_T2 + off) = round8(t2[ci], pre2);
        }
        if (KEYS && tid < KT) {
            reinterpret_cast<float*>(st + Lds<KEYS>::OFF_ST)[tid] = st_lse;
            reinterpret_cast<float*>(st + Lds<KEYS>::OFF_ST)[KT + tid] = ldexpf(st_delta, dexp);
        }
    }
};

template <bool KEYS>
__global__ __launch_bounds__(NT, KEYS ? 1 : 2) void k_bwd(Args a) {
    constexpr int STAGE = Lds<KEYS>::STAGE, OFF_ST = Lds<KEYS>::OFF_ST;
    __shared__ __attribute__((aligned(16))) unsigned char lds_all[2 * STAGE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    int z, Ib;                             // block -> (image-head z, row block Ib), as in the forward
    tile_coords_of(blockIdx.x, a.nI, a.Z * a.H, z, Ib);
    const int n = z / a.H, hh = z - n * a.H;
    const int Rn = KEYS ? a.S : a.L;       // owned axis
    const int Wn = KEYS ? a.L : a.S;       // walked axis
    const int i0 = Ib * ROWS + 32 * wave;
    const int irow = i0 + l31;
    const bool ook = irow < Rn;

    int ge, eds;
    image_exponents<6>(a.scal, n, a.act_exp, ge, eds);
    const float gpre = ldexpf(1.0f, ge);
    const float dsmul = ldexpf(1.0f, eds);
    const int dexp = ge + a.act_exp;                       // dp = (g 2^ge) . (v 2^act_exp): delta joins it at that scale

    const float* const qb = a.q + (size_t)n * a.q_img + (size_t)hh * a.q_head;
    const float* const kb = a.k + (size_t)n * a.kv_img + (size_t)hh * a.kv_head;
    const float* const vb = a.v + (size_t)n * a.kv_img + (size_t)hh * a.kv_head;
    const float* const gb = a.g + (size_t)n * a.L * a.H * D + (size_t)hh * D;
    const long g_row = (long)a.H * D;
    const float* const lse_z = a.lse + (size_t)z * a.L;
    const float* const delta_z = a.delta + (size_t)z * a.L;

    // ---- this lane's owned row: channels 16 s + 8 h .. + 7 of both planes of both operands (the B operands of the two first products)
    f16x8 xh[QS], xl[QS], yh[QS], yl[QS];
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, y[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (ook) {
            const int co = 16 * s + 8 * h;
            if (KEYS) {
                load8(kb + (size_t)irow * a.kv_row + co, x);
                load8(vb + (size_t)irow * a.kv_row + co, y);
            } else {
                load8(qb + (size_t)irow * a.q_row + co, x);
                load8(gb + (size_t)irow * g_row + co, y);
            }
        }
        split8(x, a.pre, xh[s], xl[s]);
        split8(y, KEYS ? a.pre : gpre, yh[s], yl[s]);
    }
    float lse_l = LSE_NONE, dl = 0.f;                      // !KEYS: this lane's query
    if (!KEYS && ook) {
        lse_l = lse_z[irow];
        dl = ldexpf(delta_z[irow], dexp);
    }

    f32x16 o1[NOB], o2[KEYS ? NOB : 1];
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            o1[ob][r] = 0.f;
            if constexpr (KEYS) o2[ob][r] = 0.f;
        }

    const float* const b1 = KEYS ? qb : kb;
    const float* const b2 = KEYS ? gb : vb;
    const long r1 = KEYS ? a.q_row : a.kv_row, r2 = KEYS ? g_row : a.kv_row;
    const int ntile = (Wn + KT - 1) / KT;
    const float pre2 = KEYS ? gpre : a.pre;
    Staged<KEYS> st;
    st.load(b1, r1, b2, r2, lse_z, delta_z, Wn, 0, tid);
    st.store(lds_all, a.pre, pre2, dexp, tid);
    __syncthreads();
    for (int jt = 0; jt < ntile; ++jt) {
        // tile jt is in stage jt & 1; the other stage was last read before the barrier that ended the previous iteration
        const unsigned char* const lds = lds_all + (jt & 1) * STAGE;
        const bool more = jt + 1 < ntile;
        if (more) st.load(b1, r1, b2, r2, lse_z, delta_z, Wn, jt + 1, tid);

        f32x16 acc[NCT], dpa[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] = dpa[ct][r] = 0.f;
        // attention_f16s.h: score_tile, written out for the scores: with both products through the call the dk / dv kernel takes two
        // more registers
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            f16x8 ch[NCT], cl[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const int off = row_off(32 * ct + l31, 2 * s + h);
                ch[ct] = *reinterpret_cast<const f16x8*>(lds + off);
                cl[ct] = *reinterpret_cast<const f16x8*>(lds + PLANE + off);
            }
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch[ct], xh[s], acc[ct], 0, 0, 0);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch[ct], xl[s], acc[ct], 0, 0, 0);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl[ct], xh[s], acc[ct], 0, 0, 0);
        }
        score_tile<row_off, PLANE>(dpa, lds + OFF_A2, l31, h, yh, yl);
        // accumulator register r of tile column ct is walked row 32 ct + mfma32_row(r, h); the lane is the owned row
        const int nvalid = Wn - jt * KT;                                       // >= 1: walked rows of this tile that exist
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                float ls[8], dd[8];
                if (KEYS) {                                                    // the statistics of this register group's 8 queries
                    const float* const sl = reinterpret_cast<const float*>(lds + OFF_ST) + 32 * ct + 16 * u + 4 * h;
                    const float4 l0 = *reinterpret_cast<const float4*>(sl), l1 = *reinterpret_cast<const float4*>(sl + 8);
                    const float4 d0 = *reinterpret_cast<const float4*>(sl + KT), d1 = *reinterpret_cast<const float4*>(sl + KT + 8);
                    ls[0] = l0.x; ls[1] = l0.y; ls[2] = l0.z; ls[3] = l0.w; ls[4] = l1.x; ls[5] = l1.y; ls[6] = l1.z; ls[7] = l1.w;
                    dd[0] = d0.x; dd[1] = d0.y; dd[2] = d0.z; dd[3] = d0.w; dd[4] = d1.x; dd[5] = d1.y; dd[6] = d1.z; dd[7] = d1.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) { ls[e] = lse_l; dd[e] = dl; }
                }
                f16x8 dsh, ph;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int r = 8 * u + e;
                    float p = __builtin_amdgcn_exp2f(fmaf(acc[ct][r], a.c1, -ls[e]));
                    // a walked row past the end is selected out, whatever the score was (KEYS: its lse2 is 1e30 already)
                    const bool ok = KEYS ? ook : (32 * ct + mfma32_row(r, h) < nvalid);
                    p = ok ? p : 0.f;
                    dsh[e] = (_Float16)(p * ((dpa[ct][r] - dd[e]) * dsmul));
                    if (KEYS) ph[e] = (_Float16)(p * (float)(1 << P_EXP_BWD));
                }
#pragma unroll
                for (int ob = 0; ob < NOB; ++ob) {
                    const int off = row_off(32 * ob + l31, 4 * ct + 2 * u + h);
                    o1[ob] = __builtin_amdgcn_mfma_f32_32x32x16_f16(dsh, *reinterpret_cast<const f16x8*>(lds + OFF_T1 + off), o1[ob], 0, 0, 0);
                    if (KEYS)
                        o2[ob] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ph, *reinterpret_cast<const f16x8*>(lds + OFF_T2 + off), o2[ob], 0, 0, 0);
                }
            }
        }
        if (more) st.store(lds_all + ((jt + 1) & 1) * STAGE, a.pre, pre2, dexp, tid);
        __syncthreads();
    }

    // ---- store: the lane holds channels l31 and 32 + l31 of owned rows i0 + mfma32_row(r, h).  ds carried 2^(ge + act_exp + eds), the
    // transposed q | k plane 2^act_exp; p 2^14 and g 2^ge
    const int e1 = -(ge + 2 * a.act_exp + eds), e2 = -(P_EXP_BWD + ge);
    float* const d1 = KEYS ? a.dk + (size_t)n * a.dkv_img + (size_t)hh * a.dkv_head : a.dq + (size_t)n * a.dq_img + (size_t)hh * a.dq_head;
    float* const d2 = KEYS ? a.dv + (size_t)n * a.dkv_img + (size_t)hh * a.dkv_head : nullptr;
    const long drow = KEYS ? a.dkv_row : a.dq_row;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + mfma32_row(r, h);
        if (i < Rn) {
#pragma unroll
            for (int ob = 0; ob < NOB; ++ob) {
                const size_t o = (size_t)i * drow + 32 * ob + l31;
                d1[o] = ldexpf(o1[ob][r] * a.c, e1);
                if constexpr (KEYS) d2[o] = ldexpf(o2[ob][r], e2);
            }
        }
    }
}

// per image: 256 bytes for the two maxima, then delta (H, L) rounded up to 256 bytes -- linear in Z
inline size_t image_bytes(int L, int H) { return 256 + align256((size_t)H * L * 4); }

}  // namespace

extern "C" {

// Bytes of workspace far_vit_attention_bwd_f16s needs: the per-image maxima and delta (Z, H, L).  No GPU involved; 0 for D != 64, Z = 0
// or a size the kernels refuse; linear in Z.
size_t far_vit_attention_bwd_workspace_bytes(int Z, int L, int S, int H, int D) {
    if (Z <= 0 || L <= 0 || S <= 0 || H <= 0 || D != 64) return 0;
    return (size_t)Z * image_bytes(L, H);
}

// (dq, dk, dv) of far_vit_attention_train_f16s for the output gradient g.  q, k, v: addressed by strides as in the forward; out, g:
// (Z, L, H 64) fp32 contiguous; lse: the (Z, H, L) row statistic the training forward wrote (same act_exp).  Row (n, h, l) of dq is the
// 64 contiguous floats at dq + n dq_img + h dq_head + l dq_row; dk, dv rows likewise with the dkv strides.  Every stride a multiple of
// 4, rows at least 64 apart, base pointers 16-byte aligned, D = 64, else FAR_EINVAL.  ws: far_vit_attention_bwd_workspace_bytes bytes.
// overflow |= 1 when a q / k / v / g value is out of range or not finite.
int far_vit_attention_bwd_f16s(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* g, int Z,
                               int L, int S, int H, int D, long q_img, long q_head, long q_row, long kv_img, long kv_head, long kv_row,
                               int act_exp, float* dq, float* dk, float* dv, long dq_img, long dq_head, long dq_row, long dkv_img,
                               long dkv_head, long dkv_row, void* ws, int* overflow, hipStream_t stream) {
    far_clear_errors();
    if (Z == 0) return FAR_OK;
    if (!q || !k || !v || !out || !lse || !g || !dq || !dk || !dv || !ws || Z < 0 || L <= 0 || S <= 0 || H <= 0 || D != 64 || act_exp < -24 ||
        act_exp > 8)
        return FAR_EINVAL;
    if (((q_img | q_head | q_row | kv_img | kv_head | kv_row | dq_img | dq_head | dq_row | dkv_img | dkv_head | dkv_row) & 3) || q_img < 0 ||
        q_head < 0 || q_row < 64 || kv_img < 0 || kv_head < 0 || kv_row < 64 || dq_img < 0 || dq_head < 0 || dq_row < 64 || dkv_img < 0 ||
        dkv_head < 0 || dkv_row < 64)
        return FAR_EINVAL;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)g | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv |
         (uintptr_t)ws) & 15)
        return FAR_EINVAL;
    if ((uintptr_t)lse & 3) return FAR_EINVAL;
    const long ZH = (long)Z * H;
    const int nIq = (L + ROWS - 1) / ROWS, nIk = (S + ROWS - 1) / ROWS;
    const long bq = ZH * nIq, bk = ZH * nIk;
    const long bp = (long)Z * ((L + PREP_TOK - 1) / PREP_TOK + (S + PREP_TOK - 1) / PREP_TOK);
    if (bq > 0x7fffffffL || bk > 0x7fffffffL || ZH > 0x7fffffffL || bp > 0x7fffffffL) return FAR_EINVAL;
    unsigned char* const b = (unsigned char*)ws;
    Args a;
    a.q = q; a.k = k; a.v = v; a.g = g; a.out = out; a.lse = lse;
    a.dq = dq; a.dk = dk; a.dv = dv; a.overflow = overflow;
    a.scal = (unsigned*)b;
    a.delta = (float*)(b + (size_t)Z * 256);
    a.q_img = q_img; a.q_head = q_head; a.q_row = q_row; a.kv_img = kv_img; a.kv_head = kv_head; a.kv_row = kv_row;
    a.dq_img = dq_img; a.dq_head = dq_head; a.dq_row = dq_row; a.dkv_img = dkv_img; a.dkv_head = dkv_head; a.dkv_row = dkv_row;
    a.Z = Z; a.L = L; a.S = S; a.H = H; a.act_exp = act_exp; a.nI = 0;
    a.pre = ldexpf(1.0f, act_exp);
    a.c1 = ldexpf(1.44269504088896341f / 8.0f, -2 * act_exp);                  // scores -> log2 domain, as in the forward
    a.c = 1.0f / 8.0f;
    if (hipMemsetAsync(a.scal, 0, (size_t)Z * 2 * 4, stream) != hipSuccess) return far_check_launch();
    hipLaunchKernelGGL(k_prep, dim3((unsigned)bp), dim3(256), 0, stream, a);
    a.nI = nIq;
    hipLaunchKernelGGL(k_bwd<false>, dim3((unsigned)bq), dim3(NT), 0, stream, a);
    a.nI = nIk;
    hipLaunchKernelGGL(k_bwd<true>, dim3((unsigned)bk), dim3(NT), 0, stream, a);
    return far_check_launch();
}

}  // extern "C"

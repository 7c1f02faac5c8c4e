// K22 backward: the gradients of LoFTR's full (softmax) attention core (full_attention_f16s.hip) on the f16 matrix cores.
//
// Per (image n, head h), c = 1 / sqrt(D), with the forward's saved row statistic lse2_i = log2 sum_j 2^(c log2(e) q_i.k_j):
//   p_ij = 2^(x_ij - lse2_i)      delta_i = g_i.o_i      dv_j = sum_i p_ij g_i      dp_ij = g_i.v_j      ds_ij = p_ij (dp_ij - delta_i)
//   dq_i = c sum_j ds_ij k_j                            dk_j = c sum_i ds_ij q_i
// No (L, S)-sized tensor exists: both kernels recompute score tiles as the forward does.  Three launches (+ a combine where an axis is split):
//   k_prep   one wave per token: delta (N, H, L) from g and the saved output, the per-image max |g| (rows that take part) and max |v|
//            (valid keys) as integer atomicMax on the float bits -- order-independent --, and the range guard of q, k, v, g.
//   k_bwd<KEYS = false>  dq: a workgroup owns 128 query rows (a lane ONE query, as in the forward) and walks the keys in tiles of 64.
//   k_bwd<KEYS = true>   dk, dv: a workgroup owns 128 keys (a lane ONE key) and walks the queries in tiles of 64; dk and dv come from
//            the same recomputed tile.
// One template is both kernels, on the backward recipe of attention_f16s.h (read its header first): the owned side's two operands
// (q, g | k, v) sit in registers as the B operands of the two first products, the walked side's tile (k, v | q, g) is staged through
// LDS exactly like the forward's k tile (fp32 loads of the NEXT tile in flight during the MFMAs, XOR-swizzled 16-byte slots), plus
// its transpose for the output products.
//   scores   x = A1 . X, split operands around the forward's activation exponent: p = 2^(x c1 - lse2) agrees with the saved
//            statistic (a plain-fp16 recompute would be off by percent at |score| ~ 60).
//   dp       A2 . Y the same way (split operands): dp - delta cancels, plain fp16 g and v would cost 1e-3 on dq and dk.
//   outputs  ds and p go from the accumulator registers into the next MFMA as plain fp16 A operands (the forward's P V step), against
//            the transposed hi plane of k (dq), q (dk) and g (dv).
// Gradient scale: g is multiplied by 2^ge so that the image's max |g| lands in [2^12, 2^13), ds by 2^eds chosen from max |v| so that
// |ds| <= 2 D max|g| max|v| stays below 2^15: both exponents are read from device memory (no host synchronisation), the results are
// scaled back by exact powers of two.  They are per IMAGE: an image's bits do not depend on the rest of the batch.
// Masks: a masked key takes no part (p selected to 0: dk = dv = exact 0 there, its k / v values are never read); a padded query row
// carries lse2 = +1e30 (p = 0) and g read as 0: dq = exact 0 there; an image without a valid key has lse2 = +1e30 everywhere.
// Short owned side: the walked axis is split across workgroups (split_plan, as the forward), partial sums go to the workspace and
// k_bwd_combine adds them in split order.  No float atomics, no data handed between the workgroups of one launch.
#include "attention_f16s.h"

namespace {

template <int D_, int NCT_, int WAVES_, bool KEYS_>
struct Cfg {
    static constexpr int D = D_, NCT = NCT_, WAVES = WAVES_;
    static constexpr bool KEYS = KEYS_;
    static constexpr int KT = 32 * NCT;              // walked rows per tile
    static constexpr int NT = 64 * WAVES;            // threads
    static constexpr int NS = D / 8;                 // 16-byte slots of a row
    static constexpr int VS = KT / 8;                // 16-byte slots of a transposed row
    static constexpr int A_PLANE = KT * D * 2;       // bytes of one row-major plane (hi or lo)
    static constexpr int T_PLANE = 32 * KT * 2;      // bytes of one transposed plane: 32 rows (d; rows >= D are zero) x KT
    static constexpr int OFF_A2 = 2 * A_PLANE;
    static constexpr int OFF_T1 = 4 * A_PLANE;
    static constexpr int OFF_T2 = OFF_T1 + T_PLANE;
    static constexpr int OFF_ST = OFF_T1 + (KEYS ? 2 : 1) * T_PLANE;   // KEYS: lse2[KT], delta[KT] floats; else the 64-bit validity word
    static constexpr int STAGE = OFF_ST + (KEYS ? KT * 8 : 16);
    static constexpr int KCH = (KT * NS + NT - 1) / NT;      // row-major chunks (8 channels of one row) per thread and operand
    static constexpr int VCH = (32 * VS + NT - 1) / NT;      // transposed items (8 rows of one channel) per thread and operand
    static constexpr int K_SW = D == 32 ? 2 : 3;
    static constexpr int V_SW = VS == 8 ? 1 : 2;
    static __device__ __forceinline__ int a_off(int row, int c) { return row * (D * 2) + ((c ^ ((row >> K_SW) & (NS - 1))) * 16); }
    static __device__ __forceinline__ int t_off(int d, int slot) { return d * (KT * 2) + ((slot ^ ((d >> V_SW) & (VS - 1))) * 16); }
};

struct Args {
    const float *q, *k, *v, *g, *out, *lse;
    const unsigned char *qm, *kvm;
    float *dq, *dk, *dv;
    unsigned* scal;        // [N][2]: bits of max |g|, max |v| of the image
    float* delta;          // [N H][L]
    float *part1, *part2;  // split runs: [z][split][owned rows][D] partial dq | dk, dv
    int* overflow;
    int N, L, S, H, nI, nsplit, tps, act_exp;
    float pre, c1, c;
};

// ---- delta, the per-image maxima and the range guard: one wave per token (query rows first, then key rows), four per workgroup
__global__ __launch_bounds__(256) void k_prep(Args a, int D) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long nq = (long)a.N * a.L, total = nq + (long)a.N * a.S;
    if (row >= total) return;
    const int Cst = a.H * D;
    unsigned mx = 0;
    bool bad = false;
    int slot;
    if (row < nq) {
        const int n = (int)(row / a.L), l = (int)(row - (long)n * a.L);
        const bool ok = !a.qm || a.qm[row];
        slot = 2 * n;
        for (int c0 = 0; c0 < Cst; c0 += 64) {
            const int c = c0 + lane;
            float pr = 0.f;
            if (ok && c < Cst) {
                const float gv = a.g[row * Cst + c];
                pr = gv * a.out[row * Cst + c];
                const unsigned gb = __float_as_uint(fabsf(gv));
                mx = gb > mx ? gb : mx;
                bad |= gb >= 0x7f800000u;
                bad |= !(fabsf(a.q[row * Cst + c]) * a.pre <= 65504.0f);
            }
            for (int m = 1; m < D; m <<= 1) pr += shfl_xor_f(pr, m);          // the D channels of a head: a fixed tree
            if (c < Cst && (c % D) == 0) a.delta[((size_t)n * a.H + c / D) * a.L + l] = pr;
        }
    } else {
        const long r = row - nq;
        const int n = (int)(r / a.S);
        const bool ok = !a.kvm || a.kvm[r];
        slot = 2 * n + 1;
        for (int c = lane; ok && c < Cst; c += 64) {
            const float vv = a.v[r * Cst + c];
            const unsigned vb = __float_as_uint(fabsf(vv));
            mx = vb > mx ? vb : mx;
            bad |= !(fabsf(vv) * a.pre <= 65504.0f);
            bad |= !(fabsf(a.k[r * Cst + c]) * a.pre <= 65504.0f);
        }
    }
    for (int m = 1; m < 64; m <<= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)mx, m, 64);
        mx = o > mx ? o : mx;
    }
    if (lane == 0 && mx) atomicMax(a.scal + slot, mx);
    if (a.overflow && __any(bad) && lane == 0) atomicOr(a.overflow, 1);
}

// One walked tile on its way from global memory to LDS: fp32 in registers while the previous tile is computed.
template <class C>
struct Staged {
    float a1[C::KCH][8], a2[C::KCH][8];
    float t1[C::VCH][8], t2[C::KEYS ? C::VCH : 1][8];
    float st_lse, st_delta;    // KEYS, thread t < KT: the statistics of query t of the tile
    bool valid;                // else, thread t < KT: key t of the tile takes part

    __device__ __forceinline__ void load(const Args& a, int n, int hh, int z, int jt, int tid) {
        const int Cst = a.H * C::D;
        const int j0 = jt * C::KT;
        const int Wn = C::KEYS ? a.L : a.S;
        const unsigned char* const wm0 = C::KEYS ? a.qm : a.kvm;
        const unsigned char* const wm = wm0 ? wm0 + (size_t)n * Wn : nullptr;
        const float* const b1 = (C::KEYS ? a.q : a.k) + (size_t)n * Wn * Cst + hh * C::D;
        const float* const b2 = (C::KEYS ? a.g : a.v) + (size_t)n * Wn * Cst + hh * C::D;
#pragma unroll
        for (int ci = 0; ci < C::KCH; ++ci) {
            const int c = tid + ci * C::NT;
            const int row = c / C::NS, sl = c % C::NS;
            const int j = j0 + row;
            const bool ok = c < C::KT * C::NS && j < Wn && (!wm || wm[j]);
#pragma unroll
            for (int e = 0; e < 8; ++e) a1[ci][e] = a2[ci][e] = 0.f;
            if (ok) {
                load8(b1 + (size_t)j * Cst + sl * 8, a1[ci]);
                load8(b2 + (size_t)j * Cst + sl * 8, a2[ci]);
            }
        }
#pragma unroll
        for (int ci = 0; ci < C::VCH; ++ci) {
            const int c = tid + ci * C::NT;
            const int d = c & 31, g = c >> 5;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int j = tplane_row(j0, g, e);
                const bool ok = c < 32 * C::VS && d < C::D && j < Wn && (!wm || wm[j]);
                t1[ci][e] = ok ? b1[(size_t)j * Cst + d] : 0.f;
                if (C::KEYS) t2[ci][e] = ok ? b2[(size_t)j * Cst + d] : 0.f;
            }
        }
        const int j = j0 + tid;
        valid = tid < C::KT && j < Wn && (!wm || wm[j]);
        if (C::KEYS) {
            st_lse = valid ? a.lse[(size_t)z * a.L + j] : LSE_NONE;
            st_delta = valid ? a.delta[(size_t)z * a.L + j] : 0.f;
        }
    }

    // pre1 / pre2: the power of two of the first (q | k) and the second (g | v) operand; dexp: delta's exponent
    __device__ __forceinline__ void store(unsigned char* st, float pre1, float pre2, int dexp, int tid) {
#pragma unroll
        for (int ci = 0; ci < C::KCH; ++ci) {
            const int c = tid + ci * C::NT;
            if (c < C::KT * C::NS) {
                f16x8 hi, lo;
                const int off = C::a_off(c / C::NS, c % C::NS);
                split8(a1[ci], pre1, hi, lo);
                *reinterpret_cast<f16x8*>(st + off) = hi;
                *reinterpret_cast<f16x8*>(st + C::A_PLANE + off) = lo;
                split8(a2[ci], pre2, hi, lo);
                *reinterpret_cast<f16x8*>(st + C::OFF_A2 + off) = hi;
                *reinterpret_cast<f16x8*>(st + C::OFF_A2 + C::A_PLANE + off) = lo;
            }
        }
#pragma unroll
        for (int ci = 0; ci < C::VCH; ++ci) {
            const int c = tid + ci * C::NT;
            if (c < 32 * C::VS) {
                const int off = C::t_off(c & 31, c >> 5);
                *reinterpret_cast<f16x8*>(st + C::OFF_T1 + off) = round8(t1[ci], pre1);
                if (C::KEYS) *reinterpret_cast<f16x8*>(st + C::OFF_T2 + off) = round8(t2[ci], pre2);
            }
        }
        if (C::KEYS) {
            if (tid < C::KT) {
                reinterpret_cast<float*>(st + C::OFF_ST)[tid] = st_lse;
                reinterpret_cast<float*>(st + C::OFF_ST)[C::KT + tid] = ldexpf(st_delta, dexp);
            }
        } else if (tid < 64) {                                       // wave 0: lane t = key t
            const unsigned long long m = __ballot(valid);
            if (tid == 0) *reinterpret_cast<unsigned long long*>(st + C::OFF_ST) = m;
        }
    }
};

template <int D, int NCT, int WAVES, bool KEYS>
__global__ __launch_bounds__(64 * WAVES, 2) void k_bwd(Args a) {
    typedef Cfg<D, NCT, WAVES, KEYS> C;
    constexpr int KT = C::KT, QS = D / 16, ROWS = 32 * WAVES;
    __shared__ __attribute__((aligned(16))) unsigned char lds_all[2 * C::STAGE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    // block -> (split, image-head z, row block Ib), as in the forward
    const int Z = a.N * a.H;
    const int per = a.nI * Z;
    const int sp = blockIdx.x / per;
    int z, Ib;
    tile_coords_of(blockIdx.x - sp * per, a.nI, Z, z, Ib);
    const int n = z / a.H, hh = z - n * a.H;
    const int Cst = a.H * D;
    const int Rn = KEYS ? a.S : a.L;       // owned axis
    const int Wn = KEYS ? a.L : a.S;       // walked axis
    const int i0 = Ib * ROWS + 32 * wave;
    const int irow = i0 + l31;
    const unsigned char* const om = KEYS ? a.kvm : a.qm;
    const bool ook = irow < Rn && (!om || om[(size_t)n * Rn + irow]);

    int ge, eds;
    image_exponents<D == 32 ? 5 : 4>(a.scal, n, a.act_exp, ge, eds);
    const float gpre = ldexpf(1.0f, ge);
    const float dsmul = ldexpf(1.0f, eds);
    const int dexp = ge + a.act_exp;                       // dp = (g 2^ge) . (v 2^act_exp): delta joins it at that scale

    // ---- this lane's owned row: channels 16 s + 8 h .. + 7 of both planes of both operands (the B operands of the two first products)
    f16x8 xh[QS], xl[QS], yh[QS], yl[QS];
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, y[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (ook) {
            const size_t o = ((size_t)n * Rn + irow) * Cst + hh * D + 16 * s + 8 * h;
            load8((KEYS ? a.k : a.q) + o, x);
            load8((KEYS ? a.v : a.g) + o, y);
        }
        split8(x, a.pre, xh[s], xl[s]);
        split8(y, KEYS ? a.pre : gpre, yh[s], yl[s]);
    }
    float lse_l = LSE_NONE, dl = 0.f;                      // !KEYS: this lane's query
    if (!KEYS && ook) {
        lse_l = a.lse[(size_t)z * a.L + irow];
        dl = ldexpf(a.delta[(size_t)z * a.L + irow], dexp);
    }

    f32x16 o1, o2;
#pragma unroll
    for (int r = 0; r < 16; ++r) o1[r] = o2[r] = 0.f;

    const int ntile = (Wn + KT - 1) / KT;
    const int t0 = sp * a.tps;
    const int t1 = t0 + a.tps < ntile ? t0 + a.tps : ntile;
    const float pre2 = KEYS ? gpre : a.pre;
    Staged<C> st;
    if (t0 < t1) {
        st.load(a, n, hh, z, t0, tid);
        st.store(lds_all, a.pre, pre2, dexp, tid);
    }
    __syncthreads();
    for (int jt = t0; jt < t1; ++jt) {
        // tile jt is in stage (jt - t0) & 1; the other stage was last read before the barrier that ended the previous iteration
        const unsigned char* const lds = lds_all + ((jt - t0) & 1) * C::STAGE;
        const bool more = jt + 1 < t1;
        if (more) st.load(a, n, hh, z, jt + 1, tid);

        f32x16 acc[NCT], dpa[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] = dpa[ct][r] = 0.f;
        score_tile<C::a_off, C::A_PLANE>(acc, lds, l31, h, xh, xl);
        // the same for dp, written out: with both products through the call the D = 32 one-wave dq form changes its register count
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            f16x8 ch[NCT], cl[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const int off = C::OFF_A2 + C::a_off(32 * ct + l31, 2 * s + h);
                ch[ct] = *reinterpret_cast<const f16x8*>(lds + off);
                cl[ct] = *reinterpret_cast<const f16x8*>(lds + C::A_PLANE + off);
            }
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) dpa[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch[ct], yh[s], dpa[ct], 0, 0, 0);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) dpa[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch[ct], yl[s], dpa[ct], 0, 0, 0);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) dpa[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl[ct], yh[s], dpa[ct], 0, 0, 0);
        }
        // accumulator register r of tile column ct is walked row 32 ct + mfma32_row(r, h); the lane is the owned row
        unsigned kv[NCT] = {};
        if (!KEYS) {
            const unsigned long long km = *reinterpret_cast<const unsigned long long*>(lds + C::OFF_ST);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) kv[ct] = (unsigned)(km >> (32 * ct)) >> (4 * h);
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                float ls[8], dd[8];
                if (KEYS) {                                                    // the statistics of this register group's 8 queries
                    const float* const sl = reinterpret_cast<const float*>(lds + C::OFF_ST) + 32 * ct + 16 * u + 4 * h;
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
                    const bool ok = KEYS ? ook : (((kv[ct] >> ((r & 3) + 8 * (r >> 2))) & 1u) != 0);
                    p = ok ? p : 0.f;                                          // a masked key is selected out, whatever the score was
                    dsh[e] = (_Float16)(p * ((dpa[ct][r] - dd[e]) * dsmul));
                    if (KEYS) ph[e] = (_Float16)(p * (float)(1 << P_EXP_BWD));
                }
                const int off = C::t_off(l31, 4 * ct + 2 * u + h);
                o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(dsh, *reinterpret_cast<const f16x8*>(lds + C::OFF_T1 + off), o1, 0, 0, 0);
                if (KEYS) o2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ph, *reinterpret_cast<const f16x8*>(lds + C::OFF_T2 + off), o2, 0, 0, 0);
            }
        }
        if (more) st.store(lds_all + ((jt + 1 - t0) & 1) * C::STAGE, a.pre, pre2, dexp, tid);
        __syncthreads();
    }

    // ---- store: the lane holds channel d = l31 of owned rows i0 + mfma32_row(r, h).  ds carried 2^(ge + act_exp + eds), the
    // transposed q | k plane 2^act_exp; p 2^14 and g 2^ge
    const int e1 = -(ge + 2 * a.act_exp + eds), e2 = -(P_EXP_BWD + ge);
    float* const d1 = KEYS ? a.dk : a.dq;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + mfma32_row(r, h);
        if (l31 < D && i < Rn) {
            const float y1 = ldexpf(o1[r] * a.c, e1);
            const float y2 = KEYS ? ldexpf(o2[r], e2) : 0.f;
            if (a.nsplit > 1) {
                const size_t o = ((((size_t)z * a.nsplit + sp) * Rn) + i) * D + l31;
                a.part1[o] = y1;
                if (KEYS) a.part2[o] = y2;
            } else {
                const size_t o = ((size_t)n * Rn + i) * Cst + hh * D + l31;
                d1[o] = y1;
                if (KEYS) a.dv[o] = y2;
            }
        }
    }
}

// The partial gradients of a split run, added in split order: one thread per value.
__global__ __launch_bounds__(256) void k_bwd_combine(const float* p1, const float* p2, float* d1, float* d2, int N, int H, int Rn, int D,
                                                     int nsplit) {
    const size_t total = (size_t)N * H * Rn * D;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int d = (int)(t % D);
    const size_t row = t / D;
    const int i = (int)(row % Rn);
    const size_t z = row / Rn;
    const int n = (int)(z / H), hh = (int)(z - (size_t)n * H);
    float s1 = 0.f, s2 = 0.f;
    for (int sp = 0; sp < nsplit; ++sp) {
        const size_t o = ((z * nsplit + sp) * Rn + i) * D + d;
        s1 += p1[o];
        if (p2) s2 += p2[o];
    }
    const size_t o = ((size_t)n * Rn + i) * ((size_t)H * D) + hh * D + d;
    d1[o] = s1;
    if (p2) d2[o] = s2;
}

struct Layout {
    bool small;
    SplitPlan pq, pk;          // dq: owns L, walks S; dk / dv: owns S, walks L
    size_t off_delta, off_pq, off_pk, off_pv, bytes;
};
inline Layout layout(int N, int L, int S, int H, int D) {
    Layout w;
    w.small = L <= 32 && S <= 32;          // both axes are walked: the one-wave form needs both short
    w.pq = split_plan(L, S, H, w.small);
    w.pk = split_plan(S, L, H, w.small);
    size_t o = align256((size_t)N * 2 * 4);
    w.off_delta = o; o += align256((size_t)N * H * L * 4);
    w.off_pq = o; if (w.pq.nsplit > 1) o += align256((size_t)N * H * w.pq.nsplit * L * D * 4);
    w.off_pk = o; if (w.pk.nsplit > 1) o += align256((size_t)N * H * w.pk.nsplit * S * D * 4);
    w.off_pv = o; if (w.pk.nsplit > 1) o += align256((size_t)N * H * w.pk.nsplit * S * D * 4);
    w.bytes = o;
    return w;
}

template <bool KEYS>
void launch_bwd(const Args& a, bool small, int D, long blocks, hipStream_t stream) {
    const dim3 grid((unsigned)blocks);
    if (small) {
        if (D == 32) hipLaunchKernelGGL((k_bwd<32, 1, 1, KEYS>), grid, dim3(64), 0, stream, a);
        else hipLaunchKernelGGL((k_bwd<16, 1, 1, KEYS>), grid, dim3(64), 0, stream, a);
    } else {
        if (D == 32) hipLaunchKernelGGL((k_bwd<32, 2, 4, KEYS>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((k_bwd<16, 2, 4, KEYS>), grid, dim3(256), 0, stream, a);
    }
}

}  // namespace

extern "C" {

// Bytes of workspace far_full_attention_bwd_f16s needs: the per-image maxima, delta (N, H, L) and the partial gradients of a split
// axis.  No GPU involved.
size_t far_full_attention_bwd_workspace_bytes(int N, int L, int S, int H, int D) {
    if (N <= 0 || L <= 0 || S <= 0 || H <= 0 || (D != 16 && D != 32)) return 0;
    return layout(N, L, S, H, D).bytes;
}

// (dq, dk, dv) of far_full_attention_train_f16s for the output gradient g.  q, g, out, dq: (N, L, H D); k, v, dk, dv: (N, S, H D) fp32
// contiguous; lse: the (N, H, L) row statistic the training forward wrote; masks and act_exp as in the forward.  ws:
// far_full_attention_bwd_workspace_bytes bytes.  overflow |= 1 when a q / k / v / g value that takes part is out of range or not finite.
int far_full_attention_bwd_f16s(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* g,
                                int N, int L, int S, int H, int D, const unsigned char* q_mask, const unsigned char* kv_mask,
                                int act_exp, float* dq, float* dk, float* dv, void* ws, int* overflow, hipStream_t stream) {
    far_clear_errors();
    if (N == 0) return FAR_OK;
    if (!q || !k || !v || !out || !lse || !g || !dq || !dk || !dv || !ws || N < 0 || L <= 0 || S <= 0 || H <= 0 || (D != 16 && D != 32) ||
        act_exp < -24 || act_exp > 8)
        return FAR_EINVAL;
    const Layout w = layout(N, L, S, H, D);
    const long Z = (long)N * H;
    const long bq = Z * w.pq.nI * w.pq.nsplit, bk = Z * w.pk.nI * w.pk.nsplit;
    const long tokens = (long)N * ((long)L + S);
    if (bq > 0x7fffffffL || bk > 0x7fffffffL || Z > 0x7fffffffL || (tokens + 3) / 4 > 0x7fffffffL) return FAR_EINVAL;
    unsigned char* const b = (unsigned char*)ws;
    Args a;
    a.q = q; a.k = k; a.v = v; a.g = g; a.out = out; a.lse = lse; a.qm = q_mask; a.kvm = kv_mask;
    a.dq = dq; a.dk = dk; a.dv = dv; a.overflow = overflow;
    a.scal = (unsigned*)b;
    a.delta = (float*)(b + w.off_delta);
    a.N = N; a.L = L; a.S = S; a.H = H; a.act_exp = act_exp;
    a.pre = ldexpf(1.0f, act_exp);
    a.c1 = ldexpf(1.44269504088896341f / sqrtf((float)D), -2 * act_exp);       // scores -> log2 domain, as in the forward
    a.c = 1.0f / sqrtf((float)D);
    a.nI = 0; a.nsplit = 1; a.tps = 0; a.part1 = a.part2 = nullptr;
    if (hipMemsetAsync(a.scal, 0, (size_t)N * 2 * 4, stream) != hipSuccess) return far_check_launch();
    hipLaunchKernelGGL(k_prep, dim3((unsigned)((tokens + 3) / 4)), dim3(256), 0, stream, a, D);

    a.nI = w.pq.nI; a.nsplit = w.pq.nsplit; a.tps = w.pq.tps;
    a.part1 = (float*)(b + w.off_pq); a.part2 = nullptr;
    launch_bwd<false>(a, w.small, D, bq, stream);
    if (w.pq.nsplit > 1) {
        const size_t total = (size_t)Z * L * D;
        hipLaunchKernelGGL(k_bwd_combine, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a.part1, (const float*)nullptr, dq,
                           (float*)nullptr, N, H, L, D, w.pq.nsplit);
    }
    a.nI = w.pk.nI; a.nsplit = w.pk.nsplit; a.tps = w.pk.tps;
    a.part1 = (float*)(b + w.off_pk); a.part2 = (float*)(b + w.off_pv);
    launch_bwd<true>(a, w.small, D, bk, stream);
    if (w.pk.nsplit > 1) {
        const size_t total = (size_t)Z * S * D;
        hipLaunchKernelGGL(k_bwd_combine, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a.part1, (const float*)a.part2, dk,
                           dv, N, H, S, D, w.pk.nsplit);
    }
    return far_check_launch();
}

}  // extern "C"

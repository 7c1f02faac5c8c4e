// K22: LoFTR's full (softmax) attention core on the f16 matrix cores with split-precision operands.
//
// Operator (reference: mp3d_loftr/src/loftr/loftr_module/linear_attention.py:55-88, inference, no dropout):
//   out[n, l, h, :] = sum_s softmax_s(q[n,l,h,:] . k[n,s,h,:] / sqrt(D)) v[n,s,h,:]
// q (N, L, H D), k, v (N, S, H D), out (N, L, H D): fp32, contiguous raw projections with the heads concatenated (K5's layout).
// The (N, L, S, H) score tensor of the reference never exists: one workgroup owns 128 query rows of one (image, head) -- 32 per
// wave -- and walks the keys in tiles of 64 with the forward recipe of attention_f16s.h (read its header first):
//   stage    the tile's k and v rows are read as fp32 (the NEXT tile's loads are in flight while this one is computed), scaled by
//            2^act_exp, split and written to LDS: k as [key][D] rows with XOR-swizzled 16-byte slots, v transposed to [d][keys].
//            There is no preparation launch and no operand workspace: a tile costs a thread 16 splits, against 32 exponentials.
//            Masked keys and keys past S are written as zeros and counted out in a 64-bit validity word.
//   scores   S^T tile D[m = key][n = query] = k . q: a lane owns ONE query, its 32 keys sit in the accumulator registers of the two
//            half-waves.  A rescale of the row reference is rare after the first tiles: behind a wave-uniform test.  An invalid key
//            is selected to p = 0.
//   P V      p is split straight from the accumulator registers and multiplied with the v^T tile: D[m = query][n = d], again
//            three MFMAs per product.
//   store    out = acc / rowsum 2^-act_exp; a padded query row, and every row of an image without a valid key, is exact zero.
// Sequences of at most 32 keys (the fine level's 25-token windows) run the same code as one wave per (image, head) and a
// single 32-key tile: a 64-key tile and four waves would spend three quarters of their MFMAs on padding.
// Few workgroups per image (short L, long S): the key axis is split across workgroups, the partial (R, rowsum, acc) triples
// go to the workspace and k_combine adds them in split order.  The split count depends on (L, S, H) only, never on N.
// No float atomics; an image's bits do not depend on the rest of the batch.
// Range: |x| 2^act_exp <= 65504 for every q / k / v value that takes part (valid keys, unpadded queries).
#include "attention_f16s.h"
#include <type_traits>

namespace {

template <int D_, int NCT_, int WAVES_>
struct Cfg {
    static constexpr int D = D_, NCT = NCT_, WAVES = WAVES_;
    static constexpr int KT = 32 * NCT;              // keys per tile
    static constexpr int NT = 64 * WAVES;            // threads
    static constexpr int NS = D / 8;                 // 16-byte slots of a k row
    static constexpr int VS = KT / 8;                // 16-byte slots of a v^T row
    static constexpr int K_PLANE = KT * D * 2;       // bytes of one k plane (hi or lo)
    static constexpr int V_PLANE = 32 * KT * 2;      // bytes of one v^T plane: 32 rows (d; rows >= D are zero) x KT keys
    static constexpr int MASK_OFF = 2 * K_PLANE + 2 * V_PLANE;
    static constexpr int STAGE = MASK_OFF + 16;
    static constexpr int KCH = (KT * NS + NT - 1) / NT;      // k chunks (8 channels of one key) per thread
    static constexpr int VCH = (32 * VS + NT - 1) / NT;      // v^T items (8 keys of one channel) per thread
    static constexpr int K_SW = D == 32 ? 2 : 3;
    static constexpr int V_SW = VS == 8 ? 1 : 2;
    // 16-byte slot c of key row `key`: the XOR spreads the 16 rows a quarter-wave reads over all banks
    static __device__ __forceinline__ int k_off(int key, int c) { return key * (D * 2) + ((c ^ ((key >> K_SW) & (NS - 1))) * 16); }
    static __device__ __forceinline__ int v_off(int d, int slot) { return d * (KT * 2) + ((slot ^ ((d >> V_SW) & (VS - 1))) * 16); }
};

struct Args {
    const float *q, *k, *v;
    const unsigned char *qm, *kvm;
    float* out;
    float* lse;            // training forward: (N, H, L) log2-domain log-sum-exp of each row (NULL: inference)
    float* part_acc;       // split runs: [z][split][L][D] unnormalised accumulators,
    float* part_sum;       //             [z][split][L] row sums and
    int* part_ref;         //             [z][split][L] row references
    int* overflow;
    int N, L, S, H, nI, nsplit, tps;
    float pre, c1, out_mul;
};

// One key tile on its way from global memory to LDS: fp32 in registers while the previous tile is computed.
template <class C>
struct Staged {
    float kx[C::KCH][8];
    float vx[C::VCH][8];
    bool valid;            // thread t < KT: key t of the tile takes part

    __device__ __forceinline__ void load(const Args& a, int n, int hh, int jt, int tid) {
        const int Cst = a.H * C::D;
        const int j0 = jt * C::KT;
        const unsigned char* const km = a.kvm ? a.kvm + (size_t)n * a.S : nullptr;
        const float* const kb = a.k + (size_t)n * a.S * Cst + hh * C::D;
        const float* const vb = a.v + (size_t)n * a.S * Cst + hh * C::D;
#pragma unroll
        for (int ci = 0; ci < C::KCH; ++ci) {
            const int c = tid + ci * C::NT;
            const int key = c / C::NS, sl = c % C::NS;
            const int j = j0 + key;
            const bool ok = c < C::KT * C::NS && j < a.S && (!km || km[j]);
            float4 u = make_float4(0.f, 0.f, 0.f, 0.f), w = u;                 // (load8 into a zeroed kx[ci] costs registers in every form)
            if (ok) {
                const float* p = kb + (size_t)j * Cst + sl * 8;
                u = *reinterpret_cast<const float4*>(p);
                w = *reinterpret_cast<const float4*>(p + 4);
            }
            kx[ci][0] = u.x; kx[ci][1] = u.y; kx[ci][2] = u.z; kx[ci][3] = u.w;
            kx[ci][4] = w.x; kx[ci][5] = w.y; kx[ci][6] = w.z; kx[ci][7] = w.w;
        }
#pragma unroll
        for (int ci = 0; ci < C::VCH; ++ci) {
            const int c = tid + ci * C::NT;
            const int d = c & 31, g = c >> 5;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                // attention_f16s.h: tplane_row(j0, g, e), written out: through the call the one-wave form of D = 16 takes two more registers
                const int j = j0 + (32 * (g >> 2) + 16 * ((g >> 1) & 1) + 4 * (g & 1)) + (e < 4 ? e : e + 4);
                const bool ok = c < 32 * C::VS && d < C::D && j < a.S && (!km || km[j]);
                vx[ci][e] = ok ? vb[(size_t)j * Cst + d] : 0.f;
            }
        }
        const int j = j0 + tid;
        valid = tid < C::KT && j < a.S && (!km || km[j]);
    }

    // -> true when a staged value is beyond the split's range (checked by the workgroups of row block 0 only: `check`)
    __device__ __forceinline__ bool store(unsigned char* st, float pre, int tid, bool check) {
        bool bad = false;
#pragma unroll
        for (int ci = 0; ci < C::KCH; ++ci) {
            const int c = tid + ci * C::NT;
            if (c < C::KT * C::NS) {
                f16x8 hi, lo;
                split8(kx[ci], pre, hi, lo);
                if (check) bad |= out_of_range(kx[ci], pre);
                const int off = C::k_off(c / C::NS, c % C::NS);
                *reinterpret_cast<f16x8*>(st + off) = hi;
                *reinterpret_cast<f16x8*>(st + C::K_PLANE + off) = lo;
            }
        }
#pragma unroll
        for (int ci = 0; ci < C::VCH; ++ci) {
            const int c = tid + ci * C::NT;
            if (c < 32 * C::VS) {
                f16x8 hi, lo;
                split8(vx[ci], pre, hi, lo);
                if (check) bad |= out_of_range(vx[ci], pre);
                const int off = C::v_off(c & 31, c >> 5);
                *reinterpret_cast<f16x8*>(st + 2 * C::K_PLANE + off) = hi;
                *reinterpret_cast<f16x8*>(st + 2 * C::K_PLANE + C::V_PLANE + off) = lo;
            }
        }
        if (tid < 64) {                                              // wave 0: lane t = key t
            const unsigned long long m = __ballot(valid);
            if (tid == 0) *reinterpret_cast<unsigned long long*>(st + C::MASK_OFF) = m;
        }
        return bad;
    }
};

template <int D, int NCT, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 2) void k_full_attention(Args a) {
    typedef Cfg<D, NCT, WAVES> C;
    constexpr int KT = C::KT, QS = D / 16, ROWS = 32 * WAVES;
    __shared__ __attribute__((aligned(16))) unsigned char lds_all[2 * C::STAGE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    // block -> (split, image-head z, row block Ib)
    const int Z = a.N * a.H;
    const int per = a.nI * Z;
    const int sp = blockIdx.x / per;
    int z, Ib;
    tile_coords_of(blockIdx.x - sp * per, a.nI, Z, z, Ib);
    const int n = z / a.H, hh = z - n * a.H;
    const int Cst = a.H * D;
    const int i0 = Ib * ROWS + 32 * wave;
    const int irow = i0 + l31;
    const bool qok = irow < a.L && (!a.qm || a.qm[(size_t)n * a.L + irow]);
    bool bad = false;

    // ---- this lane's query row: channels 16 s + 8 h .. + 7 of both planes (the B operand of the score MFMAs)
    f16x8 qh[QS], ql[QS];
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (qok) load8(a.q + ((size_t)n * a.L + irow) * Cst + hh * D + 16 * s + 8 * h, x);
        bad |= out_of_range(x, a.pre);
        split8(x, a.pre, qh[s], ql[s]);
    }

    f32x16 tacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) tacc[r] = 0.f;
    RowState row;

    const int ntile = (a.S + KT - 1) / KT;
    const int t0 = sp * a.tps;
    const int t1 = t0 + a.tps < ntile ? t0 + a.tps : ntile;
    const bool check = Ib == 0;
    Staged<C> st;
    if (t0 < t1) {
        st.load(a, n, hh, t0, tid);
        bad |= st.store(lds_all, a.pre, tid, check);
    }
    __syncthreads();
    for (int jt = t0; jt < t1; ++jt) {
        // tile jt is in stage (jt - t0) & 1; the other stage was last read before the barrier that ended the previous
        // iteration: tile jt + 1 goes there once its loads (issued now, in flight during the MFMAs) have arrived
        const unsigned char* const lds = lds_all + ((jt - t0) & 1) * C::STAGE;
        const unsigned char* const ldv = lds + 2 * C::K_PLANE;
        const bool more = jt + 1 < t1;
        if (more) st.load(a, n, hh, jt + 1, tid);

        f32x16 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
        // attention_f16s.h: score_tile, written out: through the call hipcc gives the one-wave form of D = 32 one register more, which
        // crosses an allocation block (168 -> 176) and costs a wave per SIMD
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            f16x8 ch[NCT], cl[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const int off = C::k_off(32 * ct + l31, 2 * s + h);
                ch[ct] = *reinterpret_cast<const f16x8*>(lds + off);
                cl[ct] = *reinterpret_cast<const f16x8*>(lds + C::K_PLANE + off);
            }
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch[ct], qh[s], acc[ct], 0, 0, 0);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch[ct], ql[s], acc[ct], 0, 0, 0);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl[ct], qh[s], acc[ct], 0, 0, 0);
        }
        // validity of this lane's keys: accumulator register r of tile column ct is key 32 ct + mfma32_row(r, h)
        const unsigned long long km = *reinterpret_cast<const unsigned long long*>(lds + C::MASK_OFF);
        const bool ragged = km != (KT == 64 ? ~0ull : (1ull << (KT & 63)) - 1);            // workgroup-uniform
        unsigned kv[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) kv[ct] = (unsigned)(km >> (32 * ct)) >> (4 * h);
        auto key_ok = [&](int ct, int r) { return ((kv[ct] >> ((r & 3) + 8 * (r >> 2))) & 1u) != 0; };

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
            for (int r = 0; r < 16; ++r) tacc[r] = ldexpf(tacc[r], __shfl(d, mfma32_row(r, h), 64));   // register r: query mfma32_row(r, h)
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
                        t += p[e];
                    }
                    f16x8 ph, pl;
                    split8(p, 1.0f, ph, pl);
                    const int off = C::v_off(l31, 4 * ct + 2 * u + h);
                    const f16x8 bh = *reinterpret_cast<const f16x8*>(ldv + off);
                    const f16x8 bl = *reinterpret_cast<const f16x8*>(ldv + C::V_PLANE + off);
                    tacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ph, bh, tacc, 0, 0, 0);
                    tacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ph, bl, tacc, 0, 0, 0);
                    tacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(pl, bh, tacc, 0, 0, 0);
                }
            }
        };
        if (ragged) pv_tile(std::true_type{});
        else pv_tile(std::false_type{});
        row.add_tile(t);

        if (more) bad |= st.store(lds_all + ((jt + 1 - t0) & 1) * C::STAGE, a.pre, tid, check);
        __syncthreads();
    }
    const float rsum = row.total();
    const int R = row.R;
    if (a.overflow && __any(bad) && lane == 0) atomicOr(a.overflow, 1);

    // ---- store: the lane holds channel d = l31 of queries i0 + mfma32_row(r, h); the row's sum sits in lane (row)
    if (a.nsplit > 1) {
        const size_t prow = ((size_t)z * a.nsplit + sp) * a.L;
        if (h == 0 && irow < a.L) {
            a.part_sum[prow + irow] = rsum;
            a.part_ref[prow + irow] = R;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + mfma32_row(r, h);
            if (l31 < D && i < a.L) a.part_acc[(prow + i) * D + l31] = tacc[r];
        }
        return;
    }
    const float den = (qok && rsum > 0.f) ? rsum : 0.f;    // 0: a padded query row / no valid key -> exact zeros
    // the row statistic the backward recomputes p from: p = 2^(x - R + 15) / rsum = 2^(x - lse2); a row without softmax gets +1e30 (p = 0)
    if (a.lse && h == 0 && irow < a.L) a.lse[(size_t)z * a.L + irow] = den > 0.f ? (float)(R - P_EXP_FWD) + log2f(rsum) : LSE_NONE;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rr = mfma32_row(r, h);
        const float dr = __shfl(den, rr, 64);
        const int i = i0 + rr;
        const float y = dr > 0.f ? tacc[r] / dr * a.out_mul : 0.f;
        if (l31 < D && i < a.L) a.out[((size_t)n * a.L + i) * Cst + hh * D + l31] = y;
    }
}

// The partial results of a key-split run, added in split order: one thread per output value.
__global__ __launch_bounds__(256) void k_combine(Args a, int D) {
    const size_t total = (size_t)a.N * a.H * a.L * D;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int d = (int)(t % D);
    const size_t row = t / D;
    const int i = (int)(row % a.L);
    const size_t z = row / a.L;
    const int n = (int)(z / a.H), hh = (int)(z - (size_t)n * a.H);
    int R = ROW_REF0;
    for (int sp = 0; sp < a.nsplit; ++sp) {
        const int r = a.part_ref[(z * a.nsplit + sp) * a.L + i];
        R = r > R ? r : R;
    }
    float num = 0.f, den = 0.f;
    for (int sp = 0; sp < a.nsplit; ++sp) {
        const size_t pr = (z * a.nsplit + sp) * a.L + i;
        const int e = rescale_exp(a.part_ref[pr], R);
        num += ldexpf(a.part_acc[pr * D + d], e);
        den += ldexpf(a.part_sum[pr], e);
    }
    const bool qok = !a.qm || a.qm[(size_t)n * a.L + i];
    a.out[((size_t)n * a.L + i) * (a.H * D) + hh * D + d] = (qok && den > 0.f) ? num / den * a.out_mul : 0.f;
    if (a.lse && d == 0) a.lse[z * a.L + i] = (qok && den > 0.f) ? (float)(R - P_EXP_FWD) + log2f(den) : LSE_NONE;
}

int launch_forward(const float* q, const float* k, const float* v, int N, int L, int S, int H, int D, const unsigned char* q_mask,
                   const unsigned char* kv_mask, int act_exp, float* out, float* lse, void* ws, int* overflow, hipStream_t stream) {
    far_clear_errors();
    if (N == 0) return FAR_OK;
    if (!q || !k || !v || !out || N < 0 || L <= 0 || S <= 0 || H <= 0 || (D != 16 && D != 32) || act_exp < -24 || act_exp > 8)
        return FAR_EINVAL;
    const bool small = S <= 32;                // one wave per (image, head, 32 queries) and a 32-key tile (attention_f16s.h: split_plan)
    const SplitPlan p = split_plan(L, S, H, small);
    const long blocks = (long)N * H * p.nI * p.nsplit;
    if (blocks > 0x7fffffffL || (long)N * H > 0x7fffffffL) return FAR_EINVAL;
    Args a;
    a.q = q; a.k = k; a.v = v; a.qm = q_mask; a.kvm = kv_mask; a.out = out; a.lse = lse; a.overflow = overflow;
    a.N = N; a.L = L; a.S = S; a.H = H; a.nI = p.nI; a.nsplit = p.nsplit; a.tps = p.tps;
    a.pre = ldexpf(1.0f, act_exp);
    a.c1 = ldexpf(1.44269504088896341f / sqrtf((float)D), -2 * act_exp);       // scores -> log2 domain
    a.out_mul = ldexpf(1.0f, -act_exp);
    a.part_acc = nullptr; a.part_sum = nullptr; a.part_ref = nullptr;
    if (p.nsplit > 1) {
        if (!ws) return FAR_EINVAL;
        const size_t rows = (size_t)N * H * p.nsplit * L;
        unsigned char* b = (unsigned char*)ws;
        a.part_acc = (float*)b;
        a.part_sum = (float*)(b + align256(rows * D * 4));
        a.part_ref = (int*)(b + align256(rows * D * 4) + align256(rows * 4));
    }
    const dim3 grid((unsigned)blocks);
    if (small) {
        if (D == 32) hipLaunchKernelGGL((k_full_attention<32, 1, 1>), grid, dim3(64), 0, stream, a);
        else hipLaunchKernelGGL((k_full_attention<16, 1, 1>), grid, dim3(64), 0, stream, a);
    } else {
        if (D == 32) hipLaunchKernelGGL((k_full_attention<32, 2, 4>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((k_full_attention<16, 2, 4>), grid, dim3(256), 0, stream, a);
    }
    if (p.nsplit > 1) {
        const size_t total = (size_t)N * H * L * D;
        hipLaunchKernelGGL(k_combine, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a, D);
    }
    return far_check_launch();
}

}  // namespace

extern "C" {

// Bytes of workspace far_full_attention_f16s needs for these sizes (0 when the key axis is not split; no GPU involved).
size_t far_full_attention_workspace_bytes(int N, int L, int S, int H, int D) {
    if (N <= 0 || L <= 0 || S <= 0 || H <= 0 || (D != 16 && D != 32)) return 0;
    const SplitPlan p = split_plan(L, S, H, S <= 32);
    if (p.nsplit <= 1) return 0;
    const size_t rows = (size_t)N * H * p.nsplit * L;
    return align256(rows * D * 4) + 2 * align256(rows * 4);
}

// out[n, l, h, :] = sum_s softmax_s(q[n,l,h,:] . k[n,s,h,:] / sqrt(D)) v[n,s,h,:]   (LoFTR's FullAttention, inference).
// q, out: (N, L, H D); k, v: (N, S, H D) fp32 contiguous.  D in {16, 32} (else FAR_EINVAL), H, L, S >= 1.  q_mask (N, L), kv_mask (N, S):
// uint8 or NULL (= all ones).  A masked key is selected out (its k / v values are never used), a padded query row and every row of
// an image without a valid key are exact zeros.  act_exp: the operands are multiplied by 2^act_exp before the fp16 split
// (4 = the default, -24 .. 8): values up to 65504 / 2^act_exp survive it; overflow (device int or NULL) |= 1 when a q / k / v
// value that takes part is beyond that or not finite -- `out` then holds inf / NaN.  ws: far_full_attention_workspace_bytes bytes
// (may be NULL when that is 0).
int far_full_attention_f16s(const float* q, const float* k, const float* v, int N, int L, int S, int H, int D,
                            const unsigned char* q_mask, const unsigned char* kv_mask, int act_exp, float* out, void* ws,
                            int* overflow, hipStream_t stream) {
    return launch_forward(q, k, v, N, L, S, H, D, q_mask, kv_mask, act_exp, out, nullptr, ws, overflow, stream);
}

// The training forward: far_full_attention_f16s (the same launches, the same `out` bits) that also writes the row statistic the
// backward (full_attention_bwd_f16s.hip) recomputes the probabilities from: lse (N, H, L) fp32, the log2-domain log-sum-exp of
// row l's scaled scores -- the integer row reference plus log2 of the running sum; +1e30 for a padded query row and for every row
// of an image without a valid key.  A split-key run writes it from k_combine.
int far_full_attention_train_f16s(const float* q, const float* k, const float* v, int N, int L, int S, int H, int D,
                                  const unsigned char* q_mask, const unsigned char* kv_mask, int act_exp, float* out, float* lse,
                                  void* ws, int* overflow, hipStream_t stream) {
    if (N != 0 && !lse) return FAR_EINVAL;
    return launch_forward(q, k, v, N, L, S, H, D, q_mask, kv_mask, act_exp, out, lse, ws, overflow, stream);
}

}  // extern "C"

// Training through the optimal-transport coarse matcher (sinkhorn_f16s.hip): the sparse loss of the 'sinkhorn' configuration
// (loftr_loss.py:86-119) reads the coupling matrix P at the M ground-truth positions, at the row-dustbin entries P[:, i, S] and at
// the column-dustbin entries P[:, L, j] only, so neither P (Z, L+1, S+1) nor its gradient is ever dense here.
//
//   forward   far_sinkhorn_pos_conf_f16s     the matcher's own T iterations (the same k_skh_stats launches: the bits of inference)
//                                            with every (u^t, v^t) kept, then the M position confidences and the two dustbin vectors
//   backward  far_sinkhorn_pos_conf_bwd_f16  the gradient of the unrolled iterations.  With G = dl/dlogP (sparse;
//             the caller passes w = dl/dp p = G), ubar = rowsum(G), vbar = colsum(G), for t = T .. 1:
//               column half-step   term (A_i, B_j) = (e^{u^t_i}, -vbar_j e^{v^t_j - lnu_j});  ubar_i -= sum_j e^{Zc_ij + u^t_i + v^t_j - lnu_j} vbar_j
//               row half-step      term (A_i, B_j) = (-ubar_i e^{u^t_i - lmu_i}, e^{v^{t-1}_j});  vbar_j = -sum_i e^{Zc_ij + u^t_i - lmu_i + v^{t-1}_j} ubar_i;  ubar = 0
//             dZc = G + e^{Zc} o sum_k A^k (B^k)^T;  ds = dZc[:L, :S] (masked entries 0);  dF0 = ds F1 / C;  dF1 = ds^T F0 / C;
//             d bin_score = sum of dZc over the dustbin row and column.
//     k_skt_adj     one adjoint half-step: the statistics tile loop (split-fp16 scores, as where the potentials were formed) with one
//                   signed weight per column; each weight multiplies a softmax weight 2^(x_ij + a_i + b_j) <= 1 -- no factor is
//                   exponentiated on its own.  The dustbin row / column are scalars per pair, reduced in a fixed order
//     k_skt_bwd     ds on the matrix core: a 32 x 32 score tile recomputed (split-fp16, as K1's backward recomputes its plain one,
//                   dual_softmax_bwd_f16.hip), 2T terms W_i W_j 2^(x_ij + E_i + E_j) per entry plus the row's own positions (fp32), fed
//                   from the accumulator registers into the second MFMA as an fp16 (hi, lo) pair against the other map's plain-fp16
//                   tile.  One kernel, launched twice with the roles of the maps swapped
//     k_skt_group   the sparse part of G: positions that share a row are found by a wave-wide scan and handled by ONE wave in position
//                   order (their sums for ubar / vbar; the first four of a row as slots for k_skt_bwd; the rest as row additions) -- no float atomics anywhere, every launch computes the same bits every time
// Dense supervision (sparse_spvs = False: far_sinkhorn_dense_focal_f16s / far_sinkhorn_dense_focal_bwd_f16) shares all of the above:
// its kernels (k_skd_*) and entry points are at the end of this file, its backward is skt_backward with k_skt_bwd<.., DENSE>.
// Potentials, adjoint vectors and the 2T-term contraction are fp32; the weights are scaled by a power of two so that the dense part
// sits in the fp16 range at any gradient scale (scale_exp).  No data is handed between the workgroups of one launch.
#include "k1_train_f16s.h"
#include <algorithm>

namespace {

constexpr float LOG2E = 1.44269504088896341f;
constexpr int MAX_ITERS = 48;            // the column terms of a tile are staged in LDS: 2 T x 256 B per stage
constexpr int KFOLD = 4;                 // positions per row whose weight joins the dense tile in fp32 (k_skt_bwd)
constexpr float FOLD_MAX = 8192.0f;      // ... unless its scaled weight is above 2^13: KFOLD slots on ONE entry (duplicate positions) stay <= 2^15
constexpr int STAGE = 2 * PLANE32 + TILE_T;  // 52 KiB: hi and lo plane tiles + the transposed tile (+ the column terms)

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

// ---- dense supervision (far_sinkhorn_dense_focal_*: the kernels are at the end of this file) ----
constexpr float LN2 = 0.693147180559945309f;
constexpr float DEAD = -0.5f * HUGE_F;               // a potential below this marks a padded or masked row / column

struct DenseK {                                      // what k_skt_bwd<.., DENSE> needs beyond the sparse kernel's arguments
    const float *dr, *dc;                            // k_skd_side's potentials of the row side [Z][Nrp] and the column side [Z][Ncp]
    const float* gup;                                // the upstream gradient, one device float
    float cneg, alpha, gamma;
};

// The negative-form focal term -alpha p^gamma log(1 - p) of an entry p = 2^xe inside the clamp's range, and W = (d term / d p) p.
// p^gamma comes from the exponent; log(1 - p) is one hardware log, except below 2^-8 where 1 - p would lose p's digits (series to
// p^4: relative error < p^4 / 5 < 5e-11).  ONE definition for the loss pass, the labels' correction and the gradient kernel: the
// same p gives the same bits everywhere.  (neg_w of dual_softmax_dense_f16s.hip is other arithmetic -- log1pf of p itself -- and is
// kept apart on purpose.)
__device__ __forceinline__ float neg_w(float p, float xe, float alpha, float gamma, float& term) {
    const float om = 1.0f - p;
    const float ser = -p * (1.0f + p * (0.5f + p * (0.333333343f + p * 0.25f)));
    const float l1 = p < 0.00390625f ? ser : __builtin_amdgcn_logf(om) * LN2;
    const float qg = ex2(gamma * xe);
    term = -alpha * qg * l1;
    return alpha * qg * (p * __builtin_amdgcn_rcpf(om) - gamma * l1);
}

// sum over the 256 threads of a workgroup in a fixed order (butterfly per wave, the four waves in order); valid in thread 0
__device__ __forceinline__ float block_sum(float s, float* red, int tid) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += shfl_xor_f(s, o);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ bool pos_ok(long z, long i, long j, int Z, int L, int S) {
    return z >= 0 && z < Z && i >= 0 && i < L && j >= 0 && j < S;
}

// conf_pos[k] = P[b_k, i_k, j_k] = 2^(x + U_i + V_j - N): one wave per position, float64 dot product of the fp32 features
__global__ __launch_bounds__(256) void k_skt_pos(const float* __restrict__ f0, const float* __restrict__ f1, int Z, int L, int S, int Lp,
                                                 int Sp, double k2, const int64_t* __restrict__ pb, const int64_t* __restrict__ pi,
                                                 const int64_t* __restrict__ pj, int M, const uint8_t* __restrict__ mask0,
                                                 const uint8_t* __restrict__ mask1, const float* __restrict__ up,
                                                 const float* __restrict__ vp, float nrm, float* __restrict__ p_out) {
    const int lane = threadIdx.x & 63;
    const int nw = gridDim.x * (blockDim.x >> 6);
    for (int k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); k < M; k += nw) {
        const long z = pb[k], i = pi[k], j = pj[k];
        if (!pos_ok(z, i, j, Z, L, S) || (mask0 && !mask0[z * L + i]) || (mask1 && !mask1[z * S + j])) {      // wave-uniform
            if (lane == 0) p_out[k] = 0.f;
            continue;
        }
        const float4 a = *reinterpret_cast<const float4*>(f0 + ((size_t)z * L + i) * C + 4 * lane);
        const float4 b = *reinterpret_cast<const float4*>(f1 + ((size_t)z * S + j) * C + 4 * lane);
        double d = (double)a.x * (double)b.x + (double)a.y * (double)b.y + (double)a.z * (double)b.z + (double)a.w * (double)b.w;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) d += __shfl_xor(d, m, 64);
        if (lane == 0) p_out[k] = ex2((float)(d * k2) + up[(size_t)z * Lp + i] + (vp[(size_t)z * Sp + j] - nrm));
    }
}

// conf_bin0[z, i] = P[z, i, S], conf_bin1[z, j] = P[z, L, j]
__global__ void k_skt_bins(const float* __restrict__ up, const float* __restrict__ vp, const float* __restrict__ bins,
                           const float* __restrict__ bin_score, int Z, int L, int S, int Lp, int Sp, float nrm,
                           float* __restrict__ bin0, float* __restrict__ bin1) {
    const int z = blockIdx.y;
    const float alpha = bin_score[0] * LOG2E;
    const float ub = bins[z], vb = bins[Z + z];
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < L + S; t += gridDim.x * blockDim.x) {
        if (t < L) bin0[(size_t)z * L + t] = ex2(alpha + up[(size_t)z * Lp + t] + vb - nrm);
        else bin1[(size_t)z * S + (t - L)] = ex2(alpha + ub + vp[(size_t)z * Sp + (t - L)] - nrm);
    }
}

// ubar^T = rowsum(G), vbar^T = colsum(G) without the positions (k_skt_group adds them): the dustbin weights, and their sums as the
// adjoints of the dustbin potentials.  One workgroup per pair.
__global__ __launch_bounds__(256) void k_skt_seed(const float* __restrict__ wb0, const float* __restrict__ wb1, int Z, int L, int S, int Lp,
                                                  int Sp, float* __restrict__ ubar, float* __restrict__ vbar, float* __restrict__ barbin) {
    __shared__ float red[4];
    const int z = blockIdx.x, tid = threadIdx.x;
    float s0 = 0.f, s1 = 0.f;
    for (int i = tid; i < Lp; i += 256) {
        const float v = i < L ? wb0[(size_t)z * L + i] : 0.f;
        ubar[(size_t)z * Lp + i] = v;
        s0 += v;
    }
    for (int j = tid; j < Sp; j += 256) {
        const float v = j < S ? wb1[(size_t)z * S + j] : 0.f;
        vbar[(size_t)z * Sp + j] = v;
        s1 += v;
    }
    s0 = block_sum(s0, red, tid);
    s1 = block_sum(s1, red, tid);
    if (tid == 0) { barbin[z] = s1; barbin[Z + z] = s0; }      // ubar_L = sum_j G[L, j], vbar_S = sum_i G[i, S]
}

// The power of two that scales a pair's adjoint weights for the fp16 tile of k_skt_bwd: the largest weight goes to
// [2^13, 2^14) / P, P = the power of two >= nterm, so that an entry of the tile (at most nterm weights times softmax weights <= 1:
// < 2^14; plus at most KFOLD slots of <= FOLD_MAX = 2^13 each, all on that entry when positions repeat: <= 2^15) stays below
// 3 x 2^14 = 49152 < 65504, while contributions 2^-27 of the largest are still normal fp16 numbers -- the many small softmax
// weights of a row without a partner must not fall into the subnormals (measured: 0.6 % error with the largest weight at 2^-4).
// Written out, not grad_scale_exp(wmax_bits, log2 P - 14) of k1_train_f16s.h: through the helper k_skt_bwd<0, 1|2> take one more
// VGPR and AGPR and k_skt_bwd<6> one more spilled SGPR.
__device__ __forceinline__ int scale_exp(const unsigned* wmax_bits, int nterm) {
    const float wmax = __uint_as_float(*wmax_bits);
    int e = 0;
    if (wmax > 0.f) {
        (void)frexpf(wmax, &e);
        e = 14 - e - (nterm > 1 ? 32 - __clz(nterm - 1) : 0);
    }
    return e;
}

// The sparse part of G.  blockIdx.y = side (0: grouped by row (b, i) of f0; 1: by row (b, j) of f1).  One wave per position k; the wave
// of the FIRST position of a group walks the group in position order:
//   MODE 0   vec[z][n] += sum of the group's w                                 (the positions' part of rowsum / colsum (G))
//   MODE 1   the group's first `kfold` members -> the row's slots (other index, w 2^e): k_skt_bwd adds them to its dense tile in
//            fp32, where G_ij and the dense part of ds_ij cancel (a confident match: dense ~ -w), before anything is rounded to fp16
//   MODE 2   d[z][n][:] += coef * sum over the members BEYOND the slots of w_k other[z][m_k][:]   (dF0 += G F1 / C, dF1 += G^T F0 / C)
// A position on a masked cell has P = 0 and no gradient.  Every sum has one owner and a fixed order: no atomics.
// Cost: finding the first of a group scans all earlier positions, k / 64 ballot rounds of three int64 loads for position k, so a
// launch is QUADRATIC in M (M^2 / 128 wave-rounds per side) -- positions need not arrive sorted, and nothing is sorted here.
// Measured at M = 1500 .. 3000 (a training batch of 1 - 2 pairs) and at M = 48 000 (32 pairs): profiles/sinkhorn_train_kernel_trace.txt
// and DESIGN.md section 4; beyond that, sort the positions by row once instead.
template <int MODE>
__global__ __launch_bounds__(256) void k_skt_group(const int64_t* __restrict__ pb, const int64_t* __restrict__ pi,
                                                   const int64_t* __restrict__ pj, const float* __restrict__ w, int M, int Z, int L, int S,
                                                   int Lp, int Sp, const uint8_t* __restrict__ mask0, const uint8_t* __restrict__ mask1,
                                                   float* __restrict__ ubar, float* __restrict__ vbar, const float* __restrict__ f0,
                                                   const float* __restrict__ f1, float coef, float* __restrict__ df0,
                                                   float* __restrict__ df1, const unsigned* __restrict__ wmax_bits, int kfold, int kfold_terms,
                                                   int* __restrict__ slot_j0, float* __restrict__ slot_w0, int* __restrict__ slot_j1,
                                                   float* __restrict__ slot_w1) {
    const int lane = threadIdx.x & 63, side = blockIdx.y;
    const int nw = gridDim.x * (blockDim.x >> 6);
    const int N = side ? S : L, Np = side ? Sp : Lp;
    auto key_of = [&](int k) -> long {
        const long z = pb[k], i = pi[k], j = pj[k];
        return pos_ok(z, i, j, Z, L, S) ? z * N + (side ? j : i) : -1L;
    };
    auto live = [&](int k) -> bool {       // in range (checked by key_of) and on an unmasked cell
        const long z = pb[k], i = pi[k], j = pj[k];
        return !(mask0 && !mask0[z * L + i]) && !(mask1 && !mask1[z * S + j]);
    };
    for (int k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); k < M; k += nw) {
        const long key = key_of(k);
        if (key < 0) continue;                                                        // wave-uniform
        bool first = true;
        for (int base = 0; base < k && first; base += 64) {
            const int kk = base + lane;
            if (__builtin_amdgcn_ballot_w64(kk < k && key_of(kk) == key) != 0ull) first = false;
        }
        if (!first) continue;
        const long z = key / N, n = key - z * N;
        const float sc = MODE != 0 && kfold > 0 ? ldexpf(1.0f, scale_exp(wmax_bits + z, 2 * kfold_terms)) : 1.0f;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        float sum = 0.f;
        int nf = 0;
        for (int base = k & ~63; base < M; base += 64) {
            const int kk = base + lane;
            unsigned long long hit = __builtin_amdgcn_ballot_w64(kk >= k && kk < M && key_of(kk) == key);
            while (hit) {
                const int q = base + __builtin_ctzll(hit);
                hit &= hit - 1;
                if (!live(q)) continue;
                const float wq = w[q];
                if (MODE == 0) {
                    sum += wq;
                    continue;
                }
                if (nf < kfold && fabsf(wq * sc) <= FOLD_MAX) {                       // a slot of the row
                    if (MODE == 1 && lane == 0) {
                        const size_t at = ((size_t)z * Np + n) * KFOLD + nf;
                        (side ? slot_j1 : slot_j0)[at] = (int)(side ? pi[q] : pj[q]);
                        (side ? slot_w1 : slot_w0)[at] = wq * sc;
                    }
                    ++nf;
                } else if (MODE == 2) {
                    const size_t orow = side ? (size_t)pb[q] * L + pi[q] : (size_t)pb[q] * S + pj[q];
                    const float4 o = *reinterpret_cast<const float4*>((side ? f0 : f1) + orow * C + 4 * lane);
                    acc.x = fmaf(wq, o.x, acc.x); acc.y = fmaf(wq, o.y, acc.y); acc.z = fmaf(wq, o.z, acc.z); acc.w = fmaf(wq, o.w, acc.w);
                }
            }
        }
        if (MODE == 2) {
            float4* dst = reinterpret_cast<float4*>((side ? df1 : df0) + (size_t)key * C + 4 * lane);
            float4 d = *dst;
            d.x = fmaf(coef, acc.x, d.x); d.y = fmaf(coef, acc.y, d.y); d.z = fmaf(coef, acc.z, d.z); d.w = fmaf(coef, acc.w, d.w);
            *dst = d;
        } else if (MODE == 0 && lane == 0) {
            float* dst = side ? vbar + (size_t)z * Sp + n : ubar + (size_t)z * Lp + n;
            *dst += sum;
        }
    }
}

// score_tile (k1_f16s.h) with the two cross terms in the other order: hi.hi + lo.hi + hi.lo in (tile, row) terms -- the order in which
// score_tile accumulates the same entry when the maps' roles are swapped
__device__ __forceinline__ void score_tile_x(f32x16 (&acc)[2], const unsigned char* lds, const RowFrags& rf, int l31, int h) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        f16x8 ch[2], cl[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const int row = 32 * ct + l31;
            const int off = row * ROWB + (((2 * s + h) ^ (row & 15)) * 16);
            ch[ct] = *reinterpret_cast<const f16x8*>(lds + off);
            cl[ct] = *reinterpret_cast<const f16x8*>(lds + TILE_PLANE + off);
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch[ct], rf.hi[s], acc[ct], 0, 0, 0);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl[ct], rf.hi[s], acc[ct], 0, 0, 0);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch[ct], rf.lo[s], acc[ct], 0, 0, 0);
    }
}

// One adjoint half-step over the rows of the (Nr x Nc) score matrix of (a, b):
//   out_r   = keep out_r   - ( sum_{c < Nc} cw_c 2^(x_rc + rpot_r + cpot_c - N)     + cwbin 2^(alpha + rpot_r + cbinpot - cmarg_bin) )
//   outbin  = keep outbin  - ( sum_{c < Nc} cw_c 2^(alpha + rbinpot + cpot_c - N)   + cwbin 2^(alpha + rbinpot + cbinpot - cmarg_bin) )
// rpot / cpot: the potentials of the two sides at this half-step (log2 units; padded: -huge), N = log2 of a real row's / column's
// marginal, cmarg_bin that of the column side's dustbin.  cw: the column side's adjoint vector (padded: 0).  The tile loop is
// k_skh_stats' (sinkhorn_f16s.hip); the workgroup of row block 0 also reduces the dustbin row.
// XORD (the dense backward): the two cross terms of a score are accumulated the other way round (score_tile_x) -- then this pass
// meets the potentials it divides by with the very scores they were summed from (the statistics launch had the maps' roles swapped),
// and a row whose mass sits on one entry gets p = 1 - (the rest) instead of 1 +- the rounding of a 768-term sum.
template <bool XORD = false>
__global__ __launch_bounds__(256, 2) void k_skt_adj(const _Float16* __restrict__ ah, const _Float16* __restrict__ al,
                                                    const _Float16* __restrict__ bh, const _Float16* __restrict__ bl,
                                                    int Z, int Nr, int Nc, int Nrp, int Ncp, float c1,
                                                    const uint8_t* __restrict__ rmask, const uint8_t* __restrict__ cmask,
                                                    const float* __restrict__ rpot, const float* __restrict__ rbinpot,
                                                    const float* __restrict__ cpot, const float* __restrict__ cbinpot,
                                                    const float* __restrict__ cw, const float* __restrict__ cwbin,
                                                    const float* __restrict__ bin_score, float nrm, float cmarg_bin, int keep,
                                                    float* __restrict__ out, float* __restrict__ outbin) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    float* const tpot = reinterpret_cast<float*>(lds + 2 * TILE_PLANE);          // this tile's 64 column potentials - N
    float* const tw = tpot + KT;                                                  // and weights
    float* const red = tw + KT;
    int z, Ib;
    tile_coords(Nrp / 128, Z, z, Ib);
    const float alpha = bin_score[0] * LOG2E;
    const float cb = cbinpot[z] - cmarg_bin, wb = cwbin[z];
    if (Ib == 0) {
        const float rb = alpha + rbinpot[z] - nrm;
        float s = 0.f;
        for (int k = tid; k < Nc; k += 256) s = fmaf(cw[(size_t)z * Ncp + k], ex2(rb + cpot[(size_t)z * Ncp + k]), s);
        s = block_sum(s, red, tid);
        if (tid == 0) {
            s = fmaf(wb, ex2(alpha + rbinpot[z] + cb), s);
            outbin[z] = (keep ? outbin[z] : 0.f) - s;
        }
    }
    const int irow = Ib * 128 + 32 * wave + l31;
    RowFrags rf;
    rf.load(ah, al, (size_t)z * Nrp + irow, irow, h);
    const bool rmasked = rmask && irow < Nr && !rmask[(size_t)z * Nr + irow];
    const float rp = rpot[(size_t)z * Nrp + irow];
    float sum = 0.f;
    const int ntile = (Nc + KT - 1) / KT;
    for (int jt = 0; jt < ntile; ++jt) {
        __syncthreads();
        dma_tile(lds, bh, bl, (size_t)z * Ncp + jt * KT, tid, wave);
        if (tid < KT) {
            tpot[tid] = cpot[(size_t)z * Ncp + jt * KT + tid] - nrm;
            tw[tid] = cw[(size_t)z * Ncp + jt * KT + tid];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        f32x16 acc[2];
        if constexpr (XORD) score_tile_x(acc, lds, rf, l31, h);
        else score_tile(acc, lds, rf, l31, h);
        const bool special = (jt + 1) * KT > Nc || cmask != nullptr || rmask != nullptr;      // wave-uniform
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 pv = *reinterpret_cast<const float4*>(tpot + 32 * ct + 8 * q4 + 4 * h);
                const float4 wv = *reinterpret_cast<const float4*>(tw + 32 * ct + 8 * q4 + 4 * h);
                const float p4[4] = {pv.x, pv.y, pv.z, pv.w}, w4[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * q4 + e;
                    float x = fmaf(acc[ct][r], c1, p4[e]);
                    if (special) {
                        const int j = jt * KT + 32 * ct + mfma32_row(r, h);
                        if (j >= Nc || rmasked || (cmask && !cmask[(size_t)z * Nc + j])) x = -HUGE_F;
                    }
                    sum = fmaf(w4[e], ex2(x + rp), sum);
                }
            }
    }
    sum += shfl_xor_f(sum, 32);
    sum = fmaf(wb, ex2(alpha + rp + cb), sum);                                    // the dustbin column
    if (h == 0) {
        float* dst = out + (size_t)z * Nrp + irow;
        *dst = irow < Nr ? (keep ? *dst : 0.f) - sum : 0.f;
    }
}

// max |adjoint weight| of each pair over every half-step (bit patterns of non-negative floats order like unsigned integers): per
// pair, so that a pair's gradients do not depend on what else is in the batch.  ubar / vbar: slices 1 .. T of [T + 1][Z][Np]
__global__ void k_skt_wmax(const float* __restrict__ ubar, const float* __restrict__ vbar, int Z, int Lp, int Sp, int T,
                           unsigned* __restrict__ wmax_bits) {
    const int z = blockIdx.y;
    float mx = 0.f;
    for (int t = 1; t <= T; ++t) {
        const float* u = ubar + ((size_t)t * Z + z) * Lp;
        const float* v = vbar + ((size_t)t * Z + z) * Sp;
        for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < Lp + Sp; q += gridDim.x * blockDim.x)
            mx = fmaxf(mx, fabsf(q < Lp ? u[q] : v[q - Lp]));
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, shfl_xor_f(mx, m));
    if ((threadIdx.x & 63) == 0 && mx > 0.f && mx < HUGE_F) atomicMax(wmax_bits + z, __float_as_uint(mx));
}

// The 2T terms of the dense part of ds, per side: ds_ij = sum_k WL^k_i WS^k_j 2^(x_ij + EL^k_i + ES^k_j), k = 2 (t - 1) + {0: column, 1: row half-step}
//   column half-step t   WL = 1, EL = U^t_i;                    WS = -vbar^t_j 2^e, ES = V^t_j - N
//   row half-step t      WL = -ubar^t_i 2^e, EL = U^t_i - N;    WS = 1, ES = V^{t-1}_j
// padded and masked rows: W = 0, E = -huge.
__global__ void k_skt_pack(const float* __restrict__ uh, const float* __restrict__ vh, const float* __restrict__ ubar,
                           const float* __restrict__ vbar, int Z, int L, int S, int Lp, int Sp, int T, float nrm,
                           const uint8_t* __restrict__ mask0, const uint8_t* __restrict__ mask1, const unsigned* __restrict__ wmax_bits,
                           float* __restrict__ wl, float* __restrict__ el, float* __restrict__ wsd, float* __restrict__ es) {
    const long nl = (long)2 * T * Z * Lp, ns = (long)2 * T * Z * Sp;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nl + ns; q += (long)gridDim.x * blockDim.x) {
        if (q < nl) {
            const int i = (int)(q % Lp);
            const long kz = q / Lp;
            const int z = (int)(kz % Z), k = (int)(kz / Z), t = k / 2 + 1;
            const bool ok = i < L && !(mask0 && !mask0[(size_t)z * L + i]);
            const size_t at = ((size_t)t * Z + z) * Lp + i;
            float W = 0.f, E = -HUGE_F;
            if (ok) {
                if (k & 1) { W = -ubar[at] * ldexpf(1.0f, scale_exp(wmax_bits + z, 2 * T)); E = uh[at] - nrm; }
                else { W = 1.0f; E = uh[at]; }
            }
            wl[q] = W; el[q] = E;
        } else {
            const long p = q - nl;
            const int j = (int)(p % Sp);
            const long kz = p / Sp;
            const int z = (int)(kz % Z), k = (int)(kz / Z), t = k / 2 + 1;
            const bool ok = j < S && !(mask1 && !mask1[(size_t)z * S + j]);
            const size_t at = ((size_t)t * Z + z) * Sp + j;
            float W = 0.f, E = -HUGE_F;
            if (ok) {
                if (k & 1) { W = 1.0f; E = vh[at - (size_t)Z * Sp]; }
                else { W = -vbar[at] * ldexpf(1.0f, scale_exp(wmax_bits + z, 2 * T)); E = vh[at] - nrm; }
            }
            wsd[p] = W; es[p] = E;
        }
    }
}

// out[z][row][256] = coef * sum_cols G[row][col] * B[col][:],   G = slots + sum_k rw^k_row cw^k_col 2^(x + re^k_row + ce^k_col)
//   ah / al   row-side hi / lo planes [Z][Nrp][256] fp16 (swizzled LDS image of k1_prep); bh / bl: column side, same layout; bt:
//   column-side transposed tiles (k1_prep_t); rw / re [nterm][Z][Nrp], cw / ce [nterm][Z][Ncp]: k_skt_pack's terms;
//   slot_j / slot_w [Z][Nrp][KFOLD]: the row's first positions (column, w 2^e; column -1: empty), k_skt_group<1>.
// The scores are the split-fp16 ones of the forward (hi.hi + hi.lo + lo.hi): where a confident match makes the dense part cancel
// the position's own weight, a relative score error delta would stay as delta |w| next to a result of (1 - P) |w|.  The sum of
// slots and terms is formed in fp32 and leaves as an fp16 (hi, lo) pair; the other map's tile is plain fp16.
// NR > 0: the lane's row terms live in registers (nterm <= NR); NR = 0: they are re-read per tile (any nterm).
// DENSE != 0 (dense supervision, far_sinkhorn_dense_focal_bwd_f16): G carries one more term per entry, the focal loss's own
//   W_ij = wsc neg_w(p_ij),  p_ij = 2^(x_ij + dr_row + dc_col)  (dr / dc: k_skd_side's potentials; wsc = cneg gup 2^e),
// recomputed from the tile's score with the expression and the MFMA order of the forward's loss pass (k_skd_pass), so that p has
// the forward's bits and falls on the same side of the clamp.  DENSE = 1: the rows are f1's, 2: the rows are f0's; both forms
// accumulate every score in both orders of its cross terms (see below).  DENSE = 0 compiles to the sparse kernel.
// grid: Z * Nrp / 128 workgroups of 4 waves; wave = 32 rows x 256 channels of the output (128 accumulator registers)
template <int NR, int DENSE = 0>
__global__ __launch_bounds__(256, 1) void k_skt_bwd(const _Float16* __restrict__ ah, const _Float16* __restrict__ al,
                                                    const _Float16* __restrict__ bh, const _Float16* __restrict__ bl,
                                                    const unsigned char* __restrict__ bt, int Z, int Nr, int Nc, int Nrp, int Ncp,
                                                    float c1, int nterm, const float* __restrict__ rw, const float* __restrict__ re,
                                                    const float* __restrict__ cw, const float* __restrict__ ce,
                                                    const int* __restrict__ slot_j, const float* __restrict__ slot_w,
                                                    const unsigned* __restrict__ wmax_bits, float kappa, float* __restrict__ out,
                                                    DenseK dk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    int z, Ib;
    tile_coords(Nrp / 128, Z, z, Ib);
    const int irow = Ib * 128 + 32 * wave + l31;
    RowFrags rf;
    rf.load(ah, al, (size_t)z * Nrp + irow, irow, h);
    const size_t rstride = (size_t)Z * Nrp, cstride = (size_t)Z * Ncp;
    float drow = 0.f, wsc = 0.f;
    if constexpr (DENSE != 0) {
        drow = dk.dr[(size_t)z * Nrp + irow];
        wsc = dk.cneg * dk.gup[0] * ldexpf(1.0f, scale_exp(wmax_bits + z, nterm));
    }
    const float* const rwp = rw + (size_t)z * Nrp + irow;
    const float* const rep = re + (size_t)z * Nrp + irow;
    float rwr[NR > 0 ? NR : 1], rer[NR > 0 ? NR : 1];
    if (NR > 0) {
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            rwr[k] = k < nterm ? rwp[k * rstride] : 0.f;
            rer[k] = k < nterm ? rep[k * rstride] : -HUGE_F;
        }
    }
    // the row's slots: tile, register and lane half of each column (column c of a tile sits in register (c & 3) + 4 (c >> 3) of the
    // lane half (c >> 2) & 1); an empty slot (-1) never meets a tile
    int sjt[KFOLD], sreg[KFOLD];
    float sw[KFOLD];
#pragma unroll
    for (int q = 0; q < KFOLD; ++q) {
        const int j = slot_j[((size_t)z * Nrp + irow) * KFOLD + q];
        const int c = j & 31;
        sjt[q] = (j >= 0 && ((c >> 2) & 1) == h) ? j >> 5 : -1;
        sreg[q] = (c & 3) + 4 * (c >> 3);
        sw[q] = slot_w[((size_t)z * Nrp + irow) * KFOLD + q];
    }
    f32x16 acc[8];                                                // [channel block nt][rows]: D[m = row][n = channel]
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
    const int stage = STAGE + nterm * 256 + (DENSE ? 256 : 0);    // tile planes + [nterm][W 32 | E 32] column terms (+ the dense term's potentials)
    const int ntile = Ncp / GT;
    auto request = [&](int jt, int st) {
        unsigned char* base = lds + st * stage;
        dma_lin(base, reinterpret_cast<const unsigned char*>(bh + ((size_t)z * Ncp + (size_t)jt * GT) * C), PLANE32, tid, wave);
        dma_lin(base + PLANE32, reinterpret_cast<const unsigned char*>(bl + ((size_t)z * Ncp + (size_t)jt * GT) * C), PLANE32, tid, wave);
        dma_lin(base + 2 * PLANE32, bt + ((size_t)z * ntile + jt) * TILE_T, TILE_T, tid, wave);
        for (int o = tid; o < nterm * 64; o += 256) {             // whole waves: nterm * 64 is a multiple of 64
            const int k = o >> 6, c = o & 31;
            const float* src = ((o & 32) ? ce : cw) + (size_t)k * cstride + (size_t)z * Ncp + jt * GT + c;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(base + STAGE + (o - lane) * 4), 4, 0, 0);
        }
        if constexpr (DENSE != 0) {
            if (wave == 0)                                        // 32 column potentials (the upper half-wave repeats them into the pad)
                __builtin_amdgcn_global_load_lds((gptr_t)(dk.dc + (size_t)z * Ncp + jt * GT + l31), (lptr_t)(base + STAGE + nterm * 256), 4, 0, 0);
        }
    };
    request(0, 0);
    for (int jt = 0; jt < ntile; ++jt) {
        const int st = jt & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                          // tile jt landed; stage st ^ 1 is free
        if (jt + 1 < ntile) request(jt + 1, st ^ 1);
        const unsigned char* xs = lds + st * stage;
        const float* const cp = reinterpret_cast<const float*>(xs + STAGE);
        // ---- scores, transposed: D[m = column of the tile][n = this lane's row], split-fp16 as in the forward
        f32x16 sc, sx;
#pragma unroll
        for (int r = 0; r < 16; ++r) { sc[r] = 0.f; sx[r] = 0.f; }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int off = l31 * ROWB + (((2 * s + h) ^ (l31 & 15)) * 16);
            const f16x8 ch = *reinterpret_cast<const f16x8*>(xs + off);
            const f16x8 cl = *reinterpret_cast<const f16x8*>(xs + PLANE32 + off);
            score_step(sc, ch, cl, rf.hi[s], rf.lo[s]);
            if constexpr (DENSE != 0) score_step_x(sx, ch, cl, rf.hi[s], rf.lo[s]);      // the same entry with the two cross terms the other way round
        }
        // ---- G for this lane's row and its 16 columns  c = (r & 3) + 8 (r >> 2) + 4 h; a score that is not finite can only come from a
        // masked row or column (W = 0, E = -huge there): taken as 0 so that it stays out of the products
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float x = sc[r] * c1;
            sc[r] = fabsf(x) < HUGE_F ? x : 0.f;
            if constexpr (DENSE != 0) {
                const float y = sx[r] * c1;
                sx[r] = fabsf(y) < HUGE_F ? y : 0.f;
            }
        }
        // Dense forms: every term meets the score its potentials were normalised with.  The column half-iterations (rows of f1, tiles
        // of f0) summed hi.hi + f0hi.f1lo + f0lo.f1hi, the row half-iterations the cross terms the other way round; `sc` is the former
        // when this launch's rows are f1's (DENSE = 1) and the latter when they are f0's (DENSE = 2).  A row whose mass sits on one
        // entry has 2^(x + U - N) = 1 - (the rest) only with the score U was summed from -- and ds = G (1 - p - (1 - p) p') is the
        // difference that remains.  Even terms and the loss's W: column order; odd terms: row order.
        const f32x16& xcol = DENSE == 2 ? sx : sc;
        const f32x16& xrow = DENSE == 2 ? sc : sx;
        f16x8 gp[2], gl[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {                             // eight columns at a time (registers)
            float g[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) g[r] = 0.f;
            auto term = [&](int k, float rwk, float rek) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const float4 w4 = *reinterpret_cast<const float4*>(cp + k * 64 + 8 * (2 * u + q) + 4 * h);
                    const float4 e4 = *reinterpret_cast<const float4*>(cp + k * 64 + 32 + 8 * (2 * u + q) + 4 * h);
                    const float ww[4] = {w4.x, w4.y, w4.z, w4.w}, ee[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if constexpr (DENSE != 0) {
                            const float xs_ = (k & 1) ? xrow[8 * u + 4 * q + e] : xcol[8 * u + 4 * q + e];
                            g[4 * q + e] = fmaf(rwk * ww[e], ex2(xs_ + (rek + ee[e])), g[4 * q + e]);
                        } else {
                            g[4 * q + e] = fmaf(rwk * ww[e], ex2(sc[8 * u + 4 * q + e] + (rek + ee[e])), g[4 * q + e]);
                        }
                }
            };
            if (NR > 0) {
#pragma unroll
                for (int k = 0; k < NR; ++k)
                    if (k < nterm) term(k, rwr[k], rer[k]);
            } else {
                for (int k = 0; k < nterm; ++k) term(k, rwp[k * rstride], rep[k * rstride]);
            }
            if constexpr (DENSE != 0) {                           // the loss's own W at every entry inside the clamp's range
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const float4 c4 = *reinterpret_cast<const float4*>(cp + nterm * 64 + 8 * (2 * u + q) + 4 * h);
                    const float cc[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float xe = xcol[8 * u + 4 * q + e] + (drow + cc[e]);
                        const float p = ex2(xe);
                        float term;
                        const float wv = neg_w(p, xe, dk.alpha, dk.gamma, term);
                        g[4 * q + e] = fmaf((p >= P_LO && p <= P_HI) ? wv : 0.f, wsc, g[4 * q + e]);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < KFOLD; ++q) {                     // the positions of this row that fall into this half tile
                const bool here = sjt[q] == jt && (sreg[q] >> 3) == u;
                if (__builtin_amdgcn_ballot_w64(here) != 0ull) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) g[r] += (here && (sreg[q] & 7) == r) ? sw[q] : 0.f;
                }
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const _Float16 hi = (_Float16)g[r];
                gp[u][r] = hi;
                gl[u][r] = (_Float16)(g[r] - (float)hi);
            }
        }
        // ---- out[row][channel] += G[row][col] * B[col][channel]: A = G (registers), B = transposed tile (LDS)
        const unsigned char* ts = xs + 2 * PLANE32;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int nt = 0; nt < 8; ++nt) {
                const f16x8 tf = *reinterpret_cast<const f16x8*>(ts + (32 * nt + l31) * TROW + (2 * u + h) * 16);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(gp[u], tf, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(gl[u], tf, acc[nt], 0, 0, 0);
            }
    }
    // ---- epilogue: undo the scalings (operand x 2^4, weights x 2^e), apply 1 / C
    const float coef = kappa * ldexpf(1.0f, -scale_exp(wmax_bits + z, nterm)) / PRESCALE;
    const int row0 = Ib * 128 + 32 * wave;
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = row0 + mfma32_row(r, h);
            if (i < Nr) out[((size_t)z * Nr + i) * C + 32 * nt + l31] = acc[nt][r] * coef;
        }
}

// d bin_score of one pair: the sum of dZc = G + e^{Zc} sum_k A^k (B^k)^T over the dustbin column, the dustbin row and the corner
// (Zc = alpha there), in a fixed order.  One workgroup per pair -> part[z].
__global__ __launch_bounds__(256) void k_skt_dbin(const float* __restrict__ wb0, const float* __restrict__ wb1, const float* __restrict__ uh,
                                                  const float* __restrict__ vh, const float* __restrict__ binh, const float* __restrict__ ubar,
                                                  const float* __restrict__ vbar, const float* __restrict__ barbin,
                                                  const float* __restrict__ bin_score, int Z, int L, int S, int Lp, int Sp, int T, float nrm,
                                                  float lmu_l, float lnu_s, float* __restrict__ part) {
    __shared__ float red[4];
    const int z = blockIdx.x, tid = threadIdx.x;
    const float alpha = bin_score[0] * LOG2E;
    float s = 0.f;
    for (int i = tid; i < L; i += 256) s += wb0[(size_t)z * L + i];
    for (int j = tid; j < S; j += 256) s += wb1[(size_t)z * S + j];
    for (int t = T; t >= 1; --t) {
        const float* ut = uh + ((size_t)t * Z + z) * Lp;
        const float* vt = vh + ((size_t)t * Z + z) * Sp;
        const float* vq = vt - (size_t)Z * Sp;                                            // v^{t-1}
        const float* ub = ubar + ((size_t)t * Z + z) * Lp;
        const float* vb = vbar + ((size_t)t * Z + z) * Sp;
        const float ubin = binh[(size_t)t * 2 * Z + z], vbin = binh[(size_t)t * 2 * Z + Z + z], vbinq = binh[(size_t)(t - 1) * 2 * Z + Z + z];
        const float ubarL = barbin[(size_t)t * 2 * Z + z], vbarS = barbin[(size_t)t * 2 * Z + Z + z];
        // column half-step: -vbar_j 2^(alpha + u^t_i + v^t_j - lnu_j)
        const float c0 = alpha + vbin - lnu_s, c1 = alpha + ubin - nrm;
        // row half-step: -ubar_i 2^(alpha + u^t_i - lmu_i + v^{t-1}_j)
        const float r0 = alpha - nrm + vbinq, r1 = alpha + ubin - lmu_l;
        for (int i = tid; i < L; i += 256) s -= fmaf(vbarS, ex2(c0 + ut[i]), ub[i] * ex2(r0 + ut[i]));
        for (int j = tid; j < S; j += 256) s -= fmaf(vb[j], ex2(c1 + vt[j]), ubarL * ex2(r1 + vq[j]));
        if (tid == 0) s -= fmaf(vbarS, ex2(alpha + ubin + vbin - lnu_s), ubarL * ex2(alpha + ubin - lmu_l + vbinq));
    }
    s = block_sum(s, red, tid);
    if (tid == 0) part[z] = s;
}

__global__ void k_skt_dbin_sum(const float* __restrict__ part, int Z, float* __restrict__ dbin) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float s = 0.f;
        for (int z = 0; z < Z; ++z) s += part[z];
        dbin[0] = s;
    }
}

// =====================================================================================================================
// Dense supervision of the optimal-transport matcher (match_type 'sinkhorn', sparse_spvs = False: the loftr_ot_dense configurations;
// loftr_loss.py:56-75, :87-89, :121-127).  The loss reads EVERY entry of conf = P[:, :L, :S] (the dustbin row and column are not
// supervised):
//     q = clamp(p, 1e-6, 1 - 1e-6);  loss = c_pos sum_pos w (-alpha (1 - q)^gamma log q) + c_neg sum_neg w (-alpha q^gamma log(1 - q))
//     c_pos = pos_weight / M,  c_neg = neg_weight / (N L S - M),  w_ij = mask0_i mask1_j
// so G = dloss/dlogP is dense on the real block, G_ij = W_ij = (dloss/dp_ij) p_ij, and zero on the dustbins.  Nothing of L x S
// elements exists: every entry is treated as a negative by tile passes, the M labels are corrected afterwards (negative term out,
// positive term in), as in dual_softmax_dense_f16s.hip.
//   forward   far_sinkhorn_dense_focal_f16s   the T statistics launches of far_sinkhorn_pos_conf_f16s (every (u^t, v^t) kept), then
//     k_skd_side       the final potentials with padded and masked rows / columns at -huge: p_ij = 2^(x_ij + (dr_i + dc_j))
//     k_skd_pass x2    32-column split-fp16 tile loop; a lane owns one row across all column tiles: ubar_i = sum_j c_neg W_ij, per
//                      workgroup one float64 partial of the loss, per pair the max of |c_neg W|; the second launch swaps the maps
//                      (vbar_j).  Both form x_ij from the three MFMAs in ONE order (that of the last column half-iteration, whose
//                      sum normalised p), so an entry has the same bits in both launches, in k_skd_pos and in the gradient kernel:
//                      it is inside or outside the clamp everywhere alike.
//     k_skd_pos        the labels: p_k with the bits of the tile pass, the correction of the loss (float64) and of W
//     k1_focal_loss    partials and corrections summed in a fixed order -> one device float
//   backward  far_sinkhorn_dense_focal_bwd_f16  k_skd_seed (ubar^T = gup ubar, vbar^T = gup vbar, dustbin seeds 0, the labels'
//             weights gup dW_k), then skt_backward: the sparse backward's launches with k_skt_bwd<.., DENSE> and the labels as its
//             positions.  gup is one device float: no host read.
// No float atomics (one integer atomicMax on float bits per wave, k_skd_pass): the same bits at every launch.
// =====================================================================================================================
__global__ void k_skd_side(const float* __restrict__ uT, const float* __restrict__ vT, const uint8_t* __restrict__ mask0,
                           const uint8_t* __restrict__ mask1, int Z, int L, int S, int Lp, int Sp, float nrm, float* __restrict__ dr,
                           float* __restrict__ dc) {
    const long nl = (long)Z * Lp, total = nl + (long)Z * Sp;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        if (t < nl) {
            const int i = (int)(t % Lp);
            const long z = t / Lp;
            dr[t] = (i < L && !(mask0 && !mask0[z * L + i])) ? uT[t] : -HUGE_F;
        } else {
            const long q = t - nl;
            const int j = (int)(q % Sp);
            const long z = q / Sp;
            dc[q] = (j < S && !(mask1 && !mask1[z * S + j])) ? vT[q] - nrm : -HUGE_F;
        }
    }
}

// the score of the loss passes from an accumulator entry: what is not finite can only come from a masked row or column (p = 0 there)
__device__ __forceinline__ float skd_score(float a, float c1) {
    const float x = a * c1;
    return fabsf(x) < HUGE_F ? x : 0.f;
}

// SWAP: the rows are f0's (the tile holds f1): the two cross terms in the order in which the column half-iteration (rows of f1, tiles
// of f0, score_tile) accumulated them.  roww[z][row] = cneg sum_cols W; lossp[workgroup] (unless null) = its share of the sum of the
// negative-form terms; gmax_bits[z] (unless null) = max |cneg W|.
// grid: Z * Nrp / 128 workgroups of 4 waves; a wave = 32 rows, its two halves take interleaved columns
template <bool SWAP>
__global__ __launch_bounds__(256, 2) void k_skd_pass(const _Float16* __restrict__ ah, const _Float16* __restrict__ al,
                                                     const _Float16* __restrict__ bh, const _Float16* __restrict__ bl, int Z, int Nr, int Nc,
                                                     int Nrp, int Ncp, float c1, const float* __restrict__ rpot,
                                                     const float* __restrict__ cpot, float* __restrict__ roww, FocalK fk,
                                                     unsigned* __restrict__ gmax_bits, double* __restrict__ lossp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ double wsum[4];
    constexpr int STG = 2 * PLANE32;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    int z, Ib;
    tile_coords(Nrp / 128, Z, z, Ib);
    const int irow = Ib * 128 + 32 * wave + l31;
    RowFrags rf;
    rf.load(ah, al, (size_t)z * Nrp + irow, irow, h);
    const float rp = rpot[(size_t)z * Nrp + irow];
    const bool rvalid = rp > DEAD;
    float usum = 0.f, wmx = 0.f;
    double lsum = 0.0;
    int nlo = 0, nhi = 0;
    float* const cw = reinterpret_cast<float*>(lds + 2 * STG);    // [2 stages][32 column potentials]
    const int ntile = (Nc + GT - 1) / GT;
    auto request = [&](int jt, int st) {
        unsigned char* base = lds + st * STG;
        const size_t row0 = (size_t)z * Ncp + (size_t)jt * GT;
        dma_lin(base, reinterpret_cast<const unsigned char*>(bh + row0 * C), PLANE32, tid, wave);
        dma_lin(base + PLANE32, reinterpret_cast<const unsigned char*>(bl + row0 * C), PLANE32, tid, wave);
        if (tid < GT) cw[st * GT + tid] = cpot[row0 + tid];
    };
    request(0, 0);
    for (int jt = 0; jt < ntile; ++jt) {
        const int st = jt & 1;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();                                          // tile jt landed; every read of stage st ^ 1 has returned
        if (jt + 1 < ntile) request(jt + 1, st ^ 1);
        const unsigned char* xs = lds + st * STG;
        f32x16 sc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int off = l31 * ROWB + (((2 * s + h) ^ (l31 & 15)) * 16);
            const f16x8 ch = *reinterpret_cast<const f16x8*>(xs + off);
            const f16x8 cl = *reinterpret_cast<const f16x8*>(xs + PLANE32 + off);
            if (SWAP) score_step_x(sc, ch, cl, rf.hi[s], rf.lo[s]);
            else score_step(sc, ch, cl, rf.hi[s], rf.lo[s]);
        }
        // ---- this lane's row and its 16 columns  c = (r & 3) + 8 (r >> 2) + 4 h
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 c4 = *reinterpret_cast<const float4*>(cw + st * GT + 8 * q + 4 * h);
            const float cc[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool ok = rvalid && cc[e] > DEAD;           // a real pair with both cells unmasked
                const float xe = skd_score(sc[4 * q + e], c1) + (rp + cc[e]);
                const float p = ex2(xe);
                if (p >= P_LO && p <= P_HI) {
                    float term;
                    const float wc = neg_w(p, xe, fk.alpha, fk.gamma, term) * fk.cneg;
                    lsum += (double)term;
                    usum += wc;
                    wmx = fmaxf(wmx, fabsf(wc));
                } else {
                    nlo += (ok && p < P_LO) ? 1 : 0;
                    nhi += p > P_HI ? 1 : 0;
                }
            }
        }
    }
    usum += shfl_xor_f(usum, 32);                                 // the two half-waves hold interleaved columns of the same rows
    if (h == 0) roww[(size_t)z * Nrp + irow] = usum;
    if (gmax_bits) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) wmx = fmaxf(wmx, shfl_xor_f(wmx, m));
        if (lane == 0 && wmx > 0.f && wmx < HUGE_F) atomicMax(gmax_bits + z, __float_as_uint(wmx));     // non-negative floats order as uints
    }
    if (lossp) {
        double tot = lsum + fk.c_lo * (double)nlo + fk.c_hi * (double)nhi;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) tot += __shfl_xor(tot, m, 64);
        if (lane == 0) wsum[wave] = tot;
        __syncthreads();
        if (tid == 0) lossp[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    }
}

// The labels: what replacing the negative term by the positive one changes, dl[k] in the loss and dw[k] in W.  p_k must be the very
// value the tile passes formed at (b_k, i_k, j_k), so it is recomputed the same way (k1d_pos of dual_softmax_dense_f16s.hip): one
// wave per 32 labels gathers their rows of the operand planes into one 32 x 32 MFMA problem (tile role: the labels' columns of f1, row
// role: their rows of f0, the order of k_skd_pass<true>) and reads its diagonal.  A label out of range or on a masked cell is not
// read and corrects nothing.
__global__ __launch_bounds__(256) void k_skd_pos(const _Float16* __restrict__ ah, const _Float16* __restrict__ al,
                                                 const _Float16* __restrict__ bh, const _Float16* __restrict__ bl, int Z, int L, int S,
                                                 int Lp, int Sp, float c1, const int64_t* __restrict__ pb, const int64_t* __restrict__ pi,
                                                 const int64_t* __restrict__ pj, int M, const float* __restrict__ dr,
                                                 const float* __restrict__ dc, FocalK fk, double cpos, double* __restrict__ dl,
                                                 float* __restrict__ dw, unsigned* __restrict__ gmax_bits) {
    const int lane = threadIdx.x & 63, l31 = lane & 31, h = lane >> 5;
    const int nw = gridDim.x * (blockDim.x >> 6);
    for (int k0 = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 32; k0 < M; k0 += nw * 32) {      // wave-uniform
        const int k = min(k0 + l31, M - 1);
        const long zb = pb[k], ib = pi[k], jb = pj[k];
        const bool inr = pos_ok(zb, ib, jb, Z, L, S);
        const size_t z = inr ? (size_t)zb : 0, i = inr ? (size_t)ib : 0, j = inr ? (size_t)jb : 0;
        const _Float16 *ra = ah + (z * Lp + i) * C, *rl = al + (z * Lp + i) * C, *ca = bh + (z * Sp + j) * C, *cb = bl + (z * Sp + j) * C;
        f32x16 sc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int so = 8 * ((2 * s + h) ^ (int)(j & 15)), ro = 8 * ((2 * s + h) ^ (int)(i & 15));
            const f16x8 ch = *reinterpret_cast<const f16x8*>(ca + so), cl = *reinterpret_cast<const f16x8*>(cb + so);
            const f16x8 rh = *reinterpret_cast<const f16x8*>(ra + ro), rlo = *reinterpret_cast<const f16x8*>(rl + ro);
            score_step_x(sc, ch, cl, rh, rlo);
        }
        // the diagonal: this lane's column l31 against tile row mfma32_row(r, h) == l31
        const int rd = (l31 & 3) + 4 * (l31 >> 3);
        float dd = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (r == rd) dd = sc[r];
        if (h == ((l31 >> 2) & 1) && k0 + l31 < M) {
            double t = 0.0, w = 0.0;
            const float rp = dr[z * Lp + i], cp = dc[z * Sp + j];
            if (inr && rp > DEAD && cp > DEAD) {
                const float xe = skd_score(dd, c1) + (rp + cp);
                const float p = ex2(xe);
                const bool in = p >= P_LO && p <= P_HI;
                float tnf = 0.f;
                const float wnf = neg_w(p, xe, fk.alpha, fk.gamma, tnf);                  // the very numbers the tile passes added
                const double q = fmin(fmax((double)p, 1e-6), 1.0 - 1e-6), al_ = fk.alpha, ga = fk.gamma;
                const double lq = log(q), og = pow(1.0 - q, ga);
                const double tn = in ? (double)tnf : (p < P_LO ? fk.c_lo : fk.c_hi);
                const double wn = in ? (double)wnf : 0.0;
                const double tp = -al_ * og * lq;
                const double wp = in ? al_ * (ga * q * (og / (1.0 - q)) * lq - og) : 0.0;
                t = cpos * tp - (double)fk.cneg * tn;
                w = cpos * wp - (double)fk.cneg * wn;
            }
            dl[k0 + l31] = t;
            dw[k0 + l31] = (float)w;
            // |dW_k| joins the pair's largest weight: the gradient kernel's power-of-two scale then keeps every label's weight within
            // the range of the slots (<= FOLD_MAX for T >= 1), so that it meets the tile's own W at that entry in fp32.  A label
            // routed past the tile instead would leave -dW_k there to be multiplied by the fp16-rounded feature row while dW_k
            // itself meets the fp32 one: where ds ~ 0 on a confidently matched row, that rounding is all that remains (measured:
            // 1.2e-2 on dF at T = 1 with pos_weight 0.3 / neg_weight 300, where |dW_k| ~ 2 max |adjoint weight|).
            const float aw = fabsf((float)w);
            if (aw > 0.f && aw < HUGE_F) atomicMax(gmax_bits + z, __float_as_uint(aw));
        }
    }
}

// The seeds of the adjoint recursion at t = T: ubar = gup ubar_dense, vbar = gup vbar_dense (the labels' part is added by
// k_skt_group<0>), dustbin seeds 0 (the dustbin row and column carry no loss term); the labels' weights gup dW_k.  One workgroup per pair.
__global__ __launch_bounds__(256) void k_skd_seed(const float* __restrict__ u, const float* __restrict__ v, const float* __restrict__ dw, int M,
                                                  const float* __restrict__ gup, int Z, int Lp, int Sp, float* __restrict__ ubar,
                                                  float* __restrict__ vbar, float* __restrict__ barbin, float* __restrict__ wpos) {
    const int z = blockIdx.x, tid = threadIdx.x;
    const float g = gup[0];
    for (int i = tid; i < Lp; i += 256) ubar[(size_t)z * Lp + i] = g * u[(size_t)z * Lp + i];
    for (int j = tid; j < Sp; j += 256) vbar[(size_t)z * Sp + j] = g * v[(size_t)z * Sp + j];
    for (int k = z * 256 + tid; k < M; k += Z * 256) wpos[k] = g * dw[k];
    if (tid == 0) { barbin[z] = 0.f; barbin[Z + z] = 0.f; }
}

// wmax[z] = max(wmax[z], |gup| gmax[z]): behind k_skt_wmax, one thread per pair
__global__ void k_skd_wjoin(const unsigned* __restrict__ gmax_bits, const float* __restrict__ gup, int Z, unsigned* __restrict__ wmax_bits) {
    for (int z = threadIdx.x; z < Z; z += blockDim.x) {
        const float m = fabsf(gup[0]) * __uint_as_float(gmax_bits[z]);
        if (m > 0.f && m < HUGE_F && __float_as_uint(m) > wmax_bits[z]) wmax_bits[z] = __float_as_uint(m);
    }
}

// d bin_score of the dense backward, from the dustbin adjoints alone.  k_skt_dbin sums dZc over the dustbin row and column term by
// term; with no loss term on the dustbins almost all of that cancels analytically -- the dustbin row of a row half-step sums to its
// marginal (sum_j Pr(L, j) = 1), the dustbin column of a column half-step likewise, and ubar_L / vbar_S are themselves minus the sums
// they meet there -- while numerically the marginals hold to ~1e-6 only, which at one iteration left 1.7e-3 of a d bin_score that is
// 1500 times smaller than the terms.  Substituting the recursion leaves, per pair,
//   d bin_score = vbar^0_S + sum_{t = 1 .. T} ( vbar^t_S Pc^t(L, S) + ubar^t_L Pr^t(L, S) )       (T >= 1; 0 for T = 0)
// with Pc^t(L, S) = 2^(alpha + U^t_L + V^t_S - lnu_S), Pr^t(L, S) = 2^(alpha + U^t_L - lmu_L + V^{t-1}_S): terms of the size of the
// result.  One thread, pairs and steps in order.
__global__ void k_skd_dbin(const float* __restrict__ binh, const float* __restrict__ barbin, const float* __restrict__ bin_score, int Z, int T,
                           float lmu_l, float lnu_s, float* __restrict__ dbin) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const float alpha = bin_score[0] * LOG2E;
    float tot = 0.f;
    for (int z = 0; z < Z; ++z) {
        float s = T > 0 ? barbin[Z + z] : 0.f;                                            // vbar^0_S
        for (int t = 1; t <= T; ++t) {
            const float ubin = binh[(size_t)t * 2 * Z + z], vbin = binh[(size_t)t * 2 * Z + Z + z], vbinq = binh[(size_t)(t - 1) * 2 * Z + Z + z];
            const float ubarL = barbin[(size_t)t * 2 * Z + z], vbarS = barbin[(size_t)t * 2 * Z + Z + z];
            s += fmaf(vbarS, ex2(alpha + ubin + vbin - lnu_s), ubarL * ex2(alpha + ubin - lmu_l + vbinq));
        }
        tot += s;
    }
    dbin[0] = tot;
}

struct WsT {
    _Float16 *ah, *al, *bh, *bl;
    float *uh, *vh, *binh;           // [(T+1)][Z][Lp], [(T+1)][Z][Sp], [(T+1)][2][Z]: every (u^t, v^t) and the dustbin potentials
    float *ubar, *vbar, *barbin;     // the adjoint vectors at every half-step, same shapes
    unsigned char *at, *bt;          // transposed tiles of f0 / f1
    float *wl, *el, *wsd, *es;       // [2T][Z][Lp] x2, [2T][Z][Sp] x2
    unsigned* wmax;                  // [Z]
    int *sj0, *sj1;                  // [Z][Lp][KFOLD], [Z][Sp][KFOLD]: the rows' slots (column, -1: empty)
    float *sw0, *sw1;                // ... and their scaled weights
    float* part;                     // [Z]
    size_t bytes;
};
inline WsT carve_t(void* ws, int Z, int L, int S, int T) {
    WsT w;
    const int Lp = pad128(L), Sp = pad128(S);
    Carver c{(unsigned char*)ws, 0};
    w.ah = c.take<_Float16>((size_t)Z * Lp * C * 2); w.al = c.take<_Float16>((size_t)Z * Lp * C * 2);
    w.bh = c.take<_Float16>((size_t)Z * Sp * C * 2); w.bl = c.take<_Float16>((size_t)Z * Sp * C * 2);
    const size_t nu = (size_t)(T + 1) * Z * Lp * 4, nv = (size_t)(T + 1) * Z * Sp * 4, nb = (size_t)(T + 1) * 2 * Z * 4;
    w.uh = c.take<float>(nu); w.vh = c.take<float>(nv); w.binh = c.take<float>(nb);
    w.ubar = c.take<float>(nu); w.vbar = c.take<float>(nv); w.barbin = c.take<float>(nb);
    w.at = c.take((size_t)Z * (Lp / GT) * TILE_T);
    w.bt = c.take((size_t)Z * (Sp / GT) * TILE_T);
    const int nt = 2 * T > 0 ? 2 * T : 1;
    w.wl = c.take<float>((size_t)nt * Z * Lp * 4); w.el = c.take<float>((size_t)nt * Z * Lp * 4);
    w.wsd = c.take<float>((size_t)nt * Z * Sp * 4); w.es = c.take<float>((size_t)nt * Z * Sp * 4);
    w.wmax = c.take<unsigned>((size_t)Z * 4);
    w.sj0 = c.take<int>((size_t)Z * Lp * KFOLD * 4); w.sj1 = c.take<int>((size_t)Z * Sp * KFOLD * 4);
    w.sw0 = c.take<float>((size_t)Z * Lp * KFOLD * 4); w.sw1 = c.take<float>((size_t)Z * Sp * KFOLD * 4);
    w.part = c.take<float>((size_t)Z * 4);
    w.bytes = c.o;
    return w;
}

inline bool dims_ok(int Z, int L, int S, int Cc, int T) {
    return Z > 0 && L > 0 && S > 0 && Cc == C && T >= 0 && T <= MAX_ITERS && (long)Z * ((L > S ? L : S) + 128) <= 0x7ff00000L;
}

struct WsD {                         // behind WsT in the workspace of the dense entry points
    float *pr, *pc;                  // [Z][Lp], [Z][Sp]: k_skd_side
    float *u, *v;                    // [Z][Lp], [Z][Sp]: ubar / vbar of the dense part (unscaled)
    double *lossp, *dl;              // [Z Lp / 128], [max(M, 1)]
    float *dw, *wpos;                // [max(M, 1)] x2: the labels' correction of W, and gup times it
    unsigned* gmax;                  // [Z]
    size_t bytes;
};
inline WsD carve_d(void* ws, size_t o, int Z, int L, int S, int M) {
    WsD w;
    const int Lp = pad128(L), Sp = pad128(S);
    const size_t Mc = M > 0 ? M : 1;
    Carver c{(unsigned char*)ws, o};
    w.pr = c.take<float>((size_t)Z * Lp * 4); w.pc = c.take<float>((size_t)Z * Sp * 4);
    w.u = c.take<float>((size_t)Z * Lp * 4); w.v = c.take<float>((size_t)Z * Sp * 4);
    w.lossp = c.take<double>((size_t)Z * (Lp / 128) * 8);
    w.dl = c.take<double>(Mc * 8);
    w.dw = c.take<float>(Mc * 4); w.wpos = c.take<float>(Mc * 4);
    w.gmax = c.take<unsigned>((size_t)Z * 4);
    w.bytes = c.o;
    return w;
}

struct DenseRun {
    const float *pr, *pc, *gup;
    const unsigned* gmax;
    float cneg, alpha, gamma;
};
int skt_backward(const WsT& w, const float* f0, const float* f1, int Z, int L, int S, const float* bin_score, int T,
                 const uint8_t* mask0, const uint8_t* mask1, const int64_t* pb, const int64_t* pi, const int64_t* pj, int M,
                 const float* w_pos, const float* w_bin0, const float* w_bin1, float* df0, float* df1, float* dbin, const DenseRun* dn,
                 hipStream_t stream);

}  // namespace

extern "C" {

size_t far_sinkhorn_pos_conf_workspace_bytes(int Z, int L, int S, int Cc, int iters) {
    if (!dims_ok(Z, L, S, Cc, iters)) return 0;
    return carve_t(nullptr, Z, L, S, iters).bytes;
}

int far_sinkhorn_pos_conf_f16s(const float* f0, const float* f1, int Z, int L, int S, int Cc, const float* bin_score, int iters,
                               const uint8_t* mask0, const uint8_t* mask1, const int64_t* pb, const int64_t* pi, const int64_t* pj,
                               int M, float* conf_pos, float* conf_bin0, float* conf_bin1, void* ws, int* overflow,
                               hipStream_t stream) {
    far_clear_errors();
    if (!f0 || !f1 || !bin_score || !ws || !conf_bin0 || !conf_bin1 || !dims_ok(Z, L, S, Cc, iters) || M < 0 ||
        (M > 0 && (!pb || !pi || !pj || !conf_pos)))
        return FAR_EINVAL;
    const WsT w = carve_t(ws, Z, L, S, iters);
    const int Lp = pad128(L), Sp = pad128(S);
    const int rc = far_skh_history_launch(f0, f1, Z, L, S, bin_score, iters, mask0, mask1, w.ah, w.al, w.bh, w.bl, w.uh, w.vh, w.binh,
                                          overflow, stream);
    if (rc != FAR_OK) return rc;
    const float nrm = (float)(-std::log2((double)L + (double)S));
    const float* uT = w.uh + (size_t)iters * Z * Lp;
    const float* vT = w.vh + (size_t)iters * Z * Sp;
    if (M > 0)
        hipLaunchKernelGGL(k_skt_pos, dim3(std::min((M + 3) / 4, 2048)), dim3(256), 0, stream, f0, f1, Z, L, S, Lp, Sp,
                           1.4426950408889634 / (double)C, pb, pi, pj, M, mask0, mask1, uT, vT, nrm, conf_pos);
    hipLaunchKernelGGL(k_skt_bins, dim3((L + S + 255) / 256, Z), dim3(256), 0, stream, uT, vT, (const float*)(w.binh + (size_t)iters * 2 * Z),
                       bin_score, Z, L, S, Lp, Sp, nrm, conf_bin0, conf_bin1);
    return far_check_launch();
}

int far_sinkhorn_pos_conf_bwd_f16(const float* f0, const float* f1, int Z, int L, int S, int Cc, const float* bin_score, int iters,
                                  const uint8_t* mask0, const uint8_t* mask1, const int64_t* pb, const int64_t* pi, const int64_t* pj,
                                  int M, const float* w_pos, const float* w_bin0, const float* w_bin1, float* df0, float* df1,
                                  float* dbin, void* ws, hipStream_t stream) {
    far_clear_errors();
    if (!f0 || !f1 || !bin_score || !ws || !w_bin0 || !w_bin1 || !df0 || !df1 || !dbin || !dims_ok(Z, L, S, Cc, iters) || M < 0 ||
        (M > 0 && (!pb || !pi || !pj || !w_pos)))
        return FAR_EINVAL;
    const WsT w = carve_t(ws, Z, L, S, iters);
    const int T = iters, Lp = pad128(L), Sp = pad128(S);
    const size_t nu = (size_t)Z * Lp, nv = (size_t)Z * Sp;
    // ---- ubar^T = rowsum(G), vbar^T = colsum(G) without the positions
    hipLaunchKernelGGL(k_skt_seed, dim3(Z), dim3(256), 0, stream, w_bin0, w_bin1, Z, L, S, Lp, Sp, w.ubar + T * nu, w.vbar + T * nv,
                       w.barbin + (size_t)T * 2 * Z);
    return skt_backward(w, f0, f1, Z, L, S, bin_score, T, mask0, mask1, pb, pi, pj, M, w_pos, w_bin0, w_bin1, df0, df1, dbin, nullptr, stream);
}

}  // extern "C"

namespace {

// Everything of the backward behind the seeds ubar^T / vbar^T (the caller has written them without the positions' part): the
// positions' sums, the 2T adjoint half-steps, ds on the matrix core, the positions' own part, d bin_score (dense: k_skd_dbin).  dn: the dense term of
// far_sinkhorn_dense_focal_bwd_f16 (null: the sparse backward, launch for launch what it was).
int skt_backward(const WsT& w, const float* f0, const float* f1, int Z, int L, int S, const float* bin_score, int T,
                 const uint8_t* mask0, const uint8_t* mask1, const int64_t* pb, const int64_t* pi, const int64_t* pj, int M,
                 const float* w_pos, const float* w_bin0, const float* w_bin1, float* df0, float* df1, float* dbin, const DenseRun* dn,
                 hipStream_t stream) {
    const int Lp = pad128(L), Sp = pad128(S);
    const float c1 = (float)(1.4426950408889634 / ((double)C * PRESCALE * PRESCALE));
    const double n2 = -std::log2((double)L + (double)S);
    const float nrm = (float)n2, lmu_l = (float)(std::log2((double)S) + n2), lnu_s = (float)(std::log2((double)L) + n2);
    const size_t nu = (size_t)Z * Lp, nv = (size_t)Z * Sp;
    const unsigned gpos = (unsigned)std::min((M + 3) / 4, 2048);
    if (M > 0)
        hipLaunchKernelGGL(k_skt_group<0>, dim3(gpos, 2), dim3(256), 0, stream, pb, pi, pj, w_pos, M, Z, L, S, Lp, Sp, mask0, mask1,
                           w.ubar + T * nu, w.vbar + T * nv, (const float*)nullptr, (const float*)nullptr, 0.f, (float*)nullptr,
                           (float*)nullptr, (const unsigned*)nullptr, 0, 0, (int*)nullptr, (float*)nullptr, (int*)nullptr, (float*)nullptr);
    // ---- the adjoint half-steps, t = T .. 1
    const size_t smem_a = 2 * TILE_PLANE + (2 * KT + 8) * sizeof(float);
    FAR_ONCE_PER_DEVICE(hipFuncSetAttribute((const void*)k_skt_adj<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_a);
                        hipFuncSetAttribute((const void*)k_skt_adj<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_a));
    auto* adj = dn ? k_skt_adj<true> : k_skt_adj<false>;
    for (int t = T; t >= 1; --t) {
        const float* bt = w.binh + (size_t)t * 2 * Z;            // (U_L, V_S) at t
        const float* bq = w.binh + (size_t)(t - 1) * 2 * Z;
        float* ab = w.barbin + (size_t)t * 2 * Z;                // (ubar_L, vbar_S) at t
        float* aq = w.barbin + (size_t)(t - 1) * 2 * Z;
        // column half-step: rows = the L side, weights vbar^t, potentials (u^t, v^t)
        hipLaunchKernelGGL(adj, dim3((Lp / 128) * Z), dim3(256), smem_a, stream, w.ah, w.al, w.bh, w.bl, Z, L, S, Lp, Sp, c1,
                           mask0, mask1, (const float*)(w.uh + t * nu), bt, (const float*)(w.vh + t * nv), bt + Z,
                           (const float*)(w.vbar + t * nv), (const float*)(ab + Z), bin_score, nrm, lnu_s, t == T ? 1 : 0,
                           w.ubar + t * nu, ab);
        // row half-step: rows = the S side, weights ubar^t, potentials (v^{t-1}, u^t)
        hipLaunchKernelGGL(adj, dim3((Sp / 128) * Z), dim3(256), smem_a, stream, w.bh, w.bl, w.ah, w.al, Z, S, L, Sp, Lp, c1,
                           mask1, mask0, (const float*)(w.vh + (t - 1) * nv), bq + Z, (const float*)(w.uh + t * nu), bt,
                           (const float*)(w.ubar + t * nu), (const float*)ab, bin_score, nrm, lmu_l, 0, w.vbar + (t - 1) * nv, aq + Z);
    }
    // ---- dense part of ds on the matrix core
    if (T > 0 || dn) {
        hipMemsetAsync(w.wmax, 0, (size_t)Z * 4, stream);
        hipLaunchKernelGGL(k_skt_wmax, dim3(8, Z), dim3(256), 0, stream, (const float*)w.ubar, (const float*)w.vbar, Z, Lp, Sp, T, w.wmax);
        if (dn)       // the dense term's largest weight joins the pair's maximum: it shares the fp16 tile with the 2T terms
            hipLaunchKernelGGL(k_skd_wjoin, dim3(1), dim3(256), 0, stream, dn->gmax, dn->gup, Z, w.wmax);
        hipLaunchKernelGGL(k_skt_pack, dim3(gridp((long)2 * T * (nu + nv))), dim3(256), 0, stream, (const float*)w.uh, (const float*)w.vh,
                           (const float*)w.ubar, (const float*)w.vbar, Z, L, S, Lp, Sp, T, nrm, mask0, mask1, (const unsigned*)w.wmax,
                           w.wl, w.el, w.wsd, w.es);
        // the rows' slots: every column -1 (empty), then the first KFOLD positions of each row / column
        hipMemsetAsync(w.sj0, 0xff, (size_t)Z * Lp * KFOLD * 4, stream);
        hipMemsetAsync(w.sj1, 0xff, (size_t)Z * Sp * KFOLD * 4, stream);
        if (M > 0)
            hipLaunchKernelGGL(k_skt_group<1>, dim3(gpos, 2), dim3(256), 0, stream, pb, pi, pj, w_pos, M, Z, L, S, Lp, Sp, mask0, mask1,
                               (float*)nullptr, (float*)nullptr, (const float*)nullptr, (const float*)nullptr, 0.f, (float*)nullptr,
                               (float*)nullptr, (const unsigned*)w.wmax, KFOLD, T, w.sj0, w.sw0, w.sj1, w.sw1);
        hipLaunchKernelGGL(k1_prep_t, dim3(gridp((long)Z * (Lp / GT) * C * 4)), dim3(256), 0, stream, f0, Z, L, Lp, mask0, w.at);
        hipLaunchKernelGGL(k1_prep_t, dim3(gridp((long)Z * (Sp / GT) * C * 4)), dim3(256), 0, stream, f1, Z, S, Sp, mask1, w.bt);
        const int nterm = 2 * T;
        const size_t smem = 2 * (size_t)(STAGE + nterm * 256 + (dn ? 256 : 0));
        const size_t smem_max = 2 * (size_t)(STAGE + 2 * MAX_ITERS * 256);
        const size_t smem_maxd = smem_max + 2 * 256;
        FAR_ONCE_PER_DEVICE(
            hipFuncSetAttribute((const void*)k_skt_bwd<6>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_max);
            hipFuncSetAttribute((const void*)k_skt_bwd<12>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_max);
            hipFuncSetAttribute((const void*)k_skt_bwd<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_max);
            hipFuncSetAttribute((const void*)k_skt_bwd<6, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_maxd);
            hipFuncSetAttribute((const void*)k_skt_bwd<6, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_maxd);
            hipFuncSetAttribute((const void*)k_skt_bwd<0, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_maxd);
            hipFuncSetAttribute((const void*)k_skt_bwd<0, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_maxd));
        // the dense forms: rows of f0 meet the scores in the order <.., 2>, rows of f1 in the order <.., 1> (k_skd_pass's two launches)
        auto* kern0 = !dn ? (nterm <= 6 ? k_skt_bwd<6> : nterm <= 12 ? k_skt_bwd<12> : k_skt_bwd<0>) : (nterm <= 6 ? k_skt_bwd<6, 2> : k_skt_bwd<0, 2>);
        auto* kern1 = !dn ? kern0 : (nterm <= 6 ? k_skt_bwd<6, 1> : k_skt_bwd<0, 1>);
        DenseK d0{}, d1{};
        if (dn) {
            d0 = DenseK{dn->pr, dn->pc, dn->gup, dn->cneg, dn->alpha, dn->gamma};
            d1 = DenseK{dn->pc, dn->pr, dn->gup, dn->cneg, dn->alpha, dn->gamma};
        }
        const float kappa = (float)(1.0 / (double)C);
        hipLaunchKernelGGL(kern0, dim3((Lp / 128) * Z), dim3(256), smem, stream, (const _Float16*)w.ah, (const _Float16*)w.al,
                           (const _Float16*)w.bh, (const _Float16*)w.bl, (const unsigned char*)w.bt, Z, L, S, Lp, Sp, c1, nterm,
                           (const float*)w.wl, (const float*)w.el, (const float*)w.wsd, (const float*)w.es, (const int*)w.sj0,
                           (const float*)w.sw0, (const unsigned*)w.wmax, kappa, df0, d0);
        hipLaunchKernelGGL(kern1, dim3((Sp / 128) * Z), dim3(256), smem, stream, (const _Float16*)w.bh, (const _Float16*)w.bl,
                           (const _Float16*)w.ah, (const _Float16*)w.al, (const unsigned char*)w.at, Z, S, L, Sp, Lp, c1, nterm,
                           (const float*)w.wsd, (const float*)w.es, (const float*)w.wl, (const float*)w.el, (const int*)w.sj1,
                           (const float*)w.sw1, (const unsigned*)w.wmax, kappa, df1, d1);
    } else {
        hipMemsetAsync(df0, 0, (size_t)Z * L * C * 4, stream);
        hipMemsetAsync(df1, 0, (size_t)Z * S * C * 4, stream);
    }
    // ---- sparse part of G, and d bin_score
    if (M > 0)
        hipLaunchKernelGGL(k_skt_group<2>, dim3(gpos, 2), dim3(256), 0, stream, pb, pi, pj, w_pos, M, Z, L, S, Lp, Sp, mask0, mask1,
                           (float*)nullptr, (float*)nullptr, f0, f1, (float)(1.0 / (double)C), df0, df1, (const unsigned*)w.wmax,
                           (T > 0 || dn) ? KFOLD : 0, T, (int*)nullptr, (float*)nullptr, (int*)nullptr, (float*)nullptr);
    if (dn) {
        hipLaunchKernelGGL(k_skd_dbin, dim3(1), dim3(64), 0, stream, (const float*)w.binh, (const float*)w.barbin, bin_score, Z, T, lmu_l, lnu_s, dbin);
        return far_check_launch();
    }
    hipLaunchKernelGGL(k_skt_dbin, dim3(Z), dim3(256), 0, stream, w_bin0, w_bin1, (const float*)w.uh, (const float*)w.vh,
                       (const float*)w.binh, (const float*)w.ubar, (const float*)w.vbar, (const float*)w.barbin, bin_score, Z, L, S, Lp, Sp,
                       T, nrm, lmu_l, lnu_s, w.part);
    hipLaunchKernelGGL(k_skt_dbin_sum, dim3(1), dim3(64), 0, stream, (const float*)w.part, Z, dbin);
    return far_check_launch();
}

}  // namespace

extern "C" {

size_t far_sinkhorn_dense_focal_workspace_bytes(int Z, int L, int S, int Cc, int iters, int M) {
    if (!dims_ok(Z, L, S, Cc, iters) || M < 0) return 0;
    return carve_d(nullptr, carve_t(nullptr, Z, L, S, iters).bytes, Z, L, S, M).bytes;
}

int far_sinkhorn_dense_focal_f16s(const float* f0, const float* f1, int Z, int L, int S, int Cc, const float* bin_score, int iters,
                                  const uint8_t* mask0, const uint8_t* mask1, const int64_t* pb, const int64_t* pi, const int64_t* pj,
                                  int M, float alpha, float gamma, float pos_weight, float neg_weight, int no_gt, float* loss_out,
                                  void* ws, int* overflow, hipStream_t stream) {
    far_clear_errors();
    if (!f0 || !f1 || !bin_score || !ws || !loss_out || !dims_ok(Z, L, S, Cc, iters) || M < 0 || (M > 0 && (!pb || !pi || !pj)))
        return FAR_EINVAL;
    const WsT w = carve_t(ws, Z, L, S, iters);
    const WsD d = carve_d(ws, w.bytes, Z, L, S, M);
    const int Lp = pad128(L), Sp = pad128(S);
    // no_gt: every entry is a negative; the labels handed over then only leave the negative term (the caller passes the dummy entry
    // (0, 0, 0) for a weighted batch)
    const FocalPlan pl = make_plan(Z, L, S, M, alpha, gamma, pos_weight, neg_weight, no_gt);
    const FocalK& fk = pl.fk;
    const int rc = far_skh_history_launch(f0, f1, Z, L, S, bin_score, iters, mask0, mask1, w.ah, w.al, w.bh, w.bl, w.uh, w.vh, w.binh,
                                          overflow, stream);
    if (rc != FAR_OK) return rc;
    const float c1 = (float)(1.4426950408889634 / ((double)C * PRESCALE * PRESCALE));
    const float nrm = (float)(-std::log2((double)L + (double)S));
    hipLaunchKernelGGL(k_skd_side, dim3(gridp((long)Z * (Lp + Sp))), dim3(256), 0, stream, (const float*)(w.uh + (size_t)iters * Z * Lp),
                       (const float*)(w.vh + (size_t)iters * Z * Sp), mask0, mask1, Z, L, S, Lp, Sp, nrm, d.pr, d.pc);
    hipMemsetAsync(d.gmax, 0, (size_t)Z * 4, stream);
    if (M > 0)
        hipLaunchKernelGGL(k_skd_pos, dim3(std::min((M + 127) / 128, 2048)), dim3(256), 0, stream, (const _Float16*)w.ah, (const _Float16*)w.al,
                           (const _Float16*)w.bh, (const _Float16*)w.bl, Z, L, S, Lp, Sp, c1, pb, pi, pj, M, (const float*)d.pr,
                           (const float*)d.pc, fk, pl.cpos, d.dl, d.dw, d.gmax);
    const size_t smem = 2 * (2 * PLANE32) + 2 * GT * sizeof(float);
    FAR_ONCE_PER_DEVICE(hipFuncSetAttribute((const void*)k_skd_pass<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
                        hipFuncSetAttribute((const void*)k_skd_pass<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const int nparts = (Lp / 128) * Z;
    hipLaunchKernelGGL(k_skd_pass<true>, dim3(nparts), dim3(256), smem, stream, (const _Float16*)w.ah, (const _Float16*)w.al,
                       (const _Float16*)w.bh, (const _Float16*)w.bl, Z, L, S, Lp, Sp, c1, (const float*)d.pr, (const float*)d.pc, d.u, fk,
                       d.gmax, d.lossp);
    hipLaunchKernelGGL(k_skd_pass<false>, dim3((Sp / 128) * Z), dim3(256), smem, stream, (const _Float16*)w.bh, (const _Float16*)w.bl,
                       (const _Float16*)w.ah, (const _Float16*)w.al, Z, S, L, Sp, Lp, c1, (const float*)d.pc, (const float*)d.pr, d.v, fk,
                       (unsigned*)nullptr, (double*)nullptr);
    hipLaunchKernelGGL(k1_focal_loss, dim3(1), dim3(256), 0, stream, (const double*)d.lossp, nparts, (const double*)d.dl, M, (double)fk.cneg,
                       loss_out);
    return far_check_launch();
}

int far_sinkhorn_dense_focal_bwd_f16(const float* f0, const float* f1, int Z, int L, int S, int Cc, const float* bin_score, int iters,
                                     const uint8_t* mask0, const uint8_t* mask1, const int64_t* pb, const int64_t* pi, const int64_t* pj,
                                     int M, float alpha, float gamma, float pos_weight, float neg_weight, int no_gt, const float* gup,
                                     float* df0, float* df1, float* dbin, void* ws, hipStream_t stream) {
    far_clear_errors();
    if (!f0 || !f1 || !bin_score || !ws || !gup || !df0 || !df1 || !dbin || !dims_ok(Z, L, S, Cc, iters) || M < 0 ||
        (M > 0 && (!pb || !pi || !pj)))
        return FAR_EINVAL;
    const WsT w = carve_t(ws, Z, L, S, iters);
    const WsD d = carve_d(ws, w.bytes, Z, L, S, M);
    const int T = iters, Lp = pad128(L), Sp = pad128(S);
    const FocalK fk = make_plan(Z, L, S, M, alpha, gamma, pos_weight, neg_weight, no_gt).fk;
    hipLaunchKernelGGL(k_skd_seed, dim3(Z), dim3(256), 0, stream, (const float*)d.u, (const float*)d.v, (const float*)d.dw, M, gup, Z, Lp, Sp,
                       w.ubar + (size_t)T * Z * Lp, w.vbar + (size_t)T * Z * Sp, w.barbin + (size_t)T * 2 * Z, d.wpos);
    const DenseRun dn{d.pr, d.pc, gup, d.gmax, fk.cneg, fk.alpha, fk.gamma};
    return skt_backward(w, f0, f1, Z, L, S, bin_score, T, mask0, mask1, pb, pi, pj, M, (const float*)d.wpos, (const float*)nullptr,
                        (const float*)nullptr, df0, df1, dbin, &dn, stream);
}

}  // extern "C"

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
// Potentials, adjoint vectors and the 2T-term contraction are fp32; the weights are scaled by a power of two so that the dense part
// sits in the fp16 range at any gradient scale (scale_exp).  No data is handed between the workgroups of one launch.
#include "k1_f16s.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr float LOG2E = 1.44269504088896341f;
constexpr int MAX_ITERS = 48;            // the column terms of a tile are staged in LDS: 2 T x 256 B per stage
constexpr int KFOLD = 4;                 // positions per row whose weight joins the dense tile in fp32 (k_skt_bwd)
constexpr float FOLD_MAX = 8192.0f;      // ... unless its scaled weight is above 2^13: KFOLD slots on ONE entry (duplicate positions) stay <= 2^15
constexpr int KB = 32;                   // columns per tile of the gradient kernel
constexpr int TILE_X = KB * ROWB;        // 16 KiB: row-major (swizzled) hi plane tile, for the score recompute
constexpr int TROW = 80;                 // bytes per channel row of a transposed tile: 32 positions x 2 B + 16 B pad
constexpr int TILE_T = C * TROW;         // 20 KiB
constexpr int STAGE = 2 * TILE_X + TILE_T;   // 52 KiB: hi and lo plane tiles + the transposed tile (+ the column terms)

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

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

// One adjoint half-step over the rows of the (Nr x Nc) score matrix of (a, b):
//   out_r   = keep out_r   - ( sum_{c < Nc} cw_c 2^(x_rc + rpot_r + cpot_c - N)     + cwbin 2^(alpha + rpot_r + cbinpot - cmarg_bin) )
//   outbin  = keep outbin  - ( sum_{c < Nc} cw_c 2^(alpha + rbinpot + cpot_c - N)   + cwbin 2^(alpha + rbinpot + cbinpot - cmarg_bin) )
// rpot / cpot: the potentials of the two sides at this half-step (log2 units; padded: -huge), N = log2 of a real row's / column's
// marginal, cmarg_bin that of the column side's dustbin.  cw: the column side's adjoint vector (padded: 0).  The tile loop is
// k_skh_stats' (sinkhorn_f16s.hip); the workgroup of row block 0 also reduces the dustbin row.
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
        score_tile(acc, lds, rf, l31, h);
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

// x [Z][N][256] fp32 -> transposed fp16 tiles [Z][Np / 32][256 ch][TROW] of K1's backward (columns in the order in which the
// accumulator registers hold G), value * 2^4; rows >= N and MASKED rows zero (a masked row may hold anything, also non-finite values)
__global__ void k_skt_prep_t(const float* __restrict__ x, int Z, int N, int Np, const uint8_t* __restrict__ mask,
                             unsigned char* __restrict__ out) {
    const long total = (long)Z * (Np / KB) * C * 4;                       // one thread = 8 positions of one channel row
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const int q = (int)(t & 3);
        const int ch = (int)((t >> 2) & (C - 1));
        const long zt = t >> 10;                                          // z * ntile + tile
        const int ntile = Np / KB;
        const int jt = (int)(zt % ntile);
        const long z = zt / ntile;
        f16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = 16 * (q >> 1) + 4 * (q & 1) + (e & 3) + 8 * (e >> 2);
            const int i = jt * KB + c;
            const bool ok = i < N && !(mask && !mask[(size_t)z * N + i]);
            v[e] = ok ? (_Float16)(x[((size_t)z * N + i) * C + ch] * PRESCALE) : (_Float16)0.f;
        }
        *reinterpret_cast<f16x8*>(out + (size_t)zt * TILE_T + ch * TROW + q * 16) = v;
    }
}

__device__ __forceinline__ void dma_lin(unsigned char* lds, const unsigned char* g, int bytes, int tid, int wave) {
    for (int o = 0; o < bytes; o += 4096)
        __builtin_amdgcn_global_load_lds((gptr_t)(g + o + tid * 16), (lptr_t)(lds + o + wave * 1024), 16, 0, 0);
}

// out[z][row][256] = coef * sum_cols G[row][col] * B[col][:],   G = slots + sum_k rw^k_row cw^k_col 2^(x + re^k_row + ce^k_col)
//   ah / al   row-side hi / lo planes [Z][Nrp][256] fp16 (swizzled LDS image of k1_prep); bh / bl: column side, same layout; bt:
//   column-side transposed tiles (k_skt_prep_t); rw / re [nterm][Z][Nrp], cw / ce [nterm][Z][Ncp]: k_skt_pack's terms;
//   slot_j / slot_w [Z][Nrp][KFOLD]: the row's first positions (column, w 2^e; column -1: empty), k_skt_group<1>.
// The scores are the split-fp16 ones of the forward (hi.hi + hi.lo + lo.hi): where a confident match makes the dense part cancel
// the position's own weight, a relative score error delta would stay as delta |w| next to a result of (1 - P) |w|.  The sum of
// slots and terms is formed in fp32 and leaves as an fp16 (hi, lo) pair; the other map's tile is plain fp16.
// NR > 0: the lane's row terms live in registers (nterm <= NR); NR = 0: they are re-read per tile (any nterm).
// grid: Z * Nrp / 128 workgroups of 4 waves; wave = 32 rows x 256 channels of the output (128 accumulator registers)
template <int NR>
__global__ __launch_bounds__(256, 1) void k_skt_bwd(const _Float16* __restrict__ ah, const _Float16* __restrict__ al,
                                                    const _Float16* __restrict__ bh, const _Float16* __restrict__ bl,
                                                    const unsigned char* __restrict__ bt, int Z, int Nr, int Nc, int Nrp, int Ncp,
                                                    float c1, int nterm, const float* __restrict__ rw, const float* __restrict__ re,
                                                    const float* __restrict__ cw, const float* __restrict__ ce,
                                                    const int* __restrict__ slot_j, const float* __restrict__ slot_w,
                                                    const unsigned* __restrict__ wmax_bits, float kappa, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    int z, Ib;
    tile_coords(Nrp / 128, Z, z, Ib);
    const int irow = Ib * 128 + 32 * wave + l31;
    RowFrags rf;
    rf.load(ah, al, (size_t)z * Nrp + irow, irow, h);
    const size_t rstride = (size_t)Z * Nrp, cstride = (size_t)Z * Ncp;
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
    const int stage = STAGE + nterm * 256;                        // tile planes + [nterm][W 32 | E 32] column terms
    const int ntile = Ncp / KB;
    auto request = [&](int jt, int st) {
        unsigned char* base = lds + st * stage;
        dma_lin(base, reinterpret_cast<const unsigned char*>(bh + ((size_t)z * Ncp + (size_t)jt * KB) * C), TILE_X, tid, wave);
        dma_lin(base + TILE_X, reinterpret_cast<const unsigned char*>(bl + ((size_t)z * Ncp + (size_t)jt * KB) * C), TILE_X, tid, wave);
        dma_lin(base + 2 * TILE_X, bt + ((size_t)z * ntile + jt) * TILE_T, TILE_T, tid, wave);
        for (int o = tid; o < nterm * 64; o += 256) {             // whole waves: nterm * 64 is a multiple of 64
            const int k = o >> 6, c = o & 31;
            const float* src = ((o & 32) ? ce : cw) + (size_t)k * cstride + (size_t)z * Ncp + jt * KB + c;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(base + STAGE + (o - lane) * 4), 4, 0, 0);
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
        f32x16 sc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int off = l31 * ROWB + (((2 * s + h) ^ (l31 & 15)) * 16);
            const f16x8 ch = *reinterpret_cast<const f16x8*>(xs + off);
            const f16x8 cl = *reinterpret_cast<const f16x8*>(xs + TILE_X + off);
            sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, rf.hi[s], sc, 0, 0, 0);
            sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, rf.lo[s], sc, 0, 0, 0);
            sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl, rf.hi[s], sc, 0, 0, 0);
        }
        // ---- G for this lane's row and its 16 columns  c = (r & 3) + 8 (r >> 2) + 4 h; a score that is not finite can only come from a
        // masked row or column (W = 0, E = -huge there): taken as 0 so that it stays out of the products
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float x = sc[r] * c1;
            sc[r] = fabsf(x) < HUGE_F ? x : 0.f;
        }
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
                        g[4 * q + e] = fmaf(rwk * ww[e], ex2(sc[8 * u + 4 * q + e] + (rek + ee[e])), g[4 * q + e]);
                }
            };
            if (NR > 0) {
#pragma unroll
                for (int k = 0; k < NR; ++k)
                    if (k < nterm) term(k, rwr[k], rer[k]);
            } else {
                for (int k = 0; k < nterm; ++k) term(k, rwp[k * rstride], rep[k * rstride]);
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
        const unsigned char* ts = xs + 2 * TILE_X;
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
    const int Lp = (L + 127) / 128 * 128, Sp = (S + 127) / 128 * 128;
    unsigned char* p = (unsigned char*)ws;
    size_t o = 0;
    auto take = [&](size_t n) { unsigned char* r = p ? p + o : nullptr; o += align256(n); return r; };
    w.ah = (_Float16*)take((size_t)Z * Lp * C * 2); w.al = (_Float16*)take((size_t)Z * Lp * C * 2);
    w.bh = (_Float16*)take((size_t)Z * Sp * C * 2); w.bl = (_Float16*)take((size_t)Z * Sp * C * 2);
    const size_t nu = (size_t)(T + 1) * Z * Lp * 4, nv = (size_t)(T + 1) * Z * Sp * 4, nb = (size_t)(T + 1) * 2 * Z * 4;
    w.uh = (float*)take(nu); w.vh = (float*)take(nv); w.binh = (float*)take(nb);
    w.ubar = (float*)take(nu); w.vbar = (float*)take(nv); w.barbin = (float*)take(nb);
    w.at = take((size_t)Z * (Lp / KB) * TILE_T);
    w.bt = take((size_t)Z * (Sp / KB) * TILE_T);
    const int nt = 2 * T > 0 ? 2 * T : 1;
    w.wl = (float*)take((size_t)nt * Z * Lp * 4); w.el = (float*)take((size_t)nt * Z * Lp * 4);
    w.wsd = (float*)take((size_t)nt * Z * Sp * 4); w.es = (float*)take((size_t)nt * Z * Sp * 4);
    w.wmax = (unsigned*)take((size_t)Z * 4);
    w.sj0 = (int*)take((size_t)Z * Lp * KFOLD * 4); w.sj1 = (int*)take((size_t)Z * Sp * KFOLD * 4);
    w.sw0 = (float*)take((size_t)Z * Lp * KFOLD * 4); w.sw1 = (float*)take((size_t)Z * Sp * KFOLD * 4);
    w.part = (float*)take((size_t)Z * 4);
    w.bytes = o;
    return w;
}

inline bool dims_ok(int Z, int L, int S, int Cc, int T) {
    return Z > 0 && L > 0 && S > 0 && Cc == C && T >= 0 && T <= MAX_ITERS && (long)Z * ((L > S ? L : S) + 128) <= 0x7ff00000L;
}

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
    const int Lp = (L + 127) / 128 * 128, Sp = (S + 127) / 128 * 128;
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
    const int T = iters, Lp = (L + 127) / 128 * 128, Sp = (S + 127) / 128 * 128;
    const float c1 = (float)(1.4426950408889634 / ((double)C * PRESCALE * PRESCALE));
    const double n2 = -std::log2((double)L + (double)S);
    const float nrm = (float)n2, lmu_l = (float)(std::log2((double)S) + n2), lnu_s = (float)(std::log2((double)L) + n2);
    const size_t nu = (size_t)Z * Lp, nv = (size_t)Z * Sp;
    auto gridp = [](long n) { long g = (n + 255) / 256; return (unsigned)(g < 16384 ? (g > 0 ? g : 1) : 16384); };
    const unsigned gpos = (unsigned)std::min((M + 3) / 4, 2048);
    // ---- ubar^T = rowsum(G), vbar^T = colsum(G)
    hipLaunchKernelGGL(k_skt_seed, dim3(Z), dim3(256), 0, stream, w_bin0, w_bin1, Z, L, S, Lp, Sp, w.ubar + T * nu, w.vbar + T * nv,
                       w.barbin + (size_t)T * 2 * Z);
    if (M > 0)
        hipLaunchKernelGGL(k_skt_group<0>, dim3(gpos, 2), dim3(256), 0, stream, pb, pi, pj, w_pos, M, Z, L, S, Lp, Sp, mask0, mask1,
                           w.ubar + T * nu, w.vbar + T * nv, (const float*)nullptr, (const float*)nullptr, 0.f, (float*)nullptr,
                           (float*)nullptr, (const unsigned*)nullptr, 0, 0, (int*)nullptr, (float*)nullptr, (int*)nullptr, (float*)nullptr);
    // ---- the adjoint half-steps, t = T .. 1
    const size_t smem_a = 2 * TILE_PLANE + (2 * KT + 8) * sizeof(float);
    FAR_ONCE_PER_DEVICE(hipFuncSetAttribute((const void*)k_skt_adj, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_a));
    for (int t = T; t >= 1; --t) {
        const float* bt = w.binh + (size_t)t * 2 * Z;            // (U_L, V_S) at t
        const float* bq = w.binh + (size_t)(t - 1) * 2 * Z;
        float* ab = w.barbin + (size_t)t * 2 * Z;                // (ubar_L, vbar_S) at t
        float* aq = w.barbin + (size_t)(t - 1) * 2 * Z;
        // column half-step: rows = the L side, weights vbar^t, potentials (u^t, v^t)
        hipLaunchKernelGGL(k_skt_adj, dim3((Lp / 128) * Z), dim3(256), smem_a, stream, w.ah, w.al, w.bh, w.bl, Z, L, S, Lp, Sp, c1,
                           mask0, mask1, (const float*)(w.uh + t * nu), bt, (const float*)(w.vh + t * nv), bt + Z,
                           (const float*)(w.vbar + t * nv), (const float*)(ab + Z), bin_score, nrm, lnu_s, t == T ? 1 : 0,
                           w.ubar + t * nu, ab);
        // row half-step: rows = the S side, weights ubar^t, potentials (v^{t-1}, u^t)
        hipLaunchKernelGGL(k_skt_adj, dim3((Sp / 128) * Z), dim3(256), smem_a, stream, w.bh, w.bl, w.ah, w.al, Z, S, L, Sp, Lp, c1,
                           mask1, mask0, (const float*)(w.vh + (t - 1) * nv), bq + Z, (const float*)(w.uh + t * nu), bt,
                           (const float*)(w.ubar + t * nu), (const float*)ab, bin_score, nrm, lmu_l, 0, w.vbar + (t - 1) * nv, aq + Z);
    }
    // ---- dense part of ds on the matrix core
    if (T > 0) {
        hipMemsetAsync(w.wmax, 0, (size_t)Z * 4, stream);
        hipLaunchKernelGGL(k_skt_wmax, dim3(8, Z), dim3(256), 0, stream, (const float*)w.ubar, (const float*)w.vbar, Z, Lp, Sp, T, w.wmax);
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
        hipLaunchKernelGGL(k_skt_prep_t, dim3(gridp((long)Z * (Lp / KB) * C * 4)), dim3(256), 0, stream, f0, Z, L, Lp, mask0, w.at);
        hipLaunchKernelGGL(k_skt_prep_t, dim3(gridp((long)Z * (Sp / KB) * C * 4)), dim3(256), 0, stream, f1, Z, S, Sp, mask1, w.bt);
        const int nterm = 2 * T;
        const size_t smem = 2 * (size_t)(STAGE + nterm * 256);
        const size_t smem_max = 2 * (size_t)(STAGE + 2 * MAX_ITERS * 256);
        FAR_ONCE_PER_DEVICE(
            hipFuncSetAttribute((const void*)k_skt_bwd<6>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_max);
            hipFuncSetAttribute((const void*)k_skt_bwd<12>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_max);
            hipFuncSetAttribute((const void*)k_skt_bwd<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_max));
        auto* kern = nterm <= 6 ? k_skt_bwd<6> : nterm <= 12 ? k_skt_bwd<12> : k_skt_bwd<0>;
        const float kappa = (float)(1.0 / (double)C);
        hipLaunchKernelGGL(kern, dim3((Lp / 128) * Z), dim3(256), smem, stream, (const _Float16*)w.ah, (const _Float16*)w.al,
                           (const _Float16*)w.bh, (const _Float16*)w.bl, (const unsigned char*)w.bt, Z, L, S, Lp, Sp, c1, nterm,
                           (const float*)w.wl, (const float*)w.el, (const float*)w.wsd, (const float*)w.es, (const int*)w.sj0,
                           (const float*)w.sw0, (const unsigned*)w.wmax, kappa, df0);
        hipLaunchKernelGGL(kern, dim3((Sp / 128) * Z), dim3(256), smem, stream, (const _Float16*)w.bh, (const _Float16*)w.bl,
                           (const _Float16*)w.ah, (const _Float16*)w.al, (const unsigned char*)w.at, Z, S, L, Sp, Lp, c1, nterm,
                           (const float*)w.wsd, (const float*)w.es, (const float*)w.wl, (const float*)w.el, (const int*)w.sj1,
                           (const float*)w.sw1, (const unsigned*)w.wmax, kappa, df1);
    } else {
        hipMemsetAsync(df0, 0, (size_t)Z * L * C * 4, stream);
        hipMemsetAsync(df1, 0, (size_t)Z * S * C * 4, stream);
    }
    // ---- sparse part of G, and d bin_score
    if (M > 0)
        hipLaunchKernelGGL(k_skt_group<2>, dim3(gpos, 2), dim3(256), 0, stream, pb, pi, pj, w_pos, M, Z, L, S, Lp, Sp, mask0, mask1,
                           (float*)nullptr, (float*)nullptr, f0, f1, (float)(1.0 / (double)C), df0, df1, (const unsigned*)w.wmax,
                           T > 0 ? KFOLD : 0, T, (int*)nullptr, (float*)nullptr, (int*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(k_skt_dbin, dim3(Z), dim3(256), 0, stream, w_bin0, w_bin1, (const float*)w.uh, (const float*)w.vh,
                       (const float*)w.binh, (const float*)w.ubar, (const float*)w.vbar, (const float*)w.barbin, bin_score, Z, L, S, Lp, Sp,
                       T, nrm, lmu_l, lnu_s, w.part);
    hipLaunchKernelGGL(k_skt_dbin_sum, dim3(1), dim3(64), 0, stream, (const float*)w.part, Z, dbin);
    return far_check_launch();
}

}  // extern "C"

// K1 on the training path with DENSE coarse supervision (match_type 'dual_softmax', coarse_type 'focal', sparse_spvs = False:
// loftr_loss.py:56-75, :87-89, :121-127 -- the loftr_ds_dense configurations).  The loss reads every entry of conf_matrix:
//     q = clamp(p, 1e-6, 1 - 1e-6)
//     loss = c_pos sum_pos w (-alpha (1 - q)^gamma log q) + c_neg sum_neg w (-alpha q^gamma log(1 - q))
//     c_pos = pos_weight / #positives,  c_neg = neg_weight / (N L S - #positives),  w_ab = mask0_a mask1_b
// and neither the (N, L, S) matrix nor anything else of that size exists here.  Every entry is treated as a negative by the tile
// passes; the M positives (spv_b/i/j_ids) are corrected afterwards (negative term out, positive term in).
//
//   forward   far_coarse_dense_focal_f16s     statistics passes of the matcher (dual_softmax_f16s.hip, masks included), then
//               k1d_pass<0> x2  a 32-column split-fp16 tile loop (the three MFMAs per 16 channels of k1_f16s.h, in both orders in which
//                               the two statistics passes accumulated them: each statistic meets the score it was summed from); a lane owns one row: p = R C per entry, the focal term and W = (dLoss/dp) p in
//                               closed form for the entries inside the clamp's range (the others are constants with W = 0);
//                               per row u_a = sum_b W_ab (complete: the workgroup walks every column tile), per workgroup one
//                               float64 partial of the loss.  The second launch swaps the maps' roles: v_b = sum_a W_ab.
//               k1d_pos         p_k at the positives, bit for bit as the tile pass formed it; the correction of the loss and of W
//               k1d_finish      u, v += the positives' corrections (each row scans the M labels in order), device max of |W|, |u|, |v|
//               k1_focal_loss   partials + corrections summed in a fixed order
//             No float atomics anywhere: the same bits at every launch.
//   backward  far_coarse_dense_focal_bwd_f16  dLoss/dx = 2 W - u R - v C (log p = 2 x - lse_row - lse_col);  dF0 = kappa G F1,
//             dF1 = kappa G^T F0.  k1d_pass<1|2> recomputes the score tile exactly as the forward did, forms G in the accumulator
//             registers (W again in closed form from p) and feeds it into the second MFMA against the other map's transposed
//             fp16 tile, as k1_bwd does (dual_softmax_bwd_f16.hip); launched twice with the roles swapped.  G is scaled by a
//             power of two read from device memory (the forward's max) and carried as ONE fp16 (<1>) or as a hi + lo pair (<2>).
//             The positives' correction 2 kappa dW_k F[other] is added by k1d_pos_rows: one wave per output row, labels in order.
#include "k1_train_f16s.h"
#include <algorithm>

namespace {

constexpr float VALID_BELOW = 1.0e29f;     // a statistic below this marks a real, unmasked position (+HUGE_F otherwise)

// the negative-form focal term of an entry inside the clamp's range, and W = (d term / d p) p.  (neg_w of sinkhorn_train_f16s.hip is
// other arithmetic -- a hardware log plus a series, from the exponent of p -- and is kept apart on purpose.)
__device__ __forceinline__ float neg_w(float p, float alpha, float gamma, float& term) {
    const float l1 = log1pf(-p);
    const float qg = __builtin_amdgcn_exp2f(gamma * __builtin_amdgcn_logf(p));
    term = -alpha * qg * l1;
    return alpha * qg * (p / (1.0f - p) - gamma * l1);
}

// padded statistics of one side: (max, 1 / sum) of a real, unmasked position; (+huge, 0) otherwise
__global__ void k1d_side(const float2* __restrict__ stat, const uint8_t* __restrict__ mask, int Z, int N, int Np,
                         float* __restrict__ dmax, float* __restrict__ dinv) {
    const long total = (long)Z * Np;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const int i = (int)(t % Np);
        const long z = t / Np;
        float m = HUGE_F, r = 0.f;
        if (i < N && (!mask || mask[z * N + i])) {
            const float2 st = stat[z * N + i];
            m = st.x;
            r = 1.0f / st.y;
        }
        dmax[t] = m;
        dinv[t] = r;
    }
}

__device__ __forceinline__ float scale_of(const unsigned* gmax_bits, int& e) {
    e = grad_scale_exp(gmax_bits, 2);                                     // 4 gmax 2^e <= 1
    e = e < -100 ? -100 : (e > 100 ? 100 : e);
    return ldexpf(1.0f, e);
}

// MODE 0 (loss pass): roww[z][row] = sum_cols W (written), lossp[workgroup] = the workgroup's share of sum_entries term (unless null),
//                     gmax_bits = atomic max of |W| (unless null)
// MODE 1 / 2 (gradient pass): out[z][row][256] = kappa g sum_cols G[row][col] B[col][:],  G = 2 W - roww_row R - colw_col C
//   ah, al   row-side planes [Z][Nrp][256] fp16 (k1_prep); bh, bl: column-side planes; bt: column-side transposed tiles (k1_prep_t)
//   rmax, rinv [Z][Nrp] / cmax, cinv [Z][Ncp]: k1d_side
// grid: Z * Nrp / 128 workgroups of 4 waves; wave = 32 rows (x 256 channels of the output: 128 accumulator registers)
template <int MODE>
__global__ __launch_bounds__(256, 1) void k1d_pass(const _Float16* __restrict__ ah, const _Float16* __restrict__ al,
                                                   const _Float16* __restrict__ bh, const _Float16* __restrict__ bl,
                                                   const unsigned char* __restrict__ bt, int Z, int Nr, int Nc, int Nrp, int Ncp, float c1,
                                                   const float* __restrict__ rmax, const float* __restrict__ rinv,
                                                   const float* __restrict__ cmax, const float* __restrict__ cinv,
                                                   float* __restrict__ roww, const float* __restrict__ colw, FocalK fk,
                                                   unsigned* __restrict__ gmax_bits, double* __restrict__ lossp,
                                                   const float* __restrict__ gup, float kappa, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ double wsum[4];
    constexpr int STAGE = 2 * PLANE32 + (MODE ? TILE_T : 0);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    int z, Ib;
    tile_coords(Nrp / 128, Z, z, Ib);
    const int irow = Ib * 128 + 32 * wave + l31;
    RowFrags rf;
    rf.load(ah, al, (size_t)z * Nrp + irow, irow, h);
    const float rm = rmax[(size_t)z * Nrp + irow], ri = rinv[(size_t)z * Nrp + irow];
    const bool rvalid = rm < VALID_BELOW;
    int ge = 0;
    float gs = 1.0f, us = 0.f;
    if constexpr (MODE != 0) {
        gs = scale_of(gmax_bits, ge);
        us = roww[(size_t)z * Nrp + irow] * gs;
    }
    const float w2 = 2.0f * fk.cneg * gs;
    f32x16 acc[MODE ? 8 : 1];                                     // [channel block nt][rows]: D[m = row][n = channel]
#pragma unroll
    for (int nt = 0; nt < (MODE ? 8 : 1); ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
    float usum = 0.f, wmx = 0.f;
    double lsum = 0.0;
    int nlo = 0, nhi = 0;
    float* const cw = reinterpret_cast<float*>(lds + 2 * STAGE);  // [2 stages][cmax 32 | cinv 32 | colw 32]
    const int ntile = (Nc + GT - 1) / GT;
    auto request = [&](int jt, int st) {
        unsigned char* base = lds + st * STAGE;
        const size_t row0 = (size_t)z * Ncp + (size_t)jt * GT;
        dma_lin(base, reinterpret_cast<const unsigned char*>(bh + row0 * C), PLANE32, tid, wave);
        dma_lin(base + PLANE32, reinterpret_cast<const unsigned char*>(bl + row0 * C), PLANE32, tid, wave);
        if (MODE) dma_lin(base + 2 * PLANE32, bt + ((size_t)z * (Ncp / GT) + jt) * TILE_T, TILE_T, tid, wave);
        if (tid < GT) {
            cw[st * 96 + tid] = cmax[row0 + tid];
            cw[st * 96 + 32 + tid] = cinv[row0 + tid];
            if (MODE) cw[st * 96 + 64 + tid] = colw[row0 + tid] * gs;
        }
    };
    request(0, 0);
    for (int jt = 0; jt < ntile; ++jt) {
        const int st = jt & 1;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();                                          // tile jt landed; every read of stage st ^ 1 has returned
        if (jt + 1 < ntile) request(jt + 1, st ^ 1);
        const unsigned char* xs = lds + st * STAGE;
        // ---- scores, transposed: D[m = column of the tile][n = this lane's row], TWICE: hi.hi + hi.lo + lo.hi accumulated in the order
        // of the statistics pass that owns this launch's rows (xr: score_tile's order) and in the order of the pass that owns its
        // columns, where the maps' roles were swapped (xc: the two cross terms the other way round).  The two differ by the fp32
        // rounding of a 768-term sum, ~1e-5 in the log2 domain -- and only the score a statistic was summed FROM cancels against it:
        // R = 2^(xr - rowmax) / rowsum is exactly 1 / rowsum at the row's maximum, C likewise from xc.  With one score for both, a
        // confident entry (1 - p ~ 1e-13) would come out as p = 1 +- 7e-6, inside the clamp, with W ~ 1e5 times too large.
        f32x16 sc, sx;
#pragma unroll
        for (int r = 0; r < 16; ++r) { sc[r] = 0.f; sx[r] = 0.f; }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int off = l31 * ROWB + (((2 * s + h) ^ (l31 & 15)) * 16);
            const f16x8 ch = *reinterpret_cast<const f16x8*>(xs + off);
            const f16x8 cl = *reinterpret_cast<const f16x8*>(xs + PLANE32 + off);
            score_step_both(sc, sx, ch, cl, rf.hi[s], rf.lo[s]);
        }
        // ---- this lane's row and its 16 columns  c = (r & 3) + 8 (r >> 2) + 4 h
        f16x8 gh[2], gl[2];
#pragma unroll
        for (int q = 0; q < 4; ++q) {                             // streamed: four columns' statistics at a time
            const float4 m4 = *reinterpret_cast<const float4*>(cw + st * 96 + 8 * q + 4 * h);
            const float4 i4 = *reinterpret_cast<const float4*>(cw + st * 96 + 32 + 8 * q + 4 * h);
            float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (MODE) v4 = *reinterpret_cast<const float4*>(cw + st * 96 + 64 + 8 * q + 4 * h);
            const float cm[4] = {m4.x, m4.y, m4.z, m4.w}, ci[4] = {i4.x, i4.y, i4.z, i4.w}, vs[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * q + e;
                const bool ok = rvalid && cm[e] < VALID_BELOW;    // a real pair with both cells unmasked
                const float xr = ok ? sc[r] * c1 : -HUGE_F, xc = ok ? sx[r] * c1 : -HUGE_F;
                const float R = __builtin_amdgcn_exp2f(xr - rm) * ri, Cc = __builtin_amdgcn_exp2f(xc - cm[e]) * ci[e];
                const float p = R * Cc;
                float w = 0.f;
                if (p >= P_LO && p <= P_HI) {
                    float term;
                    w = neg_w(p, fk.alpha, fk.gamma, term);
                    if (MODE == 0) lsum += (double)term;
                } else if (MODE == 0) {
                    nlo += (ok && p < P_LO) ? 1 : 0;
                    nhi += p > P_HI ? 1 : 0;
                }
                if (MODE == 0) {
                    const float wc = w * fk.cneg;
                    usum += wc;
                    wmx = fmaxf(wmx, fabsf(wc));
                } else {
                    const float g = (w * w2 - us * R) - vs[e] * Cc;
                    const _Float16 g16 = (_Float16)g;
                    gh[r >> 3][r & 7] = g16;
                    if (MODE == 2) gl[r >> 3][r & 7] = (_Float16)(g - (float)g16);
                }
            }
        }
        if constexpr (MODE != 0) {
            // ---- out[row][channel] += G[row][col] * B[col][channel]: A = G (registers), B = transposed tile (LDS)
            const unsigned char* ts = xs + 2 * PLANE32;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int nt = 0; nt < 8; ++nt) {
                    const f16x8 tf = *reinterpret_cast<const f16x8*>(ts + (32 * nt + l31) * TROW + (2 * u + h) * 16);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh[u], tf, acc[nt], 0, 0, 0);
                    if (MODE == 2) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(gl[u], tf, acc[nt], 0, 0, 0);
                }
        }
    }
    if constexpr (MODE == 0) {
        usum += shfl_xor_f(usum, 32);                             // the two half-waves hold interleaved columns of the same rows
        if (h == 0) roww[(size_t)z * Nrp + irow] = usum;
        if (gmax_bits) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) wmx = fmaxf(wmx, shfl_xor_f(wmx, m));
            if (lane == 0 && wmx > 0.f) atomicMax(gmax_bits, __float_as_uint(wmx));          // non-negative floats order as uints
        }
        if (lossp) {
            double tot = lsum + fk.c_lo * (double)nlo + fk.c_hi * (double)nhi;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) tot += __shfl_xor(tot, m, 64);
            if (lane == 0) wsum[wave] = tot;
            __syncthreads();
            if (tid == 0) lossp[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        }
    } else {
        // ---- epilogue: undo the scalings (tile x 2^4, G x 2^ge), apply kappa and the upstream gradient
        const float coef = kappa * gup[0] * ldexpf(1.0f, -ge) / PRESCALE;
        const int row0 = Ib * 128 + 32 * wave;
#pragma unroll
        for (int nt = 0; nt < 8; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = row0 + mfma32_row(r, h);
                if (i < Nr) out[((size_t)z * Nr + i) * C + 32 * nt + l31] = acc[nt][r] * coef;
            }
    }
}

// The positives: what replacing the negative term by the positive one changes, dl[k] in the loss and dw[k] in W.  p_k must be the very
// value the tile pass formed at (b_k, i_k, j_k) -- on which side of the clamp it fell decides what there is to take out -- so it is
// recomputed the same way: one wave per 32 labels gathers their rows of the operand planes into one 32 x 32 MFMA problem (tile role:
// the labels' columns, row role: their rows) and reads its diagonal; an accumulator entry depends on its own row and column only, so
// these are the bits of k1d_pass.  dummy: the single label is entry (0, 0, 0) whatever the id arrays hold.
__global__ __launch_bounds__(256) void k1d_pos(const _Float16* __restrict__ ah, const _Float16* __restrict__ al,
                                               const _Float16* __restrict__ bh, const _Float16* __restrict__ bl, int Lp, int Sp, float c1,
                                               const int64_t* __restrict__ pb, const int64_t* __restrict__ pi,
                                               const int64_t* __restrict__ pj, int M, int dummy, const float* __restrict__ rmax,
                                               const float* __restrict__ rinv, const float* __restrict__ cmax,
                                               const float* __restrict__ cinv, FocalK fk, double cpos, double* __restrict__ dl,
                                               float* __restrict__ dw) {
    const int lane = threadIdx.x & 63, l31 = lane & 31, h = lane >> 5;
    const int nw = gridDim.x * (blockDim.x >> 6);
    for (int k0 = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 32; k0 < M; k0 += nw * 32) {      // wave-uniform
        const int k = min(k0 + l31, M - 1);
        const size_t z = dummy ? 0 : (size_t)pb[k], i = dummy ? 0 : (size_t)pi[k], j = dummy ? 0 : (size_t)pj[k];
        const _Float16 *ra = ah + (z * Lp + i) * C, *rl = al + (z * Lp + i) * C, *ca = bh + (z * Sp + j) * C, *cb = bl + (z * Sp + j) * C;
        f32x16 sc, sx;
#pragma unroll
        for (int r = 0; r < 16; ++r) { sc[r] = 0.f; sx[r] = 0.f; }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int so = 8 * ((2 * s + h) ^ (int)(j & 15)), ro = 8 * ((2 * s + h) ^ (int)(i & 15));
            const f16x8 ch = *reinterpret_cast<const f16x8*>(ca + so), cl = *reinterpret_cast<const f16x8*>(cb + so);
            const f16x8 rh = *reinterpret_cast<const f16x8*>(ra + ro), rlo = *reinterpret_cast<const f16x8*>(rl + ro);
            score_step_both(sc, sx, ch, cl, rh, rlo);
        }
        // the diagonal: this lane's column l31 against tile row mfma32_row(r, h) == l31
        const int rd = (l31 & 3) + 4 * (l31 >> 3);
        float dr = 0.f, dc = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (r == rd) { dr = sc[r]; dc = sx[r]; }
        if (h == ((l31 >> 2) & 1) && k0 + l31 < M) {
            const float rm = rmax[z * Lp + i], cm = cmax[z * Sp + j];
            double t = 0.0, w = 0.0;
            if (rm < VALID_BELOW && cm < VALID_BELOW) {
                const float R = __builtin_amdgcn_exp2f(dr * c1 - rm) * rinv[z * Lp + i];
                const float Cc = __builtin_amdgcn_exp2f(dc * c1 - cm) * cinv[z * Sp + j];
                const float p = R * Cc;
                const bool in = p >= P_LO && p <= P_HI;
                const double q = fmin(fmax((double)p, 1e-6), 1.0 - 1e-6), al_ = fk.alpha, ga = fk.gamma;
                const double lq = log(q), l1 = log1p(-q), qg = pow(q, ga), og = pow(1.0 - q, ga);
                const double tn = in ? -al_ * qg * l1 : (p < P_LO ? fk.c_lo : fk.c_hi);
                const double wn = in ? al_ * qg * (q / (1.0 - q) - ga * l1) : 0.0;
                const double tp = -al_ * og * lq;
                const double wp = in ? al_ * (ga * q * (og / (1.0 - q)) * lq - og) : 0.0;
                t = cpos * tp - (double)fk.cneg * tn;
                w = cpos * wp - (double)fk.cneg * wn;
            }
            dl[k0 + l31] = t;
            dw[k0 + l31] = (float)w;
        }
    }
}

// u[z][i] += sum_{k: (b_k, i_k) = (z, i)} dw_k and v[z][j] likewise, the labels in order (one thread per row / column: no atomics),
// then the device maximum of |u|, |v| joins that of |W|
__global__ void k1d_finish(const int64_t* __restrict__ pb, const int64_t* __restrict__ pi, const int64_t* __restrict__ pj, int M, int dummy,
                           const float* __restrict__ dw, int Z, int L, int S, int Lp, int Sp, float* __restrict__ u, float* __restrict__ v,
                           unsigned* __restrict__ gmax_bits) {
    const long nL = (long)Z * L, total = nL + (long)Z * S;
    float mx = 0.f;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const bool side1 = t >= nL;
        const long r = side1 ? t - nL : t;
        const int N = side1 ? S : L, Np = side1 ? Sp : Lp;
        const int64_t z = r / N, i = r % N;
        const int64_t* const px = side1 ? pj : pi;
        float* const dst = (side1 ? v : u) + z * Np + i;
        float s = *dst;
        if (dummy) {
            if (z == 0 && i == 0) s += dw[0];
        } else {
            for (int k = 0; k < M; ++k)
                if (pb[k] == z && px[k] == i) s += dw[k];
        }
        *dst = s;
        mx = fmaxf(mx, fabsf(s));
    }
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < M; k += gridDim.x * blockDim.x) mx = fmaxf(mx, fabsf(dw[k]));
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, shfl_xor_f(mx, m));
    if ((threadIdx.x & 63) == 0 && mx > 0.f) atomicMax(gmax_bits, __float_as_uint(mx));
}

// the positives' part of the gradient: df0[z, i] += 2 kappa g sum_{k: (b_k, i_k) = (z, i)} dw_k F1[z, j_k] and df1[z, j] likewise;
// one wave per output row scans the labels in order (no atomics)
__global__ __launch_bounds__(256) void k1d_pos_rows(const float* __restrict__ f0, const float* __restrict__ f1, int Z, int L, int S,
                                                    const int64_t* __restrict__ pb, const int64_t* __restrict__ pi,
                                                    const int64_t* __restrict__ pj, int M, int dummy, const float* __restrict__ dw,
                                                    float kappa2, const float* __restrict__ gup, float* __restrict__ df0,
                                                    float* __restrict__ df1) {
    const int lane = threadIdx.x & 63;
    const long nL = (long)Z * L, total = nL + (long)Z * S;
    const long nw = (long)gridDim.x * (blockDim.x >> 6);
    for (long t = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < total; t += nw) {
        const bool side1 = t >= nL;
        const long r = side1 ? t - nL : t;
        const int N = side1 ? S : L, No = side1 ? L : S;
        const int64_t z = r / N, i = r % N;
        const int64_t* const px = side1 ? pj : pi;
        const int64_t* const po = side1 ? pi : pj;
        const float* const fo = side1 ? f0 : f1;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        bool any = false;
        if (dummy) {
            if (z == 0 && i == 0) {
                const float4 b = *reinterpret_cast<const float4*>(fo + 4 * lane);
                const float w = dw[0];
                s = make_float4(w * b.x, w * b.y, w * b.z, w * b.w);
                any = true;
            }
        } else {
            for (int k = 0; k < M; ++k)
                if (pb[k] == z && px[k] == i) {
                    const float4 b = *reinterpret_cast<const float4*>(fo + ((size_t)z * No + (size_t)po[k]) * C + 4 * lane);
                    const float w = dw[k];
                    s.x += w * b.x; s.y += w * b.y; s.z += w * b.z; s.w += w * b.w;
                    any = true;
                }
        }
        if (any) {
            const float c = kappa2 * gup[0];
            float4* const dst = reinterpret_cast<float4*>((side1 ? df1 : df0) + (size_t)r * C + 4 * lane);
            float4 o = *dst;
            o.x += c * s.x; o.y += c * s.y; o.z += c * s.z; o.w += c * s.w;
            *dst = o;
        }
    }
}

struct WsD {
    unsigned char *at, *bt;                // transposed tiles of f0 / f1 (backward)
    float *rmax, *rinv, *u;                // [Z][Lp]
    float *cmax, *cinv, *v;                // [Z][Sp]
    double *lossp, *dl;                    // [Z Lp / 128], [max(M, 1)]
    float* dw;                             // [max(M, 1)]
    unsigned* gmax;
    size_t bytes;
};
inline WsD carve_d(unsigned char* p, size_t o, int Z, int L, int S, int M) {
    WsD w;
    const int Lp = pad128(L), Sp = pad128(S);
    const size_t Mc = M > 0 ? M : 1;
    Carver c{p, o};
    w.at = c.take((size_t)Z * (Lp / GT) * TILE_T);
    w.bt = c.take((size_t)Z * (Sp / GT) * TILE_T);
    w.rmax = c.take<float>((size_t)Z * Lp * 4); w.rinv = c.take<float>((size_t)Z * Lp * 4); w.u = c.take<float>((size_t)Z * Lp * 4);
    w.cmax = c.take<float>((size_t)Z * Sp * 4); w.cinv = c.take<float>((size_t)Z * Sp * 4); w.v = c.take<float>((size_t)Z * Sp * 4);
    w.lossp = c.take<double>((size_t)Z * (Lp / 128) * 8);
    w.dl = c.take<double>(Mc * 8);
    w.dw = c.take<float>(Mc * 4);
    w.gmax = c.take<unsigned>(256);
    w.bytes = c.o;
    return w;
}

struct Plan : FocalPlan {
    int Meff, dummy;
};
// make_plan with the label set of a call: without ground truth, a weighted batch has the single label (0, 0, 0), which leaves the
// negative term as well (loftr_loss.py:63-70)
inline Plan make_plan_ds(int Z, int L, int S, int M, float alpha, float gamma, float pos_weight, float neg_weight, int no_gt, bool masks) {
    return Plan{make_plan(Z, L, S, M, alpha, gamma, pos_weight, neg_weight, no_gt), no_gt ? (masks ? 1 : 0) : M, no_gt && masks};
}

constexpr size_t SMEM_F = 2 * (2 * PLANE32) + 2 * 96 * sizeof(float);
constexpr size_t SMEM_B = 2 * (2 * PLANE32 + TILE_T) + 2 * 96 * sizeof(float);

inline bool bad_shape(int Z, int L, int S, int Cc, int M) {
    return Z <= 0 || L <= 0 || S <= 0 || Cc != C || M < 0 || (long)Z * (L > S ? L : S) > 0x7ff00000L;
}

}  // namespace

extern "C" {

size_t far_coarse_dense_focal_workspace_bytes(int Z, int L, int S, int Cc, int M) {
    if (bad_shape(Z, L, S, Cc, M)) return 0;
    return carve_d(nullptr, far_k1_fwd_ws_bytes(Z, L, S), Z, L, S, M).bytes;
}

int far_coarse_dense_focal_f16s(const float* f0, const float* f1, int Z, int L, int S, int Cc, float temperature,
                                const uint8_t* mask0, const uint8_t* mask1, const int64_t* pb, const int64_t* pi, const int64_t* pj,
                                int M, float alpha, float gamma, float pos_weight, float neg_weight, int no_gt, float* loss_out,
                                void* ws, int* overflow, hipStream_t stream) {
    far_clear_errors();
    if (!f0 || !f1 || !ws || !loss_out || bad_shape(Z, L, S, Cc, M) || (M > 0 && (!pb || !pi || !pj)) || !(temperature > 0.f)) return FAR_EINVAL;
    const Plan pl = make_plan_ds(Z, L, S, M, alpha, gamma, pos_weight, neg_weight, no_gt, mask0 || mask1);
    int rc = far_k1_stats_launch_masked(f0, f1, Z, L, S, temperature, mask0, mask1, ws, overflow, stream);
    if (rc != FAR_OK) return rc;
    const WsD d = carve_d((unsigned char*)ws, far_k1_fwd_ws_bytes(Z, L, S), Z, L, S, M);
    const int Lp = pad128(L), Sp = pad128(S);
    const _Float16 *ah, *al, *bh, *bl;
    const float2 *rowstat, *colstat;
    far_k1_fwd_planes(ws, Z, L, S, &ah, &al, &bh, &bl, &rowstat, &colstat);
    const float c1 = (float)(1.4426950408889634 / ((double)C * (double)temperature * PRESCALE * PRESCALE));   // log2-domain score per unit dot
    hipLaunchKernelGGL(k1d_side, dim3(gridp((long)Z * Lp)), dim3(256), 0, stream, rowstat, mask0, Z, L, Lp, d.rmax, d.rinv);
    hipLaunchKernelGGL(k1d_side, dim3(gridp((long)Z * Sp)), dim3(256), 0, stream, colstat, mask1, Z, S, Sp, d.cmax, d.cinv);
    hipMemsetAsync(d.gmax, 0, 4, stream);
    if (pl.Meff > 0)
        hipLaunchKernelGGL(k1d_pos, dim3(std::min((pl.Meff + 127) / 128, 2048)), dim3(256), 0, stream, ah, al, bh, bl, Lp, Sp, c1, pb, pi, pj,
                           pl.Meff, pl.dummy, (const float*)d.rmax, (const float*)d.rinv, (const float*)d.cmax, (const float*)d.cinv, pl.fk,
                           pl.cpos, d.dl, d.dw);
    FAR_ONCE_PER_DEVICE(hipFuncSetAttribute((const void*)k1d_pass<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMEM_F));
    const int nparts = (Lp / 128) * Z;
    hipLaunchKernelGGL(k1d_pass<0>, dim3(nparts), dim3(256), SMEM_F, stream, ah, al, bh, bl, (const unsigned char*)nullptr, Z, L, S, Lp, Sp,
                       c1, (const float*)d.rmax, (const float*)d.rinv, (const float*)d.cmax, (const float*)d.cinv, d.u,
                       (const float*)nullptr, pl.fk, d.gmax, d.lossp, (const float*)nullptr, 0.f, (float*)nullptr);
    hipLaunchKernelGGL(k1d_pass<0>, dim3((Sp / 128) * Z), dim3(256), SMEM_F, stream, bh, bl, ah, al, (const unsigned char*)nullptr, Z, S, L, Sp,
                       Lp, c1, (const float*)d.cmax, (const float*)d.cinv, (const float*)d.rmax, (const float*)d.rinv, d.v,
                       (const float*)nullptr, pl.fk, (unsigned*)nullptr, (double*)nullptr, (const float*)nullptr, 0.f, (float*)nullptr);
    hipLaunchKernelGGL(k1d_finish, dim3(gridp((long)Z * (L + S))), dim3(256), 0, stream, pb, pi, pj, pl.Meff, pl.dummy, (const float*)d.dw, Z,
                       L, S, Lp, Sp, d.u, d.v, d.gmax);
    hipLaunchKernelGGL(k1_focal_loss, dim3(1), dim3(256), 0, stream, (const double*)d.lossp, nparts, (const double*)d.dl, pl.Meff,
                       (double)pl.fk.cneg, loss_out);
    return far_check_launch();
}

int far_coarse_dense_focal_bwd_f16(const float* f0, const float* f1, int Z, int L, int S, int Cc, float temperature,
                                   const uint8_t* mask0, const uint8_t* mask1, const int64_t* pb, const int64_t* pi, const int64_t* pj,
                                   int M, float alpha, float gamma, float pos_weight, float neg_weight, int no_gt, const float* gup,
                                   int split_g, float* df0, float* df1, void* ws, hipStream_t stream) {
    far_clear_errors();
    if (!f0 || !f1 || !ws || !gup || !df0 || !df1 || bad_shape(Z, L, S, Cc, M) || (M > 0 && (!pb || !pi || !pj)) || !(temperature > 0.f))
        return FAR_EINVAL;
    const Plan pl = make_plan_ds(Z, L, S, M, alpha, gamma, pos_weight, neg_weight, no_gt, mask0 || mask1);
    const WsD d = carve_d((unsigned char*)ws, far_k1_fwd_ws_bytes(Z, L, S), Z, L, S, M);
    const int Lp = pad128(L), Sp = pad128(S);
    const _Float16 *ah, *al, *bh, *bl;
    const float2 *rowstat, *colstat;
    far_k1_fwd_planes(ws, Z, L, S, &ah, &al, &bh, &bl, &rowstat, &colstat);
    const float c1 = (float)(1.4426950408889634 / ((double)C * (double)temperature * PRESCALE * PRESCALE));
    const float kappa = (float)(1.0 / ((double)C * (double)temperature));
    hipLaunchKernelGGL(k1_prep_t, dim3(gridp((long)Z * (Lp / GT) * C * 4)), dim3(256), 0, stream, f0, Z, L, Lp, (const uint8_t*)nullptr, d.at);
    hipLaunchKernelGGL(k1_prep_t, dim3(gridp((long)Z * (Sp / GT) * C * 4)), dim3(256), 0, stream, f1, Z, S, Sp, (const uint8_t*)nullptr, d.bt);
    FAR_ONCE_PER_DEVICE(
        hipFuncSetAttribute((const void*)k1d_pass<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMEM_B);
        hipFuncSetAttribute((const void*)k1d_pass<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMEM_B));
    auto pass = split_g ? k1d_pass<2> : k1d_pass<1>;
    // dF0: rows = L side (u, row statistics), columns = S side (v, column statistics)
    hipLaunchKernelGGL(pass, dim3((Lp / 128) * Z), dim3(256), SMEM_B, stream, ah, al, bh, bl, (const unsigned char*)d.bt, Z, L, S, Lp, Sp, c1,
                       (const float*)d.rmax, (const float*)d.rinv, (const float*)d.cmax, (const float*)d.cinv, d.u, (const float*)d.v, pl.fk,
                       d.gmax, (double*)nullptr, gup, kappa, df0);
    // dF1: roles swapped
    hipLaunchKernelGGL(pass, dim3((Sp / 128) * Z), dim3(256), SMEM_B, stream, bh, bl, ah, al, (const unsigned char*)d.at, Z, S, L, Sp, Lp, c1,
                       (const float*)d.cmax, (const float*)d.cinv, (const float*)d.rmax, (const float*)d.rinv, d.v, (const float*)d.u, pl.fk,
                       d.gmax, (double*)nullptr, gup, kappa, df1);
    if (pl.Meff > 0)
        hipLaunchKernelGGL(k1d_pos_rows, dim3(std::min((long)((long)Z * (L + S) + 3) / 4, 16384L)), dim3(256), 0, stream, f0, f1, Z, L, S, pb, pi,
                           pj, pl.Meff, pl.dummy, (const float*)d.dw, 2.0f * kappa, gup, df0, df1);
    return far_check_launch();
}

}  // extern "C"

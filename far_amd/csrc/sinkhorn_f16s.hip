// LoFTR's optimal-transport coarse matcher (match_type 'sinkhorn', reference mp3d_loftr/src/loftr/utils/coarse_matching.py:120-142)
// on K1's split-fp16 operands, without the dense (Z, L+1, S+1) coupling matrix.
//
// The operator (SuperGlue's log-domain Sinkhorn with a dustbin row and column; the reference imports it from a superglue.py that
// is not in its tree, so it is defined here):
//   s_ij = <f0_i, f1_j> / C  (-1e9 where not (mask0_i and mask1_j));  Zc = s bordered by the dustbin score alpha (row L, column S)
//   norm = -log(L + S);  log mu = norm (i < L), log S + norm (i = L);  log nu = norm (j < S), log L + norm (j = S)
//   u = v = 0;  T times:  u_i = log mu_i - LSE_j (Zc_ij + v_j),  v_j = log nu_j - LSE_i (Zc_ij + u_i)
//   conf_ij = exp(Zc_ij + u_i + v_j - norm)  (i < L, j < S)
// Everything here is in log2 units (U = u log2 e, V = v log2 e, x_ij = s_ij log2 e).
//   k1_prep            operand planes, as for K1 (k1_f16s.h); the overflow flag means what it means there
//   k_skh_stats<true>  one half-iteration: per row i of (f0, f1) U_i = log mu_i - log2 (sum_j 2^(x_ij + V_j) + 2^(alpha + V_S)) --
//                      K1's statistics tile loop with the column potential added to every score (one FMA replaces K1's multiply);
//                      the column half-iteration is the same kernel on (f1, f0).  The workgroup of row block 0 of each pair also
//                      reduces the OTHER side's potentials (which this launch only reads) to this side's dustbin potential
//                      U_L = log mu_L - alpha - log2 sum_{j <= S} 2^V_j, in a fixed order: one number per pair, read by later launches
//   k_skh_stats<false> max_j (x_ij + V_j) only (the prefilter's row filter after the last column pass)
//   k_skh_match        conf = 2^(x_ij + V_j + (U_i - N)): ONE exp per score; per row the best (conf, j) (ties -> smaller j) and the
//                      column maxima of the entries above thr, as K1's match pass; optional (Z, L+1, S+1) matrix
// then k_finalize / k_compact of dual_softmax_common.h, unchanged.  No float atomics, no data handed between the workgroups of
// one launch: every launch computes the same bits every time.
#include "k1_f16s.h"

namespace {

constexpr float LOG2E = 1.44269504088896341f;
constexpr float LN2 = 0.693147180559945309f;
constexpr float DEAD = -0.5f * HUGE_F;     // below this a log2 term is an empty one (masked, padded, filtered)

// (m, s) <- (m, s) + 2^v in a running maximum / scaled sum; commutative merge below (identical bits in every lane of a butterfly)
__device__ __forceinline__ void lse_add(float& m, float& s, float v) {
    if (v > m) { s = s * __builtin_amdgcn_exp2f(m - v) + 1.0f; m = v; }
    else s += __builtin_amdgcn_exp2f(v - m);
}
__device__ __forceinline__ void lse_merge(float& m, float& s, float mo, float so) {
    const float mn = fmaxf(m, mo);
    s = s * __builtin_amdgcn_exp2f(m - mn) + so * __builtin_amdgcn_exp2f(mo - mn);
    m = mn;
}

// Zero potentials (u = v = 0 before the first half-iteration; padded entries -huge) and zero dustbin potentials.
__global__ void k_skh_init(float* __restrict__ up, int L, int Lp, float* __restrict__ vp, int S, int Sp, float* __restrict__ bins, int Z) {
    const long n = (long)Z * (Lp + Sp);
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
        if (t < (long)Z * Lp) up[t] = (int)(t % Lp) < L ? 0.f : -HUGE_F;
        else { const long q = t - (long)Z * Lp; vp[q] = (int)(q % Sp) < S ? 0.f : -HUGE_F; }
    }
    if (blockIdx.x == 0)
        for (int t = threadIdx.x; t < 2 * Z; t += blockDim.x) bins[t] = 0.f;
}

// One half-iteration over the rows of the (Nr x Nc) score matrix of (a, b) -- or, FULL = false, the row maxima only.
//   cpot [Z][Ncp]  potentials of the columns (padded: -huge), cbin [Z]: the column side's dustbin potential
//   rpot [Z][Nrp]  out (FULL): the rows' new potentials (padded: -huge); rbin [Z] out (FULL): the row side's dustbin potential
//   rmax [Z][Nrp]  out (optional): max_j (x_ij + V_j) over the real columns (masked: -huge)
// lmu / lmu_bin: log2 of the real rows' / the dustbin row's marginal.
template <bool FULL>
__global__ __launch_bounds__(256, 2) void k_skh_stats(const _Float16* __restrict__ ah, const _Float16* __restrict__ al,
                                                      const _Float16* __restrict__ bh, const _Float16* __restrict__ bl,
                                                      int Z, int Nr, int Nc, int Nrp, int Ncp, float c1,
                                                      const uint8_t* __restrict__ rmask, const uint8_t* __restrict__ cmask,
                                                      const float* __restrict__ cpot, const float* __restrict__ cbin,
                                                      const float* __restrict__ bin_score, float lmu, float lmu_bin,
                                                      float* __restrict__ rpot, float* __restrict__ rbin, float* __restrict__ rmax) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    float* const tpot = reinterpret_cast<float*>(lds + 2 * TILE_PLANE);          // this tile's 64 column potentials
    float* const red = tpot + KT;                                                 // [4][2] wave partials of the dustbin reduction
    int z, Ib;
    tile_coords(Nrp / 128, Z, z, Ib);
    const float alpha = bin_score[0] * LOG2E;
    const float cb = cbin[z];
    if (FULL && Ib == 0) {
        // this side's dustbin potential: lmu_bin - alpha - log2 (sum_{j < Nc} 2^cpot_j + 2^cbin); strided per thread, butterfly per
        // wave, the four waves in order: the same order in every launch
        float m = -HUGE_F, s = 0.f;
        for (int k = tid; k < Nc; k += 256) lse_add(m, s, cpot[(size_t)z * Ncp + k]);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) lse_merge(m, s, shfl_xor_f(m, o), shfl_xor_f(s, o));
        if (lane == 0) { red[2 * wave] = m; red[2 * wave + 1] = s; }
        __syncthreads();
        if (tid == 0) {
            float mm = red[0], ss = red[1];
            for (int w = 1; w < 4; ++w) lse_merge(mm, ss, red[2 * w], red[2 * w + 1]);
            lse_merge(mm, ss, cb, 1.0f);
            rbin[z] = lmu_bin - alpha - (mm + __builtin_amdgcn_logf(ss));
        }
    }
    const int irow = Ib * 128 + 32 * wave + l31;
    RowFrags rf;
    rf.load(ah, al, (size_t)z * Nrp + irow, irow, h);
    const bool rmasked = rmask && irow < Nr && !rmask[(size_t)z * Nr + irow];
    float m = -HUGE_F, sum = 0.f, comp = 0.f;
    const int ntile = (Nc + KT - 1) / KT;
    for (int jt = 0; jt < ntile; ++jt) {
        __syncthreads();
        dma_tile(lds, bh, bl, (size_t)z * Ncp + jt * KT, tid, wave);
        if (tid < KT) tpot[tid] = cpot[(size_t)z * Ncp + jt * KT + tid];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        f32x16 acc[2];
        score_tile(acc, lds, rf, l31, h);
        const bool special = (jt + 1) * KT > Nc || cmask != nullptr || rmask != nullptr;      // wave-uniform
        float tm = -HUGE_F;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 pv = *reinterpret_cast<const float4*>(tpot + 32 * ct + 8 * q4 + 4 * h);
                const float p4[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * q4 + e;
                    float x = fmaf(acc[ct][r], c1, p4[e]);
                    if (special) {
                        const int j = jt * KT + 32 * ct + mfma32_row(r, h);
                        if (j >= Nc || rmasked || (cmask && !cmask[(size_t)z * Nc + j])) x = -HUGE_F;
                    }
                    acc[ct][r] = x;
                    tm = fmaxf(tm, x);
                }
            }
        const float mn = fmaxf(m, tm);
        if (FULL) {
            // K1's tile sum + Kahan-compensated running sum (dual_softmax_f16s.hip, k1_rowstats); a row with nothing but empty
            // terms so far keeps sum = 0
            const float resc = __builtin_amdgcn_exp2f(m - mn);
            float t = 0.f;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) t += __builtin_amdgcn_exp2f(acc[ct][r] - mn);
            if (!(mn > DEAD)) t = 0.f;
            sum *= resc;
            comp *= resc;
            const float y = t - comp;
            const float ns = sum + y;
            comp = (ns - sum) - y;
            sum = ns;
        }
        m = mn;
    }
    const float mo = shfl_xor_f(m, 32);
    const float mn = fmaxf(m, mo);
    if (FULL) {
        sum -= comp;
        const float so = shfl_xor_f(sum, 32);
        float st = sum * __builtin_amdgcn_exp2f(m - mn) + so * __builtin_amdgcn_exp2f(mo - mn);
        float M = mn;
        lse_merge(M, st, alpha + cb, 1.0f);                                       // the dustbin column
        if (h == 0) rpot[(size_t)z * Nrp + irow] = irow < Nr ? lmu - (M + __builtin_amdgcn_logf(st)) : -HUGE_F;
    }
    if (rmax && h == 0) rmax[(size_t)z * Nrp + irow] = irow < Nr ? mn : -HUGE_F;
}

// The prefilter's column filter (coarse_matching.py:134-139): column j loses to its dustbin entry when alpha + U_L > max_i (x_ij + U_i).
// vm = V with the filtered columns at -huge: the match pass then gives them conf = 0 without a test per score.
__global__ void k_skh_colfilter(const float* __restrict__ vp, const float* __restrict__ cmax, const float* __restrict__ ubin,
                                const float* __restrict__ bin_score, int Z, int S, int Sp, float* __restrict__ vm) {
    const long n = (long)Z * Sp;
    const float alpha = bin_score[0] * LOG2E;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
        const int z = (int)(t / Sp), j = (int)(t - (long)z * Sp);
        vm[t] = (j < S && !(alpha + ubin[z] > cmax[t])) ? vp[t] : -HUGE_F;
    }
}

// Match pass (K1's k1_match with the Sinkhorn confidence).  vp: the columns' potentials (the prefilter's filtered ones at -huge);
// rmax (prefilter, or null): the row maxima max_j (x_ij + V_j) -- a row whose dustbin entry alpha + V_S beats it keeps conf = 0.
// conf (optional): the (Z, L+1, S+1) matrix, real block only (k_skh_bins writes the dustbin row and column).
template <bool CONF>
__global__ __launch_bounds__(256, 2) void k_skh_match(const _Float16* __restrict__ ah, const _Float16* __restrict__ al,
                                                      const _Float16* __restrict__ bh, const _Float16* __restrict__ bl,
                                                      int Z, int L, int S, int Lp, int Sp, float c1,
                                                      const uint8_t* __restrict__ mask0, const uint8_t* __restrict__ mask1,
                                                      const float* __restrict__ up, const float* __restrict__ vp,
                                                      const float* __restrict__ vbin, const float* __restrict__ rmax,
                                                      const float* __restrict__ bin_score, float nrm, float* __restrict__ conf,
                                                      float* __restrict__ rowbest_v, int* __restrict__ rowbest_j,
                                                      unsigned* __restrict__ colbest, float thr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int nI = Lp / 128;
    int z, Ib;
    tile_coords(nI, Z, z, Ib);
    const int irow = Ib * 128 + 32 * wave + l31;
    const bool ivalid = irow < L;
    RowFrags rf;
    rf.load(ah, al, (size_t)z * Lp + irow, irow, h);
    const float alpha = bin_score[0] * LOG2E;
    float un = up[(size_t)z * Lp + irow] - nrm;                                  // U_i - N (padded rows: -huge)
    if (rmax && !(rmax[(size_t)z * Lp + irow] >= alpha + vbin[z])) un = -HUGE_F;     // row filter: the dustbin wins
    const bool rmasked = mask0 && ivalid && !mask0[(size_t)z * L + irow];
    const bool masks = mask0 != nullptr || mask1 != nullptr;                     // wave-uniform
    float bestv = -1.f;
    int bestj = 0x7fffffff;
    const int ntile = (S + KT - 1) / KT;
    for (int jt = 0; jt < ntile; ++jt) {
        __syncthreads();                       // previous tile's fragments consumed
        dma_tile(lds, bh, bl, (size_t)z * Sp + jt * KT, tid, wave);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        f32x16 acc[2];
        score_tile(acc, lds, rf, l31, h);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 pv = *reinterpret_cast<const float4*>(vp + (size_t)z * Sp + jt * KT + 32 * ct + 8 * q4 + 4 * h);
                const float p4[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * q4 + e;
                    const int j = jt * KT + 32 * ct + mfma32_row(r, h);
                    float p = __builtin_amdgcn_exp2f(fmaf(acc[ct][r], c1, p4[e]) + un);
                    if (masks && j < S && (rmasked || (mask1 && !mask1[(size_t)z * S + j]))) p = 0.f;
                    const bool valid = ivalid && j < S;
                    acc[ct][r] = valid ? p : -1.f;
                    if (valid && p > bestv) { bestv = p; bestj = j; }
                }
            }
            if (CONF && ivalid) {
                float* dst = conf + ((size_t)z * (L + 1) + irow) * (S + 1);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = jt * KT + 32 * ct + mfma32_row(r, h);
                    if (j < S) dst[j] = acc[ct][r];
                }
            }
            // column maxima of the entries above thr (the only ones the mutual-nearest test can need), by atomic max on the bit
            // patterns of positive floats: order-independent, as in K1's match pass
            float tmax = fmaxf(fmaxf(acc[ct][0], acc[ct][1]), fmaxf(acc[ct][2], acc[ct][3]));
#pragma unroll
            for (int r = 4; r < 16; r += 2) tmax = fmaxf(tmax, fmaxf(acc[ct][r], acc[ct][r + 1]));
            if (__builtin_amdgcn_ballot_w64(tmax > thr) != 0ull) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (acc[ct][r] > thr)
                        atomicMax(colbest + (size_t)z * S + jt * KT + 32 * ct + mfma32_row(r, h), __float_as_uint(acc[ct][r]));
            }
        }
    }
    // merge the two half-waves (same rows, interleaved columns): larger value, ties -> smaller j
    const float vo = shfl_xor_f(bestv, 32);
    const int jo = shfl_xor_i(bestj, 32);
    if (vo > bestv || (vo == bestv && jo < bestj)) { bestv = vo; bestj = jo; }
    if (h == 0 && ivalid) {
        rowbest_v[(size_t)z * L + irow] = bestv;
        rowbest_j[(size_t)z * L + irow] = bestj;
    }
}

// The optional outputs that involve a dustbin: log_u (Z, L+1), log_v (Z, S+1) in natural-log units, and the dustbin column / row of
// the (Z, L+1, S+1) matrix (never filtered: the prefilter zeroes conf_matrix = assign[:, :L, :S] only).
__global__ void k_skh_bins(const float* __restrict__ up, const float* __restrict__ vp, const float* __restrict__ bins,
                           const float* __restrict__ bin_score, int Z, int L, int S, int Lp, int Sp, float nrm,
                           float* __restrict__ conf, float* __restrict__ log_u, float* __restrict__ log_v) {
    const int z = blockIdx.y;
    const float alpha = bin_score[0] * LOG2E;
    const float ub = bins[z], vb = bins[Z + z];
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < (L + 1) + (S + 1); t += gridDim.x * blockDim.x) {
        if (t <= L) {
            const float u = t < L ? up[(size_t)z * Lp + t] : ub;
            if (log_u) log_u[(size_t)z * (L + 1) + t] = u * LN2;
            if (conf) conf[((size_t)z * (L + 1) + t) * (S + 1) + S] = __builtin_amdgcn_exp2f(alpha + u + vb - nrm);
        } else {
            const int j = t - (L + 1);
            const float v = j < S ? vp[(size_t)z * Sp + j] : vb;
            if (log_v) log_v[(size_t)z * (S + 1) + j] = v * LN2;
            if (conf && j < S) conf[((size_t)z * (L + 1) + L) * (S + 1) + j] = __builtin_amdgcn_exp2f(alpha + ub + v - nrm);
        }
    }
}

struct WsSkh {
    _Float16 *ah, *al, *bh, *bl;
    float *up, *vp, *vm;         // [Z][Lp], [Z][Sp], [Z][Sp]: U, V, V with the prefilter's columns at -huge
    float *rmax, *cmax;          // [Z][Lp], [Z][Sp]: the prefilter's maxima
    float* bins;                 // [2][Z]: U_L, V_S
    float* rowbest_v; int* rowbest_j; unsigned* colbest; int* match_j; int* counts;
    size_t bytes;
};
inline WsSkh carve_skh(void* ws, int Z, int L, int S) {
    WsSkh w;
    const int Lp = (L + 127) / 128 * 128, Sp = (S + 127) / 128 * 128;
    unsigned char* p = (unsigned char*)ws;
    size_t o = 0;
    auto take = [&](size_t n) { unsigned char* r = p ? p + o : nullptr; o += align256(n); return r; };
    w.ah = (_Float16*)take((size_t)Z * Lp * C * 2); w.al = (_Float16*)take((size_t)Z * Lp * C * 2);
    w.bh = (_Float16*)take((size_t)Z * Sp * C * 2); w.bl = (_Float16*)take((size_t)Z * Sp * C * 2);
    w.up = (float*)take((size_t)Z * Lp * 4); w.vp = (float*)take((size_t)Z * Sp * 4); w.vm = (float*)take((size_t)Z * Sp * 4);
    w.rmax = (float*)take((size_t)Z * Lp * 4); w.cmax = (float*)take((size_t)Z * Sp * 4);
    w.bins = (float*)take((size_t)2 * Z * 4);
    w.rowbest_v = (float*)take((size_t)Z * L * 4); w.rowbest_j = (int*)take((size_t)Z * L * 4);
    w.colbest = (unsigned*)take((size_t)Z * S * 4); w.match_j = (int*)take((size_t)Z * L * 4);
    w.counts = (int*)take((size_t)(Z + 1) * 4);
    w.bytes = o;
    return w;
}

}  // namespace

extern "C" {

size_t far_coarse_match_sinkhorn_f16s_workspace_bytes(int Z, int L, int S, int Cc) {
    if (Z <= 0 || L <= 0 || S <= 0 || Cc != C) return 0;
    return carve_skh(nullptr, Z, L, S).bytes;
}

int far_coarse_match_sinkhorn_f16s(const float* f0, const float* f1, int Z, int L, int S, int Cc,
                                   const float* bin_score, int iters, int prefilter, float thr, int border,
                                   int h0, int w0, int h1, int w1, float cell_scale, const uint8_t* mask0, const uint8_t* mask1,
                                   const int* valid_hw, const float* scale0, const float* scale1,
                                   float* conf_with_bin, float* log_u, float* log_v,
                                   int64_t* b_ids, int64_t* i_ids, int64_t* j_ids, float* mconf,
                                   float* mkpts0_c, float* mkpts1_c, int* counts_out, int* total_out,
                                   void* ws, int* overflow, hipStream_t stream) {
    far_clear_errors();
    if (!f0 || !f1 || !bin_score || !ws || !b_ids || !i_ids || !j_ids || !mconf || !mkpts0_c || !mkpts1_c || !total_out)
        return FAR_EINVAL;
    if (Z <= 0 || L <= 0 || S <= 0 || Cc != C || iters < 0 || h0 * w0 != L || h1 * w1 != S ||
        (long)Z * ((L > S ? L : S) + 128) > 0x7ff00000L)
        return FAR_EINVAL;
    const WsSkh w = carve_skh(ws, Z, L, S);
    const int Lp = (L + 127) / 128 * 128, Sp = (S + 127) / 128 * 128;
    // s = <f0, f1> / C (no temperature) -> log2 domain, operands pre-scaled by 2^4 each
    const float c1 = (float)(1.4426950408889634 / ((double)C * PRESCALE * PRESCALE));
    const double n2 = -std::log2((double)L + (double)S);                          // norm in log2 units
    const float nrm = (float)n2, lmu_l = (float)(std::log2((double)S) + n2), lnu_s = (float)(std::log2((double)L) + n2);
    auto gridp = [](long n) { long b = (n + 255) / 256; return (unsigned)(b < 65536L * 4 ? b : 65536L * 4); };
    hipLaunchKernelGGL(k1_prep, dim3(gridp((long)Z * Lp * 32)), dim3(256), 0, stream, f0, Z, L, Lp, w.ah, w.al, overflow, (unsigned*)nullptr);
    hipLaunchKernelGGL(k1_prep, dim3(gridp((long)Z * Sp * 32)), dim3(256), 0, stream, f1, Z, S, Sp, w.bh, w.bl, overflow, (unsigned*)nullptr);
    hipLaunchKernelGGL(k_skh_init, dim3(gridp((long)Z * (Lp + Sp))), dim3(256), 0, stream, w.up, L, Lp, w.vp, S, Sp, w.bins, Z);
    int* counts = counts_out ? counts_out : w.counts;
    hipMemsetAsync(counts, 0, sizeof(int) * Z, stream);
    const size_t smem_s = 2 * TILE_PLANE + (KT + 8) * sizeof(float), smem_m = 2 * TILE_PLANE;
    FAR_ONCE_PER_DEVICE(
        hipFuncSetAttribute((const void*)k_skh_stats<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_s);
        hipFuncSetAttribute((const void*)k_skh_stats<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_s);
        hipFuncSetAttribute((const void*)k_skh_match<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_m);
        hipFuncSetAttribute((const void*)k_skh_match<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_m));
    float* const ubin = w.bins;
    float* const vbin = w.bins + Z;
    auto row_pass = [&](bool full, float* rmax) {       // (f0, f1): U from V
        hipLaunchKernelGGL(full ? k_skh_stats<true> : k_skh_stats<false>, dim3((Lp / 128) * Z), dim3(256), smem_s, stream,
                           w.ah, w.al, w.bh, w.bl, Z, L, S, Lp, Sp, c1, mask0, mask1, (const float*)w.vp, (const float*)vbin, bin_score,
                           nrm, lmu_l, w.up, ubin, rmax);
    };
    auto col_pass = [&](bool full, float* rmax) {       // (f1, f0): V from U
        hipLaunchKernelGGL(full ? k_skh_stats<true> : k_skh_stats<false>, dim3((Sp / 128) * Z), dim3(256), smem_s, stream,
                           w.bh, w.bl, w.ah, w.al, Z, S, L, Sp, Lp, c1, mask1, mask0, (const float*)w.up, (const float*)ubin, bin_score,
                           nrm, lnu_s, w.vp, vbin, rmax);
    };
    for (int t = 0; t < iters; ++t) {
        row_pass(true, nullptr);
        col_pass(true, prefilter && t == iters - 1 ? w.cmax : nullptr);       // the last column pass leaves the column maxima
    }
    if (prefilter) {
        if (iters == 0) col_pass(false, w.cmax);
        row_pass(false, w.rmax);                                             // row maxima under the final V
        hipLaunchKernelGGL(k_skh_colfilter, dim3(gridp((long)Z * Sp)), dim3(256), 0, stream, (const float*)w.vp, (const float*)w.cmax,
                           (const float*)ubin, bin_score, Z, S, Sp, w.vm);
    }
    const float* vmatch = prefilter ? w.vm : w.vp;
    const float* rfilt = prefilter ? w.rmax : nullptr;
    const int nI = Lp / 128;
    hipMemsetAsync(w.colbest, 0, sizeof(unsigned) * (size_t)Z * S, stream);      // the atomic column maxima start at 0
    if (conf_with_bin)
        hipLaunchKernelGGL(k_skh_match<true>, dim3(nI * Z), dim3(256), smem_m, stream, w.ah, w.al, w.bh, w.bl, Z, L, S, Lp, Sp, c1,
                           mask0, mask1, (const float*)w.up, vmatch, (const float*)vbin, rfilt, bin_score, nrm, conf_with_bin,
                           w.rowbest_v, w.rowbest_j, w.colbest, thr);
    else
        hipLaunchKernelGGL(k_skh_match<false>, dim3(nI * Z), dim3(256), smem_m, stream, w.ah, w.al, w.bh, w.bl, Z, L, S, Lp, Sp, c1,
                           mask0, mask1, (const float*)w.up, vmatch, (const float*)vbin, rfilt, bin_score, nrm, conf_with_bin,
                           w.rowbest_v, w.rowbest_j, w.colbest, thr);
    if (conf_with_bin || log_u || log_v)
        hipLaunchKernelGGL(k_skh_bins, dim3((L + S + 2 + 255) / 256, Z), dim3(256), 0, stream, (const float*)w.up, (const float*)w.vp,
                           (const float*)w.bins, bin_score, Z, L, S, Lp, Sp, nrm, conf_with_bin, log_u, log_v);
    hipLaunchKernelGGL(k_finalize, dim3((L + 255) / 256, Z), dim3(256), 0, stream, w.rowbest_v, w.rowbest_j,
                       reinterpret_cast<const float*>(w.colbest), 1, L, S, thr, border, h0, w0, h1, w1, valid_hw, w.match_j, counts);
    hipLaunchKernelGGL(k_compact, dim3(Z), dim3(256), 0, stream, w.match_j, w.rowbest_v, counts, L, w0, w1,
                       cell_scale, scale0, scale1, b_ids, i_ids, j_ids, mconf, mkpts0_c, mkpts1_c, total_out);
    return far_check_launch();
}

}  // extern "C"

// ---- glue with sinkhorn_train_f16s.hip (declared in k1_f16s.h): it lives here because it launches this file's k_skh_stats, so that
// the training forward runs the very kernels of inference ----
int far_skh_history_launch(const float* f0, const float* f1, int Z, int L, int S, const float* bin_score, int iters,
                           const uint8_t* mask0, const uint8_t* mask1, _Float16* ah, _Float16* al, _Float16* bh, _Float16* bl,
                           float* uh, float* vh, float* binh, int* overflow, hipStream_t stream) {
    const int Lp = (L + 127) / 128 * 128, Sp = (S + 127) / 128 * 128;
    const float c1 = (float)(1.4426950408889634 / ((double)C * PRESCALE * PRESCALE));
    const double n2 = -std::log2((double)L + (double)S);
    const float nrm = (float)n2, lmu_l = (float)(std::log2((double)S) + n2), lnu_s = (float)(std::log2((double)L) + n2);
    auto gridp = [](long n) { long b = (n + 255) / 256; return (unsigned)(b < 65536L * 4 ? b : 65536L * 4); };
    hipLaunchKernelGGL(k1_prep, dim3(gridp((long)Z * Lp * 32)), dim3(256), 0, stream, f0, Z, L, Lp, ah, al, overflow, (unsigned*)nullptr);
    hipLaunchKernelGGL(k1_prep, dim3(gridp((long)Z * Sp * 32)), dim3(256), 0, stream, f1, Z, S, Sp, bh, bl, overflow, (unsigned*)nullptr);
    hipLaunchKernelGGL(k_skh_init, dim3(gridp((long)Z * (Lp + Sp))), dim3(256), 0, stream, uh, L, Lp, vh, S, Sp, binh, Z);
    const size_t smem_s = 2 * TILE_PLANE + (KT + 8) * sizeof(float);
    FAR_ONCE_PER_DEVICE(hipFuncSetAttribute((const void*)k_skh_stats<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_s));
    const size_t nu = (size_t)Z * Lp, nv = (size_t)Z * Sp;
    for (int t = 1; t <= iters; ++t) {
        float* const bt = binh + (size_t)t * 2 * Z;
        const float* const bp = binh + (size_t)(t - 1) * 2 * Z;
        hipLaunchKernelGGL(k_skh_stats<true>, dim3((Lp / 128) * Z), dim3(256), smem_s, stream, ah, al, bh, bl, Z, L, S, Lp, Sp, c1,
                           mask0, mask1, (const float*)(vh + (t - 1) * nv), bp + Z, bin_score, nrm, lmu_l, uh + t * nu, bt,
                           (float*)nullptr);
        hipLaunchKernelGGL(k_skh_stats<true>, dim3((Sp / 128) * Z), dim3(256), smem_s, stream, bh, bl, ah, al, Z, S, L, Sp, Lp, c1,
                           mask1, mask0, (const float*)(uh + t * nu), (const float*)bt, bin_score, nrm, lnu_s, vh + t * nv, bt + Z,
                           (float*)nullptr);
    }
    return far_check_launch();
}

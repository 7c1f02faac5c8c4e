// K24's tile loop, once for the forward (conv_valid_f16s.hip) and the input gradient (conv_valid_bwd_f16s.hip): the zeroed accumulator
// pairs, the B-fragment fetch, the patch staging, the MFMA step, the tap walk with its one-k-step-ahead prefetch, the merge and the
// non-finite guard.  Included INTO the body of a kernel of NTHR threads (conv_valid_f16s.h describes the scheme), which has defined
//   constexpr int MT, NTW, PAD   M-tiles (4 x 8 pixels) and 32-channel N-tiles per wave; patch pixel (py, px) of the workgroup is
//                                src[oy0 + py - PAD][ox0 + px - PAD] (forward 0; dgrad KS - 1, and the lower bound is checked)
//   tid, lane, l31, h, mh        threadIdx.x, tid & 63, lane & 31, lane >> 5, the wave's half of the tile's rows
//   oy0, ox0                     the tile's origin
//   src, src_rows, src_cols, src_C, src_scale   image n of the operand [rows][cols][C] fp32, multiplied by src_scale before the split
//   wimg, NT, nt0, nchunks       the packed image, its N-tile count, this wave's first N-tile, the 32-channel chunks of the reduction
//   out_rows                     rows of the result: a wave whose rows lie below it, or without an N-tile, is not `live` and stages its
//                                share of the patch only
//   overflow                     int* or NULL: OR-ed with 1 when a sum is not finite
// and leaves f32x16 acc[MT][NTW], the sums of the wave's tiles; a wave that is not live has returned.
// A fragment and no __device__ function: hipcc optimises a callee on its own before it inlines it, and what it then knows about the
// arguments changes the staging code around the tap loop; k_conv_valid<3> fills the register file (a few more live registers make
// its accumulators spill), one accumulator tile moves between the two register files in every k-step, and with the loop in a function
// those moves came out in runs of 16 in front of their MFMA instead of between the MFMAs: 5 % on the forward at 64 images
// (profiles/k24_shared_recipe_ab.txt).  As text in the kernel, with the names bound as the two kernels bind them, both compile to the
// instructions they had when each held its own copy of the loop.  It is macro-like code: it declares the kernel's __shared__ planes and
// holds a `return`; keep the order of its statements (`live` behind the accumulators), the generated code follows it.
    constexpr int PH = 8 * MT + KS - 1;
    constexpr int NITEMS = PH * PW * 8;                 // float4 loads per chunk (MT = 3: 2688)
    constexpr int ITEMS = (NITEMS + NTHR - 1) / NTHR;   // per thread (11, the last round half full)
    __shared__ __attribute__((aligned(16))) _Float16 hi[PH * PW * PSTR];
    __shared__ __attribute__((aligned(16))) _Float16 lo[PH * PW * PSTR];

    // Two accumulators per tile: the hi.hi products, and the two cross terms (2^-11 of them).  Kept apart, the large sum is rounded
    // once per k-step instead of three times (its rounding is the kernel's whole deviation from an fp32 convolution: the operands carry
    // 22 bits), and the two MFMA chains are independent.
    f32x16 acc[MT][NTW], accs[MT][NTW];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = accs[mt][nt][r] = 0.f;

    // wave-uniform: this wave's 4 MT rows hold a row of the result and its N-tiles exist
    const bool live = oy0 + 4 * MT * mh < out_rows && nt0 < NT;
    const int abase = ((4 * MT * mh + (l31 >> 3)) * PW + (l31 & 7)) * PSTR + 8 * h;
    const f32x2 s2 = {src_scale, src_scale};

    // the B fragments of k-step j (tap j / 2, channels 16 (j & 1) ..) of chunk c, requested one k-step ahead of their MFMAs
    f16x8 bh[2][NTW], bl[2][NTW];
    auto fetch = [&](int c, int j, int slot) {
        const _Float16* wt = wimg + ((size_t)(c * STEPS + j) * NT + nt0) * 1024 + lane * 8;
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
            if (nt0 + nt < NT) {                                   // wave-uniform
                bh[slot][nt] = *reinterpret_cast<const f16x8*>(wt + nt * 1024);
                bl[slot][nt] = *reinterpret_cast<const f16x8*>(wt + nt * 1024 + 512);
            }
    };

    for (int c = 0; c < nchunks; ++c) {
        if (live) fetch(c, 0, 0);                                  // in flight under the staging below
        __syncthreads();                                           // the previous chunk's planes are consumed
        {
            // one global round trip per chunk, not hidden: ~2 us against the ~20 us of the chunk's 1350 MFMAs per wave -- keeping the next
            // chunk's 44 registers alive through the MFMA loop instead made the accumulators spill
            float4 v[ITEMS];
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) {
                const int i = tid + NTHR * j, pix = i >> 3, q = i & 7;
                const int py = pix / PW, px = pix - py * PW;
                const int y = oy0 + py - PAD, x = ox0 + px - PAD;    // PAD > 0: the border, outside the image is zero
                v[j] = (i < NITEMS && (PAD == 0 || y >= 0) && y < src_rows && (PAD == 0 || x >= 0) && x < src_cols)
                           ? *reinterpret_cast<const float4*>(src + ((size_t)y * src_cols + x) * src_C + 32 * c + 4 * q)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) {
                const int i = tid + NTHR * j, pix = i >> 3, q = i & 7;
                f16x2 h0, l0, h1, l1;
                split2(f32x2{v[j].x, v[j].y} * s2, h0, l0);
                split2(f32x2{v[j].z, v[j].w} * s2, h1, l1);
                if (i < NITEMS) {
                    *reinterpret_cast<f16x4*>(hi + pix * PSTR + 4 * q) = f16x4{h0.x, h0.y, h1.x, h1.y};
                    *reinterpret_cast<f16x4*>(lo + pix * PSTR + 4 * q) = f16x4{l0.x, l0.y, l1.x, l1.y};
                }
            }
        }
        __syncthreads();
        if (!live) continue;
        auto step = [&](int off, int cur) {
            f16x8 ah[MT], al[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                ah[mt] = *reinterpret_cast<const f16x8*>(hi + off + 4 * mt * PW * PSTR);
                al[mt] = *reinterpret_cast<const f16x8*>(lo + off + 4 * mt * PW * PSTR);
            }
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                if (nt0 + nt < NT) {
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mt], bh[cur][nt], acc[mt][nt], 0, 0, 0);
                        accs[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mt], bl[cur][nt], accs[mt][nt], 0, 0, 0);
                        accs[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[mt], bh[cur][nt], accs[mt][nt], 0, 0, 0);
                    }
                }
            }
        };
#pragma unroll 1
        for (int dy = 0; dy < KS; ++dy) {
#pragma unroll 1
            for (int dx = 0; dx < KS; ++dx) {
                const int tap = dy * KS + dx, off = abase + (dy * PW + dx) * PSTR;
                fetch(c, 2 * tap + 1, 1);
                step(off, 0);                                      // channels 0 .. 15 of the chunk
                if (tap + 1 < TAPS) fetch(c, 2 * tap + 2, 0);
                step(off + 16, 1);                                 // channels 16 .. 31
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] += accs[mt][nt];

    // Range guard (as K9): an input beyond the split's range (|a| scale > 65504) or a non-finite one reaches the accumulators as inf /
    // NaN, and the sum of a wave's accumulators is not finite exactly then; one integer atomic per wave that saw it, none otherwise.
    if (overflow) {
        float chk = 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) chk += acc[mt][nt][r];
        if (__any(!(fabsf(chk) <= FLT_MAX)) && lane == 0) atomicOr(overflow, 1);
    }

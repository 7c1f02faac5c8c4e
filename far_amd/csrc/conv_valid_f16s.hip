// K24: K x K unpadded ('valid') stride-1 convolution, K = 5, NHWC fp32 in and out, on the f16 matrix cores with split-precision
// operands (hi.hi + hi.lo + lo.hi, fp32 accumulation: K9's recipe), with K9's epilogue: acc * scale + shift (+ residual), ReLU.
//
// Replaces interiornetStreetlearn_8ptVit/src/modules/extractor.py:11 (conv2, 192 -> 192) and :46-47 (downsample.0, 128 -> 192) of the
// ResidualBlock model.py:60 builds with kernel_size 5: 28 x 28 -> 24 x 24, half of the extractor's arithmetic.
//
// An implicit GEMM, M = output pixels, N = Cout, K = 25 taps x Cin.  One workgroup = 4 waves = one 24 x 8 output tile x 192 output
// channels; a wave owns 12 rows (three 4 x 8 M-tiles) x three 32-channel N-tiles: 24 x 24 outputs are three workgroups, none idle.
// (Small launches take an 8-row form of the same kernel, see k_conv_valid.)  Per 32-channel chunk of the input the 28 x 12 patch is
// scaled by 2^act_exp, split once into fp16 hi / lo planes in LDS (80 B per pixel and plane: the 16-byte fragment reads of eight
// neighbouring pixels fall into distinct banks) and the 25 taps walk over it: an A fragment is a shifted 16-byte read, no im2col.
// The B fragments come pre-split from the packed image [chunk][tap][k-step][N-tile][plane][lane][8] in 1 KB coalesced reads
// (every workgroup reads the same image: L2 resident), requested one k-step (27 MFMAs) ahead of their use.  The sum of an output runs over (chunk, tap, k-step) in that order whatever the batch: run-to-run and batch-to-batch the
// same bits; no atomics on floats.
#include "common.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr int KS = 5, TAPS = KS * KS;
constexpr int TW = 8, PW = TW + KS - 1;                 // output tile width of a workgroup; input patch width 12
constexpr int PSTR = 40;                                // fp16 per patch pixel and plane: 32 channels + 8 of padding
constexpr int NTW = 3;                                  // 32-channel N-tiles per wave
constexpr int NTHR = 256;
constexpr int SMALL_GRID = 128;                         // fewer 24-row workgroups than this: the 8-row form (MT = 1) fills more CUs
constexpr int STEPS = TAPS * 2;                         // k-steps of 16 channels per chunk
constexpr int ACT_EXP_DEFAULT = 4;

struct ValidArgs {
    const float* x;
    const _Float16* w;
    const float* scale;
    const float* shift;
    const float* res;
    float* y;
    int H, W, Ho, Wo, Cin, Cout, tilesX, tilesY, act;
    float act_scale, out_mul;
    int* overflow;
};

// MT: 4 x 8-pixel M-tiles per wave; the workgroup's tile is 8 MT output rows x 8 columns (MT = 3: 24 rows, the workload's whole
// height; MT = 1: 8 rows, nine workgroups per 24 x 24 image, for launches that would leave most CUs idle).  An output's sum is the
// same sequence of MFMAs in both forms: the same bits.
template <int MT>
__global__ __launch_bounds__(NTHR) void k_conv_valid(const ValidArgs p) {
    constexpr int TH = 8 * MT, PH = TH + KS - 1;
    constexpr int NITEMS = PH * PW * 8;                 // float4 loads per chunk (MT = 3: 2688)
    constexpr int ITEMS = (NITEMS + NTHR - 1) / NTHR;   // per thread (11, the last round half full)
    __shared__ __attribute__((aligned(16))) _Float16 hi[PH * PW * PSTR];
    __shared__ __attribute__((aligned(16))) _Float16 lo[PH * PW * PSTR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int mh = wave & 1, nh = wave >> 1;                       // this wave's half of the rows / of the workgroup's six N-tiles
    int t = blockIdx.x;
    const int tx = t % p.tilesX;
    t /= p.tilesX;
    const int ty = t % p.tilesY, n = t / p.tilesY;
    const int oy0 = ty * TH, ox0 = tx * TW;
    const int NT = p.Cout >> 5, nt0 = (blockIdx.y * 2 + nh) * NTW, nchunks = p.Cin >> 5;
    const float* xin = p.x + (size_t)n * p.H * p.W * p.Cin;

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

    // wave-uniform: this wave's twelve rows hold an output row and its N-tiles exist (Cout = 192: always)
    const bool live = oy0 + 4 * MT * mh < p.Ho && nt0 < NT;
    const int abase = ((4 * MT * mh + (l31 >> 3)) * PW + (l31 & 7)) * PSTR + 8 * h;
    const f32x2 as2 = {p.act_scale, p.act_scale};

    // the B fragments of k-step j (tap j / 2, channels 16 (j & 1) ..) of chunk c, requested one k-step ahead of their MFMAs
    f16x8 bh[2][NTW], bl[2][NTW];
    auto fetch = [&](int c, int j, int slot) {
        const _Float16* wt = p.w + ((size_t)(c * STEPS + j) * NT + nt0) * 1024 + lane * 8;
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
                const int iy = oy0 + py, ix = ox0 + px;
                v[j] = (i < NITEMS && iy < p.H && ix < p.W) ? *reinterpret_cast<const float4*>(xin + ((size_t)iy * p.W + ix) * p.Cin + 32 * c + 4 * q)
                                                            : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) {
                const int i = tid + NTHR * j, pix = i >> 3, q = i & 7;
                f16x2 h0, l0, h1, l1;
                split2(f32x2{v[j].x, v[j].y} * as2, h0, l0);
                split2(f32x2{v[j].z, v[j].w} * as2, h1, l1);
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

    // Activation-range guard (as K9): an input beyond the split's range (|a| 2^act_exp > 65504) reaches the accumulators as inf / NaN,
    // and the sum of a wave's accumulators is not finite exactly then; one integer atomic per wave that saw it, none otherwise.
    if (p.overflow) {
        float chk = 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) chk += acc[mt][nt][r];
        if (__any(!(fabsf(chk) <= FLT_MAX)) && lane == 0) atomicOr(p.overflow, 1);
    }

#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        if (nt0 + nt >= NT) continue;
        const int co = 32 * (nt0 + nt) + l31;
        const float sc = p.scale[co] * p.out_mul, sh = p.shift ? p.shift[co] : 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mfma32_row(r, h);
                const int oy = oy0 + 4 * MT * mh + 4 * mt + (m >> 3), ox = ox0 + (m & 7);
                if (oy < p.Ho && ox < p.Wo) {
                    const size_t o = (((size_t)n * p.Ho + oy) * p.Wo + ox) * p.Cout + co;
                    float v = acc[mt][nt][r] * sc + sh;
                    if (p.res) v += p.res[o];
                    if (p.act == 1) v = v < 0.f ? 0.f : v;          // a ReLU that keeps NaN (as K10: a non-finite input stays loud)
                    p.y[o] = v;
                }
            }
        }
    }
}

// The packed image: item (chunk c, tap t, k-step s, N-tile nt, lane): the eight input channels 32 c + 16 s + 8 (lane >> 5) + e of
// output channel 32 nt + (lane & 31) at tap t, times pack_scale[0], as a hi and a lo fp16 plane of 512 values each.
__global__ __launch_bounds__(256) void k_valid_pack(const float* __restrict__ w, int Cin, int Cout, const float* __restrict__ pack_scale,
                                                    _Float16* __restrict__ packed, const float* __restrict__ base_scale,
                                                    float* __restrict__ scale_vec) {
    const int NT = Cout >> 5;
    const long items = (long)(Cin >> 5) * TAPS * 2 * NT * 64;
    const float wmul = pack_scale[0];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        const int ln = (int)(i & 63);
        long u = i >> 6;
        const int nt = (int)(u % NT);
        u /= NT;
        const int s = (int)(u & 1);
        u >>= 1;
        const int t = (int)(u % TAPS), c = (int)(u / TAPS);
        const int co = 32 * nt + (ln & 31);
        f16x8 vh, vl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ci = 32 * c + 16 * s + 8 * (ln >> 5) + e;
            const float v = w[((size_t)co * Cin + ci) * TAPS + t] * wmul;
            const _Float16 hh = (_Float16)v;
            vh[e] = hh;
            vl[e] = (_Float16)(v - (float)hh);
        }
        _Float16* dst = packed + (size_t)(i >> 6) * 1024 + ln * 8;
        *reinterpret_cast<f16x8*>(dst) = vh;
        *reinterpret_cast<f16x8*>(dst + 512) = vl;
    }
    if (scale_vec)
        for (int co = blockIdx.x * 256 + threadIdx.x; co < Cout; co += gridDim.x * 256)
            scale_vec[co] = (base_scale ? base_scale[co] : 1.0f) * pack_scale[1];
}

bool valid_shape(int Cin, int Cout, int ksize) {
    return ksize == KS && Cin > 0 && Cout > 0 && (Cin & 31) == 0 && (Cout & 31) == 0;
}

}  // namespace

extern "C" {

// Bytes of the packed split-fp16 image of a (Cout, Cin, 5, 5) weight; 0 for a shape K24 does not cover (ksize != 5, Cin or Cout not a
// multiple of 32).
size_t far_conv_valid_packed_bytes(int Cin, int Cout, int ksize) {
    if (!valid_shape(Cin, Cout, ksize)) return 0;
    return (size_t)Cin * Cout * TAPS * 2 * sizeof(_Float16);
}

// Packs w [Cout][Cin][5][5] (torch layout, contiguous) times pack_scale[0] (far_weight_scale_f32's two device floats { 2^w_exp,
// 2^-(w_exp + 4) }) and writes the launch's epilogue scale vector scale_vec[co] = base_scale[co] (1 when NULL) * pack_scale[1].
int far_conv_valid_pack_f32(const float* w, int Cin, int Cout, int ksize, const float* pack_scale, void* packed, const float* base_scale,
                            float* scale_vec, hipStream_t stream) {
    far_clear_errors();
    if (!w || !pack_scale || !packed || !scale_vec || !valid_shape(Cin, Cout, ksize)) return FAR_EINVAL;
    const long items = (long)(Cin >> 5) * TAPS * 2 * (Cout >> 5) * 64;
    long blocks = (items + 255) / 256;
    blocks = blocks > 1024 ? 1024 : blocks;
    hipLaunchKernelGGL(k_valid_pack, dim3((unsigned)blocks), dim3(256), 0, stream, w, Cin, Cout, pack_scale, (_Float16*)packed, base_scale,
                       scale_vec);
    return far_check_launch();
}

// y[n][oy][ox][co] = act(scale[co] 2^(4 - act_exp) sum_{ky, kx, ci} x[n][oy + ky][ox + kx][ci] W[co][ci][ky][kx] + shift[co] (+ res))
// x [N][H][W][Cin], res / y [N][H - 4][W - 4][Cout], fp32 NHWC contiguous, 16-byte aligned; H, W >= 5; Cin, Cout multiples of 32;
// `scale` includes 2^-(w_exp + 4) (far_conv_valid_pack_f32 writes it), shift may be NULL; act: 0 none, 1 ReLU.  act_exp and overflow
// as far_conv_nhwc_f32: activations are split around 2^act_exp, the device int is OR-ed with 1 when an input left the split's range.
// y must alias neither x nor res.
int far_conv_valid_f16s(const float* x, const void* packed, const float* scale, const float* shift, const float* res, float* y, long N,
                        int H, int W, int Cin, int Cout, int ksize, int act, int act_exp, int* overflow, hipStream_t stream) {
    far_clear_errors();
    if (act_exp < -24 || act_exp > 8 || act < 0 || act > 1 || N < 0) return FAR_EINVAL;
    if (!valid_shape(Cin, Cout, ksize) || H < KS || W < KS) return FAR_EINVAL;
    if (N == 0) return FAR_OK;
    if (!x || !packed || !scale || !y || x == y || (res && res == y) || (reinterpret_cast<uintptr_t>(x) & 15)) return FAR_EINVAL;
    ValidArgs a;
    a.x = x; a.w = (const _Float16*)packed; a.scale = scale; a.shift = shift; a.res = res; a.y = y;
    a.H = H; a.W = W; a.Ho = H - KS + 1; a.Wo = W - KS + 1; a.Cin = Cin; a.Cout = Cout;
    a.tilesX = (a.Wo + TW - 1) / TW; a.tilesY = (a.Ho + 23) / 24; a.act = act;
    a.act_scale = ldexpf(1.0f, act_exp); a.out_mul = ldexpf(1.0f, ACT_EXP_DEFAULT - act_exp); a.overflow = overflow;
    long nbx = N * a.tilesX * a.tilesY;
    const bool small = nbx < SMALL_GRID;
    if (small) { a.tilesY = (a.Ho + 7) / 8; nbx = N * a.tilesX * a.tilesY; }
    const int nby = ((Cout >> 5) + 2 * NTW - 1) / (2 * NTW);
    if (nbx > 0x7fffffffL || nby > 65535) return FAR_EINVAL;
    if (small) hipLaunchKernelGGL(k_conv_valid<1>, dim3((unsigned)nbx, (unsigned)nby), dim3(NTHR), 0, stream, a);
    else hipLaunchKernelGGL(k_conv_valid<3>, dim3((unsigned)nbx, (unsigned)nby), dim3(NTHR), 0, stream, a);
    return far_check_launch();
}

}  // extern "C"

// K24: K x K unpadded ('valid') stride-1 convolution, K = 5, NHWC fp32 in and out, on the f16 matrix cores with split-precision
// operands (hi.hi + hi.lo + lo.hi, fp32 accumulation: K9's recipe), with K9's epilogue: acc * scale + shift (+ residual), ReLU.
//
// Replaces interiornetStreetlearn_8ptVit/src/modules/extractor.py:11 (conv2, 192 -> 192) and :46-47 (downsample.0, 128 -> 192) of the
// ResidualBlock model.py:60 builds with kernel_size 5: 28 x 28 -> 24 x 24, half of the extractor's arithmetic.
//
// An implicit GEMM, M = output pixels, N = Cout, K = 25 taps x Cin.  One workgroup = 4 waves = one 24 x 8 output tile x 192 output
// channels; a wave owns 12 rows (three 4 x 8 M-tiles) x three 32-channel N-tiles: 24 x 24 outputs are three workgroups, none idle.
// (Small launches take an 8-row form of the same kernel, see k_conv_valid.)  The tile loop (conv_valid_tile.inc: patch staging, the tap
// walk over the pre-split weight image, the order of an output's sum, the range guard) and the pack kernel (conv_valid_f16s.h) are
// shared with the input gradient; this file holds the launch geometry, the patch's origin (x itself, no border) and the epilogue.
#include "conv_valid_f16s.h"

namespace {

constexpr int NTW = 3;                                  // 32-channel N-tiles per wave
constexpr int SMALL_GRID = 128;                         // fewer 24-row workgroups than this: the 8-row form (MT = 1) fills more CUs
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
    constexpr int TH = 8 * MT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int mh = wave & 1, nh = wave >> 1;                       // this wave's half of the rows / of the workgroup's six N-tiles
    int t = blockIdx.x;
    const int tx = t % p.tilesX;
    t /= p.tilesX;
    const int ty = t % p.tilesY, n = t / p.tilesY;
    const int oy0 = ty * TH, ox0 = tx * TW;
    const int NT = p.Cout >> 5, nt0 = (blockIdx.y * 2 + nh) * NTW, nchunks = p.Cin >> 5;
    // The fragment's names.  The references exist only to steer code generation: each field is then read where the loop uses it, as
    // when the loop stood here, and the kernel compiles to the same instructions as then.  Plain copies, or another order of these
    // lines, change the generated code (conv_valid_tile.inc).
    constexpr int PAD = 0;                                         // the patch is x itself
    const float* const src = p.x + (size_t)n * p.H * p.W * p.Cin;
    const int &src_rows = p.H, &src_cols = p.W, &src_C = p.Cin;
    const float& src_scale = p.act_scale;
    const _Float16* const& wimg = p.w;
    int* const& overflow = p.overflow;
    const int& out_rows = p.Ho;                                    // (Cout = 192: every wave has its N-tiles)
#include "conv_valid_tile.inc"

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
    valid_pack<false>(w, Cin, Cout, pack_scale, packed, base_scale, scale_vec, stream);
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

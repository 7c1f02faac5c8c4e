// K24 backward: input gradient and weight gradient of the 5 x 5 unpadded ('valid') stride-1 convolution of conv_valid_f16s.hip, NHWC fp32,
// split-fp16 operands (hi.hi + hi.lo + lo.hi, fp32 accumulation) on the matrix cores.
//
// Replaces autograd's backward of interiornetStreetlearn_8ptVit/src/modules/extractor.py:11 (conv2, 192 -> 192) and :46-47 (downsample.0,
// 128 -> 192) of the ResidualBlock model.py:60 builds with kernel_size 5, which train.py fine-tunes with the trunk.
//
// dgrad  dx[n][iy][ix][ci] = sum_{ky, kx, co} dy[n][iy - ky][ix - kx][co] w[co][ci][ky][kx]  (terms outside dy are zero): the 'full'
//   correlation of dy with the flipped, channel-transposed kernel.  K24's tile loop (conv_valid_tile.inc) and pack kernel
//   (conv_valid_f16s.h) on the dgrad form of the weight image; the patch load knows the border: pixel (py, px) of a workgroup's patch
//   is dy[oy0 + py - 4][ox0 + px - 4] or zero, no padded copy of dy exists.  dy is multiplied by far_grad_scale_f32's device power of
//   two before the split, the epilogue takes it out again.
//   One form for every launch size: a 16 x 8 tile of dx per workgroup, a wave owns 8 rows x two or three 32-channel N-tiles.  The sum
//   of an element runs over (chunk, tap, k-step) in that order whatever N is.
// wgrad  dw[co][ci][ky][kx] = sum_{n, oy, ox} dy[n][oy][ox][co] x[n][oy + ky][ox + kx][ci]: a GEMM whose reduction runs over pixels, so
//   an MFMA operand is 8 consecutive pixels of ONE channel.  A workgroup (five waves, one per kernel row ky) owns 64 co x 32 ci x 25 taps
//   and walks 16-pixel-wide column strips downwards: every x row is read from memory once, scaled, split and written TRANSPOSED
//   ([channel][pixel], 48 B per channel: conflict-free 16-byte reads) into a ring of eight rows in LDS; wave ky reads row oy + ky of the
//   ring, and the five kx-shifted operands are cut from one 16-pixel fragment in registers.  The (image, strip, row) sequence is cut
//   into ranges, each range writes its partial dw to a workspace slab, K16's reduction (wgrad_reduce.h) adds the slabs in index order:
//   deterministic, no atomics on floats (K16's contract).
#include "conv_valid_f16s.h"
#include "wgrad_reduce.h"

extern "C" int far_grad_scale_f32(const float* x, long n, float* out2, hipStream_t stream);

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------------------------ dgrad

constexpr int MTD = 2;                                  // 4 x 8-pixel M-tiles per wave: a 16 x 8 tile of dx per workgroup

struct DgradArgs {
    const float* dy;         // [N][Ho][Wo][Cout]
    const _Float16* w;       // k_valid_pack<true>'s image
    const float* sg_dev;     // { 2^e, 2^(4 - e) }: dy is multiplied by [0] before the split
    const float* pack_scale; // { 2^w_exp, 2^-(w_exp + 4) } of the image
    float* dx;               // [N][H][W][Cin]
    int H, W, Ho, Wo, Cin, Cout, tilesX, tilesY;
    int* overflow;
};

// NTW: 32-channel N-tiles (of Cin) per wave; the workgroup covers 2 NTW of them per blockIdx.y.
template <int NTW>
__global__ __launch_bounds__(NTHR) void k_valid_dgrad(const DgradArgs p) {
    constexpr int MT = MTD, TH = 8 * MT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int mh = wave & 1, nh = wave >> 1;
    int t = blockIdx.x;
    const int tx = t % p.tilesX;
    t /= p.tilesX;
    const int ty = t % p.tilesY, n = t / p.tilesY;
    const int oy0 = ty * TH, ox0 = tx * TW;                        // of dx; the patch starts at dy[oy0 - 4][ox0 - 4]
    const int NT = p.Cin >> 5, nt0 = (blockIdx.y * 2 + nh) * NTW, nchunks = p.Cout >> 5;
    // The fragment's names.  The references exist only to steer code generation: each field is then read where the loop uses it, as
    // when the loop stood here, and the kernel compiles to the same instructions as then.  Plain copies, or another order of these
    // lines, change the generated code (conv_valid_tile.inc).
    constexpr int PAD = KS - 1;
    const float* const src = p.dy + (size_t)n * p.Ho * p.Wo * p.Cout;
    const int &src_rows = p.Ho, &src_cols = p.Wo, &src_C = p.Cout;
    const float src_scale = p.sg_dev[0];
    const _Float16* const& wimg = p.w;
    int* const& overflow = p.overflow;
    const int& out_rows = p.H;
#include "conv_valid_tile.inc"

    const float inv_g = p.sg_dev[1] * 0.0625f, inv_w = p.pack_scale[1] * 16.0f;    // 2^-e and 2^-w_exp
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        if (nt0 + nt >= NT) continue;
        const int ci = 32 * (nt0 + nt) + l31;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mfma32_row(r, h);
                const int iy = oy0 + 4 * MT * mh + 4 * mt + (m >> 3), ix = ox0 + (m & 7);
                if (iy < p.H && ix < p.W) p.dx[(((size_t)n * p.H + iy) * p.W + ix) * p.Cin + ci] = acc[mt][nt][r] * inv_w * inv_g;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ wgrad

constexpr int WTHR = 64 * KS;                           // one wave per kernel row
constexpr int SW = 16;                                  // output pixels per strip row: the K of one MFMA
constexpr int XW = 24;                                  // fp16 per (row, channel) in LDS: 16 + 4 pixels of x, 48 B apart
constexpr int RING = 8;                                 // x rows in LDS: five being read, one being written
constexpr int COT = 2;                                  // 32-channel co tiles per workgroup

struct WgArgs {
    const float* x;          // [N][H][W][Cin]
    const float* dy;         // [N][Ho][Wo][Cout]
    float* part;             // [ranges][taps][Cout][Cin]
    const float* sg_dev;
    float sx;                // 2^act_exp
    int N, H, W, Ho, Wo, Cin, Cout;
    int strips, cpairs;      // 16-pixel strips per row; pairs of co tiles
    long units, units_per_range;   // a unit = one output row of one strip; ranges are runs of units in (n, strip, oy) order
};

__device__ __forceinline__ void split8(const float (&v)[8], float s, f16x8& hi, f16x8& lo) {
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        f16x2 a, b;
        split2(f32x2{v[i], v[i + 1]} * f32x2{s, s}, a, b);
        hi[i] = a.x; hi[i + 1] = a.y;
        lo[i] = b.x; lo[i + 1] = b.y;
    }
}

// elements kx .. kx + 7 of the 16 fp16 in a[0..3], b[0..3] (two per word, the even one in the low half)
template <int KX>
__device__ __forceinline__ f16x8 window(const u32x4 a, const u32x4 b) {
    const unsigned w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    u32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (KX & 1) ? (w[KX / 2 + j] >> 16) | (w[KX / 2 + j + 1] << 16) : w[KX / 2 + j];
    return __builtin_bit_cast(f16x8, o);
}

__global__ __launch_bounds__(WTHR) void k_valid_wgrad(const WgArgs p) {
    __shared__ __attribute__((aligned(16))) _Float16 xh[RING * 32 * XW], xl[RING * 32 * XW];
    __shared__ __attribute__((aligned(16))) _Float16 gh[2 * 32 * COT * XW], gl[2 * 32 * COT * XW];
    const int tid = threadIdx.x, lane = tid & 63, ky = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int cot0 = COT * (blockIdx.x % p.cpairs), ci0 = 32 * (blockIdx.x / p.cpairs);
    const float sg = p.sg_dev[0];

    f32x16 acc[COT][KS];
#pragma unroll
    for (int t = 0; t < COT; ++t)
#pragma unroll
        for (int k = 0; k < KS; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][k][r] = 0.f;

    // x row iy of image n, pixels c0 + 8 g + 0..7 of channel ci0 + ch -> the ring, transposed; a lane reads one channel (4-byte loads
    // contiguous across the 32 lanes of a half-wave: the layout NHWC already has), pixels right of the image are zero
    auto stage_x = [&](int n, int iy, int c0, int g, int ch) {
        float v[8];
        const float* row = p.x + (((size_t)n * p.H + iy) * p.W) * p.Cin + ci0 + ch;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = c0 + 8 * g + e;
            v[e] = col < p.W ? row[(size_t)col * p.Cin] : 0.f;
        }
        f16x8 a, b;
        split8(v, p.sx, a, b);
        const int o = ((iy & (RING - 1)) * 32 + ch) * XW + 8 * g;
        *reinterpret_cast<f16x8*>(xh + o) = a;
        *reinterpret_cast<f16x8*>(xl + o) = b;
    };
    auto stage_dy = [&](int n, int oy, int c0, int g, int ch) {
        float v[8];
        const int co = 32 * cot0 + ch;
        const float* row = p.dy + (((size_t)n * p.Ho + oy) * p.Wo) * p.Cout + co;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = c0 + 8 * g + e;
            v[e] = (col < p.Wo && co < p.Cout) ? row[(size_t)col * p.Cout] : 0.f;
        }
        f16x8 a, b;
        split8(v, sg, a, b);
        const int o = ((oy & 1) * 32 * COT + ch) * XW + 8 * g;
        *reinterpret_cast<f16x8*>(gh + o) = a;
        *reinterpret_cast<f16x8*>(gl + o) = b;
    };

    long u = (long)blockIdx.y * p.units_per_range;
    const long u1 = u + p.units_per_range < p.units ? u + p.units_per_range : p.units;
    while (u < u1) {                                               // segments: rows [y0, y1) of one strip of one image
        const int col = (int)(u / p.Ho), strip = col % p.strips, n = col / p.strips;
        const int y0 = (int)(u - (long)col * p.Ho);
        const int y1 = (long)y0 + (u1 - u) < p.Ho ? y0 + (int)(u1 - u) : p.Ho;
        u += y1 - y0;
        const int c0 = strip * SW;
        __syncthreads();                                           // the previous segment's rows are consumed
        for (int i = tid; i < 4 * 96; i += WTHR) {                 // rows y0 .. y0 + 3; every step below adds row oy + 4 (<= H - 1)
            const int r = i / 96, q = i - r * 96;
            stage_x(n, y0 + r, c0, q >> 5, q & 31);
        }
        for (int oy = y0; oy < y1; ++oy) {
            // the slot written here held row oy - 4, last read in step oy - 4; dy rows alternate between two buffers: one barrier per step
            if (tid < 96) stage_x(n, oy + KS - 1, c0, tid >> 5, tid & 31);
            else if (tid < 96 + 64 * COT) stage_dy(n, oy, c0, ((tid - 96) >> 5) & 1, ((tid - 96) & 31) + 32 * ((tid - 96) >> 6));
            __syncthreads();
            const int xo = (((oy + ky) & (RING - 1)) * 32 + l31) * XW + 8 * h;
            const u32x4 h0 = *reinterpret_cast<const u32x4*>(xh + xo), h1 = *reinterpret_cast<const u32x4*>(xh + xo + 8);
            const u32x4 l0 = *reinterpret_cast<const u32x4*>(xl + xo), l1 = *reinterpret_cast<const u32x4*>(xl + xo + 8);
            f16x8 ah[COT], al[COT];
#pragma unroll
            for (int t = 0; t < COT; ++t) {
                const int go = ((oy & 1) * 32 * COT + 32 * t + l31) * XW + 8 * h;
                ah[t] = *reinterpret_cast<const f16x8*>(gh + go);
                al[t] = *reinterpret_cast<const f16x8*>(gl + go);
            }
            const f16x8 bh[KS] = {window<0>(h0, h1), window<1>(h0, h1), window<2>(h0, h1), window<3>(h0, h1), window<4>(h0, h1)};
            const f16x8 bl[KS] = {window<0>(l0, l1), window<1>(l0, l1), window<2>(l0, l1), window<3>(l0, l1), window<4>(l0, l1)};
#pragma unroll
            for (int t = 0; t < COT; ++t) {
#pragma unroll
                for (int k = 0; k < KS; ++k) acc[t][k] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[t], bh[k], acc[t][k], 0, 0, 0);
#pragma unroll
                for (int k = 0; k < KS; ++k) acc[t][k] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[t], bl[k], acc[t][k], 0, 0, 0);
#pragma unroll
                for (int k = 0; k < KS; ++k) acc[t][k] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[t], bh[k], acc[t][k], 0, 0, 0);
            }
        }
    }

    // partial dw of this range: accumulator register r of lane (l31, h) = D[co = row(r, h)][ci = l31]
    float* const slab = p.part + (size_t)blockIdx.y * TAPS * p.Cout * p.Cin;
#pragma unroll
    for (int t = 0; t < COT; ++t)
#pragma unroll
        for (int k = 0; k < KS; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = 32 * (cot0 + t) + mfma32_row(r, h);
                if (co < p.Cout) slab[((size_t)(ky * KS + k) * p.Cout + co) * p.Cin + ci0 + l31] = acc[t][k][r];
            }
}

struct WgPlan {
    int strips, cpairs, tiles;
    long units, units_per_range, slabs;
};

// Ranges: about two workgroups per CU (512) over the channel tiles, at least eight rows per range (a segment start stages four rows
// that give no products), at most 64 slabs of partial sums.
WgPlan wg_plan(int N, int Ho, int Wo, int Cin, int Cout) {
    WgPlan pl;
    pl.strips = (Wo + SW - 1) / SW;
    pl.cpairs = ((Cout >> 5) + COT - 1) / COT;
    pl.tiles = pl.cpairs * (Cin >> 5);
    pl.units = (long)N * pl.strips * Ho;
    long r = 512 / pl.tiles;
    if (r > 64) r = 64;
    if (r > pl.units / 8) r = pl.units / 8;
    if (r < 1) r = 1;
    pl.units_per_range = (pl.units + r - 1) / r;
    pl.slabs = (pl.units + pl.units_per_range - 1) / pl.units_per_range;
    return pl;
}

}  // namespace

extern "C" {

// The dgrad image of w [Cout][Cin][5][5] (far_conv_valid_packed_bytes(Cin, Cout, 5) bytes): channels exchanged, taps reversed, times
// pack_scale[0] -- the two device floats of the forward image of the same weight (same maximum: no reduction of its own).
int far_conv_valid_pack_dgrad_f32(const float* w, int Cin, int Cout, int ksize, const float* pack_scale, void* packed, hipStream_t stream) {
    far_clear_errors();
    if (!w || !pack_scale || !packed || !valid_shape(Cin, Cout, ksize)) return FAR_EINVAL;
    valid_pack<true>(w, Cin, Cout, pack_scale, packed, nullptr, nullptr, stream);
    return far_check_launch();
}

// dx [N][H][W][Cin] (overwritten) = the input gradient of y = conv5x5_valid(x, w) from dy [N][H - 4][W - 4][Cout], fp32 NHWC contiguous,
// dy 16-byte aligned; shapes as far_conv_valid_f16s.  packed_dgrad / pack_scale: far_conv_valid_pack_dgrad_f32's image and the scale
// it was packed with; dy_scale_dev: far_grad_scale_f32's two device floats of dy.  overflow: device int OR-ed with 1 when a sum is
// not finite, or NULL.  Deterministic; image n's dx does not depend on N.
int far_conv_valid_dgrad_f16s(const float* dy, const void* packed_dgrad, const float* pack_scale, const float* dy_scale_dev, float* dx, long N,
                              int H, int W, int Cin, int Cout, int ksize, int* overflow, hipStream_t stream) {
    far_clear_errors();
    if (N < 0 || !valid_shape(Cin, Cout, ksize) || H < KS || W < KS) return FAR_EINVAL;
    if (N == 0) return FAR_OK;
    if (!dy || !packed_dgrad || !pack_scale || !dy_scale_dev || !dx || dy == dx || (reinterpret_cast<uintptr_t>(dy) & 15)) return FAR_EINVAL;
    DgradArgs a;
    a.dy = dy; a.w = (const _Float16*)packed_dgrad; a.sg_dev = dy_scale_dev; a.pack_scale = pack_scale; a.dx = dx;
    a.H = H; a.W = W; a.Ho = H - KS + 1; a.Wo = W - KS + 1; a.Cin = Cin; a.Cout = Cout;
    a.tilesX = (W + TW - 1) / TW; a.tilesY = (H + 8 * MTD - 1) / (8 * MTD); a.overflow = overflow;
    const long nbx = N * a.tilesX * a.tilesY;
    const int NT = Cin >> 5;
    const int ntw = NT % 6 == 0 || NT % 4 != 0 ? 3 : 2;            // 128 channels: two waves x two N-tiles, none idle
    const int nby = (NT + 2 * ntw - 1) / (2 * ntw);
    if (nbx > 0x7fffffffL || nby > 65535) return FAR_EINVAL;
    if (ntw == 3) hipLaunchKernelGGL(k_valid_dgrad<3>, dim3((unsigned)nbx, (unsigned)nby), dim3(NTHR), 0, stream, a);
    else hipLaunchKernelGGL(k_valid_dgrad<2>, dim3((unsigned)nbx, (unsigned)nby), dim3(NTHR), 0, stream, a);
    return far_check_launch();
}

// Bytes of workspace far_conv_valid_wgrad_f16s needs for this shape (0 for a shape it does not cover).
long far_conv_valid_wgrad_ws_bytes(int N, int H, int W, int Cin, int Cout, int ksize) {
    if (N <= 0 || H < KS || W < KS || !valid_shape(Cin, Cout, ksize)) return 0;
    const WgPlan pl = wg_plan(N, H - KS + 1, W - KS + 1, Cin, Cout);
    return 256 + pl.slabs * (long)TAPS * Cout * Cin * (long)sizeof(float);
}

// dw [Cout][Cin][5][5] (torch layout, fp32, overwritten) = the weight gradient of y = conv5x5_valid(x, w) from x [N][H][W][Cin] and
// dy [N][H - 4][W - 4][Cout] (NHWC fp32 contiguous).  x is multiplied by 2^act_exp before the fp16 split (the exponent the forward
// consumed it with), dy by dy_scale_dev[0] (far_grad_scale_f32's two device floats; NULL: computed here).  ws:
// far_conv_valid_wgrad_ws_bytes() bytes of device scratch.  overflow: device int OR-ed with 1 when a sum came out non-finite, or NULL.
int far_conv_valid_wgrad_f16s(const float* x, const float* dy, int N, int H, int W, int Cin, int Cout, int ksize, int act_exp,
                              const float* dy_scale_dev, void* ws, long ws_bytes, float* dw, int* overflow, hipStream_t stream) {
    far_clear_errors();
    const long need = far_conv_valid_wgrad_ws_bytes(N, H, W, Cin, Cout, ksize);
    if (!x || !dy || !dw || !ws || need == 0 || ws_bytes < need || act_exp < -24 || act_exp > 15) return FAR_EINVAL;
    WgArgs a;
    a.x = x; a.dy = dy; a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.Ho = H - KS + 1; a.Wo = W - KS + 1;
    const WgPlan pl = wg_plan(N, a.Ho, a.Wo, Cin, Cout);
    a.strips = pl.strips; a.cpairs = pl.cpairs; a.units = pl.units; a.units_per_range = pl.units_per_range;
    float* const scale = reinterpret_cast<float*>(ws);
    a.part = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + 256);
    if (!dy_scale_dev) {
        const int rc = far_grad_scale_f32(dy, (long)N * a.Ho * a.Wo * Cout, scale, stream);
        if (rc != FAR_OK) return rc;
        dy_scale_dev = scale;
    }
    a.sg_dev = dy_scale_dev;
    a.sx = ldexpf(1.0f, act_exp);
    if (pl.slabs > 65535) return FAR_EINVAL;
    hipLaunchKernelGGL(k_valid_wgrad, dim3((unsigned)pl.tiles, (unsigned)pl.slabs), dim3(WTHR), 0, stream, a);
    wgrad_reduce(a.part, pl.slabs, TAPS, (long)Cout * Cin, dy_scale_dev, ldexpf(1.0f, -act_exp), dw, overflow, stream);
    return far_check_launch();
}

}  // extern "C"

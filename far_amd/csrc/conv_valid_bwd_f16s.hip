// K24 backward: input gradient and weight gradient of the 5 x 5 unpadded ('valid') stride-1 convolution of conv_valid_f16s.hip, NHWC fp32,
// split-fp16 operands (hi.hi + hi.lo + lo.hi, fp32 accumulation) on the matrix cores.
//
// Replaces autograd's backward of interiornetStreetlearn_8ptVit/src/modules/extractor.py:11 (conv2, 192 -> 192) and :46-47 (downsample.0,
// 128 -> 192) of the ResidualBlock model.py:60 builds with kernel_size 5, which train.py fine-tunes with the trunk.
//
// dgrad  dx[n][iy][ix][ci] = sum_{ky, kx, co} dy[n][iy - ky][ix - kx][co] w[co][ci][ky][kx]  (terms outside dy are zero): the 'full'
//   correlation of dy with the flipped, channel-transposed kernel.  K24's tile loop on its own weight image (k_valid_pack_dgrad); the
//   patch load knows the border: pixel (py, px) of a workgroup's patch is dy[oy0 + py - 4][ox0 + px - 4] or zero, no padded copy of dy
//   exists.  dy is multiplied by far_grad_scale_f32's device power of two before the split, the epilogue takes it out again.
//   One form for every launch size: a 16 x 8 tile of dx per workgroup, a wave owns 8 rows x two or three 32-channel N-tiles.  The sum
//   of an element runs over (chunk, tap, k-step) in that order whatever N is.
// wgrad  dw[co][ci][ky][kx] = sum_{n, oy, ox} dy[n][oy][ox][co] x[n][oy + ky][ox + kx][ci]: a GEMM whose reduction runs over pixels, so
//   an MFMA operand is 8 consecutive pixels of ONE channel.  A workgroup (five waves, one per kernel row ky) owns 64 co x 32 ci x 25 taps
//   and walks 16-pixel-wide column strips downwards: every x row is read from memory once, scaled, split and written TRANSPOSED
//   ([channel][pixel], 48 B per channel: conflict-free 16-byte reads) into a ring of eight rows in LDS; wave ky reads row oy + ky of the
//   ring, and the five kx-shifted operands are cut from one 16-pixel fragment in registers.  The (image, strip, row) sequence is cut
//   into ranges, each range writes its partial dw to a workspace slab, k_valid_wgrad_reduce adds the slabs in index order:
//   deterministic, no atomics on floats (K16's contract).
#include "common.h"

extern "C" int far_grad_scale_f32(const float* x, long n, float* out2, hipStream_t stream);

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int KS = 5, TAPS = KS * KS;

bool valid_shape(int Cin, int Cout, int ksize) {
    return ksize == KS && Cin > 0 && Cout > 0 && (Cin & 31) == 0 && (Cout & 31) == 0;
}

// ------------------------------------------------------------------------------------------------------------------ dgrad

constexpr int TW = 8, PW = TW + KS - 1;                 // tile width of a workgroup; patch width 12
constexpr int PSTR = 40;                                // fp16 per patch pixel and plane: 32 channels + 8 of padding (K24's layout)
constexpr int NTHR = 256;
constexpr int STEPS = TAPS * 2;                         // k-steps of 16 channels per chunk
constexpr int MTD = 2;                                  // 4 x 8-pixel M-tiles per wave: a 16 x 8 tile of dx per workgroup

struct DgradArgs {
    const float* dy;         // [N][Ho][Wo][Cout]
    const _Float16* w;       // k_valid_pack_dgrad's image
    const float* sg_dev;     // { 2^e, 2^(4 - e) }: dy is multiplied by [0] before the split
    const float* pack_scale; // { 2^w_exp, 2^-(w_exp + 4) } of the image
    float* dx;               // [N][H][W][Cin]
    int H, W, Ho, Wo, Cin, Cout, tilesX, tilesY;
    int* overflow;
};

// NTW: 32-channel N-tiles (of Cin) per wave; the workgroup covers 2 NTW of them per blockIdx.y.
template <int NTW>
__global__ __launch_bounds__(NTHR) void k_valid_dgrad(const DgradArgs p) {
    constexpr int MT = MTD, TH = 8 * MT, PH = TH + KS - 1;
    constexpr int NITEMS = PH * PW * 8;                 // float4 loads per chunk
    constexpr int ITEMS = (NITEMS + NTHR - 1) / NTHR;
    __shared__ __attribute__((aligned(16))) _Float16 hi[PH * PW * PSTR];
    __shared__ __attribute__((aligned(16))) _Float16 lo[PH * PW * PSTR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int mh = wave & 1, nh = wave >> 1;
    int t = blockIdx.x;
    const int tx = t % p.tilesX;
    t /= p.tilesX;
    const int ty = t % p.tilesY, n = t / p.tilesY;
    const int oy0 = ty * TH, ox0 = tx * TW;                        // of dx; the patch starts at dy[oy0 - 4][ox0 - 4]
    const int NT = p.Cin >> 5, nt0 = (blockIdx.y * 2 + nh) * NTW, nchunks = p.Cout >> 5;
    const float* gin = p.dy + (size_t)n * p.Ho * p.Wo * p.Cout;
    const float sg = p.sg_dev[0];

    f32x16 acc[MT][NTW], accs[MT][NTW];                            // hi.hi apart from the cross terms, as K24
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = accs[mt][nt][r] = 0.f;

    const bool live = oy0 + 4 * MT * mh < p.H && nt0 < NT;         // wave-uniform
    const int abase = ((4 * MT * mh + (l31 >> 3)) * PW + (l31 & 7)) * PSTR + 8 * h;
    const f32x2 sg2 = {sg, sg};

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
        if (live) fetch(c, 0, 0);
        __syncthreads();                                           // the previous chunk's planes are consumed
        {
            float4 v[ITEMS];
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) {
                const int i = tid + NTHR * j, pix = i >> 3, q = i & 7;
                const int py = pix / PW, px = pix - py * PW;
                const int gy = oy0 + py - (KS - 1), gx = ox0 + px - (KS - 1);      // the border: outside dy is zero
                v[j] = (i < NITEMS && gy >= 0 && gy < p.Ho && gx >= 0 && gx < p.Wo)
                           ? *reinterpret_cast<const float4*>(gin + ((size_t)gy * p.Wo + gx) * p.Cout + 32 * c + 4 * q)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) {
                const int i = tid + NTHR * j, pix = i >> 3, q = i & 7;
                f16x2 h0, l0, h1, l1;
                split2(f32x2{v[j].x, v[j].y} * sg2, h0, l0);
                split2(f32x2{v[j].z, v[j].w} * sg2, h1, l1);
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
                step(off, 0);
                if (tap + 1 < TAPS) fetch(c, 2 * tap + 2, 0);
                step(off + 16, 1);
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] += accs[mt][nt];

    if (p.overflow) {                                              // a non-finite dy reaches the accumulators: as K24's guard
        float chk = 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) chk += acc[mt][nt][r];
        if (__any(!(fabsf(chk) <= FLT_MAX)) && lane == 0) atomicOr(p.overflow, 1);
    }

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

// The dgrad image: K24's layout with the channels exchanged and the taps reversed.  Item (chunk c, tap t, k-step s, N-tile nt, lane):
// the eight OUTPUT channels co = 32 c + 16 s + 8 (lane >> 5) + e of the forward layer (the reduction of the dgrad) for its input channel
// ci = 32 nt + (lane & 31) at tap 24 - t, times pack_scale[0] (the forward image's scale: the same maximum).
__global__ __launch_bounds__(256) void k_valid_pack_dgrad(const float* __restrict__ w, int Cin, int Cout, const float* __restrict__ pack_scale,
                                                          _Float16* __restrict__ packed) {
    const int NT = Cin >> 5;
    const long items = (long)(Cout >> 5) * TAPS * 2 * NT * 64;
    const float wmul = pack_scale[0];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        const int ln = (int)(i & 63);
        long u = i >> 6;
        const int nt = (int)(u % NT);
        u /= NT;
        const int s = (int)(u & 1);
        u >>= 1;
        const int t = (int)(u % TAPS), c = (int)(u / TAPS);
        const int ci = 32 * nt + (ln & 31);
        f16x8 vh, vl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int co = 32 * c + 16 * s + 8 * (ln >> 5) + e;
            const float v = w[((size_t)co * Cin + ci) * TAPS + (TAPS - 1 - t)] * wmul;
            const _Float16 hh = (_Float16)v;
            vh[e] = hh;
            vl[e] = (_Float16)(v - (float)hh);
        }
        _Float16* dst = packed + (size_t)(i >> 6) * 1024 + ln * 8;
        *reinterpret_cast<f16x8*>(dst) = vh;
        *reinterpret_cast<f16x8*>(dst + 512) = vl;
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

// dw[co][ci][t] = (sum over slabs of part[slab][t][co][ci]) / (sx sg), slabs in index order; overflow |= a non-finite sum.
__global__ void k_valid_wgrad_reduce(const float* __restrict__ part, int slabs, long cc, const float* __restrict__ sg_dev, float inv_sx,
                                     float* __restrict__ dw, int* __restrict__ overflow) {
    const long total = cc * TAPS;
    const float inv = inv_sx / sg_dev[0];
    bool bad = false;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int k = 0; k < slabs; ++k) s += part[(size_t)k * total + i];
        const long t = i / cc, e = i - t * cc;
        bad |= !(fabsf(s) <= FLT_MAX);
        dw[e * TAPS + t] = s * inv;
    }
    if (overflow && bad) atomicOr(overflow, 1);
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
    const long items = (long)(Cout >> 5) * TAPS * 2 * (Cin >> 5) * 64;
    long blocks = (items + 255) / 256;
    blocks = blocks > 1024 ? 1024 : blocks;
    hipLaunchKernelGGL(k_valid_pack_dgrad, dim3((unsigned)blocks), dim3(256), 0, stream, w, Cin, Cout, pack_scale, (_Float16*)packed);
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
    const long cc = (long)Cout * Cin, total = cc * TAPS;
    hipLaunchKernelGGL(k_valid_wgrad_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a.part, (int)pl.slabs, cc, dy_scale_dev,
                       ldexpf(1.0f, -act_exp), dw, overflow);
    return far_check_launch();
}

}  // extern "C"

// The second stage of the weight gradients (K16: conv_wgrad_f16s.hip; K24: conv_valid_bwd_f16s.hip): the first stage cuts the pixels
// into ranges and writes one slab [taps][Cout][Cin] of partial sums per range; this adds the slabs in index order, takes the two operand
// scales out and writes torch's layout.  One thread per element, no atomics on floats: the same bits in every launch.
// Each including file gets its own copy in its anonymous namespace.
#pragma once
#include "common.h"

namespace {

// dw[co][ci][t] = (sum over slabs of part[slab][t][co][ci]) / (sx sg), slabs in index order; overflow |= a non-finite sum.
__global__ void k_wgrad_reduce(const float* __restrict__ part, int slabs, int taps, long cc, const float* __restrict__ sg_dev, float inv_sx,
                               float* __restrict__ dw, int* __restrict__ overflow) {
    const long total = cc * taps;
    const float inv = inv_sx / sg_dev[0];
    bool bad = false;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int k = 0; k < slabs; ++k) s += part[(size_t)k * total + i];
        const long t = i / cc, e = i - t * cc;
        bad |= !(fabsf(s) <= FLT_MAX);
        dw[e * taps + t] = s * inv;
    }
    if (overflow && bad) atomicOr(overflow, 1);
}

// cc = Cout * Cin; sg_dev: far_grad_scale_f32's device floats of dy; inv_sx = 2^-act_exp
void wgrad_reduce(const float* part, long slabs, int taps, long cc, const float* sg_dev, float inv_sx, float* dw, int* overflow,
                  hipStream_t stream) {
    const long total = cc * taps;
    hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, part, (int)slabs, taps, cc, sg_dev, inv_sx,
                       dw, overflow);
}

}  // namespace

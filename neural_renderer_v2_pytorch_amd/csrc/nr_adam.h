// nr_adam.h -- multi-tensor Adam: one tick launch and one update launch for up to NR_ADAM_MAX_TENSORS tensors
// Part of nr_raster.hip (one translation unit); see that file, include/nr_raster.h (the update rule) and
// DESIGN.md section 4 ("Optimiser").
//
// Conventions (those of nr_image_loss.h, whose il_load / il_store / il_valid these kernels reuse):
// 256-thread blocks, plain pointers, no float atomics, no contraction.  k_adam_tick: one thread per tensor
// adds 1 to the tensor's step and writes its two bias-correction factors, computed in double, to the
// factor scratch.  k_adam_update: the tensor descriptors and the prefix table of block starts arrive by
// value in the kernel arguments (gradient pointers change with every eager step: no device table to
// refresh, nothing to synchronise); a block finds its tensor by a scan of at most NR_ADAM_MAX_TENSORS
// starts and streams one AD_CHUNK-element chunk of it.  A chunk wholly inside its tensor takes an
// unguarded body.  The access width is the host's choice per tensor (block-uniform): 16-byte accesses
// when all four bases are on 16 bytes, lane-consecutive scalar accesses otherwise; the arithmetic is per
// element and the same on both, so the results are bitwise identical.
//
// SKIP = false: every lane issues all its loads of g, p, m, v before the first use.
// SKIP = true:  a lane loads its gradients first, and loads and stores p, m, v only for the groups (4
//               elements on the vector path, 1 on the scalar path) that hold a nonzero gradient; inside
//               such a group an element with a zero gradient is written back unchanged.
//
// Limits (checked by nr_adam_step): numel <= INT_MAX - AD_CHUNK per tensor, blocks of a launch <= INT_MAX.
#pragma once

#pragma clang fp contract(off)

namespace {

constexpr int AD_BLOCK = IL_BLOCK;
constexpr int AD_CHUNK = NR_ADAM_CHUNK;  // elements per block: 4 float4 (or 16 float) per lane and operand
static_assert(AD_CHUNK % (AD_BLOCK * 4) == 0, "a chunk is a whole number of 16-byte accesses per lane");
// The measured alternative of the skipping kernel (tools/bench_adam.py builds it with this define, never the
// product): load p, m, v of every group and skip only the stores.  Same results.
#ifdef NR_ADAM_SKIP_LOADS_ALL
constexpr bool AD_SKIP_LOADS_ALL = true;
#else
constexpr bool AD_SKIP_LOADS_ALL = false;
#endif

struct AdamTick {
    float* step[NR_ADAM_MAX_TENSORS];
    double lr_scale[NR_ADAM_MAX_TENSORS];
    int slot[NR_ADAM_MAX_TENSORS];  // the tensor's pair in the factor scratch
    double lr, beta1, beta2;
    const float* lr_device;  // non-null: the rate is read here (a schedule under graph replay)
    float* factors;
    int n;
};

// step += 1; factors[slot] = (step_size, inv_sqrt_bc2) of the new step, from double arithmetic
__global__ __launch_bounds__(64) void k_adam_tick(const AdamTick a) {
    const int i = (int)threadIdx.x;
    if (i >= a.n) return;
    float* sp = a.step[i];
    const float t = *sp + 1.f;
    *sp = t;
    const double lr = a.lr_device ? (double)*a.lr_device : a.lr;
    const double bc1 = 1.0 - pow(a.beta1, (double)t);
    const double bc2 = 1.0 - pow(a.beta2, (double)t);
    float* f = a.factors + 2 * (long long)a.slot[i];
    f[0] = (float)(lr * a.lr_scale[i] / bc1);
    f[1] = (float)(1.0 / sqrt(bc2));
}

struct AdamDesc {
    float* p;
    const float* g;
    float* m;
    float* v;
    int numel;
    int vec;   // 1: all four bases on 16 bytes
    int slot;  // the tensor's pair in the factor scratch
    int pad;
};

struct AdamLaunch {
    AdamDesc t[NR_ADAM_MAX_TENSORS];
    int start[NR_ADAM_MAX_TENSORS + 1];  // tensor k owns blocks [start[k], start[k + 1]); every tensor has at least one
    int n;
    float c1, c2, eps;
    const float* factors;
};

// The rule of include/nr_raster.h for one element, every operation a correctly rounded float32 one.
__device__ __forceinline__ void ad_rule(float g, float& p, float& m, float& v, float c1, float c2, float eps, float step_size,
                                        float inv_sqrt_bc2) {
    const float m2 = m + c1 * (g - m);
    float v2 = v + c2 * (g * g - v);
    v2 = v2 < 0.f ? 0.f : v2;  // the reference's clamp; a NaN stays
    const float denom = sqrtf(v2) * inv_sqrt_bc2 + eps;
    p = p - step_size * (m2 / denom);
    m = m2, v = v2;
}

template <int VW, bool FULL, bool SKIP>
__device__ __forceinline__ void ad_chunk(const AdamDesc& d, int c0, float c1, float c2, float eps, float step_size,
                                         float inv_sqrt_bc2) {
    constexpr int U = AD_CHUNK / (AD_BLOCK * VW);
    float gv[U][VW], pv[U][VW], mv[U][VW], vv[U][VW];
    bool live[U];
    const int i0 = c0 + (int)threadIdx.x * VW;
#pragma unroll
    for (int j = 0; j < U; j++) il_load<VW, FULL>(d.g, i0 + j * AD_BLOCK * VW, il_valid<VW>(i0 + j * AD_BLOCK * VW, d.numel), gv[j]);
#pragma unroll
    for (int j = 0; j < U; j++) {
        live[j] = !SKIP;
        if (SKIP) {
            // elements past numel were loaded as zeros: a group wholly past the end is never live
#pragma unroll
            for (int k = 0; k < VW; k++) live[j] = live[j] || gv[j][k] != 0.f;  // -0 is zero, NaN is not
        }
    }
#pragma unroll
    for (int j = 0; j < U; j++)
        if (live[j] || AD_SKIP_LOADS_ALL) {
            const int off = i0 + j * AD_BLOCK * VW, valid = il_valid<VW>(off, d.numel);
            il_load<VW, FULL>(d.p, off, valid, pv[j]);
            il_load<VW, FULL>(d.m, off, valid, mv[j]);
            il_load<VW, FULL>(d.v, off, valid, vv[j]);
        }
    // keep the scheduler from sinking loads below the first group's arithmetic and stores: all of a
    // lane's loads are in flight before the first use
    if (!SKIP) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < U; j++)
        if (live[j]) {
            const int off = i0 + j * AD_BLOCK * VW, valid = il_valid<VW>(off, d.numel);
#pragma unroll
            for (int k = 0; k < VW; k++) {
                float p = pv[j][k], m = mv[j][k], v = vv[j][k];
                ad_rule(gv[j][k], p, m, v, c1, c2, eps, step_size, inv_sqrt_bc2);
                const bool keep = SKIP && gv[j][k] == 0.f;
                pv[j][k] = keep ? pv[j][k] : p, mv[j][k] = keep ? mv[j][k] : m, vv[j][k] = keep ? vv[j][k] : v;
            }
            il_store<VW, FULL>(d.p, off, valid, pv[j]);
            il_store<VW, FULL>(d.m, off, valid, mv[j]);
            il_store<VW, FULL>(d.v, off, valid, vv[j]);
        }
}

// grid: start[n] blocks
template <bool SKIP>
__global__ __launch_bounds__(AD_BLOCK) void k_adam_update(const AdamLaunch a) {
    const int blk = (int)blockIdx.x;
    int k = 0;
    for (int i = 1; i < a.n; i++) k = blk >= a.start[i] ? i : k;
    const AdamDesc d = a.t[k];
    const int c0 = (blk - a.start[k]) * AD_CHUNK;
    const float step_size = a.factors[2 * d.slot], inv_sqrt_bc2 = a.factors[2 * d.slot + 1];
    const bool full = c0 + AD_CHUNK <= d.numel;
    if (d.vec) {
        if (full) ad_chunk<4, true, SKIP>(d, c0, a.c1, a.c2, a.eps, step_size, inv_sqrt_bc2);
        else ad_chunk<4, false, SKIP>(d, c0, a.c1, a.c2, a.eps, step_size, inv_sqrt_bc2);
    } else {
        if (full) ad_chunk<1, true, SKIP>(d, c0, a.c1, a.c2, a.eps, step_size, inv_sqrt_bc2);
        else ad_chunk<1, false, SKIP>(d, c0, a.c1, a.c2, a.eps, step_size, inv_sqrt_bc2);
    }
}

}  // namespace

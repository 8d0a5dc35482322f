// nr_image_loss.h -- per-item image losses: weighted squared error, Huber and silhouette IoU, forward and backward
// Part of nr_raster.hip (one translation unit); see that file, include/nr_raster.h (the formulas) and
// DESIGN.md section 4 ("Image losses").
//
// Conventions (those of nr_mesh_loss.h, whose ml_wave_sum / ml_block_sum / k_mesh_loss_sum these kernels
// reuse): 256-thread blocks that never straddle an item, plain pointers, every output fully written, no
// float atomics.  Block (b, c) streams chunk c -- elements [IL_CHUNK c, IL_CHUNK c + IL_CHUNK) -- of item b:
// every lane issues all its loads of every operand (16 bytes each on the vector path) before the first
// use, reduces in registers, and the block writes one partial (IoU: two) per chunk; a second launch adds
// an item's partials in a fixed order.  The backward is one elementwise launch over the same chunks that
// recomputes from the inputs.  Losses and gradients are bitwise reproducible from run to run.
//
// The host picks the instantiation per launch from what is aligned (nr_raster.hip, il_aligned): VW = 4
// needs every item base of images, targets (and the gradient) on 16 bytes; an N that is no multiple of 4
// then ends in one partly filled group that takes scalar accesses.  Vector weight loads (IL_W_VECTOR) need
// that of the weights, and a period that is a multiple of 4.  Everything else runs VW = 1: lane-consecutive
// scalar accesses over the same chunks.
//
// Limits (checked by the host entry points): N <= INT_MAX - IL_CHUNK, B * ceil(N / IL_CHUNK) <= INT_MAX.
#pragma once

#pragma clang fp contract(off)

namespace {

constexpr int IL_BLOCK = ML_BLOCK;  // threads per block
constexpr int IL_CHUNK = 4096;      // elements of one item per block: 4 float4 (or 16 float) per lane and operand
enum { IL_W_NONE = 0, IL_W_SCALAR = 1, IL_W_VECTOR = 2 };

// v = p[off .. off + VW), of which the first `valid` exist (FULL: all of them); zeros for the rest.
template <int VW, bool FULL>
__device__ __forceinline__ void il_load(const float* __restrict__ p, int off, int valid, float (&v)[VW]) {
    if (VW == 4 && (FULL || valid >= 4)) {
        const float4 q = *reinterpret_cast<const float4*>(p + off);
        v[0] = q.x, v[VW > 1 ? 1 : 0] = q.y, v[VW > 2 ? 2 : 0] = q.z, v[VW > 3 ? 3 : 0] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < VW; k++) v[k] = (FULL || k < valid) ? p[off + k] : 0.f;
    }
}

template <int VW, bool FULL>
__device__ __forceinline__ void il_store(float* __restrict__ p, int off, int valid, const float (&v)[VW]) {
    if (VW == 4 && (FULL || valid >= 4)) {
        *reinterpret_cast<float4*>(p + off) = make_float4(v[0], v[VW > 1 ? 1 : 0], v[VW > 2 ? 2 : 0], v[VW > 3 ? 3 : 0]);
    } else {
#pragma unroll
        for (int k = 0; k < VW; k++)
            if (FULL || k < valid) p[off + k] = v[k];
    }
}

// how many of the elements [i, i + VW) lie below N, in [0, VW]
template <int VW>
__device__ __forceinline__ int il_valid(int i, int N) { return min(max(N - i, 0), VW); }

struct ILPointwise {
    const float* images;   // item b at images + b * istride
    const float* targets;  // item b at targets + b * tstride (0: shared)
    const float* weights;  // element i of item b: weights[b * wstride + i % period]; unused with IL_W_NONE
    long long istride, tstride, wstride;
    int period, wstep;     // wstep = (IL_BLOCK * 4) % period: the weight offset's advance per vector load
    float delta;           // Huber's; unused by the squared error
    int N, nchunk;
};

// The pointwise term h(d) and its derivative, d = x - t.
template <bool HUBER>
__device__ __forceinline__ float il_term(float d, float delta) {
    const float a = fabsf(d);
    const float sq = d * d;
    return HUBER ? (a < delta ? 0.5f * sq : delta * (a - 0.5f * delta)) : sq;
}
template <bool HUBER>
__device__ __forceinline__ float il_dterm(float d, float delta) {
    return HUBER ? (fabsf(d) < delta ? d : copysignf(delta, d)) : 2.f * d;
}

// One lane's share of chunk c0 of an item (x, t, w at the item's base): all loads, then the arithmetic.
// !GRAD: returns the lane's sum of w h(x - t).  GRAD: writes gscale w h'(x - t) to gout, returns 0.
template <int VW, int WM, bool HUBER, bool FULL, bool GRAD>
__device__ __forceinline__ float il_pointwise_chunk(const ILPointwise& a, const float* __restrict__ x, const float* __restrict__ t,
                                                    const float* __restrict__ w, int c0, float gscale, float* __restrict__ gout) {
    constexpr int U = IL_CHUNK / (IL_BLOCK * VW);
    static_assert(WM != IL_W_VECTOR || VW == 4, "vector weight loads belong to the vector path");
    float xv[U][VW], tv[U][VW], wv[U][VW];
    const int i0 = c0 + (int)threadIdx.x * VW;
#pragma unroll
    for (int j = 0; j < U; j++) il_load<VW, FULL>(x, i0 + j * IL_BLOCK * VW, il_valid<VW>(i0 + j * IL_BLOCK * VW, a.N), xv[j]);
#pragma unroll
    for (int j = 0; j < U; j++) il_load<VW, FULL>(t, i0 + j * IL_BLOCK * VW, il_valid<VW>(i0 + j * IL_BLOCK * VW, a.N), tv[j]);
    if (WM == IL_W_VECTOR) {
        // period and i0 are multiples of 4, so is every offset r, and r + 3 < period; N is a multiple of
        // the period: no partly filled group
        unsigned r = (unsigned)i0 % (unsigned)a.period;  // unsigned: r + wstep < 2 period may pass 2^31
#pragma unroll
        for (int j = 0; j < U; j++) {
            il_load<VW, FULL>(w, (int)r, il_valid<VW>(i0 + j * IL_BLOCK * VW, a.N), wv[j]);
            r += (unsigned)a.wstep;
            if (r >= (unsigned)a.period) r -= (unsigned)a.period;
        }
    } else if (WM == IL_W_SCALAR) {
#pragma unroll
        for (int j = 0; j < U; j++) {
            const int i = i0 + j * IL_BLOCK * VW;
#pragma unroll
            for (int k = 0; k < VW; k++) wv[j][k] = (FULL || i + k < a.N) ? w[(unsigned)(i + k) % (unsigned)a.period] : 0.f;
        }
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < U; j++) {
        float g[VW];
#pragma unroll
        for (int k = 0; k < VW; k++) {
            const float d = xv[j][k] - tv[j][k];
            if (GRAD) {
                const float dh = il_dterm<HUBER>(d, a.delta);
                g[k] = gscale * (WM != IL_W_NONE ? wv[j][k] * dh : dh);
            } else {
                const float h = il_term<HUBER>(d, a.delta);
                s += WM != IL_W_NONE ? wv[j][k] * h : h;
            }
        }
        if (GRAD) il_store<VW, FULL>(gout, i0 + j * IL_BLOCK * VW, il_valid<VW>(i0 + j * IL_BLOCK * VW, a.N), g);
    }
    return s;
}

// grid: B * nchunk blocks.  partial[b][c] = sum over chunk c of item b of w_i h(x_i - t_i).
template <int VW, int WM, bool HUBER>
__global__ __launch_bounds__(IL_BLOCK) void k_pointwise_fwd(const ILPointwise a, float* __restrict__ partial) {
    __shared__ float red[IL_BLOCK / 64];
    const int b = blockIdx.x / a.nchunk, c = blockIdx.x - b * a.nchunk;
    const float* x = a.images + (long long)b * a.istride;
    const float* t = a.targets + (long long)b * a.tstride;
    const float* w = WM != IL_W_NONE ? a.weights + (long long)b * a.wstride : nullptr;
    const int c0 = c * IL_CHUNK;
    const float s = c0 + IL_CHUNK <= a.N ? il_pointwise_chunk<VW, WM, HUBER, true, false>(a, x, t, w, c0, 0.f, nullptr)
                                         : il_pointwise_chunk<VW, WM, HUBER, false, false>(a, x, t, w, c0, 0.f, nullptr);
    const float tot = ml_block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// grad_images[b][i] = grad_loss[b] w_i h'(x_i - t_i), contiguous [B, N], every element written.
template <int VW, int WM, bool HUBER>
__global__ __launch_bounds__(IL_BLOCK) void k_pointwise_bwd(const ILPointwise a, const float* __restrict__ grad_loss,
                                                            float* __restrict__ grad_images) {
    const int b = blockIdx.x / a.nchunk, c = blockIdx.x - b * a.nchunk;
    const float* x = a.images + (long long)b * a.istride;
    const float* t = a.targets + (long long)b * a.tstride;
    const float* w = WM != IL_W_NONE ? a.weights + (long long)b * a.wstride : nullptr;
    float* go = grad_images + (long long)b * a.N;
    const float g = grad_loss[b];
    const int c0 = c * IL_CHUNK;
    if (c0 + IL_CHUNK <= a.N) il_pointwise_chunk<VW, WM, HUBER, true, true>(a, x, t, w, c0, g, go);
    else il_pointwise_chunk<VW, WM, HUBER, false, true>(a, x, t, w, c0, g, go);
}

// The forward (grad_loss == nullptr: out = the partials) or backward (out = grad_images) of the
// instantiation (vec ? 4 : 1, wm, huber) on B * nchunk blocks.
template <int VW, int WM, bool HUBER>
void il_launch_pointwise(const ILPointwise& a, dim3 grid, hipStream_t st, const float* grad_loss, float* out) {
    if (grad_loss) nr_launch(k_pointwise_bwd<VW, WM, HUBER>, grid, dim3(IL_BLOCK), 0, st, a, grad_loss, out);
    else nr_launch(k_pointwise_fwd<VW, WM, HUBER>, grid, dim3(IL_BLOCK), 0, st, a, out);
}

template <bool HUBER>
void il_launch_pointwise(const ILPointwise& a, bool vec, int wm, dim3 grid, hipStream_t st, const float* grad_loss, float* out) {
    if (vec && wm == IL_W_VECTOR) il_launch_pointwise<4, IL_W_VECTOR, HUBER>(a, grid, st, grad_loss, out);
    else if (vec && wm == IL_W_SCALAR) il_launch_pointwise<4, IL_W_SCALAR, HUBER>(a, grid, st, grad_loss, out);
    else if (vec) il_launch_pointwise<4, IL_W_NONE, HUBER>(a, grid, st, grad_loss, out);
    else if (wm == IL_W_SCALAR) il_launch_pointwise<1, IL_W_SCALAR, HUBER>(a, grid, st, grad_loss, out);
    else il_launch_pointwise<1, IL_W_NONE, HUBER>(a, grid, st, grad_loss, out);
}

void launch_pointwise(const ILPointwise& a, bool vec, int wm, bool huber, int B, hipStream_t st, const float* grad_loss, float* out) {
    const dim3 grid((unsigned)(B * a.nchunk));
    if (huber) il_launch_pointwise<true>(a, vec, wm, grid, st, grad_loss, out);
    else il_launch_pointwise<false>(a, vec, wm, grid, st, grad_loss, out);
}

// ---- silhouette IoU ----
template <int VW, bool FULL>
__device__ __forceinline__ void il_iou_chunk(const float* __restrict__ p, const float* __restrict__ t, int c0, int N, float& si,
                                             float& su) {
    constexpr int U = IL_CHUNK / (IL_BLOCK * VW);
    float pv[U][VW], tv[U][VW];
    const int i0 = c0 + (int)threadIdx.x * VW;
#pragma unroll
    for (int j = 0; j < U; j++) il_load<VW, FULL>(p, i0 + j * IL_BLOCK * VW, il_valid<VW>(i0 + j * IL_BLOCK * VW, N), pv[j]);
#pragma unroll
    for (int j = 0; j < U; j++) il_load<VW, FULL>(t, i0 + j * IL_BLOCK * VW, il_valid<VW>(i0 + j * IL_BLOCK * VW, N), tv[j]);
    si = su = 0.f;
#pragma unroll
    for (int j = 0; j < U; j++)
#pragma unroll
        for (int k = 0; k < VW; k++) {
            const float pt = pv[j][k] * tv[j][k];
            si += pt;
            su += (pv[j][k] + tv[j][k]) - pt;
        }
}

// grid: B * nchunk blocks.  partial[b][c] = (sum p t, sum (p + t - p t)) over chunk c of item b.
template <int VW>
__global__ __launch_bounds__(IL_BLOCK) void k_iou_fwd(const float* __restrict__ images, long long istride,
                                                      const float* __restrict__ targets, long long tstride, int N, int nchunk,
                                                      float* __restrict__ partial) {
    __shared__ float red_i[IL_BLOCK / 64], red_u[IL_BLOCK / 64];
    const int b = blockIdx.x / nchunk, c = blockIdx.x - b * nchunk;
    const float* p = images + (long long)b * istride;
    const float* t = targets + (long long)b * tstride;
    const int c0 = c * IL_CHUNK;
    float si, su;
    if (c0 + IL_CHUNK <= N) il_iou_chunk<VW, true>(p, t, c0, N, si, su);
    else il_iou_chunk<VW, false>(p, t, c0, N, si, su);
    const float ti = ml_block_sum(si, red_i), tu = ml_block_sum(su, red_u);
    if (threadIdx.x == 0) partial[2 * (long long)blockIdx.x] = ti, partial[2 * (long long)blockIdx.x + 1] = tu;
}

// Second stage: block b adds the nchunk partial pairs of item b (thread t takes chunks t, t + 256, ... in
// order, then the block sum) and writes sums[b] = (I, U) and loss[b] = 1 - I / (U + eps).
__global__ __launch_bounds__(IL_BLOCK) void k_iou_finish(const float* __restrict__ partial, int nchunk, float eps,
                                                         float* __restrict__ sums, float* __restrict__ loss) {
    __shared__ float red_i[IL_BLOCK / 64], red_u[IL_BLOCK / 64];
    const int b = blockIdx.x;
    float si = 0.f, su = 0.f;
    for (int e = threadIdx.x; e < nchunk; e += IL_BLOCK) {
        const float* q = partial + 2 * ((long long)b * nchunk + e);
        si += q[0], su += q[1];
    }
    const float ti = ml_block_sum(si, red_i), tu = ml_block_sum(su, red_u);
    if (threadIdx.x == 0) {
        sums[2 * b] = ti, sums[2 * b + 1] = tu;
        loss[b] = 1.f - ti / (tu + eps);
    }
}

// grad_images[b][i] = -g_b (t_i (U + eps) - I (1 - t_i)) / (U + eps)^2 from the forward's sums: the
// gradient does not depend on p_i itself, so the silhouettes are not read again.
template <int VW, bool FULL>
__device__ __forceinline__ void il_iou_bwd_chunk(const float* __restrict__ t, int c0, int N, float I, float Ue, float scale,
                                                 float* __restrict__ gout) {
    constexpr int U = IL_CHUNK / (IL_BLOCK * VW);
    float tv[U][VW];
    const int i0 = c0 + (int)threadIdx.x * VW;
#pragma unroll
    for (int j = 0; j < U; j++) il_load<VW, FULL>(t, i0 + j * IL_BLOCK * VW, il_valid<VW>(i0 + j * IL_BLOCK * VW, N), tv[j]);
#pragma unroll
    for (int j = 0; j < U; j++) {
        float g[VW];
#pragma unroll
        for (int k = 0; k < VW; k++) g[k] = scale * (tv[j][k] * Ue - I * (1.f - tv[j][k]));
        il_store<VW, FULL>(gout, i0 + j * IL_BLOCK * VW, il_valid<VW>(i0 + j * IL_BLOCK * VW, N), g);
    }
}

template <int VW>
__global__ __launch_bounds__(IL_BLOCK) void k_iou_bwd(const float* __restrict__ targets, long long tstride,
                                                      const float* __restrict__ sums, const float* __restrict__ grad_loss,
                                                      float eps, int N, int nchunk, float* __restrict__ grad_images) {
    const int b = blockIdx.x / nchunk, c = blockIdx.x - b * nchunk;
    const float* t = targets + (long long)b * tstride;
    float* go = grad_images + (long long)b * N;
    const float I = sums[2 * b], Ue = sums[2 * b + 1] + eps;
    const float scale = -grad_loss[b] / (Ue * Ue);
    const int c0 = c * IL_CHUNK;
    if (c0 + IL_CHUNK <= N) il_iou_bwd_chunk<VW, true>(t, c0, N, I, Ue, scale, go);
    else il_iou_bwd_chunk<VW, false>(t, c0, N, I, Ue, scale, go);
}

}  // namespace

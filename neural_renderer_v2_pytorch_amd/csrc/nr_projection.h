// nr_projection.h -- calibrated camera (K, R, t + OpenCV distortion) forward and backward kernels
// Part of nr_raster.hip (one translation unit); see that file, include/nr_raster.h (the formulas) and
// DESIGN.md section 4.
#pragma once

#pragma clang fp contract(off)

namespace {

constexpr int PROJ_BLOCK = 256;  // threads per block; a block never straddles items
constexpr int PROJ_SUMS = 23;    // per-item parameter sums: g_p v^T (9), g_p (3), K rows 0-1 (6), dist (5)
constexpr int PROJ_SLOT = 24;    // floats per (item, block) record of the partial slab

// one item's parameters, wave-uniform
struct ProjItem {
    float R[9], t[3], K[6], d[5];  // d = (k1, k2, p1, p2, k3)
};

// parameter q of item b in the order of the sums: R 0-8, t 9-11, K rows 0-1 12-17, dist 18-22
__device__ __forceinline__ float proj_param(const NrProjectionArgs& a, int b, int q) {
    if (q < 9) return a.R[(long long)b * a.r_batch_stride + q];
    if (q < 12) return a.t[(long long)b * a.t_batch_stride + (q - 9)];
    if (q < 18) return a.K[(long long)b * a.k_batch_stride + (q - 12)];
    return a.dist ? a.dist[(long long)b * a.dist_batch_stride + (q - 18)] : 0.f;
}

// Lane q of the wave loads parameter q (one load per wave and value), and every lane then takes the 23
// values as scalars.  Every lane of the wave must be active here (callers test their bounds afterwards).
__device__ __forceinline__ void proj_load(const NrProjectionArgs& a, int b, ProjItem& m) {
    const int lane = threadIdx.x & 63;
    const int mine = __float_as_int(lane < PROJ_SUMS ? proj_param(a, b, lane) : 0.f);
#pragma unroll
    for (int q = 0; q < 9; q++) m.R[q] = __int_as_float(__builtin_amdgcn_readlane(mine, q));
#pragma unroll
    for (int q = 0; q < 3; q++) m.t[q] = __int_as_float(__builtin_amdgcn_readlane(mine, 9 + q));
#pragma unroll
    for (int q = 0; q < 6; q++) m.K[q] = __int_as_float(__builtin_amdgcn_readlane(mine, 12 + q));
#pragma unroll
    for (int q = 0; q < 5; q++) m.d[q] = __int_as_float(__builtin_amdgcn_readlane(mine, 18 + q));
}

// the forward's intermediates of one vertex
struct ProjPoint {
    float z, zi, xp, yp, r2, rad, xpp, ypp;
};

__device__ __forceinline__ void proj_point(const ProjItem& m, const float w[3], float eps, ProjPoint& p) {
    const float x = ((m.R[0] * w[0] + m.R[1] * w[1]) + m.R[2] * w[2]) + m.t[0];
    const float y = ((m.R[3] * w[0] + m.R[4] * w[1]) + m.R[5] * w[2]) + m.t[1];
    p.z = ((m.R[6] * w[0] + m.R[7] * w[1]) + m.R[8] * w[2]) + m.t[2];
    p.zi = p.z + eps;
    p.xp = x / p.zi;
    p.yp = y / p.zi;
    p.r2 = p.xp * p.xp + p.yp * p.yp;
    const float k1 = m.d[0], k2 = m.d[1], p1 = m.d[2], p2 = m.d[3], k3 = m.d[4];
    p.rad = 1.f + p.r2 * (k1 + p.r2 * (k2 + p.r2 * k3));
    p.xpp = (p.xp * p.rad + 2.f * p1 * p.xp * p.yp) + p2 * (p.r2 + 2.f * p.xp * p.xp);
    p.ypp = (p.yp * p.rad + p1 * (p.r2 + 2.f * p.yp * p.yp)) + 2.f * p2 * p.xp * p.yp;
}

// grid: B * nblk blocks, block (b, blk) projects vertices [256 blk, 256 blk + 256) of item b
__global__ __launch_bounds__(PROJ_BLOCK) void k_proj_fwd(NrProjectionArgs a, int nblk, float* __restrict__ out) {
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int v = blk * PROJ_BLOCK + threadIdx.x;
    ProjItem m;
    proj_load(a, b, m);
    if (v >= a.num_vertices) return;
    const float* vp = a.vertices + (long long)b * a.v_batch_stride + (long long)v * 3;
    const float w[3] = {vp[0], vp[1], vp[2]};
    ProjPoint p;
    proj_point(m, w, a.eps, p);
    const float S = a.orig_size, h = S / 2.f;
    const float u_px = (m.K[0] * p.xpp + m.K[1] * p.ypp) + m.K[2];
    const float v_px = (m.K[3] * p.xpp + m.K[4] * p.ypp) + m.K[5];
    float* o = out + ((long long)b * a.num_vertices + v) * 3;
    o[0] = 2.f * (u_px - h) / S;
    o[1] = 2.f * ((S - v_px) - h) / S;
    o[2] = p.z;
}

__device__ __forceinline__ float proj_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Backward.  grid: (shared mesh ? 1 : B) * nblk blocks; a shared mesh (v_batch_stride 0) loops over the
// items in order and sums their vertex gradients.  Each thread recomputes its vertex's forward, chains
// the gradient to the camera-space point g_p, and writes R^T g_p.  With `slab`, the block also reduces
// the 23 parameter sums of its (item, block) -- across the wave, then across the four waves through LDS in
// wave order -- and stores them into slab[b][blk][0..22] with plain stores: every record that
// k_proj_params reads is written here first, so the slab needs no zero fill and no atomics.
__global__ __launch_bounds__(PROJ_BLOCK) void k_proj_bwd(NrProjectionArgs a, int nblk, const float* __restrict__ go,
                                                         float* __restrict__ gv, float* __restrict__ slab) {
    __shared__ float red[PROJ_BLOCK / 64][PROJ_SLOT];
    const bool shared = a.v_batch_stride == 0;
    const int b0 = shared ? 0 : blockIdx.x / nblk, blk = blockIdx.x - b0 * nblk;
    const int v = blk * PROJ_BLOCK + threadIdx.x;
    const bool live = v < a.num_vertices;
    float w[3] = {0.f, 0.f, 0.f};
    if (live) {
        const float* vp = a.vertices + (long long)b0 * a.v_batch_stride + (long long)v * 3;
        w[0] = vp[0], w[1] = vp[1], w[2] = vp[2];
    }
    const float S = a.orig_size;
    float out[3] = {0.f, 0.f, 0.f};
    for (int bb = 0; bb < (shared ? a.batch_size : 1); bb++) {
        const int b = shared ? bb : b0;
        ProjItem m;
        proj_load(a, b, m);
        float part[PROJ_SUMS];
#pragma unroll
        for (int q = 0; q < PROJ_SUMS; q++) part[q] = 0.f;
        if (live) {
            ProjPoint p;
            proj_point(m, w, a.eps, p);
            const float* g = go + ((long long)b * a.num_vertices + v) * 3;
            const float k1 = m.d[0], k2 = m.d[1], p1 = m.d[2], p2 = m.d[3], k3 = m.d[4];
            // out = (2 (u - S/2) / S, 2 ((S - v) - S/2) / S, z)
            const float gu = 2.f * g[0] / S, gvp = -(2.f * g[1] / S);
            // u = K00 x'' + K01 y'' + K02, v = K10 x'' + K11 y'' + K12
            const float gxpp = m.K[0] * gu + m.K[3] * gvp, gypp = m.K[1] * gu + m.K[4] * gvp;
            // x'' = x' rad + 2 p1 x' y' + p2 (r2 + 2 x'^2), y'' = y' rad + p1 (r2 + 2 y'^2) + 2 p2 x' y'
            const float xy2 = 2.f * p.xp * p.yp;
            const float ax = p.r2 + 2.f * p.xp * p.xp, ay = p.r2 + 2.f * p.yp * p.yp;
            const float grad = gxpp * p.xp + gypp * p.yp;  // d / d rad
            const float drad = k1 + p.r2 * (2.f * k2 + p.r2 * (3.f * k3));
            const float gr2 = (grad * drad + gxpp * p2) + gypp * p1;
            const float gxp = (gxpp * ((p.rad + 2.f * p1 * p.yp) + 4.f * p2 * p.xp) + gypp * (2.f * p2 * p.yp)) + gr2 * (2.f * p.xp);
            const float gyp = (gxpp * (2.f * p1 * p.xp) + gypp * ((p.rad + 4.f * p1 * p.yp) + 2.f * p2 * p.xp)) + gr2 * (2.f * p.yp);
            // x' = x / (z + eps), y' = y / (z + eps); out z = z
            const float gp[3] = {gxp / p.zi, gyp / p.zi, g[2] - (gxp * p.xp + gyp * p.yp) / p.zi};
#pragma unroll
            for (int j = 0; j < 3; j++) out[j] += (gp[0] * m.R[j] + gp[1] * m.R[3 + j]) + gp[2] * m.R[6 + j];
#pragma unroll
            for (int k = 0; k < 3; k++) {
#pragma unroll
                for (int j = 0; j < 3; j++) part[3 * k + j] = gp[k] * w[j];
                part[9 + k] = gp[k];
            }
            part[12] = gu * p.xpp, part[13] = gu * p.ypp, part[14] = gu;
            part[15] = gvp * p.xpp, part[16] = gvp * p.ypp, part[17] = gvp;
            part[18] = grad * p.r2;
            part[19] = grad * (p.r2 * p.r2);
            part[20] = gxpp * xy2 + gypp * ay;
            part[21] = gxpp * ax + gypp * xy2;
            part[22] = grad * ((p.r2 * p.r2) * p.r2);
        }
        if (slab) {
            const int wave = threadIdx.x >> 6;
#pragma unroll
            for (int q = 0; q < PROJ_SUMS; q++) {
                const float s = proj_wave_sum(part[q]);
                if ((threadIdx.x & 63) == 0) red[wave][q] = s;
            }
            __syncthreads();
            if (threadIdx.x < PROJ_SUMS)
                slab[((long long)b * nblk + blk) * PROJ_SLOT + threadIdx.x] =
                    ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
            __syncthreads();  // the next item reuses red
        }
    }
    if (gv && live) {
        float* o = gv + ((long long)b0 * a.num_vertices + v) * 3;
        o[0] = out[0], o[1] = out[1], o[2] = out[2];
    }
}

// Sums the slab in a fixed order and writes the parameter gradients.  Block ob serves output item ob:
// thread (slice = tid / 32, q = tid % 32) adds records slice, slice + 8, ... of sum q, then the eight
// slices are added in slice order.  A per-item parameter sums the nblk records of item ob; a shared one
// (batch stride 0) sums all B * nblk records, items in order, in block 0.
__global__ __launch_bounds__(PROJ_BLOCK) void k_proj_params(NrProjectionArgs a, int nblk, const float* __restrict__ slab,
                                                            float* __restrict__ gK, float* __restrict__ gR,
                                                            float* __restrict__ gt, float* __restrict__ gd) {
    __shared__ float red[PROJ_BLOCK / 32][32];
    const int ob = blockIdx.x, q = threadIdx.x & 31, slice = threadIdx.x >> 5;
    float* dst = nullptr;
    long long stride = 0;
    int off = 0, per = 0;
    if (q < 9) dst = gR, stride = a.r_batch_stride, off = q, per = 9;
    else if (q < 12) dst = gt, stride = a.t_batch_stride, off = q - 9, per = 3;
    else if (q < 18) dst = gK, stride = a.k_batch_stride, off = q - 12, per = 9;
    else if (q < PROJ_SUMS) dst = gd, stride = a.dist_batch_stride, off = q - 18, per = 5;
    const bool shared = stride == 0;
    if (shared && ob > 0) dst = nullptr;  // block 0 writes the shared parameters
    const long long first = shared ? 0 : (long long)ob * nblk;
    const long long count = shared ? (long long)a.batch_size * nblk : nblk;
    float s = 0.f;
    if (dst)
        for (long long e = slice; e < count; e += PROJ_BLOCK / 32) s += slab[(first + e) * PROJ_SLOT + q];
    red[slice][q] = s;
    __syncthreads();
    if (dst && slice == 0) {
        float tot = red[0][q];
#pragma unroll
        for (int k = 1; k < PROJ_BLOCK / 32; k++) tot += red[k][q];
        dst[(long long)ob * per + off] = tot;
    }
    // row 2 of K is not read by the forward
    if (gK && threadIdx.x >= 24 && threadIdx.x < 27 && (a.k_batch_stride != 0 || ob == 0))
        gK[(long long)ob * 9 + 6 + (threadIdx.x - 24)] = 0.f;
}

}  // namespace

// nr_mesh_loss.h -- mesh regularizers: uniform Laplacian loss and dihedral flatten loss, forward and backward
// Part of nr_raster.hip (one translation unit); see that file, include/nr_raster.h (the formulas) and
// DESIGN.md section 4 ("Mesh regularizers").
//
// Conventions (those of nr_projection.h): 256-thread blocks that never straddle an item, plain pointers,
// every output fully written, no float atomics: each loss is the sum of per-block partials added in a
// fixed order, each vertex gradient is gathered by the vertex's own thread through a CSR whose lists
// are ascending.  Losses and gradients are bitwise reproducible from run to run.
//
// Limits (checked by the host entry points): B * ceil(V / 256) and B * ceil(E2 / 256) <= INT_MAX,
// 4 * E2 < 2^31 (edge slots are int32), the neighbour count < 2^31.  The topology arrays are trusted:
// every index in them is below V (slots: below 4 * E2); mesh_loss.py builds them from checked faces.
#pragma once

#pragma clang fp contract(off)

namespace {

constexpr int ML_BLOCK = 256;  // threads per block; a block never straddles items

__device__ __forceinline__ float ml_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum of `term` over the block (every thread of the block calls this), valid in thread 0: across each
// wave, then the four waves in wave order.
__device__ __forceinline__ float ml_block_sum(float term, float* red) {
    const float s = ml_wave_sum(term);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// Second stage of both losses: block b adds the nblk partials of item b -- thread t takes partials
// t, t + 256, ... in order, then the block sum -- and writes loss[b] (0 when nblk == 0).
__global__ __launch_bounds__(ML_BLOCK) void k_mesh_loss_sum(const float* __restrict__ partial, int nblk,
                                                            float* __restrict__ loss) {
    __shared__ float red[ML_BLOCK / 64];
    const int b = blockIdx.x;
    float s = 0.f;
    for (int e = threadIdx.x; e < nblk; e += ML_BLOCK) s += partial[(long long)b * nblk + e];
    const float tot = ml_block_sum(s, red);
    if (threadIdx.x == 0) loss[b] = tot;
}

// ---- Laplacian ----
// grid: B * nblk blocks, block (b, blk) serves vertices [256 blk, 256 blk + 256) of item b.
// delta_i = v_i - (sum of the neighbours, ascending) / |N(i)|, 0 for a vertex without neighbours.
__global__ __launch_bounds__(ML_BLOCK) void k_lap_fwd(const float* __restrict__ vertices, const int32_t* __restrict__ nbr_off,
                                                      const int32_t* __restrict__ nbr_idx, int V, int nblk,
                                                      float* __restrict__ delta, float* __restrict__ partial) {
    __shared__ float red[ML_BLOCK / 64];
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int v = blk * ML_BLOCK + threadIdx.x;
    float term = 0.f;
    if (v < V) {
        const float* vb = vertices + (long long)b * V * 3;
        const int lo = nbr_off[v], hi = nbr_off[v + 1];
        float d[3] = {0.f, 0.f, 0.f};
        if (hi > lo) {
            float s[3] = {0.f, 0.f, 0.f};
            for (int e = lo; e < hi; e++) {
                const float* p = vb + (long long)nbr_idx[e] * 3;
                s[0] += p[0], s[1] += p[1], s[2] += p[2];
            }
            const float n = (float)(hi - lo);
            const float* p = vb + (long long)v * 3;
            d[0] = p[0] - s[0] / n, d[1] = p[1] - s[1] / n, d[2] = p[2] - s[2] / n;
        }
        if (delta) {
            float* o = delta + ((long long)b * V + v) * 3;
            o[0] = d[0], o[1] = d[1], o[2] = d[2];
        }
        term = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    }
    const float tot = ml_block_sum(term, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// grad v_i = 2 g_b (delta_i - sum_{j in N(i)} delta_j / |N(j)|): the neighbour relation is symmetric, so
// the forward's CSR lists the vertices whose delta holds v_i.
__global__ __launch_bounds__(ML_BLOCK) void k_lap_bwd(const float* __restrict__ delta, const int32_t* __restrict__ nbr_off,
                                                      const int32_t* __restrict__ nbr_idx, const float* __restrict__ grad_loss,
                                                      int V, int nblk, float* __restrict__ gv) {
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int v = blk * ML_BLOCK + threadIdx.x;
    if (v >= V) return;
    const float* db = delta + (long long)b * V * 3;
    const float g2 = 2.f * grad_loss[b];
    const int lo = nbr_off[v], hi = nbr_off[v + 1];
    float s[3] = {0.f, 0.f, 0.f};
    for (int e = lo; e < hi; e++) {
        const int j = nbr_idx[e];
        const float n = (float)(nbr_off[j + 1] - nbr_off[j]);  // >= 1: v is a neighbour of j
        const float* p = db + (long long)j * 3;
        s[0] += p[0] / n, s[1] += p[1] / n, s[2] += p[2] / n;
    }
    const float* p = db + (long long)v * 3;
    float* o = gv + ((long long)b * V + v) * 3;
    o[0] = g2 * (p[0] - s[0]), o[1] = g2 * (p[1] - s[1]), o[2] = g2 * (p[2] - s[2]);
}

// ---- flatten ----
__device__ __forceinline__ float ml_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// One edge (v0, v1, v2, v3) at the positions p[0..3]: returns (cos + 1)^2 and, with GRAD, its gradient
// to the four positions in g[0..3] (include/nr_raster.h has the formulas).
template <bool GRAD>
__device__ __forceinline__ float ml_flat_edge(const float p[4][3], float eps, float g[4][3]) {
    float a[3], b1[3], b2[3], c1[3], c2[3];
#pragma unroll
    for (int j = 0; j < 3; j++) a[j] = p[1][j] - p[0][j], b1[j] = p[2][j] - p[0][j], b2[j] = p[3][j] - p[0][j];
    const float la = ml_dot(a, a) + eps;
    const float t1 = ml_dot(a, b1) / la, t2 = ml_dot(a, b2) / la;
#pragma unroll
    for (int j = 0; j < 3; j++) c1[j] = b1[j] - a[j] * t1, c2[j] = b2[j] - a[j] * t2;
    const float n1 = ml_dot(c1, c1) + eps, n2 = ml_dot(c2, c2) + eps;
    const float l12 = sqrtf(n1) * sqrtf(n2);
    const float cs = ml_dot(c1, c2) / l12;
    const float h = cs + 1.f;
    if (GRAD) {
        const float dc = 2.f * h;  // d loss / d cos
        float g1[3], g2[3];        // d loss / d c1, d c2
#pragma unroll
        for (int j = 0; j < 3; j++) {
            g1[j] = dc * (c2[j] / l12 - cs * c1[j] / n1);
            g2[j] = dc * (c1[j] / l12 - cs * c2[j] / n2);
        }
        // c_k = b_k - a t_k, t_k = (a . b_k) / la, la = a . a + eps
        const float u1 = -ml_dot(a, g1) / la, u2 = -ml_dot(a, g2) / la;  // d loss / d (a . b_k)
        const float dla = -(u1 * t1 + u2 * t2);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const float ga = (((b1[j] * u1 + b2[j] * u2) - t1 * g1[j]) - t2 * g2[j]) + 2.f * a[j] * dla;
            const float gb1 = g1[j] + a[j] * u1, gb2 = g2[j] + a[j] * u2;
            g[1][j] = ga, g[2][j] = gb1, g[3][j] = gb2;
            g[0][j] = -((ga + gb1) + gb2);
        }
    }
    return h * h;
}

__device__ __forceinline__ void ml_load_edge(const float* __restrict__ vb, const int32_t* __restrict__ edges, int e, float p[4][3]) {
    const int4 q = *reinterpret_cast<const int4*>(edges + (long long)e * 4);
    const int idx[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float* s = vb + (long long)idx[k] * 3;
        p[k][0] = s[0], p[k][1] = s[1], p[k][2] = s[2];
    }
}

// grid: B * nblk blocks, block (b, blk) serves edges [256 blk, 256 blk + 256) of item b.  With REC the
// edge's gradient record (d loss_e / d v0..v3, 12 floats) goes to records[b][e] for k_flat_bwd_gather.
template <bool REC>
__global__ __launch_bounds__(ML_BLOCK) void k_flat_fwd(const float* __restrict__ vertices, const int32_t* __restrict__ edges, int V,
                                                       int E2, int nblk, float eps, float* __restrict__ records,
                                                       float* __restrict__ partial) {
    __shared__ float red[ML_BLOCK / 64];
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int e = blk * ML_BLOCK + threadIdx.x;
    float term = 0.f;
    if (e < E2) {
        float p[4][3], g[4][3];
        ml_load_edge(vertices + (long long)b * V * 3, edges, e, p);
        term = ml_flat_edge<REC>(p, eps, g);
        if (REC) {
            float4* o = reinterpret_cast<float4*>(records + ((long long)b * E2 + e) * 12);
            o[0] = make_float4(g[0][0], g[0][1], g[0][2], g[1][0]);
            o[1] = make_float4(g[1][1], g[1][2], g[2][0], g[2][1]);
            o[2] = make_float4(g[2][2], g[3][0], g[3][1], g[3][2]);
        }
    }
    const float tot = ml_block_sum(term, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// Vertex gather of the forward's records: grad v = g_b * sum over the vertex's slots 4 e + k, ascending,
// of record[b][e][k].
__global__ __launch_bounds__(ML_BLOCK) void k_flat_bwd_gather(const float* __restrict__ records, const int32_t* __restrict__ edge_off,
                                                              const int32_t* __restrict__ edge_slots,
                                                              const float* __restrict__ grad_loss, int V, int E2, int nblk,
                                                              float* __restrict__ gv) {
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int v = blk * ML_BLOCK + threadIdx.x;
    if (v >= V) return;
    const float* rb = records + (long long)b * E2 * 12;
    float s[3] = {0.f, 0.f, 0.f};
    const int lo = edge_off[v], hi = edge_off[v + 1];
    for (int i = lo; i < hi; i++) {
        const float* r = rb + (long long)edge_slots[i] * 3;
        s[0] += r[0], s[1] += r[1], s[2] += r[2];
    }
    const float gb = grad_loss[b];
    float* o = gv + ((long long)b * V + v) * 3;
    o[0] = gb * s[0], o[1] = gb * s[1], o[2] = gb * s[2];
}

}  // namespace

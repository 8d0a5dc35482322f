// nr_mesh_loss.h -- mesh regularizers: uniform and cotangent Laplacian losses, dihedral flatten loss and edge-length
// loss, forward and backward
// Part of nr_raster.hip (one translation unit); see that file, include/nr_raster.h (the formulas) and
// DESIGN.md section 4 ("Mesh regularizers").
//
// Conventions (those of nr_projection.h): 256-thread blocks that never straddle an item, plain pointers,
// every output fully written, no float atomics: each loss is the sum of per-block partials added in a
// fixed order, each vertex gradient is gathered by the vertex's own thread through a CSR whose lists
// are ascending.  Losses and gradients are bitwise reproducible from run to run.
//
// Limits (checked by the host entry points): B * ceil(V / 256) and B * ceil(E2 / 256) <= INT_MAX,
// 4 * E2 < 2^31 (edge slots are int32), the neighbour count < 2^31; for the cotangent Laplacian also
// B * ceil(F / 256) <= INT_MAX and 3 * F < 2^31 (corners are int32).  The topology arrays are trusted:
// every index in them is below V (slots: below 4 * E2, corners: below 3 * F); topology.py builds them from
// checked faces.
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

// ---- edge length ----
// grid: B * nblk blocks over the vertices, as k_lap_fwd.  Every undirected edge {i, j} is counted once, by
// the thread of its lower vertex: term_i = sum_{j in N(i), j > i} (|v_i - v_j| - L)^2, ascending j.
__global__ __launch_bounds__(ML_BLOCK) void k_edge_fwd(const float* __restrict__ vertices, const int32_t* __restrict__ nbr_off,
                                                       const int32_t* __restrict__ nbr_idx, int V, int nblk, float target,
                                                       float* __restrict__ partial) {
    __shared__ float red[ML_BLOCK / 64];
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int v = blk * ML_BLOCK + threadIdx.x;
    float term = 0.f;
    if (v < V) {
        const float* vb = vertices + (long long)b * V * 3;
        const float* p = vb + (long long)v * 3;
        const float x[3] = {p[0], p[1], p[2]};
        const int hi = nbr_off[v + 1];
        for (int e = nbr_off[v]; e < hi; e++) {
            const int j = nbr_idx[e];
            if (j <= v) continue;
            const float* q = vb + (long long)j * 3;
            const float d[3] = {x[0] - q[0], x[1] - q[1], x[2] - q[2]};
            const float r = sqrtf(ml_dot(d, d)) - target;
            term += r * r;
        }
    }
    const float tot = ml_block_sum(term, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// grad v_i = 2 g_b sum_{j in N(i)} (len_ij - L) / len_ij * (v_i - v_j), recomputed from the vertices; an
// edge of length 0 gives nothing.
__global__ __launch_bounds__(ML_BLOCK) void k_edge_bwd(const float* __restrict__ vertices, const int32_t* __restrict__ nbr_off,
                                                       const int32_t* __restrict__ nbr_idx, const float* __restrict__ grad_loss,
                                                       int V, int nblk, float target, float* __restrict__ gv) {
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int v = blk * ML_BLOCK + threadIdx.x;
    if (v >= V) return;
    const float* vb = vertices + (long long)b * V * 3;
    const float* p = vb + (long long)v * 3;
    const float x[3] = {p[0], p[1], p[2]};
    const float g2 = 2.f * grad_loss[b];
    float s[3] = {0.f, 0.f, 0.f};
    const int hi = nbr_off[v + 1];
    for (int e = nbr_off[v]; e < hi; e++) {
        const float* q = vb + (long long)nbr_idx[e] * 3;
        const float d[3] = {x[0] - q[0], x[1] - q[1], x[2] - q[2]};
        const float len = sqrtf(ml_dot(d, d));
        if (len > 0.f) {
            const float c = (len - target) / len;
            s[0] += c * d[0], s[1] += c * d[1], s[2] += c * d[2];
        }
    }
    float* o = gv + ((long long)b * V + v) * 3;
    o[0] = g2 * s[0], o[1] = g2 * s[1], o[2] = g2 * s[2];
}

// ---- cotangent Laplacian ----
constexpr float ML_COT_MIN_WEIGHT = NR_COT_MIN_WEIGHT;  // a vertex whose weights sum to no more has delta = 0

// 0.5 (a . b) / sqrt(|a x b|^2 + eps) for the edge vectors a = q - p, b = r - p leaving the corner at p
__device__ __forceinline__ float ml_half_cot(const float p[3], const float q[3], const float r[3], float eps) {
    const float a[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]}, b[3] = {r[0] - p[0], r[1] - p[1], r[2] - p[2]};
    const float n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    return 0.5f * ml_dot(a, b) / sqrtf(ml_dot(n, n) + eps);
}

// First pass, grid: B * nblk blocks over the faces: cot[b][3 f + k] = the half-cotangent at corner k of
// face f.  A face with a repeated index gets zeros (no list of nbr_corners names it).
__global__ __launch_bounds__(ML_BLOCK) void k_cot_face(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int V,
                                                       int F, int nblk, float eps, float* __restrict__ cot) {
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int f = blk * ML_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int i0 = faces[(long long)f * 3], i1 = faces[(long long)f * 3 + 1], i2 = faces[(long long)f * 3 + 2];
    float c[3] = {0.f, 0.f, 0.f};
    if (i0 != i1 && i1 != i2 && i0 != i2) {
        const float* vb = vertices + (long long)b * V * 3;
        float p[3][3];
        const int idx[3] = {i0, i1, i2};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float* s = vb + (long long)idx[k] * 3;
            p[k][0] = s[0], p[k][1] = s[1], p[k][2] = s[2];
        }
        c[0] = ml_half_cot(p[0], p[1], p[2], eps);
        c[1] = ml_half_cot(p[1], p[2], p[0], eps);
        c[2] = ml_half_cot(p[2], p[0], p[1], eps);
    }
    float* o = cot + ((long long)b * F + f) * 3;
    o[0] = c[0], o[1] = c[1], o[2] = c[2];
}

// Second pass, grid: B * nblk blocks over the vertices.  Entry e = (i, j) of the neighbour CSR has the
// weight w_e = max(0, sum of cot over nbr_corners[corner_off[e] .. corner_off[e + 1]), ascending): (i, j)
// and (j, i) hold the same list, so w_ij == w_ji bit for bit.  W_i = sum_e w_e (CSR order),
// delta_i = v_i - (sum_e w_e v_j) / W_i when W_i > ML_COT_MIN_WEIGHT, else 0.  w [B, nnz], winv [B, V]
// (1 / W_i, or 0) and delta [B, V, 3] are what the backward reads; each may be NULL.
__global__ __launch_bounds__(ML_BLOCK) void k_cotlap_fwd(const float* __restrict__ vertices, const int32_t* __restrict__ nbr_off,
                                                         const int32_t* __restrict__ nbr_idx,
                                                         const int32_t* __restrict__ corner_off,
                                                         const int32_t* __restrict__ corners, const float* __restrict__ cot, int V,
                                                         int F, int nnz, int nblk, float* __restrict__ w,
                                                         float* __restrict__ winv, float* __restrict__ delta,
                                                         float* __restrict__ partial) {
    __shared__ float red[ML_BLOCK / 64];
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int v = blk * ML_BLOCK + threadIdx.x;
    float term = 0.f;
    if (v < V) {
        const float* vb = vertices + (long long)b * V * 3;
        const float* cb = cot + (long long)b * F * 3;
        const int hi = nbr_off[v + 1];
        float W = 0.f, s[3] = {0.f, 0.f, 0.f};
        for (int e = nbr_off[v]; e < hi; e++) {
            float we = 0.f;
            const int chi = corner_off[e + 1];
            for (int c = corner_off[e]; c < chi; c++) we += cb[corners[c]];
            we = fmaxf(we, 0.f);
            if (w) w[(long long)b * nnz + e] = we;
            const float* q = vb + (long long)nbr_idx[e] * 3;
            W += we;
            s[0] += we * q[0], s[1] += we * q[1], s[2] += we * q[2];
        }
        const bool ok = W > ML_COT_MIN_WEIGHT;
        float d[3] = {0.f, 0.f, 0.f};
        if (ok) {
            const float* p = vb + (long long)v * 3;
            d[0] = p[0] - s[0] / W, d[1] = p[1] - s[1] / W, d[2] = p[2] - s[2] / W;
        }
        if (winv) winv[(long long)b * V + v] = ok ? 1.f / W : 0.f;
        if (delta) {
            float* o = delta + ((long long)b * V + v) * 3;
            o[0] = d[0], o[1] = d[1], o[2] = d[2];
        }
        term = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    }
    const float tot = ml_block_sum(term, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// grad v_k = 2 g_b (delta_k - sum_{i in N(k)} w_ki Winv_i delta_i): k_lap_bwd with the forward's weights,
// which are constants of the backward.  Entry (k, i) of w holds w_ki == w_ik.
__global__ __launch_bounds__(ML_BLOCK) void k_cotlap_bwd(const float* __restrict__ delta, const float* __restrict__ w,
                                                         const float* __restrict__ winv, const int32_t* __restrict__ nbr_off,
                                                         const int32_t* __restrict__ nbr_idx, const float* __restrict__ grad_loss,
                                                         int V, int nnz, int nblk, float* __restrict__ gv) {
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int v = blk * ML_BLOCK + threadIdx.x;
    if (v >= V) return;
    const float* db = delta + (long long)b * V * 3;
    const float* wb = w + (long long)b * nnz;
    const float* ib = winv + (long long)b * V;
    const float g2 = 2.f * grad_loss[b];
    float s[3] = {0.f, 0.f, 0.f};
    const int hi = nbr_off[v + 1];
    for (int e = nbr_off[v]; e < hi; e++) {
        const int j = nbr_idx[e];
        const float c = wb[e] * ib[j];
        const float* p = db + (long long)j * 3;
        s[0] += c * p[0], s[1] += c * p[1], s[2] += c * p[2];
    }
    const float* p = db + (long long)v * 3;
    float* o = gv + ((long long)b * V + v) * 3;
    o[0] = g2 * (p[0] - s[0]), o[1] = g2 * (p[1] - s[1]), o[2] = g2 * (p[2] - s[2]);
}

}  // namespace

// nr_rigid.h -- rigid registration of point sets: the closed-form weighted similarity between corresponding points
// (rigid_align), forward and backward, and the nearest-neighbour pass of point-to-point ICP under a transform
// Part of nr_raster.hip (one translation unit); see that file, include/nr_raster.h (the formulas) and
// DESIGN.md section 4 ("Rigid registration").
//
// Conventions (those of nr_point_loss.h and nr_arap.h, whose ml_wave_sum, arap_rotate and arap_matrix these
// kernels use): 256-thread blocks that never straddle an item, plain pointers, every output fully written, no
// float atomics and one fixed order for every sum: R, t, s, condition, rmse and both gradients are bitwise
// reproducible from run to run, and an item's results do not depend on the batch it is in.
//
// The moments are never accumulated raw.  Pass (a), k_rigid_sums, adds w, w (x - x_0), w (y - y_0) and w dist2
// per chunk of RG_CHUNK points, x_0 and y_0 the item's first pair: the differences are small even where the
// cloud is far from the origin.  Pass (b), k_rigid_moments, first re-sums (a)'s partials -- every block in the
// same order, so all of them hold the same centroid bit for bit -- and adds the centred A and var per chunk.
// Pass (c), k_rigid_solve, one block per item, re-sums both, and its thread 0 runs Horn's quaternion method
// (nr_arap.h's Jacobi sweeps; the two largest eigenvalues left on the diagonal give `condition`).
//
// Limits (checked by the host entry points): N, M >= 1; B <= 65535 (grid.y); B * max(N, M) <= INT_MAX - 4096.
// A nearest index is always inside the target set, whatever the coordinates hold (k_chamfer_nn's argument).
#pragma once

#pragma clang fp contract(off)

namespace {

constexpr int RG_BLOCK = 256;                  // threads per block
constexpr int RG_PER = 4;                      // points per thread of the two moment passes
constexpr int RG_CHUNK = RG_BLOCK * RG_PER;    // points per block of the two moment passes
constexpr int RG_SUMS = 8;                     // pass (a)'s partial: W, w (x - x_0) [3], w (y - y_0) [3], w dist2
constexpr int RG_MOM = 12;                     // pass (b)'s partial: A [9] row-major, var, two unused
constexpr int RG_T = 13;                       // a transform in device memory: R [9] row-major, t [3], s
constexpr int RG_GRAD = 16;                    // the backward's per-item record: gA [9], g_var, g_xbar / W [3], g_ybar / W [3]
// the forward's per-item record, what the backward reads: R [9], A [9], xbar - x_0 [3], ybar - y_0 [3], xbar [3],
// W, var, s, condition, one unused
constexpr int RG_REC = 32;
constexpr int RG_R = 0, RG_A = 9, RG_DX = 18, RG_DY = 21, RG_XBAR = 24, RG_W = 27, RG_VAR = 28, RG_S = 29, RG_COND = 30;
static_assert(RG_REC == NR_RIGID_RECORD_FLOATS && RG_T == NR_RIGID_TRANSFORM_FLOATS, "include/nr_raster.h");

LaunchSlot g_last_icp;

// The correspondences of one call: pair i of item b is (x[b][i], y[b][index ? index[b][i] : i]) with the weight
// (w ? w[b][i] : 1), or 0 where dist2[b][i] > max_d2 when dist2 is given (the ICP rejection).
struct RgPairs {
    const float* x;         // [B, N, 3]
    const float* y;         // item stride y_stride (elements; 0 = shared)
    const float* w;         // [B, N] at the item stride w_stride, or null
    const int32_t* index;   // [B, N], or null
    const float* dist2;     // [B, N], or null
    long long y_stride, w_stride;
    float max_d2;
    int N;
};

// One item's view of the pairs, and its first pair: the origin of pass (a)'s sums.
struct RgItem {
    const float *x, *y, *w, *dist2;
    const int32_t* index;
    float max_d2;
    float x0[3], y0[3];
};

__device__ __forceinline__ RgItem rg_item(const RgPairs& p, int b) {
    RgItem it;
    it.x = p.x + (long long)b * p.N * 3;
    it.y = p.y + (long long)b * p.y_stride;
    it.w = p.w ? p.w + (long long)b * p.w_stride : nullptr;
    it.index = p.index ? p.index + (long long)b * p.N : nullptr;
    it.dist2 = p.dist2 ? p.dist2 + (long long)b * p.N : nullptr;
    it.max_d2 = p.max_d2;
    const float* q = it.y + (long long)(it.index ? it.index[0] : 0) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) it.x0[c] = it.x[c], it.y0[c] = q[c];
    return it;
}

// pair i relative to the first pair, its weight, and its squared distance (0 without dist2)
__device__ __forceinline__ void rg_pair(const RgItem& it, int i, float dx[3], float dy[3], float& w, float& d2) {
    const float* px = it.x + (long long)i * 3;
    const float* py = it.y + (long long)(it.index ? it.index[i] : i) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) dx[c] = px[c] - it.x0[c], dy[c] = py[c] - it.y0[c];
    w = it.w ? it.w[i] : 1.f;
    d2 = 0.f;
    if (it.dist2) {
        d2 = it.dist2[i];
        w = d2 > it.max_d2 ? 0.f : w;
    }
}

// The sums of v[0..K) over the block, in every thread (all of which call this): across each wave (the butterfly
// leaves the same bits in every lane), then the four waves in wave order.
template <int K>
__device__ __forceinline__ void rg_block_sums(float (&v)[K], float (*red)[RG_BLOCK / 64]) {
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = ml_wave_sum(v[k]);
    __syncthreads();  // an earlier use of red has been read
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
}

// An item's nchunk partials of K floats (stride STRIDE) to their sums, in every thread: thread t adds partials
// t, t + 256, ... in order, then the block sum.  The same bits in every block that calls it on the same partials.
template <int K, int STRIDE>
__device__ __forceinline__ void rg_resum(const float* __restrict__ part, int nchunk, float (&tot)[K], float (*red)[RG_BLOCK / 64]) {
#pragma unroll
    for (int k = 0; k < K; k++) tot[k] = 0.f;
    for (int c = threadIdx.x; c < nchunk; c += RG_BLOCK) {
#pragma unroll
        for (int k = 0; k < K; k++) tot[k] += part[(long long)c * STRIDE + k];
    }
    rg_block_sums<K>(tot, red);
}

// ---- pass (a): grid (nchunk, B) ----
__global__ __launch_bounds__(RG_BLOCK) void k_rigid_sums(RgPairs p, int nchunk, float* __restrict__ part_a) {
    __shared__ float red[RG_SUMS][RG_BLOCK / 64];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const RgItem it = rg_item(p, b);
    float acc[RG_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < RG_PER; k++) {
        const int i = chunk * RG_CHUNK + k * RG_BLOCK + (int)threadIdx.x;
        if (i < p.N) {
            float dx[3], dy[3], w, d2;
            rg_pair(it, i, dx, dy, w, d2);
            acc[0] += w;
#pragma unroll
            for (int c = 0; c < 3; c++) acc[1 + c] += w * dx[c], acc[4 + c] += w * dy[c];
            acc[7] += w * d2;
        }
    }
    rg_block_sums<RG_SUMS>(acc, red);
    if (threadIdx.x < RG_SUMS) {
        float v = acc[0];
#pragma unroll
        for (int k = 1; k < RG_SUMS; k++) v = (int)threadIdx.x == k ? acc[k] : v;
        part_a[((long long)b * nchunk + chunk) * RG_SUMS + threadIdx.x] = v;
    }
}

// ---- pass (b): grid (nchunk, B) ----
// A = sum w (y - ybar) (x - xbar)^T and var = sum w |x - xbar|^2 over the chunk, the centroids from (a)'s partials.
// W == 0 (no weight at all) gives partials of 0.
__global__ __launch_bounds__(RG_BLOCK) void k_rigid_moments(RgPairs p, int nchunk, const float* __restrict__ part_a,
                                                            float* __restrict__ part_b) {
    __shared__ float red[RG_MOM][RG_BLOCK / 64];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const RgItem it = rg_item(p, b);
    float tot[RG_SUMS];
    rg_resum<RG_SUMS, RG_SUMS>(part_a + (long long)b * nchunk * RG_SUMS, nchunk, tot, red);
    const bool any = tot[0] > 0.f;
    float cx[3], cy[3];
#pragma unroll
    for (int c = 0; c < 3; c++) cx[c] = any ? tot[1 + c] / tot[0] : 0.f, cy[c] = any ? tot[4 + c] / tot[0] : 0.f;
    float acc[RG_MOM] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < RG_PER; k++) {
        const int i = chunk * RG_CHUNK + k * RG_BLOCK + (int)threadIdx.x;
        if (i < p.N) {
            float dx[3], dy[3], w, d2;
            rg_pair(it, i, dx, dy, w, d2);
#pragma unroll
            for (int c = 0; c < 3; c++) dx[c] -= cx[c], dy[c] -= cy[c];
#pragma unroll
            for (int a = 0; a < 3; a++)
                acc[3 * a] += w * (dy[a] * dx[0]), acc[3 * a + 1] += w * (dy[a] * dx[1]), acc[3 * a + 2] += w * (dy[a] * dx[2]);
            acc[9] += w * ((dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2]);
        }
    }
    rg_block_sums<RG_MOM>(acc, red);
    if (threadIdx.x < RG_MOM) {
        float v = acc[0];
#pragma unroll
        for (int k = 1; k < RG_MOM; k++) v = (int)threadIdx.x == k ? acc[k] : v;
        part_b[((long long)b * nchunk + chunk) * RG_MOM + threadIdx.x] = v;
    }
}

// arap_quaternion (nr_arap.h) with the two largest eigenvalues of Horn's matrix as well: the unit quaternion
// (w, x, y, z) of the rotation R that maximises tr(R S), S row-major, and l1 >= l2, the diagonal the sweeps leave.
// With S = A^T: l1 = s1 + s2 + d s3 and l2 = s1 - s2 - d s3 of A's singular values, d = sign det A.
__device__ __forceinline__ void rigid_quaternion(const float S[9], float q[4], float& l1, float& l2) {
    float n00 = (S[0] + S[4]) + S[8], n11 = (S[0] - S[4]) - S[8], n22 = (S[4] - S[0]) - S[8], n33 = (S[8] - S[0]) - S[4];
    float n01 = S[5] - S[7], n02 = S[6] - S[2], n03 = S[1] - S[3];
    float n12 = S[1] + S[3], n13 = S[6] + S[2], n23 = S[5] + S[7];
    float c0[4] = {1.f, 0.f, 0.f, 0.f}, c1[4] = {0.f, 1.f, 0.f, 0.f}, c2[4] = {0.f, 0.f, 1.f, 0.f}, c3[4] = {0.f, 0.f, 0.f, 1.f};
#pragma unroll
    for (int sweep = 0; sweep < ARAP_SWEEPS; sweep++) {
        arap_rotate(n00, n11, n01, n02, n12, n03, n13, c0, c1);
        arap_rotate(n00, n22, n02, n01, n12, n03, n23, c0, c2);
        arap_rotate(n00, n33, n03, n01, n13, n02, n23, c0, c3);
        arap_rotate(n11, n22, n12, n01, n02, n13, n23, c1, c2);
        arap_rotate(n11, n33, n13, n01, n03, n12, n23, c1, c3);
        arap_rotate(n22, n33, n23, n02, n03, n12, n13, c2, c3);
    }
    // the first of equal diagonal entries, as arap_quaternion takes it
    int best = 0;
    l1 = n00;
    if (n11 > l1) l1 = n11, best = 1;
    if (n22 > l1) l1 = n22, best = 2;
    if (n33 > l1) l1 = n33, best = 3;
    l2 = -INFINITY;
    if (best != 0) l2 = fmaxf(l2, n00);
    if (best != 1) l2 = fmaxf(l2, n11);
    if (best != 2) l2 = fmaxf(l2, n22);
    if (best != 3) l2 = fmaxf(l2, n33);
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = best == 0 ? c0[k] : best == 1 ? c1[k] : best == 2 ? c2[k] : c3[k];
    const float inv = 1.f / sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] *= inv;
}

// What pass (c) writes, each where non-null.
struct RgOut {
    float* R;           // [B, 9]
    float* t;           // [B, 3]
    float* s;           // [B]
    float* transform;   // [B, RG_T]: the ICP's transform in device memory
    float* condition;   // [B]
    float* record;      // [B, RG_REC]
    float* rmse;        // entry b * rmse_stride: sqrt(sum w dist2 / W), 0 when W == 0
    long long rmse_stride;
};

// ---- pass (c): grid B, one block per item; thread 0 solves ----
// mode 0: the solve.  W == 0 gives R = I, t = 0, s = 1 -- or, with keep, leaves `transform` as it is (the ICP
// iteration without a kept pair).  mode 1: the ICP's evaluation pass, rmse alone (part_b is not read).
__global__ __launch_bounds__(RG_BLOCK) void k_rigid_solve(RgPairs p, int nchunk, const float* __restrict__ part_a,
                                                          const float* __restrict__ part_b, int scale, int keep, int mode, RgOut o) {
    __shared__ float red[RG_MOM][RG_BLOCK / 64];
    const int b = blockIdx.x;
    float tot[RG_SUMS], mom[RG_MOM];
    rg_resum<RG_SUMS, RG_SUMS>(part_a + (long long)b * nchunk * RG_SUMS, nchunk, tot, red);
    if (mode == 0) rg_resum<RG_MOM, RG_MOM>(part_b + (long long)b * nchunk * RG_MOM, nchunk, mom, red);
    if (threadIdx.x != 0) return;
    const float W = tot[0];
    const bool any = W > 0.f;
    if (o.rmse) o.rmse[(long long)b * o.rmse_stride] = any ? sqrtf(tot[7] / W) : 0.f;
    if (mode != 0) return;
    const RgItem it = rg_item(p, b);
    float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, A[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float dx[3] = {0.f, 0.f, 0.f}, dy[3] = {0.f, 0.f, 0.f}, xbar[3] = {0.f, 0.f, 0.f}, t[3] = {0.f, 0.f, 0.f};
    float s = 1.f, cond = 0.f, var = 0.f;
    if (any) {
        float ybar[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            dx[c] = tot[1 + c] / W, dy[c] = tot[4 + c] / W;
            xbar[c] = it.x0[c] + dx[c], ybar[c] = it.y0[c] + dy[c];
        }
#pragma unroll
        for (int k = 0; k < 9; k++) A[k] = mom[k];
        var = mom[9];
        const float S[9] = {A[0], A[3], A[6], A[1], A[4], A[7], A[2], A[5], A[8]};  // A^T: R takes x - xbar onto y - ybar
        float q[4], l1, l2;
        rigid_quaternion(S, q, l1, l2);
        arap_matrix(make_float4(q[0], q[1], q[2], q[3]), R);
        cond = (l1 + l2) > 0.f ? fmaxf((l1 - l2) / (l1 + l2), 0.f) : 0.f;
        float tau = 0.f;
#pragma unroll
        for (int k = 0; k < 9; k++) tau += R[k] * A[k];
        s = (scale && var > 0.f) ? tau / var : 1.f;
        float rx[3];
        arap_apply(R, xbar, rx);
#pragma unroll
        for (int c = 0; c < 3; c++) t[c] = ybar[c] - s * rx[c];
    }
    if (o.condition) o.condition[b] = cond;
    if (o.record) {
        float* r = o.record + (long long)b * RG_REC;
#pragma unroll
        for (int k = 0; k < 9; k++) r[RG_R + k] = R[k], r[RG_A + k] = A[k];
#pragma unroll
        for (int c = 0; c < 3; c++) r[RG_DX + c] = dx[c], r[RG_DY + c] = dy[c], r[RG_XBAR + c] = xbar[c];
        r[RG_W] = any ? W : 0.f, r[RG_VAR] = var, r[RG_S] = s, r[RG_COND] = cond, r[31] = 0.f;
    }
    if (o.R) {
#pragma unroll
        for (int k = 0; k < 9; k++) o.R[(long long)b * 9 + k] = R[k];
    }
    if (o.t) {
#pragma unroll
        for (int c = 0; c < 3; c++) o.t[(long long)b * 3 + c] = t[c];
    }
    if (o.s) o.s[b] = s;
    if (o.transform && (any || !keep)) {
        float* T = o.transform + (long long)b * RG_T;
#pragma unroll
        for (int k = 0; k < 9; k++) T[k] = R[k];
#pragma unroll
        for (int c = 0; c < 3; c++) T[9 + c] = t[c];
        T[12] = s;
    }
}

// ---- backward, per item: grid ceil(B / 256), one thread per item ----
// From the upstream gradients gR [B, 9], gt [B, 3], gs [B] (each may be null: zero) and the forward's record:
//   through t = ybar - s R xbar:   g_ybar = gt,  g_xbar = -s R^T gt,  G = gR - s gt xbar^T,  g_s = gs - gt . (R xbar)
//   through s = tr(R^T A) / var:   g_tau = g_s / var,  g_var = -g_s s / var      (scale on and var > 0; else neither)
//   through R:  P = R^T A (symmetrised), K = tr(P) I - P, m = axial(R^T G - G^T R), u = K^{-1} m by the adjugate
//               (u = 0 where condition <= NR_RIGID_MIN_CONDITION),  gA = g_tau R + R [u]x
// and writes gA, g_var, g_xbar / W, g_ybar / W (all 0 where W == 0).
__global__ __launch_bounds__(RG_BLOCK) void k_rigid_bwd_item(const float* __restrict__ record, const float* __restrict__ gR,
                                                             const float* __restrict__ gt, const float* __restrict__ gs, int B,
                                                             int scale, float* __restrict__ gitem) {
    const int b = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (b >= B) return;
    const float* r = record + (long long)b * RG_REC;
    float* o = gitem + (long long)b * RG_GRAD;
    const float W = r[RG_W];
    if (!(W > 0.f)) {
#pragma unroll
        for (int k = 0; k < RG_GRAD; k++) o[k] = 0.f;
        return;
    }
    float R[9], A[9], G[9], xbar[3], g_t[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = r[RG_R + k], A[k] = r[RG_A + k], G[k] = gR ? gR[(long long)b * 9 + k] : 0.f;
#pragma unroll
    for (int c = 0; c < 3; c++) xbar[c] = r[RG_XBAR + c], g_t[c] = gt ? gt[(long long)b * 3 + c] : 0.f;
    const float var = r[RG_VAR], s = r[RG_S], cond = r[RG_COND];
    float rx[3];
    arap_apply(R, xbar, rx);
    float g_s = (gs ? gs[b] : 0.f) - ((g_t[0] * rx[0] + g_t[1] * rx[1]) + g_t[2] * rx[2]);
    const bool scaled = scale && var > 0.f;
    const float g_tau = scaled ? g_s / var : 0.f, g_var = scaled ? -(g_s * s) / var : 0.f;
    float g_xbar[3];
#pragma unroll
    for (int c = 0; c < 3; c++) g_xbar[c] = -s * ((R[c] * g_t[0] + R[3 + c] * g_t[1]) + R[6 + c] * g_t[2]);
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
        for (int c = 0; c < 3; c++) G[3 * a + c] -= s * (g_t[a] * xbar[c]);
    }
    // M = R^T G, P = R^T A
    float M[9], P[9];
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            M[3 * a + c] = (R[a] * G[c] + R[3 + a] * G[3 + c]) + R[6 + a] * G[6 + c];
            P[3 * a + c] = (R[a] * A[c] + R[3 + a] * A[3 + c]) + R[6 + a] * A[6 + c];
        }
    }
    const float m[3] = {M[7] - M[5], M[2] - M[6], M[3] - M[1]};
    const float p01 = 0.5f * (P[1] + P[3]), p02 = 0.5f * (P[2] + P[6]), p12 = 0.5f * (P[5] + P[7]);
    // K = tr(P) I - P
    const float k00 = P[4] + P[8], k11 = P[0] + P[8], k22 = P[0] + P[4], k01 = -p01, k02 = -p02, k12 = -p12;
    float u[3] = {0.f, 0.f, 0.f};
    if (cond > NR_RIGID_MIN_CONDITION) {
        const float a00 = k11 * k22 - k12 * k12, a01 = k02 * k12 - k01 * k22, a02 = k01 * k12 - k02 * k11;
        const float a11 = k00 * k22 - k02 * k02, a12 = k01 * k02 - k00 * k12, a22 = k00 * k11 - k01 * k01;
        const float det = (k00 * a00 + k01 * a01) + k02 * a02;
        if (det != 0.f) {
            u[0] = ((a00 * m[0] + a01 * m[1]) + a02 * m[2]) / det;
            u[1] = ((a01 * m[0] + a11 * m[1]) + a12 * m[2]) / det;
            u[2] = ((a02 * m[0] + a12 * m[1]) + a22 * m[2]) / det;
        }
    }
    // gA = g_tau R + R [u]x,  [u]x = (0, -u2, u1; u2, 0, -u0; -u1, u0, 0)
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float r0 = R[3 * a], r1 = R[3 * a + 1], r2 = R[3 * a + 2];
        o[3 * a] = g_tau * r0 + (r1 * u[2] - r2 * u[1]);
        o[3 * a + 1] = g_tau * r1 + (r2 * u[0] - r0 * u[2]);
        o[3 * a + 2] = g_tau * r2 + (r0 * u[1] - r1 * u[0]);
    }
    o[9] = g_var;
#pragma unroll
    for (int c = 0; c < 3; c++) o[10 + c] = g_xbar[c] / W, o[13 + c] = g_t[c] / W;
}

// ---- backward, per point: grid (ceil(N / 256), B) ----
//   grad x_n = w_n (gA^T (y_n - ybar) + 2 g_var (x_n - xbar) + g_xbar / W)
//   grad y_n = w_n (gA (x_n - xbar) + g_ybar / W)
// the centred points formed as the forward formed them.  Either output may be null.
__global__ __launch_bounds__(RG_BLOCK) void k_rigid_bwd_points(RgPairs p, const float* __restrict__ record,
                                                               const float* __restrict__ gitem, float* __restrict__ grad_x,
                                                               float* __restrict__ grad_y) {
    const int b = blockIdx.y, i = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (i >= p.N) return;
    const RgItem it = rg_item(p, b);
    const float* r = record + (long long)b * RG_REC;
    const float* g = gitem + (long long)b * RG_GRAD;
    float dx[3], dy[3], w, d2;
    rg_pair(it, i, dx, dy, w, d2);
#pragma unroll
    for (int c = 0; c < 3; c++) dx[c] -= r[RG_DX + c], dy[c] -= r[RG_DY + c];
    const long long at = ((long long)b * p.N + i) * 3;
    if (grad_x) {
        const float two = 2.f * g[9];
#pragma unroll
        for (int c = 0; c < 3; c++)
            grad_x[at + c] = w * ((((g[c] * dy[0] + g[3 + c] * dy[1]) + g[6 + c] * dy[2]) + two * dx[c]) + g[10 + c]);
    }
    if (grad_y) {
#pragma unroll
        for (int c = 0; c < 3; c++)
            grad_y[at + c] = w * (((g[3 * c] * dx[0] + g[3 * c + 1] * dx[1]) + g[3 * c + 2] * dx[2]) + g[13 + c]);
    }
}

// ---- the ICP's nearest-neighbour pass ----
// k_chamfer_nn (nr_point_loss.h) in one direction, with the current transform applied to every query as it is
// loaded: q = s (R x) + t, read from transform [B, RG_T].
struct IcpDir {
    const float* x;          // queries [B, nq, 3]
    const float* y;          // targets, item stride y_stride (elements; 0 = shared)
    const float* transform;  // [B, RG_T]
    long long y_stride;
    int nq, nt;
    int nsplit;              // target ranges per query block (1: results go straight to dist2 / index)
    float* dist2;            // [B, nq]  (nsplit == 1)  or the partials [B, nsplit, nq]
    int32_t* index;          // the same shape
};

// grid: (query blocks * nsplit, B).  Block (qb, split) keeps PL_QBLOCK transformed queries in registers and streams
// the targets [lo, hi) of its split through LDS in tiles of PL_TILE; strict < over ascending j, so the lowest index
// wins among exact ties; the tail of a tile is padded with +inf coordinates.
__global__ __launch_bounds__(PL_BLOCK) void k_icp_nn(IcpDir d) {
    __shared__ __attribute__((aligned(16))) float sx[PL_TILE], sy[PL_TILE], sz[PL_TILE];
    const int qb = (int)blockIdx.x / d.nsplit, split = (int)blockIdx.x - qb * d.nsplit;
    const int b = blockIdx.y;
    const float* qp = d.x + (long long)b * d.nq * 3;
    const float* tp = d.y + (long long)b * d.y_stride;
    const float* T = d.transform + (long long)b * RG_T;
    float R[9];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = T[k];
    const float t0 = T[9], t1 = T[10], t2 = T[11], s = T[12];
    const int share = d.nt / d.nsplit, rem = d.nt - share * d.nsplit;
    const int lo = split * share + (split < rem ? split : rem);
    const int hi = lo + share + (split < rem ? 1 : 0);

    float qx[PL_Q], qy[PL_Q], qz[PL_Q], best[PL_Q];
    int bj[PL_Q];
#pragma unroll
    for (int k = 0; k < PL_Q; k++) {
        int i = qb * PL_QBLOCK + k * PL_BLOCK + (int)threadIdx.x;
        if (i >= d.nq) i = d.nq - 1;  // a lane past the end repeats the last query and writes nothing
        const float* p = qp + (long long)i * 3;
        const float e[3] = {p[0], p[1], p[2]};
        float r[3];
        arap_apply(R, e, r);
        qx[k] = s * r[0] + t0, qy[k] = s * r[1] + t1, qz[k] = s * r[2] + t2;
        best[k] = INFINITY, bj[k] = lo;
    }
    for (int j0 = lo; j0 < hi; j0 += PL_TILE) {
        const int cnt = min(PL_TILE, hi - j0);
        const int cnt4 = (cnt + 3) & ~3;
        __syncthreads();  // the previous tile has been read
        for (int e = threadIdx.x; e < cnt4; e += PL_BLOCK) {
            float x = INFINITY, y = INFINITY, z = INFINITY;
            if (e < cnt) {
                const float* p = tp + (long long)(j0 + e) * 3;
                x = p[0], y = p[1], z = p[2];
            }
            sx[e] = x, sy[e] = y, sz[e] = z;
        }
        __syncthreads();
        for (int e = 0; e < cnt4; e += 4) {
            const float4 tx = *reinterpret_cast<const float4*>(sx + e);
            const float4 ty = *reinterpret_cast<const float4*>(sy + e);
            const float4 tz = *reinterpret_cast<const float4*>(sz + e);
            const float ax[4] = {tx.x, tx.y, tx.z, tx.w}, ay[4] = {ty.x, ty.y, ty.z, ty.w}, az[4] = {tz.x, tz.y, tz.z, tz.w};
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = j0 + e + u;
#pragma unroll
                for (int k = 0; k < PL_Q; k++) {
                    const float ex = qx[k] - ax[u], ey = qy[k] - ay[u], ez = qz[k] - az[u];
                    const float d2 = fmaf(ez, ez, fmaf(ey, ey, ex * ex));
                    const bool less = d2 < best[k];
                    best[k] = less ? d2 : best[k];
                    bj[k] = less ? j : bj[k];
                }
            }
        }
    }
    const long long base = ((long long)b * d.nsplit + split) * d.nq;
#pragma unroll
    for (int k = 0; k < PL_Q; k++) {
        const int i = qb * PL_QBLOCK + k * PL_BLOCK + (int)threadIdx.x;
        if (i < d.nq) {
            d.dist2[base + i] = best[k];
            d.index[base + i] = bj[k];
        }
    }
}

}  // namespace

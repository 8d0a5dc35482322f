// nr_skinning.h -- articulated meshes: forward kinematics of a joint tree (pose_transforms) and linear blend
// skinning (skin_vertices), forward and backward
// Part of nr_raster.hip (one translation unit); see that file, include/nr_raster.h (the formulas) and
// DESIGN.md section 4 ("Articulated meshes").
//
// Conventions (those of nr_mesh_loss.h): plain pointers, every output fully written, no float atomics: every
// sum runs in one fixed order, so every result is bitwise reproducible from run to run, and an item's results
// do not depend on the batch it is in.  A 3 x 4 transform is 12 floats, row-major: [R | t].
//
// The pose kernels are about launches, not throughput: one block per item and one thread per joint (at most
// four waves), walking the tree level by level with one barrier per level.  They replace the few hundred
// small launches of a per-joint loop in torch; at B = 1 one block is all the chip sees, and that is fine.
//
// Limits (checked by the host entry points): 1 <= J <= NR_SKIN_MAX_JOINTS; in the skinning kernels also
// 1 <= K <= NR_SKIN_MAX_INFLUENCES and B <= 65535 (an item is a grid row there).  The skeleton and binding arrays are trusted: every joint, vertex and
// slot index in them is in range (topology.py builds them from checked parents, indices and weights).
#pragma once

#pragma clang fp contract(off)

namespace {

constexpr int SK_BLOCK = 256;                     // threads per block of every skinning kernel
constexpr int SK_MAX_J = NR_SKIN_MAX_JOINTS;      // joints: one thread each in the pose kernels
constexpr int SK_MAX_K = NR_SKIN_MAX_INFLUENCES;  // influences per vertex
constexpr int SK_CHUNK = NR_SKIN_CHUNK;           // entries of a joint's CSR row per block of k_skin_bwd_transforms
static_assert(SK_MAX_J <= SK_BLOCK && SK_CHUNK == SK_BLOCK, "one thread per joint, one entry per thread");

// ---- rotations ----
// The coefficients of R = I + a K + b K^2 for t2 = |r|^2, and their derivatives by t2:
//   a = sin t / t, b = (1 - cos t) / t^2 = 2 sin^2(t / 2) / t^2, da/dt2 = (cos t - a) / (2 t2), db/dt2 = (a - 2 b) / (2 t2);
// below NR_RODRIGUES_SERIES the Taylor series in t2 (truncation about 2e-16 at the switch).
struct SkRodrigues {
    float a, b, da, db;
};
__device__ __forceinline__ SkRodrigues sk_rodrigues_coeffs(float t2) {
    SkRodrigues c;
    if (t2 < NR_RODRIGUES_SERIES) {
        c.a = (1.f - t2 / 6.f) + t2 * t2 / 120.f;
        c.b = (0.5f - t2 / 24.f) + t2 * t2 / 720.f;
        c.da = -1.f / 6.f + t2 / 60.f;
        c.db = -1.f / 24.f + t2 / 360.f;
    } else {
        const float t = sqrtf(t2);
        float s, co, sh, ch;
        sincosf(t, &s, &co);
        sincosf(0.5f * t, &sh, &ch);
        const float omc = 2.f * sh * sh;  // 1 - cos t without the cancellation
        c.a = s / t;
        c.b = omc / t2;
        c.da = ((1.f - omc) - c.a) / (2.f * t2);
        c.db = (c.a - 2.f * c.b) / (2.f * t2);
    }
    return c;
}

// R (row-major 3 x 3) of the axis-angle vector r: K = skew(r), K^2 = r r^T - t2 I with its diagonal formed
// as -(the two other squares)
__device__ __forceinline__ void sk_rodrigues(const float r[3], float R[9]) {
    const float x = r[0], y = r[1], z = r[2];
    const float xx = x * x, yy = y * y, zz = z * z;
    const SkRodrigues c = sk_rodrigues_coeffs((xx + yy) + zz);
    const float a = c.a, b = c.b;
    R[0] = 1.f - b * (yy + zz), R[1] = b * (x * y) - a * z, R[2] = b * (x * z) + a * y;
    R[3] = b * (x * y) + a * z, R[4] = 1.f - b * (xx + zz), R[5] = b * (y * z) - a * x;
    R[6] = b * (x * z) - a * y, R[7] = b * (y * z) + a * x, R[8] = 1.f - b * (xx + yy);
}

// gr = the gradient to r of a loss whose gradient to R(r) is g (row-major 3 x 3)
__device__ __forceinline__ void sk_rodrigues_bwd(const float r[3], const float g[9], float gr[3]) {
    const float x = r[0], y = r[1], z = r[2];
    const float xx = x * x, yy = y * y, zz = z * z;
    const SkRodrigues c = sk_rodrigues_coeffs((xx + yy) + zz);
    // through K (K01 = -z, K02 = y, K10 = z, K12 = -x, K20 = -y, K21 = x) and through K^2's entries
    const float s01 = g[1] + g[3], s02 = g[2] + g[6], s12 = g[5] + g[7];
    const float gk0 = g[7] - g[5], gk1 = g[2] - g[6], gk2 = g[3] - g[1];
    const float d0 = g[4] + g[8], d1 = g[0] + g[8], d2 = g[0] + g[4];  // -(yy + zz) on R00, -(xx + zz) on R11, ...
    // d loss / d a = <g, K>, d loss / d b = <g, K^2>
    const float ga = (x * gk0 + y * gk1) + z * gk2;
    const float gb = (((x * y) * s01 + (x * z) * s02) + (y * z) * s12) - ((g[0] * (yy + zz) + g[4] * (xx + zz)) + g[8] * (xx + yy));
    const float gt2 = 2.f * (c.da * ga + c.db * gb);  // through t2 = |r|^2, times the 2 of d t2 / d r = 2 r
    gr[0] = (c.a * gk0 + c.b * ((y * s01 + z * s02) - 2.f * x * d0)) + x * gt2;
    gr[1] = (c.a * gk1 + c.b * ((x * s01 + z * s12) - 2.f * y * d1)) + y * gt2;
    gr[2] = (c.a * gk2 + c.b * ((x * s02 + y * s12) - 2.f * z * d2)) + z * gt2;
}

__device__ __forceinline__ void sk_matmul(const float A[9], const float B[9], float C[9]) {  // C = A B
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[i * 3 + j] = (A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j];
}
__device__ __forceinline__ void sk_matvec(const float A[9], const float v[3], float o[3]) {  // o = A v
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = (A[i * 3] * v[0] + A[i * 3 + 1] * v[1]) + A[i * 3 + 2] * v[2];
}
__device__ __forceinline__ void sk_matvec_t(const float A[9], const float v[3], float o[3]) {  // o = A^T v
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = (A[i] * v[0] + A[3 + i] * v[1]) + A[6 + i] * v[2];
}

// The local rotation of joint j of item b: Rodrigues of pose [B, J, 3], or pose [B, J, 3, 3] as given
__device__ __forceinline__ void sk_local_rotation(const float* __restrict__ pose, int is_matrix, long long bj, float R[9]) {
    if (is_matrix) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = pose[bj * 9 + i];
    } else {
        const float r[3] = {pose[bj * 3], pose[bj * 3 + 1], pose[bj * 3 + 2]};
        sk_rodrigues(r, R);
    }
}

// ---- forward kinematics ----
// grid: B blocks of SK_BLOCK threads.  Thread t serves the joint level_joints[t] (the joints sorted by depth,
// ascending within a level); level l is the threads [level_offsets[l], level_offsets[l + 1]).  G = [G.R | G.t]
// of every joint lives in LDS as 12 planes of SK_MAX_J floats (a level's threads read their parents' and write
// their own: one barrier per level).
//   root: G.R = R_j, G.t = c_j;   else: G.R = G_p.R R_j, G.t = G_p.t + G_p.R (c_j - c_p)
//   transforms[b, j] = [G.R | G.t - G.R c_j],  posed_joints[b, j] = G.t
__global__ __launch_bounds__(SK_BLOCK) void k_pose_fwd(const float* __restrict__ pose, int is_matrix,
                                                       const float* __restrict__ joints, long long joints_bstride,
                                                       const int32_t* __restrict__ parents,
                                                       const int32_t* __restrict__ level_off,
                                                       const int32_t* __restrict__ level_joints, int J, int L,
                                                       float* __restrict__ transforms, float* __restrict__ posed) {
    __shared__ float G[12][SK_MAX_J];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* cb = joints + (long long)b * joints_bstride;
    int j = 0, p = -1;
    float R[9], c[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
    if (t < J) {
        j = level_joints[t];
        p = parents[j];
        sk_local_rotation(pose, is_matrix, (long long)b * J + j, R);
#pragma unroll
        for (int i = 0; i < 3; i++) c[i] = cb[j * 3 + i], d[i] = p < 0 ? c[i] : c[i] - cb[p * 3 + i];
    }
    for (int l = 0; l < L; l++) {
        if (t >= level_off[l] && t < level_off[l + 1]) {
            float GR[9], Gt[3];
            if (p < 0) {
#pragma unroll
                for (int i = 0; i < 9; i++) GR[i] = R[i];
#pragma unroll
                for (int i = 0; i < 3; i++) Gt[i] = d[i];
            } else {
                float PR[9], Pt[3], Rd[3];
#pragma unroll
                for (int i = 0; i < 9; i++) PR[i] = G[i][p];
#pragma unroll
                for (int i = 0; i < 3; i++) Pt[i] = G[9 + i][p];
                sk_matmul(PR, R, GR);
                sk_matvec(PR, d, Rd);
#pragma unroll
                for (int i = 0; i < 3; i++) Gt[i] = Pt[i] + Rd[i];
            }
#pragma unroll
            for (int i = 0; i < 9; i++) G[i][j] = GR[i];
#pragma unroll
            for (int i = 0; i < 3; i++) G[9 + i][j] = Gt[i];
            float Rc[3];
            sk_matvec(GR, c, Rc);
            float* A = transforms + ((long long)b * J + j) * 12;
            float* P = posed + ((long long)b * J + j) * 3;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                A[i * 4] = GR[i * 3], A[i * 4 + 1] = GR[i * 3 + 1], A[i * 4 + 2] = GR[i * 3 + 2];
                A[i * 4 + 3] = Gt[i] - Rc[i];
                P[i] = Gt[i];
            }
        }
        __syncthreads();
    }
}

// Backward of k_pose_fwd, the levels walked deep to shallow.  gA = grad_transforms, gP = grad_posed_joints
// (either may be NULL: zeros).  Joint j, once its children (ascending, through the children CSR) have left
// their messages in LDS:
//   gGt_j = gA.t_j + gP_j + sum_c gGt_c
//   gGR_j = gA.R_j - gA.t_j c_j^T + sum_c (gGR_c R_c^T + gGt_c d_c^T)
//   gR_j  = G_p.R^T gGR_j (root: gGR_j)  -> grad_pose, through Rodrigues for an axis-angle pose
//   gc_j  = G_p.R^T gGt_j (root: gGt_j) - G_j.R^T (gA.t_j + sum_c gGt_c)  -> grad_joints [B, J, 3]
// and its message to its parent is (gGR_j R_j^T + gGt_j d_j^T, gGt_j): 12 planes of LDS.  G.R is read from the
// forward's transforms (their left 3 x 3 blocks).
__global__ __launch_bounds__(SK_BLOCK) void k_pose_bwd(const float* __restrict__ pose, int is_matrix,
                                                       const float* __restrict__ joints, long long joints_bstride,
                                                       const int32_t* __restrict__ parents,
                                                       const int32_t* __restrict__ level_off,
                                                       const int32_t* __restrict__ level_joints,
                                                       const int32_t* __restrict__ child_off,
                                                       const int32_t* __restrict__ children,
                                                       const float* __restrict__ transforms, const float* __restrict__ gA,
                                                       const float* __restrict__ gP, int J, int L,
                                                       float* __restrict__ grad_pose, float* __restrict__ grad_joints) {
    __shared__ float M[12][SK_MAX_J];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* cb = joints + (long long)b * joints_bstride;
    int j = 0, p = -1;
    if (t < J) {
        j = level_joints[t];
        p = parents[j];
    }
    for (int l = L - 1; l >= 0; l--) {
        if (t >= level_off[l] && t < level_off[l + 1]) {
            const long long bj = (long long)b * J + j;
            float c[3], d[3], gAt[3] = {0.f, 0.f, 0.f}, gGR[9], gGt[3], S[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 3; i++) c[i] = cb[j * 3 + i], d[i] = p < 0 ? c[i] : c[i] - cb[p * 3 + i];
            if (gA) {
#pragma unroll
                for (int i = 0; i < 3; i++) gAt[i] = gA[bj * 12 + i * 4 + 3];
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int k = 0; k < 3; k++) gGR[i * 3 + k] = gA[bj * 12 + i * 4 + k] - gAt[i] * c[k];
            } else {
#pragma unroll
                for (int i = 0; i < 9; i++) gGR[i] = 0.f;
            }
#pragma unroll
            for (int i = 0; i < 3; i++) gGt[i] = gP ? gAt[i] + gP[bj * 3 + i] : gAt[i];
            const int hi = child_off[j + 1];
            for (int e = child_off[j]; e < hi; e++) {
                const int ch = children[e];
#pragma unroll
                for (int i = 0; i < 9; i++) gGR[i] += M[i][ch];
#pragma unroll
                for (int i = 0; i < 3; i++) S[i] += M[9 + i][ch];
            }
#pragma unroll
            for (int i = 0; i < 3; i++) gGt[i] += S[i];
            float GR[9], PR[9], gR[9], gd[3], u[3], back[3];
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int k = 0; k < 3; k++) GR[i * 3 + k] = transforms[bj * 12 + i * 4 + k];
            if (p < 0) {
#pragma unroll
                for (int i = 0; i < 9; i++) gR[i] = gGR[i];
#pragma unroll
                for (int i = 0; i < 3; i++) gd[i] = gGt[i];
            } else {
                const long long bp = (long long)b * J + p;
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int k = 0; k < 3; k++) PR[i * 3 + k] = transforms[bp * 12 + i * 4 + k];
                // gR = PR^T gGR
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int k = 0; k < 3; k++) gR[i * 3 + k] = (PR[i] * gGR[k] + PR[3 + i] * gGR[3 + k]) + PR[6 + i] * gGR[6 + k];
                sk_matvec_t(PR, gGt, gd);
            }
#pragma unroll
            for (int i = 0; i < 3; i++) u[i] = gAt[i] + S[i];
            sk_matvec_t(GR, u, back);
            if (grad_joints) {
#pragma unroll
                for (int i = 0; i < 3; i++) grad_joints[bj * 3 + i] = gd[i] - back[i];
            }
            float R[9];
            if (p >= 0 || (grad_pose && !is_matrix)) sk_local_rotation(pose, is_matrix, bj, R);
            if (p >= 0) {
                // the message: gGR R^T + gGt d^T, then gGt
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int k = 0; k < 3; k++)
                        M[i * 3 + k][j] = ((gGR[i * 3] * R[k * 3] + gGR[i * 3 + 1] * R[k * 3 + 1]) + gGR[i * 3 + 2] * R[k * 3 + 2]) + gGt[i] * d[k];
#pragma unroll
                for (int i = 0; i < 3; i++) M[9 + i][j] = gGt[i];
            }
            if (grad_pose) {
                if (is_matrix) {
#pragma unroll
                    for (int i = 0; i < 9; i++) grad_pose[bj * 9 + i] = gR[i];
                } else {
                    const float r[3] = {pose[bj * 3], pose[bj * 3 + 1], pose[bj * 3 + 2]};
                    float gr[3];
                    sk_rodrigues_bwd(r, gR, gr);
#pragma unroll
                    for (int i = 0; i < 3; i++) grad_pose[bj * 3 + i] = gr[i];
                }
            }
        }
        __syncthreads();
    }
}

// ---- linear blend skinning ----
// The item's J transforms into LDS (every thread of the block calls this; ends with a barrier).  Scalar loads: the
// caller's transforms need no more than a float's alignment, and J * 12 floats are no traffic to speak of.
__device__ __forceinline__ void sk_stage(const float* __restrict__ transforms, int J, float4* T) {
    float* dst = reinterpret_cast<float*>(T);
    for (int i = threadIdx.x; i < J * 12; i += SK_BLOCK) dst[i] = transforms[i];
    __syncthreads();
}

// p = A x + t of the staged transform j
__device__ __forceinline__ void sk_apply(const float4* T, int j, const float x[3], float p[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float4 a = T[j * 3 + r];
        p[r] = ((a.x * x[0] + a.y * x[1]) + a.z * x[2]) + a.w;
    }
}

// grid: (ceil(V / SK_BLOCK), B).  out[b, v] = sum_k w[v, k] (A x + t), A = transforms[b, idx[v, k]], k ascending.
// 12-byte loads and stores, consecutive threads on consecutive vertices; the transforms are read from LDS as
// three 16-byte rows (neighbouring vertices mostly share their joints: the reads broadcast).
__global__ __launch_bounds__(SK_BLOCK) void k_skin_fwd(const float* __restrict__ vertices, long long v_bstride,
                                                       const float* __restrict__ transforms,
                                                       const float* __restrict__ weights, const int32_t* __restrict__ indices,
                                                       int V, int J, int K, float* __restrict__ out) {
    __shared__ float4 T[SK_MAX_J * 3];
    const int b = blockIdx.y;
    sk_stage(transforms + (long long)b * J * 12, J, T);
    const int v = blockIdx.x * SK_BLOCK + threadIdx.x;
    if (v >= V) return;
    const float* xp = vertices + (long long)b * v_bstride + (long long)v * 3;
    const float x[3] = {xp[0], xp[1], xp[2]};
    float o[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < K; k++) {
        const float w = weights[(long long)v * K + k];
        float p[3];
        sk_apply(T, indices[(long long)v * K + k], x, p);
        o[0] += w * p[0], o[1] += w * p[1], o[2] += w * p[2];
    }
    float* op = out + ((long long)b * V + v) * 3;
    op[0] = o[0], op[1] = o[1], op[2] = o[2];
}

// One item's share of vertex v's gradients, its transforms staged in T: gx = sum_k w_k A_k.R^T g (k ascending),
// and with gw, gw[k] += g . (A_k x + A_k.t)
__device__ __forceinline__ void sk_bwd_vertex(const float4* T, const float w[SK_MAX_K], const int idx[SK_MAX_K], int K,
                                              const float x[3], const float g[3], float gx[3], float* gw) {
    gx[0] = gx[1] = gx[2] = 0.f;
#pragma unroll
    for (int k = 0; k < SK_MAX_K; k++) {  // unrolled: w, idx and gw stay in registers
        if (k >= K) break;
        const float4 r0 = T[idx[k] * 3], r1 = T[idx[k] * 3 + 1], r2 = T[idx[k] * 3 + 2];
        gx[0] += w[k] * ((r0.x * g[0] + r1.x * g[1]) + r2.x * g[2]);
        gx[1] += w[k] * ((r0.y * g[0] + r1.y * g[1]) + r2.y * g[2]);
        gx[2] += w[k] * ((r0.z * g[0] + r1.z * g[1]) + r2.z * g[2]);
        if (gw) {
            const float p0 = ((r0.x * x[0] + r0.y * x[1]) + r0.z * x[2]) + r0.w;
            const float p1 = ((r1.x * x[0] + r1.y * x[1]) + r1.z * x[2]) + r1.w;
            const float p2 = ((r2.x * x[0] + r2.y * x[1]) + r2.z * x[2]) + r2.w;
            gw[k] += (g[0] * p0 + g[1] * p1) + g[2] * p2;
        }
    }
}

// The gradient to the vertices (and to the weights).
//   LOOP false: grid (ceil(V / SK_BLOCK), B), one thread per (item, vertex): grad_vertices [B, V, 3].
//   LOOP true:  grid (ceil(V / SK_BLOCK), 1), one thread per vertex walks the items in order, staging each
//               item's transforms in turn: what a sum over the batch needs -- grad_vertices [V, 3] of shared
//               vertices (v_bstride == 0), and grad_weights [V, K] (each may be NULL; batched vertices still get
//               their [B, V, 3]).  An item's gx is the same arithmetic either way.
template <bool LOOP>
__global__ __launch_bounds__(SK_BLOCK) void k_skin_bwd_vertices(const float* __restrict__ vertices, long long v_bstride,
                                                                const float* __restrict__ transforms,
                                                                const float* __restrict__ weights,
                                                                const int32_t* __restrict__ indices,
                                                                const float* __restrict__ grad_out, int B, int V, int J, int K,
                                                                float* __restrict__ grad_vertices,
                                                                float* __restrict__ grad_weights) {
    __shared__ float4 T[SK_MAX_J * 3];
    const int v = blockIdx.x * SK_BLOCK + threadIdx.x;
    const bool live = v < V;
    float w[SK_MAX_K];
    int idx[SK_MAX_K];
#pragma unroll
    for (int k = 0; k < SK_MAX_K; k++) {
        const bool have = live && k < K;
        w[k] = have ? weights[(long long)v * K + k] : 0.f;
        idx[k] = have ? indices[(long long)v * K + k] : 0;
    }
    if (!LOOP) {
        const int b = blockIdx.y;
        sk_stage(transforms + (long long)b * J * 12, J, T);
        if (!live) return;
        const float* xp = vertices + (long long)b * v_bstride + (long long)v * 3;
        const float* gp = grad_out + ((long long)b * V + v) * 3;
        const float x[3] = {xp[0], xp[1], xp[2]}, g[3] = {gp[0], gp[1], gp[2]};
        float gx[3];
        sk_bwd_vertex(T, w, idx, K, x, g, gx, nullptr);
        float* o = grad_vertices + ((long long)b * V + v) * 3;
        o[0] = gx[0], o[1] = gx[1], o[2] = gx[2];
    } else {
        float gw[SK_MAX_K], sum[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < SK_MAX_K; k++) gw[k] = 0.f;
        for (int b = 0; b < B; b++) {
            if (b) __syncthreads();  // every thread is done with the item before
            sk_stage(transforms + (long long)b * J * 12, J, T);
            if (!live) continue;
            const float* xp = vertices + (long long)b * v_bstride + (long long)v * 3;
            const float* gp = grad_out + ((long long)b * V + v) * 3;
            const float x[3] = {xp[0], xp[1], xp[2]}, g[3] = {gp[0], gp[1], gp[2]};
            float gx[3];
            sk_bwd_vertex(T, w, idx, K, x, g, gx, grad_weights ? gw : nullptr);
            if (grad_vertices) {
                if (v_bstride) {
                    float* o = grad_vertices + ((long long)b * V + v) * 3;
                    o[0] = gx[0], o[1] = gx[1], o[2] = gx[2];
                } else {
                    sum[0] += gx[0], sum[1] += gx[1], sum[2] += gx[2];
                }
            }
        }
        if (!live) return;
        if (grad_vertices && !v_bstride) {
            float* o = grad_vertices + (long long)v * 3;
            o[0] = sum[0], o[1] = sum[1], o[2] = sum[2];
        }
        if (grad_weights) {
#pragma unroll
            for (int k = 0; k < SK_MAX_K; k++)
                if (k < K) grad_weights[(long long)v * K + k] = gw[k];
        }
    }
}

// The gradient to the transforms, first stage.  grid: (num_chunks, B); a chunk is a run of at most SK_CHUNK
// entries of one joint's row of the joint CSR (the slots of non-zero weight of that joint, by (vertex, slot)).
// Thread i takes entry chunk_begin + i: w g (x) [x; 1], 12 floats; the block adds them in a fixed tree -- xor
// shuffles over the 64 lanes, then the four waves in wave order through LDS -- into partial[b, chunk, 12].
__global__ __launch_bounds__(SK_BLOCK) void k_skin_bwd_transforms(const float* __restrict__ vertices, long long v_bstride,
                                                                  const float* __restrict__ weights,
                                                                  const float* __restrict__ grad_out,
                                                                  const int32_t* __restrict__ entry_vertex,
                                                                  const int32_t* __restrict__ entry_slot,
                                                                  const int32_t* __restrict__ chunk_begin,
                                                                  const int32_t* __restrict__ chunk_end, int V, int K,
                                                                  float* __restrict__ partial) {
    __shared__ float red[SK_BLOCK / 64][12];
    const int ch = blockIdx.x, b = blockIdx.y;
    const int e = chunk_begin[ch] + (int)threadIdx.x;
    float val[12];
#pragma unroll
    for (int i = 0; i < 12; i++) val[i] = 0.f;
    if (e < chunk_end[ch]) {
        const int v = entry_vertex[e];
        const float w = weights[(long long)v * K + entry_slot[e]];
        const float* xp = vertices + (long long)b * v_bstride + (long long)v * 3;
        const float* gp = grad_out + ((long long)b * V + v) * 3;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const float wg = w * gp[r];
            val[r * 4] = wg * xp[0], val[r * 4 + 1] = wg * xp[1], val[r * 4 + 2] = wg * xp[2], val[r * 4 + 3] = wg;
        }
    }
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const float s = ml_wave_sum(val[i]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        const int i = threadIdx.x;
        partial[((long long)b * gridDim.x + ch) * 12 + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
    }
}

// Second stage: one thread per (b, j, 12) adds joint j's chunks in ascending order; a joint without entries
// gets exact zeros.  n = B * J * 12.
__global__ __launch_bounds__(SK_BLOCK) void k_skin_sum(const float* __restrict__ partial,
                                                       const int32_t* __restrict__ joint_chunk_off, long long n, int J,
                                                       int num_chunks, float* __restrict__ grad_transforms) {
    const long long i = (long long)blockIdx.x * SK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % 12);
    const long long bj = i / 12;
    const int j = (int)(bj % J);
    const long long b = bj / J;
    float s = 0.f;
    const int hi = joint_chunk_off[j + 1];
    for (int ch = joint_chunk_off[j]; ch < hi; ch++) s += partial[(b * num_chunks + ch) * 12 + c];
    grad_transforms[i] = s;
}

}  // namespace

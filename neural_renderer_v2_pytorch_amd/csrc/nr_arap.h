// nr_arap.h -- as-rigid-as-possible deformation energy, forward and backward, and the cotangent weights of a
// rest shape as an output of their own
// Part of nr_raster.hip (one translation unit); see that file, include/nr_raster.h (the formulas) and
// DESIGN.md section 4 ("Mesh regularizers").
//
// Conventions (those of nr_mesh_loss.h, whose ML_BLOCK, ml_block_sum and k_mesh_loss_sum these kernels use):
// 256-thread blocks that never straddle an item, one thread per vertex walking its ascending CSR row, plain
// pointers, every output fully written, no float atomics: losses, rotations and gradients are bitwise
// reproducible from run to run.
//
// The best-fitting rotation of a vertex is found by Horn's method: the unit quaternion of the rotation that
// maximises tr(R S) is the eigenvector of the largest eigenvalue of a symmetric 4 x 4 matrix N(S), so the result
// is a proper rotation by construction, also where S is a reflection or has lost rank.  The eigenvector comes
// from cyclic Jacobi sweeps, fully unrolled over named scalars and constant indices: nothing is indexed at run
// time, so everything stays in registers.
//
// Limits (checked by the host entry points): those of nr_mesh_loss.h, and B * ceil(nnz / 256) <= INT_MAX for the
// weights.  The topology arrays are trusted as there.
#pragma once

#pragma clang fp contract(off)

namespace {

constexpr int ARAP_SWEEPS = 6;  // cyclic Jacobi sweeps of the 4 x 4 problem: converged to float32 after 4 to 5

// One Jacobi rotation of the symmetric 4 x 4 matrix A in the (p, q) plane, r and s the two other indices:
// annihilates a_pq, and rotates the columns p and q of the eigenvector matrix (vp, vq).  a_pq == 0 leaves
// everything as it is.  tau may overflow to infinity where a_pq is tiny: t is 0 then, the identity again.
__device__ __forceinline__ void arap_rotate(float& app, float& aqq, float& apq, float& apr, float& aqr, float& aps, float& aqs,
                                            float (&vp)[4], float (&vq)[4]) {
    const bool live = apq != 0.f;
    const float tau = (aqq - app) / (2.f * (live ? apq : 1.f));
    const float root = sqrtf(1.f + tau * tau);
    float t = 1.f / (fabsf(tau) + root);
    t = tau < 0.f ? -t : t;
    t = live ? t : 0.f;
    const float c = 1.f / sqrtf(1.f + t * t), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.f;
    const float pr = apr, qr = aqr, ps = aps, qs = aqs;
    apr = c * pr - s * qr, aqr = s * pr + c * qr;
    aps = c * ps - s * qs, aqs = s * ps + c * qs;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float a = vp[k], b = vq[k];
        vp[k] = c * a - s * b, vq[k] = s * a + c * b;
    }
}

// The unit quaternion (w, x, y, z) of the rotation R that maximises tr(R S), S = sum w e d^T row-major (S[3 a + b]
// = sum w e_a d_b): R takes the rest edges e onto the deformed edges d.  S = 0 gives (1, 0, 0, 0), the identity:
// no rotation is ever applied and the first of the equal diagonal entries is taken.
__device__ __forceinline__ void arap_quaternion(const float S[9], float q[4]) {
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
    float best = n00;
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = c0[k];
    if (n11 > best) {
        best = n11;
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = c1[k];
    }
    if (n22 > best) {
        best = n22;
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = c2[k];
    }
    if (n33 > best) {
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = c3[k];
    }
    // the columns of a product of rotations: of length 1 up to rounding, never 0
    const float inv = 1.f / sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] *= inv;
}

// The rotation matrix, row-major, of the unit quaternion (w, x, y, z); (1, 0, 0, 0) gives the identity exactly.
__device__ __forceinline__ void arap_matrix(const float4 q, float R[9]) {
    const float w = q.x, x = q.y, y = q.z, z = q.w;
    R[0] = 1.f - 2.f * (y * y + z * z), R[1] = 2.f * (x * y - w * z), R[2] = 2.f * (x * z + w * y);
    R[3] = 2.f * (x * y + w * z), R[4] = 1.f - 2.f * (x * x + z * z), R[5] = 2.f * (y * z - w * x);
    R[6] = 2.f * (x * z - w * y), R[7] = 2.f * (y * z + w * x), R[8] = 1.f - 2.f * (x * x + y * y);
}

__device__ __forceinline__ void arap_apply(const float R[9], const float e[3], float o[3]) {
    o[0] = (R[0] * e[0] + R[1] * e[1]) + R[2] * e[2];
    o[1] = (R[3] * e[0] + R[4] * e[1]) + R[5] * e[2];
    o[2] = (R[6] * e[0] + R[7] * e[1]) + R[8] * e[2];
}

// ---- cotangent weights ----
// After k_cot_face (nr_mesh_loss.h) on the same vertices.  grid: B * nblk blocks over the entries of the neighbour
// CSR: w[b][e] = max(0, sum of cot over nbr_corners[corner_off[e] .. corner_off[e + 1]), ascending) -- the sum and
// the clamp of k_cotlap_fwd, so the weights are its weights bit for bit, and w_ij == w_ji bit for bit.
__global__ __launch_bounds__(ML_BLOCK) void k_cot_entry(const int32_t* __restrict__ corner_off, const int32_t* __restrict__ corners,
                                                        const float* __restrict__ cot, int F, int nnz, int nblk,
                                                        float* __restrict__ w) {
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int e = blk * ML_BLOCK + threadIdx.x;
    if (e >= nnz) return;
    const float* cb = cot + (long long)b * F * 3;
    float we = 0.f;
    const int chi = corner_off[e + 1];
    for (int c = corner_off[e]; c < chi; c++) we += cb[corners[c]];
    w[(long long)b * nnz + e] = fmaxf(we, 0.f);
}

// ---- ARAP energy ----
// grid: B * nblk blocks, block (b, blk) serves vertices [256 blk, 256 blk + 256) of item b.  rest and w are read
// at the item strides rest_bs and w_bs (0: shared by the items); w == NULL is the weight 1 for every entry.
//   S_i = sum_{j in N(i)} w_ij e_ij d_ij^T (ascending j),  e_ij = p_i - p_j,  d_ij = q_i - q_j
//   R_i = the rotation maximising tr(R S_i), stored as a unit quaternion in rot[b][i] when rot is given
//   term_i = sum_{j in N(i)} w_ij |d_ij - R_i e_ij|^2 (a second walk of the row)
__global__ __launch_bounds__(ML_BLOCK) void k_arap_fwd(const float* __restrict__ vertices, const float* __restrict__ rest,
                                                       long long rest_bs, const float* __restrict__ w, long long w_bs,
                                                       const int32_t* __restrict__ nbr_off, const int32_t* __restrict__ nbr_idx,
                                                       int V, int nblk, float4* __restrict__ rot, float* __restrict__ partial) {
    __shared__ float red[ML_BLOCK / 64];
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int v = blk * ML_BLOCK + threadIdx.x;
    float term = 0.f;
    if (v < V) {
        const float* qb = vertices + (long long)b * V * 3;
        const float* pb = rest + (long long)b * rest_bs;
        const float* wb = w ? w + (long long)b * w_bs : nullptr;
        const float* s = pb + (long long)v * 3;
        const float p[3] = {s[0], s[1], s[2]};
        s = qb + (long long)v * 3;
        const float x[3] = {s[0], s[1], s[2]};
        const int lo = nbr_off[v], hi = nbr_off[v + 1];
        float S[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int n = lo; n < hi; n++) {
            const int j = nbr_idx[n];
            const float* pj = pb + (long long)j * 3;
            const float* qj = qb + (long long)j * 3;
            const float we = wb ? wb[n] : 1.f;
            const float e[3] = {p[0] - pj[0], p[1] - pj[1], p[2] - pj[2]};
            const float d[3] = {x[0] - qj[0], x[1] - qj[1], x[2] - qj[2]};
            // w (e_a d_b), not (w e_a) d_b: with d == e the two products of a pair (a, b), (b, a) are the same
            // bit for bit, so S is symmetric exactly and an undeformed mesh gets the identity exactly
#pragma unroll
            for (int a = 0; a < 3; a++)
                S[3 * a] += we * (e[a] * d[0]), S[3 * a + 1] += we * (e[a] * d[1]), S[3 * a + 2] += we * (e[a] * d[2]);
        }
        float q[4];
        arap_quaternion(S, q);
        const float4 quat = make_float4(q[0], q[1], q[2], q[3]);
        if (rot) rot[(long long)b * V + v] = quat;
        float R[9];
        arap_matrix(quat, R);
        for (int n = lo; n < hi; n++) {
            const int j = nbr_idx[n];
            const float* pj = pb + (long long)j * 3;
            const float* qj = qb + (long long)j * 3;
            const float we = wb ? wb[n] : 1.f;
            const float e[3] = {p[0] - pj[0], p[1] - pj[1], p[2] - pj[2]};
            float r[3];
            arap_apply(R, e, r);
            r[0] = (x[0] - qj[0]) - r[0], r[1] = (x[1] - qj[1]) - r[1], r[2] = (x[2] - qj[2]) - r[2];
            term += we * ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
        }
    }
    const float tot = ml_block_sum(term, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// grad q_i = 2 g_b sum_{j in N(i)} w_ij (2 d_ij - (R_i + R_j) e_ij), the rotations of the forward taken as
// constants (they maximise: the envelope theorem makes this the exact gradient).  Entry (i, j) of w holds
// w_ij == w_ji.
__global__ __launch_bounds__(ML_BLOCK) void k_arap_bwd(const float* __restrict__ vertices, const float* __restrict__ rest,
                                                       long long rest_bs, const float* __restrict__ w, long long w_bs,
                                                       const float4* __restrict__ rot, const int32_t* __restrict__ nbr_off,
                                                       const int32_t* __restrict__ nbr_idx, const float* __restrict__ grad_loss,
                                                       int V, int nblk, float* __restrict__ gv) {
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int v = blk * ML_BLOCK + threadIdx.x;
    if (v >= V) return;
    const float* qb = vertices + (long long)b * V * 3;
    const float* pb = rest + (long long)b * rest_bs;
    const float* wb = w ? w + (long long)b * w_bs : nullptr;
    const float4* rb = rot + (long long)b * V;
    const float* s = pb + (long long)v * 3;
    const float p[3] = {s[0], s[1], s[2]};
    s = qb + (long long)v * 3;
    const float x[3] = {s[0], s[1], s[2]};
    float Ri[9];
    arap_matrix(rb[v], Ri);
    const float g2 = 2.f * grad_loss[b];
    float acc[3] = {0.f, 0.f, 0.f};
    const int hi = nbr_off[v + 1];
    for (int n = nbr_off[v]; n < hi; n++) {
        const int j = nbr_idx[n];
        const float* pj = pb + (long long)j * 3;
        const float* qj = qb + (long long)j * 3;
        const float we = wb ? wb[n] : 1.f;
        float Rj[9];
        arap_matrix(rb[j], Rj);
#pragma unroll
        for (int k = 0; k < 9; k++) Rj[k] += Ri[k];
        const float e[3] = {p[0] - pj[0], p[1] - pj[1], p[2] - pj[2]};
        float r[3];
        arap_apply(Rj, e, r);
        acc[0] += we * (2.f * (x[0] - qj[0]) - r[0]);
        acc[1] += we * (2.f * (x[1] - qj[1]) - r[1]);
        acc[2] += we * (2.f * (x[2] - qj[2]) - r[2]);
    }
    float* o = gv + ((long long)b * V + v) * 3;
    o[0] = g2 * acc[0], o[1] = g2 * acc[1], o[2] = g2 * acc[2];
}

}  // namespace

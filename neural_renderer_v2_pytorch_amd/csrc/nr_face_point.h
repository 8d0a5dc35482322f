// nr_face_point.h -- face-to-scan distance: for every triangle of a mesh its nearest point of a point set and
// the closest point of the triangle to it, forward and backward (the opposite direction of nr_point_mesh.h)
// Part of nr_raster.hip (one translation unit); see that file, include/nr_raster.h (the formulas) and
// DESIGN.md section 4 ("Point losses").
//
// Only what is this direction's own: the nearest-neighbour loop with its blocking and the two backward kernels.
// The face records, the pair test, the loop's arguments, the finish, the gradient term, the conventions and
// the limits are nr_point_mesh.h's.  Here the vertex gradient is the reproducible one, a gather over each
// vertex's corners in ascending order, and the point gradient is scattered with float atomics (many faces
// share a nearest point).
#pragma once

#pragma clang fp contract(off)

namespace {

constexpr int FP_Q = 1;                       // faces per lane of k_face_point_nn, their records in registers
constexpr int FP_FBLOCK = PL_BLOCK * FP_Q;    // faces per block
constexpr int FP_TILE = 64;                   // points staged in LDS at a time (xyz0, 1 KB): small, so that a few
                                              // thousand points still cut into a range for every CU
// split the points until the launch has this many blocks (the sibling's PM_SPLIT_BLOCKS)
constexpr int FP_SPLIT_BLOCKS = 4096;
static_assert(FP_TILE <= PL_BLOCK, "a tile is staged by one pass of the block, one point per thread");

LaunchSlot g_last_face_point;

// grid: (face blocks * nsplit, B).  Block (fb, split) keeps the records of the FP_FBLOCK faces fb * FP_FBLOCK +
// k * 256 + thread (k < FP_Q) in registers (bc = ac - ab formed once, in float32, as k_point_face_nn's loop
// forms it) and streams the points [lo, hi) of its split through LDS in tiles of FP_TILE.  Every lane reads
// the same point (one 16-byte broadcast read, no bank conflicts) and tests it with pm_pair_dist2.  (best d2,
// best i) starts at (+inf, lo) and advances on a strict < over ascending i: the lowest index wins among exact
// ties, and the index stays inside the range whatever the coordinates hold.
__global__ __launch_bounds__(PL_BLOCK) void k_face_point_nn(PairArgs d) {
    __shared__ float4 spt[FP_TILE];
    const int lin = blockIdx.x;
    const int fb = lin / d.nsplit, split = lin - fb * d.nsplit;
    const int b = blockIdx.y;
    const float* pp = d.points + (long long)b * d.p_stride;
    const float* rp = d.records + (long long)b * d.F * PM_REC;
    // the split's point range: equal shares, the remainder to the first ranges
    const int share = d.N / d.nsplit, rem = d.N - share * d.nsplit;
    const int lo = split * share + (split < rem ? split : rem);
    const int hi = lo + share + (split < rem ? 1 : 0);

    float4 A[FP_Q], AB[FP_Q], AC[FP_Q], GV[FP_Q], GW[FP_Q], NN[FP_Q];
    float bcx[FP_Q], bcy[FP_Q], bcz[FP_Q], best[FP_Q];
    int bi[FP_Q];
#pragma unroll
    for (int k = 0; k < FP_Q; k++) {
        int f = fb * FP_FBLOCK + k * PL_BLOCK + (int)threadIdx.x;
        if (f >= d.F) f = d.F - 1;  // a lane past the end repeats the last face and writes nothing
        const float4* r4 = reinterpret_cast<const float4*>(rp + (long long)f * PM_REC);
        A[k] = r4[0], AB[k] = r4[1], AC[k] = r4[2], GV[k] = r4[3], GW[k] = r4[4], NN[k] = r4[5];
        bcx[k] = AC[k].x - AB[k].x, bcy[k] = AC[k].y - AB[k].y, bcz[k] = AC[k].z - AB[k].z;
        best[k] = INFINITY, bi[k] = lo;
    }
    for (int i0 = lo; i0 < hi; i0 += FP_TILE) {
        const int cnt = min(FP_TILE, hi - i0);
        __syncthreads();  // the previous tile has been read
        if ((int)threadIdx.x < cnt) {
            const float* s = pp + (long long)(i0 + (int)threadIdx.x) * 3;
            spt[threadIdx.x] = make_float4(s[0], s[1], s[2], 0.f);
        }
        __syncthreads();
#pragma unroll 4  // four broadcast reads in flight: a lane has one chain per point, and a small launch few waves to hide a read
        for (int e = 0; e < cnt; e++) {
            const float4 P = spt[e];
            const int i = i0 + e;
#pragma unroll
            for (int k = 0; k < FP_Q; k++) {
                const float d2 = pm_pair_dist2(P.x, P.y, P.z, A[k], AB[k], AC[k], GV[k], GW[k], NN[k], bcx[k], bcy[k], bcz[k]);
                const bool less = d2 < best[k];
                best[k] = less ? d2 : best[k];
                bi[k] = less ? i : bi[k];
            }
        }
    }
    const long long base = ((long long)b * d.nsplit + split) * d.F;
#pragma unroll
    for (int k = 0; k < FP_Q; k++) {
        const int f = fb * FP_FBLOCK + k * PL_BLOCK + (int)threadIdx.x;
        if (f < d.F) {
            d.dist2[base + f] = best[k];
            d.index[base + f] = bi[k];
        }
    }
}

// One thread per (item, vertex): walks the vertex's corners 3 f + k in ascending order (the CSR list of
// topology.vertex_adjacency) and adds -g_b (2 / F) w_fk (p - c_f) of each: no atomics, one fixed order, every
// element written (zeros for a vertex without a face).  grid: (ceil(V / 256), B).
__global__ __launch_bounds__(PL_BLOCK) void k_face_point_bwd_vertices(const float* __restrict__ points, long long p_stride,
                                                                      const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                      const int32_t* __restrict__ corner_offsets,
                                                                      const int32_t* __restrict__ corner_index,
                                                                      const int32_t* __restrict__ point, const float* __restrict__ weights,
                                                                      const float* __restrict__ grad_loss, int V, int F,
                                                                      float* __restrict__ grad_vertices) {
    const int j = blockIdx.x * PL_BLOCK + threadIdx.x, b = blockIdx.y;
    if (j >= V) return;
    const float* pp = points + (long long)b * p_stride;
    const float* vb = vertices + (long long)b * V * 3;
    const float s = grad_loss[b] * (2.f / (float)F);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int e = corner_offsets[j]; e < corner_offsets[j + 1]; e++) {
        const int corner = corner_index[e];
        const int f = corner / 3, k = corner - 3 * f;
        float g[3], w[3];
        const long long n = (long long)b * F + f;
        pm_face_term(pp + (long long)point[n] * 3, vb, faces, weights, n, f, s, g, w);
        const float wk = k == 0 ? w[0] : k == 1 ? w[1] : w[2];
#pragma unroll
        for (int c = 0; c < 3; c++) acc[c] += -(wk * g[c]);
    }
    float* o = grad_vertices + ((long long)b * V + j) * 3;
    o[0] = acc[0], o[1] = acc[1], o[2] = acc[2];
}

// One thread per (item, face): grad_points (zero-filled by the host entry point) += g_b (2 / F) (p - c_f) at the
// face's nearest point, with float atomics.  grid: (ceil(F / 256), B).
__global__ __launch_bounds__(PL_BLOCK) void k_face_point_bwd_points(const float* __restrict__ points, long long p_stride,
                                                                    const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                    const int32_t* __restrict__ point, const float* __restrict__ weights,
                                                                    const float* __restrict__ grad_loss, int N, int V, int F,
                                                                    float* __restrict__ grad_points) {
    const int f = blockIdx.x * PL_BLOCK + threadIdx.x, b = blockIdx.y;
    if (f >= F) return;
    const long long n = (long long)b * F + f;
    float g[3], w[3];
    pm_face_term(points + (long long)b * p_stride + (long long)point[n] * 3, vertices + (long long)b * V * 3, faces, weights, n, f,
                 grad_loss[b] * (2.f / (float)F), g, w);
    float* o = grad_points + ((long long)b * N + point[n]) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) unsafeAtomicAdd(o + c, g[c]);
}

}  // namespace

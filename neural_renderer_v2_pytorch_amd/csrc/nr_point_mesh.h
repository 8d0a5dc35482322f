// nr_point_mesh.h -- point-to-surface distance: for every point its closest point on the closest
// triangle of a mesh, forward and backward; and what the opposite direction (nr_face_point.h: for every
// triangle its nearest point) shares with it: the face records, the pair test, the argument struct of the
// two nearest-neighbour loops, the float64 closest point, the finish kernel and the gradient term.  The
// two directions so choose by the same bits and apply the same degenerate-face rules.
// Part of nr_raster.hip (one translation unit); see that file, include/nr_raster.h (the formulas) and
// DESIGN.md section 4 ("Point losses").
//
// Conventions (those of nr_point_loss.h): 256-thread blocks that never straddle an item, plain pointers,
// every output fully written, no host synchronisation.  The forward uses no float atomics and every sum
// has one fixed order: dist2, the index, weights, the loss and the gradient of the queries' side (the points
// here, the vertices in nr_face_point.h) are bitwise reproducible from run to run.  The other side's gradient
// is scattered with float atomics (as k_sample_points_bwd does): it agrees from run to run up to the order of
// float additions.
//
// Limits (checked by the host entry points), the queries being the points here and the faces in
// nr_face_point.h: N, F, V >= 1; B <= 65535 (grid.y); B * queries <= INT_MAX - 4096, B * targets and 3 B V <=
// INT_MAX.  The saved indices are written by the nearest-neighbour loop / k_chamfer_combine and are always
// inside the targets' range, whatever the coordinates hold (NaN compares false and keeps the first target of
// the range), so the finish and the backward never read out of range.
#pragma once

#pragma clang fp contract(off)

namespace {

constexpr int PM_Q = 4;                       // query points per lane of k_point_face_nn, in registers
constexpr int PM_QBLOCK = PL_BLOCK * PM_Q;    // query points per block
constexpr int PM_TILE = 256;                  // face records staged in LDS at a time (24 KB)
constexpr int PM_REC = 24;                    // floats of a face record (96 bytes: six 16-byte reads)
// split the faces until the launch has this many blocks: 16 per CU, of which the LDS tile lets 6 run at once.
// Measured at 512 / 1536 / 4096: 7.45 / 6.03 / 5.13 ms at the torus cell, 3.00 / 2.51 / 2.30 ms at ico L4 B = 16
// (DESIGN.md section 4); a test costs some sixty dependent VALU instructions, which few waves per SIMD cannot hide.
constexpr int PM_SPLIT_BLOCKS = 4096;
static_assert(PM_REC % 4 == 0, "records are copied and read in 16-byte pieces");

LaunchSlot g_last_point_mesh;

// A face record, as the inner loop reads it (floats):
//    0..2  a            3  1 / |ab|^2      (0 for an edge of zero length: its clamp then stays at the start)
//    4..6  ab           7  1 / |ac|^2
//    8..10 ac          11  1 / |bc|^2
//   12..14 gv          15  lim: 1, or -1 for a degenerate face (the interior test then never passes)
//   16..18 gw          19  unused
//   20..22 n           23  unused
// gv and gw are the dual basis of (ab, ac) in the face's plane: the closest point of the plane to p is
// a + v ab + w ac with v = gv . (p - a), w = gw . (p - a); n is the unit normal.  They are formed in
// float64 from the float32 corners and rounded once, so that a thin face costs one power of its sine,
// not two.
//
// A face is degenerate if it repeats an index or if the float32 cross product of its float32 edges ab
// and ac is exactly zero (coincident or exactly collinear corners).  As a closed set it is then the
// segment between its two most distant corners, which is the union of its three edges: the loop needs
// no other case than "no interior".  (The kernels also treat a face whose float64 det = |ab|^2 |ac|^2 - (ab . ac)^2
// is not positive as degenerate, so that nothing is divided by it; for float32 corners that is the same set
// up to underflow.)
__device__ __forceinline__ bool pm_degenerate(int i0, int i1, int i2, const float* a, const float* b, const float* c) {
    const float ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const float nx = ab[1] * ac[2] - ab[2] * ac[1], ny = ab[2] * ac[0] - ab[0] * ac[2], nz = ab[0] * ac[1] - ab[1] * ac[0];
    return i0 == i1 || i0 == i2 || i1 == i2 || (nx == 0.f && ny == 0.f && nz == 0.f);
}

// One thread per (item, face).  grid: (ceil(F / 256), B).
__global__ __launch_bounds__(PL_BLOCK) void k_point_face_records(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                 int V, int F, float* __restrict__ records) {
    const int f = blockIdx.x * PL_BLOCK + threadIdx.x, b = blockIdx.y;
    if (f >= F) return;
    const float* vb = vertices + (long long)b * V * 3;
    const int i0 = faces[3 * (long long)f], i1 = faces[3 * (long long)f + 1], i2 = faces[3 * (long long)f + 2];
    const float* pa = vb + (long long)i0 * 3;
    const float* pb = vb + (long long)i1 * 3;
    const float* pc = vb + (long long)i2 * 3;
    float r[PM_REC];
#pragma unroll
    for (int k = 0; k < PM_REC; k++) r[k] = 0.f;
    double ab[3], ac[3], bc[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        r[k] = pa[k], r[4 + k] = pb[k] - pa[k], r[8 + k] = pc[k] - pa[k];
        // the loop walks the float32 edges: the edge bc is ac - ab there
        ab[k] = (double)r[4 + k], ac[k] = (double)r[8 + k], bc[k] = (double)(r[8 + k] - r[4 + k]);
    }
    const double d00 = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2], d01 = ab[0] * ac[0] + ab[1] * ac[1] + ab[2] * ac[2],
                 d11 = ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2], dbc = bc[0] * bc[0] + bc[1] * bc[1] + bc[2] * bc[2];
    r[3] = d00 > 0. ? (float)(1. / d00) : 0.f;
    r[7] = d11 > 0. ? (float)(1. / d11) : 0.f;
    r[11] = dbc > 0. ? (float)(1. / dbc) : 0.f;
    const double det = d00 * d11 - d01 * d01;
    if (pm_degenerate(i0, i1, i2, pa, pb, pc) || !(det > 0.)) {
        r[15] = -1.f;
    } else {
        const double n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
        const double inv = 1. / det, rn = 1. / sqrt(det);  // |ab x ac|^2 = det
#pragma unroll
        for (int k = 0; k < 3; k++) {
            r[12 + k] = (float)((d11 * ab[k] - d01 * ac[k]) * inv);
            r[16 + k] = (float)((d00 * ac[k] - d01 * ab[k]) * inv);
            r[20 + k] = (float)(n[k] * rn);
        }
        r[15] = 1.f;
    }
    float4* out = reinterpret_cast<float4*>(records + ((long long)b * F + f) * PM_REC);
#pragma unroll
    for (int k = 0; k < PM_REC / 4; k++) out[k] = make_float4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
}

__device__ __forceinline__ float pm_clamp01(float t) { return fminf(fmaxf(t, 0.f), 1.f); }

// Squared distance from the point o + r to the segment {o + t e, 0 <= t <= 1} (r = p - o), inv = 1 / |e|^2:
// the squared length of r - clamp(r . e inv) e, the difference to a point of the segment itself.
__device__ __forceinline__ float pm_segment(float rx, float ry, float rz, float ex, float ey, float ez, float inv) {
    const float t = pm_clamp01(fmaf(rz, ez, fmaf(ry, ey, rx * ex)) * inv);
    const float dx = fmaf(-t, ex, rx), dy = fmaf(-t, ey, ry), dz = fmaf(-t, ez, rz);
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// The float32 point-face test of both nearest-neighbour loops: the squared distance from the point q to the
// face of one record (A .. NN its six 16-byte pieces, bc = ac - ab in float32).  Branch-free: the least of the
// distances to the three edges and, where the projection falls inside, to the plane.
__device__ __forceinline__ float pm_pair_dist2(float qx, float qy, float qz, const float4& A, const float4& AB, const float4& AC,
                                               const float4& GV, const float4& GW, const float4& NN, float bcx, float bcy,
                                               float bcz) {
    const float px = qx - A.x, py = qy - A.y, pz = qz - A.z;
    const float v = fmaf(pz, GV.z, fmaf(py, GV.y, px * GV.x));
    const float w = fmaf(pz, GW.z, fmaf(py, GW.y, px * GW.x));
    const float h = fmaf(pz, NN.z, fmaf(py, NN.y, px * NN.x));
    const bool inside = (v >= 0.f) & (w >= 0.f) & (v + w <= GV.w);
    const float plane = inside ? h * h : INFINITY;
    const float e0 = pm_segment(px, py, pz, AB.x, AB.y, AB.z, A.w);
    const float e1 = pm_segment(px, py, pz, AC.x, AC.y, AC.z, AB.w);
    const float e2 = pm_segment(px - AB.x, py - AB.y, pz - AB.z, bcx, bcy, bcz, AC.w);
    return fminf(fminf(e0, e1), fminf(e2, plane));
}

// One nearest-neighbour launch of either direction: for every query (a point in k_point_face_nn, a face in
// k_face_point_nn) its nearest target (a face, a point), nq queries per item.
struct PairArgs {
    const float* points;     // [B, N, 3], item stride p_stride (elements; 0 = shared)
    long long p_stride;
    const float* records;    // [B, F, PM_REC], as k_point_face_records writes them
    int N, F;
    int nsplit;              // target ranges per query block (1: results go straight to the final arrays)
    float* dist2;            // [B, nq]  (nsplit == 1)  or the partials [B, nsplit, nq]
    int32_t* index;          // the same shape
};

// grid: (query blocks * nsplit, B).  Block (qb, split) keeps the PM_QBLOCK queries qb * PM_QBLOCK + k * 256 +
// thread (k < PM_Q) in registers and streams the face records [lo, hi) of its split through LDS in tiles
// of PM_TILE (a straight 16-byte copy: the records are stored as the loop reads them).  Every lane reads
// the same record (broadcast reads, no bank conflicts) and evaluates it branch-free: the distance to the
// face is the least of the distances to its three edges and, where the projection falls inside, to its
// plane.  Every candidate is the distance to a point of the face itself, so an error in an edge parameter
// or in (v, w) enters the result only squared.  (best d2, best f) advances on a strict < over ascending f:
// the lowest index wins among exact ties.
__global__ __launch_bounds__(PL_BLOCK) void k_point_face_nn(PairArgs d) {
    __shared__ __attribute__((aligned(16))) float srec[PM_TILE * PM_REC];
    const int lin = blockIdx.x;
    const int qb = lin / d.nsplit, split = lin - qb * d.nsplit;
    const int b = blockIdx.y;
    const float* qp = d.points + (long long)b * d.p_stride;
    const float* rp = d.records + (long long)b * d.F * PM_REC;
    // the split's face range: equal shares, the remainder to the first ranges
    const int share = d.F / d.nsplit, rem = d.F - share * d.nsplit;
    const int lo = split * share + (split < rem ? split : rem);
    const int hi = lo + share + (split < rem ? 1 : 0);

    float qx[PM_Q], qy[PM_Q], qz[PM_Q], best[PM_Q];
    int bf[PM_Q];
#pragma unroll
    for (int k = 0; k < PM_Q; k++) {
        int i = qb * PM_QBLOCK + k * PL_BLOCK + (int)threadIdx.x;
        if (i >= d.N) i = d.N - 1;  // a lane past the end repeats the last query and writes nothing
        const float* p = qp + (long long)i * 3;
        qx[k] = p[0], qy[k] = p[1], qz[k] = p[2];
        best[k] = INFINITY, bf[k] = lo;
    }
    for (int f0 = lo; f0 < hi; f0 += PM_TILE) {
        const int cnt = min(PM_TILE, hi - f0);
        __syncthreads();  // the previous tile has been read
        const float4* src = reinterpret_cast<const float4*>(rp + (long long)f0 * PM_REC);
        for (int e = threadIdx.x; e < cnt * (PM_REC / 4); e += PL_BLOCK) reinterpret_cast<float4*>(srec)[e] = src[e];
        __syncthreads();
        for (int e = 0; e < cnt; e++) {
            const float4* r4 = reinterpret_cast<const float4*>(srec + e * PM_REC);
            const float4 A = r4[0], AB = r4[1], AC = r4[2], GV = r4[3], GW = r4[4], NN = r4[5];
            const float bcx = AC.x - AB.x, bcy = AC.y - AB.y, bcz = AC.z - AB.z;
            const int f = f0 + e;
#pragma unroll
            for (int k = 0; k < PM_Q; k++) {
                const float d2 = pm_pair_dist2(qx[k], qy[k], qz[k], A, AB, AC, GV, GW, NN, bcx, bcy, bcz);
                const bool less = d2 < best[k];
                best[k] = less ? d2 : best[k];
                bf[k] = less ? f : bf[k];
            }
        }
    }
    const long long base = ((long long)b * d.nsplit + split) * d.N;
#pragma unroll
    for (int k = 0; k < PM_Q; k++) {
        const int i = qb * PM_QBLOCK + k * PL_BLOCK + (int)threadIdx.x;
        if (i < d.N) {
            d.dist2[base + i] = best[k];
            d.index[base + i] = bf[k];
        }
    }
}

// Closest point of the segment {o + t e} to o + r in float64: t in [0, 1] and the squared distance.
__device__ __forceinline__ double pm_segment64(const double* r, const double* e, double* t_out) {
    const double ee = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
    double t = ee > 0. ? (r[0] * e[0] + r[1] * e[1] + r[2] * e[2]) / ee : 0.;
    t = fmin(fmax(t, 0.), 1.);
    const double dx = r[0] - t * e[0], dy = r[1] - t * e[1], dz = r[2] - t * e[2];
    *t_out = t;
    return dx * dx + dy * dy + dz * dz;
}

// The float64 closest point of the finish: the closest point of the face (corners pa, pb, pc with the indices
// i0, i1, i2) to p, formed in float64 from the float32 values.  w takes its barycentric weights (unrounded); returns |p - (w0 a + w1 b +
// w2 c)|^2.  A regular face: the plane's closest point where it falls inside, else the nearest of the three
// edges (ab, ac, bc in this order, the first among equals).  A degenerate face (pm_degenerate): its longest edge
// in the same order, the third corner's weight 0; a point (all corners equal) gives (1, 0, 0).
__device__ __forceinline__ double pm_closest64(const float* p, int i0, int i1, int i2, const float* pa, const float* pb,
                                               const float* pc, double* wt) {
    double ab[3], ac[3], bc[3], ap[3], bp[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        ab[k] = (double)pb[k] - (double)pa[k], ac[k] = (double)pc[k] - (double)pa[k], bc[k] = (double)pc[k] - (double)pb[k];
        ap[k] = (double)p[k] - (double)pa[k], bp[k] = (double)p[k] - (double)pb[k];
    }
    const double d00 = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2], d01 = ab[0] * ac[0] + ab[1] * ac[1] + ab[2] * ac[2],
                 d11 = ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2], dbc = bc[0] * bc[0] + bc[1] * bc[1] + bc[2] * bc[2];
    const double det = d00 * d11 - d01 * d01;
    double t0, t1, t2;
    const double e0 = pm_segment64(ap, ab, &t0), e1 = pm_segment64(ap, ac, &t1), e2 = pm_segment64(bp, bc, &t2);
    double w0, w1, w2;
    if (pm_degenerate(i0, i1, i2, pa, pb, pc) || !(det > 0.)) {
        if (d00 >= d11 && d00 >= dbc) w0 = 1. - t0, w1 = t0, w2 = 0.;
        else if (d11 >= dbc) w0 = 1. - t1, w1 = 0., w2 = t1;
        else w0 = 0., w1 = 1. - t2, w2 = t2;
    } else {
        const double d1 = ap[0] * ab[0] + ap[1] * ab[1] + ap[2] * ab[2], d2 = ap[0] * ac[0] + ap[1] * ac[1] + ap[2] * ac[2];
        const double v = (d11 * d1 - d01 * d2) / det, w = (d00 * d2 - d01 * d1) / det;
        if (v >= 0. && w >= 0. && v + w <= 1.) w0 = fmax(1. - v - w, 0.), w1 = v, w2 = w;
        else if (e0 <= e1 && e0 <= e2) w0 = 1. - t0, w1 = t0, w2 = 0.;
        else if (e1 <= e2) w0 = 1. - t1, w1 = 0., w2 = t1;
        else w0 = 0., w1 = 1. - t2, w2 = t2;
    }
    double dd[3];
#pragma unroll
    for (int k = 0; k < 3; k++) dd[k] = (double)p[k] - ((w0 * (double)pa[k] + w1 * (double)pb[k]) + w2 * (double)pc[k]);
    wt[0] = w0, wt[1] = w1, wt[2] = w2;
    return (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2];
}

// The finish of both directions, one thread per (item, query): the closest point of the pair's face to the
// pair's point again, in float64 from the float32 values (the loop's float32 distance only chose the target), so
// that the weights are those of the closest point to rounding, thin faces included.  FaceQuery: the queries are
// the faces and nearest [B, F] holds points ("k_face_point_finish"); else the queries are the points and nearest
// [B, N] holds faces ("k_point_face_finish").  weights = the barycentric weights over the face's corners,
// rounded once; dist2 = |p - (w0 a + w1 b + w2 c)|^2, formed in float64 before the weights are rounded and
// rounded once (pm_closest64 has the rules); index = nearest.  Each of the three may be null.
// grid: (ceil(queries / 256), B).
template <bool FaceQuery>
__global__ __launch_bounds__(PL_BLOCK) void k_pair_finish(const float* __restrict__ points, long long p_stride,
                                                          const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                          const int32_t* __restrict__ nearest, int N, int V, int F,
                                                          float* __restrict__ dist2, int32_t* __restrict__ index,
                                                          float* __restrict__ weights) {
    const int nq = FaceQuery ? F : N;
    const int q = blockIdx.x * PL_BLOCK + threadIdx.x, b = blockIdx.y;
    if (q >= nq) return;
    const long long n = (long long)b * nq + q;
    const int t = nearest[n];
    const int i = FaceQuery ? t : q, f = FaceQuery ? q : t;
    const float* p = points + (long long)b * p_stride + (long long)i * 3;
    const float* vb = vertices + (long long)b * V * 3;
    const int i0 = faces[3 * (long long)f], i1 = faces[3 * (long long)f + 1], i2 = faces[3 * (long long)f + 2];
    double w[3];
    const double d2 = pm_closest64(p, i0, i1, i2, vb + (long long)i0 * 3, vb + (long long)i1 * 3, vb + (long long)i2 * 3, w);
    if (dist2) dist2[n] = (float)d2;
    if (index) index[n] = t;
    if (weights) weights[n * 3] = (float)w[0], weights[n * 3 + 1] = (float)w[1], weights[n * 3 + 2] = (float)w[2];
}

// The gradient term of both directions, s (p - c) of the pair (point p, face f of the mesh vb) saved as row n:
// c = (w0 a + w1 b) + w2 c of the saved weights, which w takes.
__device__ __forceinline__ void pm_face_term(const float* __restrict__ p, const float* __restrict__ vb, const int32_t* __restrict__ faces,
                                             const float* __restrict__ weights, long long n, int f, float s, float* g, float* w) {
    const float* pa = vb + (long long)faces[3 * (long long)f] * 3;
    const float* pb = vb + (long long)faces[3 * (long long)f + 1] * 3;
    const float* pc = vb + (long long)faces[3 * (long long)f + 2] * 3;
    w[0] = weights[n * 3], w[1] = weights[n * 3 + 1], w[2] = weights[n * 3 + 2];
#pragma unroll
    for (int k = 0; k < 3; k++) g[k] = s * (p[k] - ((w[0] * pa[k] + w[1] * pb[k]) + w[2] * pc[k]));
}

// One thread per point: c = w0 a + w1 b + w2 c of the saved face and weights, d = p - c,
// grad_points = g_b (2 / N) d (plain stores, one fixed order), grad_vertices (zero-filled by the host entry
// point) += -g_b (2 / N) w_k d at the face's corners with float atomics.  Either may be null.
// grid: (ceil(N / 256), B).
__global__ __launch_bounds__(PL_BLOCK) void k_point_mesh_bwd(const float* __restrict__ points, long long p_stride,
                                                             const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                             const int32_t* __restrict__ face, const float* __restrict__ weights,
                                                             const float* __restrict__ grad_loss, int N, int V,
                                                             float* __restrict__ grad_points, float* __restrict__ grad_vertices) {
    const int i = blockIdx.x * PL_BLOCK + threadIdx.x, b = blockIdx.y;
    if (i >= N) return;
    const long long n = (long long)b * N + i;
    const int f = face[n];
    const float* p = points + (long long)b * p_stride + (long long)i * 3;
    const int id[3] = {faces[3 * (long long)f], faces[3 * (long long)f + 1], faces[3 * (long long)f + 2]};
    float g[3], w[3];
    pm_face_term(p, vertices + (long long)b * V * 3, faces, weights, n, f, grad_loss[b] * (2.f / (float)N), g, w);
    if (grad_points) {
#pragma unroll
        for (int k = 0; k < 3; k++) grad_points[n * 3 + k] = g[k];
    }
    if (grad_vertices) {
        float* gb = grad_vertices + (long long)b * V * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float* o = gb + (long long)id[k] * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) unsafeAtomicAdd(o + c, -(w[k] * g[c]));
        }
    }
}

}  // namespace

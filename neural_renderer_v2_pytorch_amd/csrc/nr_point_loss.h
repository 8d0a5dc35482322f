// nr_point_loss.h -- 3-D point losses: nearest neighbours / chamfer distance between two point sets, and
// area-weighted surface sampling of a mesh, forward and backward
// Part of nr_raster.hip (one translation unit); see that file, include/nr_raster.h (the formulas) and
// DESIGN.md section 4 ("Point losses").
//
// Conventions (those of nr_mesh_loss.h): 256-thread blocks that never straddle an item, plain pointers,
// every output fully written.  The chamfer kernels use no float atomics and every sum has one fixed
// order: losses and gradients are bitwise reproducible from run to run.  The sampling backward scatters
// with float atomics (as the attribute backward does): its vertex gradient agrees from run to run up to
// the order of float additions.
//
// Limits (checked by the host entry points): N, M, S >= 1; B <= 65535 (grid.y) for the chamfer kernels;
// B * max(N, M) <= INT_MAX - 4096, B * S, B * F and 3 B V <= INT_MAX.  The saved nearest indices are written by k_chamfer_nn / k_chamfer_combine and are
// always inside the other set, whatever the coordinates hold (NaN compares false and keeps the first
// target of the range).
#pragma once

#pragma clang fp contract(off)

namespace {

constexpr int PL_BLOCK = 256;                 // threads per block
constexpr int PL_Q = 4;                       // query points per lane of k_chamfer_nn, in registers
constexpr int PL_QBLOCK = PL_BLOCK * PL_Q;    // query points per block
constexpr int PL_TILE = 1024;                 // targets staged in LDS at a time (structure of arrays, 12 KB)
constexpr int PL_SPLIT_BLOCKS = 512;          // split the targets until a direction has this many blocks
static_assert(PL_TILE % PL_BLOCK == 0 && PL_TILE % 4 == 0, "tile layout");

LaunchSlot g_last_chamfer;

// One direction of a chamfer launch: for every query point its nearest target.
struct PlDir {
    const float* q;        // queries [B, nq, 3], item stride q_stride (elements; 0 = shared)
    const float* t;        // targets [B, nt, 3], item stride t_stride
    long long q_stride, t_stride;
    int nq, nt;
    int nqb;               // query blocks per item: ceil(nq / PL_QBLOCK)
    int nsplit;            // target ranges per query block (1: results go straight to dist2 / index)
    float* dist2;          // [B, nq]  (nsplit == 1)  or the partials [B, nsplit, nq]
    int32_t* index;        // the same shape
};

// grid: (blocks of direction 0 + blocks of direction 1, B).  Block (qb, split) of a direction keeps the
// PL_QBLOCK queries qb * PL_QBLOCK + k * 256 + thread (k < PL_Q) in registers and streams the targets
// [lo, hi) of its split through LDS in tiles of PL_TILE, structure of arrays: every lane reads the same
// four consecutive coordinates (one 16-byte broadcast read per axis and four targets).  (best d2, best j)
// advances on a strict < over ascending j: the lowest index wins among exact ties.  The tail of a tile is
// padded with +inf coordinates, whose distance is +inf and never below the best.
__global__ __launch_bounds__(PL_BLOCK) void k_chamfer_nn(PlDir d0, PlDir d1, int blocks0) {
    __shared__ __attribute__((aligned(16))) float sx[PL_TILE], sy[PL_TILE], sz[PL_TILE];
    const bool second = (int)blockIdx.x >= blocks0;
    const PlDir d = second ? d1 : d0;
    const int lin = second ? (int)blockIdx.x - blocks0 : (int)blockIdx.x;
    const int qb = lin / d.nsplit, split = lin - qb * d.nsplit;
    const int b = blockIdx.y;
    const float* qp = d.q + (long long)b * d.q_stride;
    const float* tp = d.t + (long long)b * d.t_stride;
    // the split's target range: equal shares, the remainder to the first ranges
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
        qx[k] = p[0], qy[k] = p[1], qz[k] = p[2];
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
                    const float dx = qx[k] - ax[u], dy = qy[k] - ay[u], dz = qz[k] - az[u];
                    const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
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

// The split path's second stage: the lexicographic (d2, j) minimum over a query's nsplit partials, in
// ascending split order with a strict < (the ranges ascend, so the lowest index still wins a tie).
// grid: (ceil(nq / 256), B).
__global__ __launch_bounds__(PL_BLOCK) void k_chamfer_combine(const float* __restrict__ pd, const int32_t* __restrict__ pj, int nq,
                                                              int nsplit, float* __restrict__ dist2, int32_t* __restrict__ index) {
    const int i = blockIdx.x * PL_BLOCK + threadIdx.x, b = blockIdx.y;
    if (i >= nq) return;
    const long long base = (long long)b * nsplit * nq + i;
    float best = pd[base];
    int bj = pj[base];
    for (int s = 1; s < nsplit; s++) {
        const float d2 = pd[base + (long long)s * nq];
        const int j = pj[base + (long long)s * nq];
        if (d2 < best) best = d2, bj = j;
    }
    dist2[(long long)b * nq + i] = best;
    index[(long long)b * nq + i] = bj;
}

constexpr int PL_WIDE = 1024;                  // threads of the one-block-per-item kernels (k_chamfer_sum, k_sample_scan)

// Sum of `term` over a PL_WIDE block (every thread calls this), valid in thread 0: across each wave,
// then the sixteen waves in wave order.
__device__ __forceinline__ float pl_wide_sum(float term, float* red) {
    const float s = ml_wave_sum(term);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    float t = red[0];
#pragma unroll
    for (int w = 1; w < PL_WIDE / 64; w++) t += red[w];
    return t;
}

// loss[b] = (sum_i dist2_xy[b, i]) / N + (sum_j dist2_yx[b, j]) / M, either term absent with a null array.
// Block b; thread t adds elements t, t + 1024, ... in order (four loads in flight), then the block sum.
__global__ __launch_bounds__(PL_WIDE) void k_chamfer_sum(const float* __restrict__ dxy, int N, const float* __restrict__ dyx, int M,
                                                         float* __restrict__ loss) {
    __shared__ float red[2][PL_WIDE / 64];
    const int b = blockIdx.x;
    float total = 0.f;
    if (dxy) {
        float s = 0.f;
#pragma unroll 4
        for (int e = threadIdx.x; e < N; e += PL_WIDE) s += dxy[(long long)b * N + e];
        total += pl_wide_sum(s, red[0]) / (float)N;
    }
    if (dyx) {
        float s = 0.f;
#pragma unroll 4
        for (int e = threadIdx.x; e < M; e += PL_WIDE) s += dyx[(long long)b * M + e];
        total += pl_wide_sum(s, red[1]) / (float)M;
    }
    if (threadIdx.x == 0) loss[b] = total;
}

// One side of the backward: the gradient of the points p [B, np, 3] against the other set o [B, no, 3].
//   direct   (own != null):   g_b (2 / np) (p_i - o[own[i]])
//   gathered (other != null): g_b (2 / no) sum over j ascending with other[j] == i of (p_i - o_j)
struct PlSide {
    const float* p;
    const float* o;
    long long p_stride, o_stride;
    int np, no;
    const int32_t* own;    // [B, np] nearest o of every p, or null
    const int32_t* other;  // [B, no] nearest p of every o, or null
    float* grad;           // [B, np, 3], or null: the side is not computed
    int nblk;              // ceil(np / 64)
};

constexpr int PL_BWD_WAVES = 8;                    // waves per block of k_chamfer_bwd: ranges the scan is cut into
constexpr int PL_BWD_BLOCK = 64 * PL_BWD_WAVES;
constexpr int PL_BWD_TILE = 256;                   // indices a wave stages in LDS at a time (four per lane)

// grid: (blocks of side 0 + blocks of side 1, B); a block serves 64 points, one per lane of every wave.
// The gathered term scans the other set's saved index array: wave w takes the w-th of PL_BWD_WAVES equal
// ranges, stages it through its own LDS tile and walks it in ascending order, one integer compare per
// pair (16-byte broadcast reads, four indices each), reading the matching o_j from global memory.  Wave 0
// then adds the waves' sums in wave order: one fixed order, whatever the timing.
__global__ __launch_bounds__(PL_BWD_BLOCK) void k_chamfer_bwd(PlSide s0, PlSide s1, int blocks0, const float* __restrict__ grad_loss) {
    __shared__ __attribute__((aligned(16))) int32_t sj[PL_BWD_WAVES][PL_BWD_TILE];
    __shared__ float part[PL_BWD_WAVES][3][64];
    const bool second = (int)blockIdx.x >= blocks0;
    const PlSide s = second ? s1 : s0;
    const int blk = second ? (int)blockIdx.x - blocks0 : (int)blockIdx.x;
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blk * 64 + lane;
    const bool live = i < s.np;
    const float* pp = s.p + (long long)b * s.p_stride;
    const float* op = s.o + (long long)b * s.o_stride;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) px = pp[(long long)i * 3], py = pp[(long long)i * 3 + 1], pz = pp[(long long)i * 3 + 2];
    float gat[3] = {0.f, 0.f, 0.f};
    if (s.other) {  // uniform over the block, and so is every trip count below: the barriers are safe
        const int32_t* idx = s.other + (long long)b * s.no;
        const int me = live ? i : -1;  // no saved index is negative
        const int seg = (((s.no + PL_BWD_WAVES - 1) / PL_BWD_WAVES) + 3) & ~3;
        const int lo = wave * seg, hi = min(s.no, lo + seg);  // empty when lo >= no
        for (int t0 = 0; t0 < seg; t0 += PL_BWD_TILE) {
            const int j0 = lo + t0;
            __syncthreads();  // the previous tile has been read
            int w4[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = j0 + lane * 4 + u;
                w4[u] = j < hi ? idx[j] : -2;
            }
            *reinterpret_cast<int4*>(&sj[wave][lane * 4]) = make_int4(w4[0], w4[1], w4[2], w4[3]);
            __syncthreads();
            const int cnt = min(PL_BWD_TILE, hi - j0);
            for (int e = 0; e < cnt; e += 4) {
                const int4 v = *reinterpret_cast<const int4*>(&sj[wave][e]);
                const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (w[u] == me) {
                        const float* t = op + (long long)(j0 + e + u) * 3;
                        gat[0] += px - t[0], gat[1] += py - t[1], gat[2] += pz - t[2];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) part[wave][c][lane] = gat[c];
    __syncthreads();
    if (wave != 0 || !live) return;
    float dir[3] = {0.f, 0.f, 0.f};
    if (s.own) {
        const float* t = op + (long long)s.own[(long long)b * s.np + i] * 3;
        dir[0] = px - t[0], dir[1] = py - t[1], dir[2] = pz - t[2];
    }
    const float g = grad_loss[b];
    const float cd = s.own ? g * (2.f / (float)s.np) : 0.f, cg = s.other ? g * (2.f / (float)s.no) : 0.f;
    float* out = s.grad + ((long long)b * s.np + i) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float sum = part[0][c][lane];
#pragma unroll
        for (int w = 1; w < PL_BWD_WAVES; w++) sum += part[w][c][lane];
        out[c] = cd * dir[c] + cg * sum;
    }
}

// ---- surface sampling ----
constexpr int SP_FACES = 4;                        // consecutive faces per thread and chunk of k_sample_scan
constexpr int SP_CHUNK = PL_WIDE * SP_FACES;

__device__ __forceinline__ float sp_face_area(const float* __restrict__ vb, const int32_t* __restrict__ faces, int f) {
    const float* p0 = vb + (long long)faces[3 * (long long)f] * 3;
    const float* p1 = vb + (long long)faces[3 * (long long)f + 1] * 3;
    const float* p2 = vb + (long long)faces[3 * (long long)f + 2] * 3;
    const float a[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, c[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    const float nx = a[1] * c[2] - a[2] * c[1], ny = a[2] * c[0] - a[0] * c[2], nz = a[0] * c[1] - a[1] * c[0];
    return 0.5f * sqrtf((nx * nx + ny * ny) + nz * nz);
}

// Block b scans item b's face areas in chunks of SP_CHUNK: cdf[b, f] = the float32 inclusive prefix sum
// of the areas up to the latest face of positive area at or before f (0 before the first one).  A face of
// zero area so repeats its predecessor's value exactly and the array never decreases, whatever grouping
// the parallel sum used: the running maximum over the positive-area faces' sums is exact.
__global__ __launch_bounds__(PL_WIDE) void k_sample_scan(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int V,
                                                          int F, float* __restrict__ cdf) {
    constexpr int NW = PL_WIDE / 64;
    __shared__ float wsum[2][NW], wmax[2][NW];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* vb = vertices + (long long)b * V * 3;
    float* out = cdf + (long long)b * F;
    float carry = 0.f, cmax = 0.f;
    int buf = 0;
    for (int f0 = 0; f0 < F; f0 += SP_CHUNK, buf ^= 1) {
        const int first = f0 + (int)threadIdx.x * SP_FACES;
        float a[SP_FACES], s[SP_FACES];
        float run = 0.f;
#pragma unroll
        for (int k = 0; k < SP_FACES; k++) {
            a[k] = first + k < F ? sp_face_area(vb, faces, first + k) : 0.f;
            run += a[k];
            s[k] = run;
        }
        // inclusive scan of the thread totals across the wave, then the waves in order
        float inc = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wsum[buf][wave] = inc;
        __syncthreads();
        float before = carry;
        for (int w = 0; w < wave; w++) before += wsum[buf][w];
        const float left = __shfl_up(inc, 1, 64);
        const float excl = lane ? before + left : before;
#pragma unroll
        for (int w = 0; w < NW; w++) carry += wsum[buf][w];
        // running maximum of the positive-area faces' sums
        float m[SP_FACES], mrun = 0.f;
#pragma unroll
        for (int k = 0; k < SP_FACES; k++) {
            mrun = fmaxf(mrun, a[k] > 0.f ? excl + s[k] : 0.f);
            m[k] = mrun;
        }
        float minc = mrun;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float up = __shfl_up(minc, o, 64);
            if (lane >= o) minc = fmaxf(minc, up);
        }
        const float prev = __shfl_up(minc, 1, 64);
        if (lane == 63) wmax[buf][wave] = minc;
        __syncthreads();
        float mbefore = fmaxf(cmax, lane ? prev : 0.f);
        for (int w = 0; w < wave; w++) mbefore = fmaxf(mbefore, wmax[buf][w]);
#pragma unroll
        for (int w = 0; w < NW; w++) cmax = fmaxf(cmax, wmax[buf][w]);
#pragma unroll
        for (int k = 0; k < SP_FACES; k++)
            if (first + k < F) out[first + k] = fmaxf(mbefore, m[k]);
    }
}

// One thread per sample: the smallest f with cdf[f] > u0 * cdf[F - 1] by binary search.  When there is
// none (u0 * total rounded up to the total) the last face of positive area, the smallest f with cdf[f] >=
// total; with a total of 0 face F - 1.  Then the weights (1 - r, r (1 - u2), r u2), r = sqrt(u1), and
// the weighted corner sum.
__global__ __launch_bounds__(PL_BLOCK) void k_sample_points(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                            const float* __restrict__ u, const float* __restrict__ cdf, int V, int F,
                                                            int S, long long total_samples, float* __restrict__ points,
                                                            int32_t* __restrict__ face, float* __restrict__ weights) {
    const long long n = (long long)blockIdx.x * PL_BLOCK + threadIdx.x;
    if (n >= total_samples) return;
    const int b = (int)(n / S);
    const float* c = cdf + (long long)b * F;
    const float* vb = vertices + (long long)b * V * 3;
    const float u0 = u[n * 3], u1 = u[n * 3 + 1], u2 = u[n * 3 + 2];
    const float total = c[F - 1];
    const float t = u0 * total;
    int lo = 0, hi = F;  // the answer is in [lo, hi]; hi == F: none
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    if (lo >= F) {
        lo = F - 1;
        if (total > 0.f) {
            int l = 0, h = F - 1;
            while (l < h) {
                const int mid = (l + h) >> 1;
                if (c[mid] >= total) h = mid;
                else l = mid + 1;
            }
            lo = l;
        }
    }
    const float r = sqrtf(u1);
    const float w0 = 1.f - r, w1 = r * (1.f - u2), w2 = r * u2;
    const float* p0 = vb + (long long)faces[3 * (long long)lo] * 3;
    const float* p1 = vb + (long long)faces[3 * (long long)lo + 1] * 3;
    const float* p2 = vb + (long long)faces[3 * (long long)lo + 2] * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) points[n * 3 + k] = (w0 * p0[k] + w1 * p1[k]) + w2 * p2[k];
    face[n] = lo;
    weights[n * 3] = w0, weights[n * 3 + 1] = w1, weights[n * 3 + 2] = w2;
}

// grad_vertices (zero-filled by the host entry point) += weights[s, k] * grad_points[s] at vertex
// faces[face[s], k]: float atomics.
__global__ __launch_bounds__(PL_BLOCK) void k_sample_points_bwd(const int32_t* __restrict__ faces, const int32_t* __restrict__ face,
                                                                const float* __restrict__ weights, const float* __restrict__ grad_points,
                                                                int V, int S, long long total_samples, float* __restrict__ grad_vertices) {
    const long long n = (long long)blockIdx.x * PL_BLOCK + threadIdx.x;
    if (n >= total_samples) return;
    const int b = (int)(n / S);
    float* gb = grad_vertices + (long long)b * V * 3;
    const int f = face[n];
    const float g[3] = {grad_points[n * 3], grad_points[n * 3 + 1], grad_points[n * 3 + 2]};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float w = weights[n * 3 + k];
        float* o = gb + (long long)faces[3 * (long long)f + k] * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) unsafeAtomicAdd(o + c, w * g[c]);
    }
}

}  // namespace

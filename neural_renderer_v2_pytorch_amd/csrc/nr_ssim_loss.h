// nr_ssim_loss.h -- per-item structural-similarity (SSIM) image loss, forward and backward
// Part of nr_raster.hip (one translation unit); see that file, include/nr_raster.h (the formulas) and
// DESIGN.md section 4 ("Image losses").
//
// Conventions (those of nr_image_loss.h): 256-thread blocks that never straddle an item or a channel, plain
// pointers, every output fully written, no float atomics: the loss is the sum of per-block partials added
// in a fixed order (ml_block_sum, then k_ssim_finish), the gradient is gathered by its own pixel's thread.
// Losses and gradients are bitwise reproducible from run to run.
//
// One block serves one SS_TILE x SS_TILE tile of one channel of one item: of the SSIM map in the forward,
// of the image in the backward.  It stages the tile with its R-pixel halo into LDS (zeros outside the
// source), filters the rows into LDS planes -- a thread takes 4 adjacent outputs of one row, so 4 + 2R
// reads serve 4 (2R + 1)-tap sums -- then the columns into registers -- a thread takes 4 adjacent outputs
// of one column the same way.  R is a template parameter, so both passes unroll, and the window weights
// are kernel arguments: scalar registers.  The filter taps are explicit fused multiply-adds, two planes to
// one packed instruction (x with t, x^2 with t^2; A with Bm) where they pair; everything else keeps the
// operation order written here (fp contract off).
//
// LDS of R = 5 (a 42 x 42 halo): forward 2 halos (42 x 43 floats) + 5 row-filtered planes (42 x 33) =
// 42.2 KB, three blocks per CU; backward 3 + 3 = 38.3 KB, four.  Paired planes lie interleaved (SSLds).  The
// odd pitches keep the reads of both passes free of bank conflicts: 32 consecutive lanes of the row pass
// read 4 rows x 8 column groups, of the column pass one row.
//
// Limits (checked by the host entry points): C H W <= INT_MAX, B C tiles <= INT_MAX.
#pragma once

#pragma clang fp contract(off)

namespace {

constexpr int SS_BLOCK = ML_BLOCK;              // threads per block
constexpr int SS_TILE = 32;                     // output tile edge (NR_SSIM_TILE)
constexpr int SS_PER = SS_TILE * SS_TILE / SS_BLOCK;  // adjacent outputs of one thread, in either pass
constexpr int SS_GROUPS = SS_TILE / SS_PER;     // column groups of a row in the row pass
constexpr int SS_PPITCH = SS_TILE + 1;          // row pitch of a row-filtered plane
constexpr int SS_MAX_R = 5;
static_assert(SS_PER == 4 && SS_BLOCK / SS_TILE * SS_PER == SS_TILE, "a thread takes 4 outputs; 8 x 32 threads cover the tile");

typedef float ss_f2 __attribute__((ext_vector_type(2)));

struct SSArgs {
    const float* images;   // channel c of item b at images + b * istride + c * H * W
    const float* targets;  // the same at tstride (0: shared)
    long long istride, tstride;
    int B, C, H, W;        // images [B, C, H, W]
    int MH, MW;            // the SSIM map: H x W ('same') or (H - 2R) x (W - 2R) ('valid')
    int pad;               // 'same': R, 'valid': 0.  Map pixel m is centred on image pixel m + R - pad
    int ntx, nty;          // tiles of the launch: over the map (forward) or the image (backward)
    float c1, c2;
    ss_f2 g[2 * SS_MAX_R + 1];  // the window, g[0 .. 2R], each weight in both halves (a packed operand as it stands)
};

template <int R>
struct SSDim {
    static constexpr int K = 2 * R + 1;             // taps
    static constexpr int HS = SS_TILE + 2 * R;      // halo edge
    static constexpr int HP = HS + 1;               // halo row pitch (odd)
    static constexpr int NE = HS * HS;              // staged elements per plane
    static constexpr int U = (NE + SS_BLOCK - 1) / SS_BLOCK;  // staging trips
    static constexpr int NI = HS * SS_GROUPS;       // row-pass items: (halo row, column group)
    static constexpr int IN = SS_PER + 2 * R;       // inputs of a thread's 4 adjacent outputs
};

// (block's item-channel, tile origin) of blockIdx.x = (b * C + c) * nty * ntx + ty * ntx + tx
__device__ __forceinline__ void ss_block(const SSArgs& a, int& bc, int& y0, int& x0) {
    const int tiles = a.ntx * a.nty;
    bc = blockIdx.x / tiles;
    const int tile = blockIdx.x - bc * tiles;
    const int ty = tile / a.ntx;
    y0 = ty * SS_TILE, x0 = (tile - ty * a.ntx) * SS_TILE;
}

// out[o] = sum_k g[k] in[o + k], o < 4
template <int R>
__device__ __forceinline__ void ss_taps(const ss_f2 (&g)[2 * SS_MAX_R + 1], const float (&in)[SSDim<R>::IN], float (&out)[SS_PER]) {
#pragma unroll
    for (int o = 0; o < SS_PER; o++) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < SSDim<R>::K; k++) s = fmaf(g[k].x, in[o + k], s);
        out[o] = s;
    }
}

// The same for two planes at once, one in each half of a two-wide vector: one packed fused multiply-add per
// tap serves both.
template <int R>
__device__ __forceinline__ void ss_taps(const ss_f2 (&g)[2 * SS_MAX_R + 1], const ss_f2 (&in)[SSDim<R>::IN], ss_f2 (&out)[SS_PER]) {
#pragma unroll
    for (int o = 0; o < SS_PER; o++) {
        ss_f2 s = {0.f, 0.f};
#pragma unroll
        for (int k = 0; k < SSDim<R>::K; k++) s = __builtin_elementwise_fma(g[k], in[o + k], s);
        out[o] = s;
    }
}

// The LDS of a block.  Planes that are filtered together lie interleaved, so a pair is one 8-byte access:
// forward  halo (x, t)   -> rows_a (G x, G t), rows_b (G x^2, G t^2), rows_c G (x t)
// backward halo (A, Bm), halo_c Cm -> rows_a (G A, G Bm), rows_c G Cm           (G: the row filter alone)
template <int R, bool FWD>
struct SSLds {
    ss_f2 halo[SSDim<R>::HS * SSDim<R>::HP];
    float halo_c[FWD ? 1 : SSDim<R>::HS * SSDim<R>::HP];
    ss_f2 rows_a[SSDim<R>::HS * SS_PPITCH];
    ss_f2 rows_b[FWD ? SSDim<R>::HS * SS_PPITCH : 1];
    float rows_c[SSDim<R>::HS * SS_PPITCH];
};

// Row pass: every halo row, the tile's 32 columns.
template <int R, bool FWD>
__device__ __forceinline__ void ss_row_pass(const SSArgs& a, SSLds<R, FWD>& l) {
    using D = SSDim<R>;
    for (int it = threadIdx.x; it < D::NI; it += SS_BLOCK) {
        const int row = it / SS_GROUPS, c0 = (it - row * SS_GROUPS) * SS_PER;
        const int h = row * D::HP + c0, r = row * SS_PPITCH + c0;
        ss_f2 p[D::IN], o2[SS_PER];
        float s[D::IN], o1[SS_PER];
#pragma unroll
        for (int k = 0; k < D::IN; k++) {
            p[k] = l.halo[h + k];
            s[k] = FWD ? p[k].x * p[k].y : l.halo_c[h + k];
        }
        ss_taps<R>(a.g, p, o2);
#pragma unroll
        for (int o = 0; o < SS_PER; o++) l.rows_a[r + o] = o2[o];
        if constexpr (FWD) {
#pragma unroll
            for (int k = 0; k < D::IN; k++) p[k] = p[k] * p[k];
            ss_taps<R>(a.g, p, o2);
#pragma unroll
            for (int o = 0; o < SS_PER; o++) l.rows_b[r + o] = o2[o];
        }
        ss_taps<R>(a.g, s, o1);
#pragma unroll
        for (int o = 0; o < SS_PER; o++) l.rows_c[r + o] = o1[o];
    }
}

// Column pass of one row-filtered plane (of floats or of pairs): out[o] = the filtered value at tile row
// r0 + o, column tx.
template <int R, typename V>
__device__ __forceinline__ void ss_col_pass(const SSArgs& a, const V* __restrict__ rows, int r0, int tx, V (&out)[SS_PER]) {
    V in[SSDim<R>::IN];
#pragma unroll
    for (int k = 0; k < SSDim<R>::IN; k++) in[k] = rows[(r0 + k) * SS_PPITCH + tx];
    ss_taps<R>(a.g, in, out);
}

// grid: B * C * nty * ntx blocks over the map.  partial[blockIdx.x] = the tile's sum of S.  SAVE: the maps
// A, Bm, Cm (include/nr_raster.h) of the tile's pixels go to saved [3][B][C][MH][MW].
template <int R, bool SAVE>
__global__ __launch_bounds__(SS_BLOCK) void k_ssim_fwd(const SSArgs a, float* __restrict__ partial, float* __restrict__ saved) {
    using D = SSDim<R>;
    __shared__ SSLds<R, true> l;
    __shared__ float red[SS_BLOCK / 64];
    int bc, y0, x0;
    ss_block(a, bc, y0, x0);
    const int b = bc / a.C, c = bc - b * a.C;
    const long long plane = (long long)a.H * a.W;
    const float* x = a.images + (long long)b * a.istride + c * plane;
    const float* t = a.targets + (long long)b * a.tstride + c * plane;

    // the tile's windows cover image rows y0 - pad .. y0 - pad + HS - 1: all loads, then the LDS stores
    ss_f2 v[D::U];
#pragma unroll
    for (int j = 0; j < D::U; j++) {
        const int e = (int)threadIdx.x + j * SS_BLOCK;
        const int i = e / D::HS, jj = e - i * D::HS;
        const int iy = y0 - a.pad + i, ix = x0 - a.pad + jj;
        const bool in = e < D::NE && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        const long long off = in ? (long long)iy * a.W + ix : 0;
        v[j] = ss_f2{in ? x[off] : 0.f, in ? t[off] : 0.f};
    }
#pragma unroll
    for (int j = 0; j < D::U; j++) {
        const int e = (int)threadIdx.x + j * SS_BLOCK;
        const int i = e / D::HS, jj = e - i * D::HS;
        if (e < D::NE) l.halo[i * D::HP + jj] = v[j];
    }
    __syncthreads();
    ss_row_pass<R, true>(a, l);
    __syncthreads();

    const int tx = threadIdx.x & (SS_TILE - 1), r0 = (threadIdx.x / SS_TILE) * SS_PER;
    ss_f2 f01[SS_PER], f23[SS_PER];  // (mu1, mu2), (G*x^2, G*t^2)
    float f4[SS_PER];                // G*(x t)
    ss_col_pass<R>(a, l.rows_a, r0, tx, f01);
    ss_col_pass<R>(a, l.rows_b, r0, tx, f23);
    ss_col_pass<R>(a, l.rows_c, r0, tx, f4);
    const long long mplane = (long long)a.MH * a.MW, mstride = (long long)a.B * a.C * mplane;
    float sum = 0.f;
#pragma unroll
    for (int o = 0; o < SS_PER; o++) {
        const int my = y0 + r0 + o, mx = x0 + tx;
        if (my >= a.MH || mx >= a.MW) continue;
        const float m1 = f01[o].x, m2 = f01[o].y;
        const float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
        const float s11 = f23[o].x - m11, s22 = f23[o].y - m22, s12 = f4[o] - m12;
        const float n1 = 2.f * m12 + a.c1, n2 = 2.f * s12 + a.c2;
        const float d1 = (m11 + m22) + a.c1, d2 = (s11 + s22) + a.c2;
        const float dd = d1 * d2;
        const float S = (n1 * n2) / dd;
        sum += S;
        if (SAVE) {
            const float Bm = -S / d2;
            const float Cm = 2.f * n1 / dd;
            const float A = ((2.f * m2 * n2 / dd - 2.f * m1 * S / d1) - 2.f * m1 * Bm) - m2 * Cm;
            float* o3 = saved + bc * mplane + (long long)my * a.MW + mx;
            o3[0] = A, o3[mstride] = Bm, o3[2 * mstride] = Cm;
        }
    }
    const float tot = ml_block_sum(sum, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// Second stage: block b adds the nblk tile partials of item b (thread t takes partials t, t + 256, ... in
// order, then the block sum) and writes loss[b] = 1 - sum / count.
__global__ __launch_bounds__(SS_BLOCK) void k_ssim_finish(const float* __restrict__ partial, int nblk, float count,
                                                          float* __restrict__ loss) {
    __shared__ float red[SS_BLOCK / 64];
    const int b = blockIdx.x;
    float s = 0.f;
    for (int e = threadIdx.x; e < nblk; e += SS_BLOCK) s += partial[(long long)b * nblk + e];
    const float tot = ml_block_sum(s, red);
    if (threadIdx.x == 0) loss[b] = 1.f - tot / count;
}

// grid: B * C * nty * ntx blocks over the image.  grad_images [B, C H W] contiguous, every element written:
// grad x(p) = -(g_b / count) ((G * A)(p) + 2 x(p) (G * Bm)(p) + t(p) (G * Cm)(p)), the maps zero outside
// their MH x MW and map pixel m sitting at image pixel m + R - pad.
template <int R>
__global__ __launch_bounds__(SS_BLOCK) void k_ssim_bwd(const SSArgs a, const float* __restrict__ saved,
                                                       const float* __restrict__ grad_loss, float count,
                                                       float* __restrict__ grad_images) {
    using D = SSDim<R>;
    __shared__ SSLds<R, false> l;
    int bc, y0, x0;
    ss_block(a, bc, y0, x0);
    const int b = bc / a.C, c = bc - b * a.C;
    const long long mplane = (long long)a.MH * a.MW, mstride = (long long)a.B * a.C * mplane;
    const float* m = saved + bc * mplane;
    const int shift = 2 * R - a.pad;  // halo element (i, jj) is map pixel (y0 + i - shift, x0 + jj - shift)

    ss_f2 v[D::U];
    float vc[D::U];
#pragma unroll
    for (int j = 0; j < D::U; j++) {
        const int e = (int)threadIdx.x + j * SS_BLOCK;
        const int i = e / D::HS, jj = e - i * D::HS;
        const int my = y0 + i - shift, mx = x0 + jj - shift;
        const bool in = e < D::NE && my >= 0 && my < a.MH && mx >= 0 && mx < a.MW;
        const long long off = in ? (long long)my * a.MW + mx : 0;
        v[j] = ss_f2{in ? m[off] : 0.f, in ? m[mstride + off] : 0.f};
        vc[j] = in ? m[2 * mstride + off] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < D::U; j++) {
        const int e = (int)threadIdx.x + j * SS_BLOCK;
        const int i = e / D::HS, jj = e - i * D::HS;
        if (e < D::NE) l.halo[i * D::HP + jj] = v[j], l.halo_c[i * D::HP + jj] = vc[j];
    }
    __syncthreads();
    ss_row_pass<R, false>(a, l);
    __syncthreads();

    const int tx = threadIdx.x & (SS_TILE - 1), r0 = (threadIdx.x / SS_TILE) * SS_PER;
    ss_f2 f01[SS_PER];  // (G * A, G * Bm)
    float f2[SS_PER];   // G * Cm
    ss_col_pass<R>(a, l.rows_a, r0, tx, f01);
    ss_col_pass<R>(a, l.rows_c, r0, tx, f2);
    const long long plane = (long long)a.H * a.W;
    const float* x = a.images + (long long)b * a.istride + c * plane;
    const float* t = a.targets + (long long)b * a.tstride + c * plane;
    float* go = grad_images + bc * plane;
    const float scale = -(grad_loss[b] / count);
    const int ix = x0 + tx;
    float xp[SS_PER], tp[SS_PER];
#pragma unroll
    for (int o = 0; o < SS_PER; o++) {
        const bool in = y0 + r0 + o < a.H && ix < a.W;
        const long long off = in ? (long long)(y0 + r0 + o) * a.W + ix : 0;
        xp[o] = in ? x[off] : 0.f;
        tp[o] = in ? t[off] : 0.f;
    }
#pragma unroll
    for (int o = 0; o < SS_PER; o++)
        if (y0 + r0 + o < a.H && ix < a.W)
            go[(long long)(y0 + r0 + o) * a.W + ix] = scale * ((f01[o].x + 2.f * xp[o] * f01[o].y) + tp[o] * f2[o]);
}

template <bool SAVE>
void ss_launch_fwd(int R, const SSArgs& a, dim3 grid, hipStream_t st, float* partial, float* saved) {
    switch (R) {
    case 1: nr_launch(k_ssim_fwd<1, SAVE>, grid, dim3(SS_BLOCK), 0, st, a, partial, saved); break;
    case 2: nr_launch(k_ssim_fwd<2, SAVE>, grid, dim3(SS_BLOCK), 0, st, a, partial, saved); break;
    case 3: nr_launch(k_ssim_fwd<3, SAVE>, grid, dim3(SS_BLOCK), 0, st, a, partial, saved); break;
    case 4: nr_launch(k_ssim_fwd<4, SAVE>, grid, dim3(SS_BLOCK), 0, st, a, partial, saved); break;
    default: nr_launch(k_ssim_fwd<5, SAVE>, grid, dim3(SS_BLOCK), 0, st, a, partial, saved); break;
    }
}

void ss_launch_bwd(int R, const SSArgs& a, dim3 grid, hipStream_t st, const float* saved, const float* grad_loss, float count,
                   float* grad_images) {
    switch (R) {
    case 1: nr_launch(k_ssim_bwd<1>, grid, dim3(SS_BLOCK), 0, st, a, saved, grad_loss, count, grad_images); break;
    case 2: nr_launch(k_ssim_bwd<2>, grid, dim3(SS_BLOCK), 0, st, a, saved, grad_loss, count, grad_images); break;
    case 3: nr_launch(k_ssim_bwd<3>, grid, dim3(SS_BLOCK), 0, st, a, saved, grad_loss, count, grad_images); break;
    case 4: nr_launch(k_ssim_bwd<4>, grid, dim3(SS_BLOCK), 0, st, a, saved, grad_loss, count, grad_images); break;
    default: nr_launch(k_ssim_bwd<5>, grid, dim3(SS_BLOCK), 0, st, a, saved, grad_loss, count, grad_images); break;
    }
}

}  // namespace

// nr_attributes.h -- per-vertex attribute rendering: k_attr_fwd (interpolation, flip, 2x2 mean), k_attr_bwd
// (soft gradient + scatter to per-face-corner records), k_attr_vertex_sum / k_attr_row_sum (records -> gradients)
// Part of nr_raster.hip (one translation unit); see that file, include/nr_raster.h (NrAttributeArgs, the
// formulas) and DESIGN.md section 4 ("Vertex attributes").
//
// The forward reads the face-index map and the face records that a silhouette-only nr_rasterize_forward
// left, so the visible face and its barycentric weights (face_weights, nr_common.h) are those of every
// other render.  Per foreground pixel with weights w_k, corner depths z_k and corner attribute rows a_k:
//   linear:               out_c = (w_0 a_0c + w_1 a_1c) + w_2 a_2c
//   perspective-correct:  q_k = w_k / (z_k + 1e-10),  Dn = sum_k (q_k + 1e-10),  out_c = ((q_0 a_0c + q_1 a_1c) + q_2 a_2c) / Dn
// The channel count is a run-time loop bound (1 .. NR_ATTR_MAX_CHANNELS): per pixel the kernels keep only
// the three coefficients and the three row indices in registers and stream the channels.
//
// The backward follows nr_bwd.h's two levels.  k_attr_bwd, one lane per internal pixel and one wave per
// 8x8 pixels: the soft gradient (gx, gy) by diff_stencil (nr_shade.h, shared with k_diff_bwd) on the saved
// internal image, the upstream gradient read through the flip and the 2x2 mean; then the lanes of a wave
// that see the same face are summed (wave_sum under the face's lane mask) and the sums added to that face's
// zero-filled record [3 corners][3 + C] with float atomics, up to 63 lanes of one atomic instruction
// each.  k_attr_vertex_sum and k_attr_row_sum then add the records per vertex and per attribute row
// through the CSR lists, in list order (and item order for a shared table).
#pragma once

#pragma clang fp contract(off)

namespace {

constexpr int AT_BLOCK = 256;
constexpr int AT_FLUSH = 21;  // channels per atomic instruction of the attribute part: 3 corners x 21 = 63 lanes

// d out_c / d a_kc of a foreground pixel: w_k (linear) or q_k / Dn (perspective-correct); q and dn as above
// (q = w, dn = 1 in the linear mode)
__device__ __forceinline__ void attr_coefs(const Face& f, const float w[3], int pc, float q[3], float& dn) {
    q[0] = w[0], q[1] = w[1], q[2] = w[2];
    dn = 1.f;
    if (pc) {
        q[0] = w[0] / (f.z0 + 1e-10f);
        q[1] = w[1] / (f.z1 + 1e-10f);
        q[2] = w[2] / (f.z2 + 1e-10f);
        dn = ((q[0] + 1e-10f) + (q[1] + 1e-10f)) + (q[2] + 1e-10f);
    }
}

// One lane per output pixel, and under anti-aliasing its 2x2 internal pixels in the reference's order
// (rasterize.py:323-327: a = (iy + 1, ix + 1), b = (iy, ix + 1), c = (iy + 1, ix), d = (iy, ix)).  No barrier
// and no cross-lane operation: lanes past the image leave at once.
template <bool AA>
__global__ __launch_bounds__(AT_BLOCK) void k_attr_fwd(const NrAttributeArgs a, int S, float* __restrict__ images) {
    constexpr int NP = AA ? 4 : 1;
    const int s = a.image_size, b = blockIdx.y, C = a.num_channels;
    const int o = blockIdx.x * AT_BLOCK + threadIdx.x;
    if (o >= s * s) return;
    const int oi = o / s, oj = o - oi * s;
    const int32_t* __restrict__ fb = a.face_index + (long long)b * S * S;
    const float* __restrict__ frb = a.face_records + (long long)b * a.num_faces * FACE_REC;
    const float* __restrict__ ab = a.attributes + (long long)b * a.attr_batch_stride;
    float q[NP][3], dn[NP];
    int row[NP][3], pix[NP];
    bool fg[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const int y = AA ? S - 2 - 2 * oi + ((p & 1) ? 0 : 1) : S - 1 - oi;
        const int x = AA ? S - 2 - 2 * oj + ((p & 2) ? 0 : 1) : S - 1 - oj;
        pix[p] = y * S + x;
        const int fi = fb[pix[p]];
        fg[p] = fi >= 0;
        q[p][0] = q[p][1] = q[p][2] = 0.f;
        dn[p] = 1.f;
        row[p][0] = row[p][1] = row[p][2] = 0;
        if (fi >= 0) {
            const Face f = load_face_rec(frb + (long long)fi * FACE_REC);
            float w[3];
            face_weights(pix_center(x, S), pix_center(y, S), f, w);
            attr_coefs(f, w, a.perspective_correct, q[p], dn[p]);
#pragma unroll
            for (int k = 0; k < 3; k++) row[p][k] = a.faces_attributes[(long long)fi * 3 + k];
        }
    }
    float* __restrict__ ib = a.internal ? a.internal + (long long)b * S * S * C : nullptr;
    float* __restrict__ ob = images + (long long)b * C * s * s + o;
    for (int c = 0; c < C; c++) {
        float v[NP];
#pragma unroll
        for (int p = 0; p < NP; p++) {
            float val = 0.f;
            if (fg[p]) {
                const float a0 = ab[(long long)row[p][0] * C + c];
                const float a1 = ab[(long long)row[p][1] * C + c];
                const float a2 = ab[(long long)row[p][2] * C + c];
                val = (q[p][0] * a0 + q[p][1] * a1) + q[p][2] * a2;
                if (a.perspective_correct) val = val / dn[p];
            }
            if (ib) ib[(long long)pix[p] * C + c] = val;
            v[p] = val;
        }
        ob[(long long)c * s * s] = AA ? (((v[0] + v[NP > 1 ? 1 : 0]) + v[NP > 2 ? 2 : 0]) + v[NP > 3 ? 3 : 0]) / 4.f : v[0];
    }
}

// One lane per internal pixel; a block is a TW x TH tile, wave w its 8x8 pixels from column 8 w.
// rec: [B, F, 3, 3 + C] zero-filled records: per corner d/d(x, y, z) then d/d a_kc.
template <bool WANT_V, bool WANT_A>
__global__ __launch_bounds__(AT_BLOCK) void k_attr_bwd(const NrAttributeArgs a, int S, const float* __restrict__ grad_images,
                                                      float* __restrict__ rec) {
    const int b = blockIdx.y, C = a.num_channels, s = a.image_size, aa = a.anti_aliasing ? 1 : 0;
    const int tiles_x = (S + TW - 1) / TW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = tx * TW + wv * 8 + (lane & 7), y = ty * TH + (lane >> 3);
    const bool inside = x < S && y < S;
    const int fi = inside ? a.face_index[(long long)b * S * S + y * S + x] : -1;
    const bool act = fi >= 0;
    if (__ballot(act) == 0) return;  // wave-uniform: a background wave adds nothing
    const int R = 3 + C;
    const long long ss = (long long)s * s;
    const float* __restrict__ gib = grad_images + (long long)b * C * ss;
    // the upstream gradient of internal pixel (yy, xx): through the flip and, with anti-aliasing, the 2x2 mean
    const auto up = [&](int yy, int xx, int c) -> float {
        const float g = gib[c * ss + (long long)((S - 1 - yy) >> aa) * s + ((S - 1 - xx) >> aa)];
        return aa ? g / 4.f : g;
    };
    float cf[3] = {0.f, 0.f, 0.f}, pos[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (act) {
        const Face f = load_face_rec(a.face_records + ((long long)b * a.num_faces + fi) * FACE_REC);
        float w[3], q[3], dn;
        face_weights(pix_center(x, S), pix_center(y, S), f, w);
        attr_coefs(f, w, a.perspective_correct, q, dn);
#pragma unroll
        for (int k = 0; k < 3; k++) cf[k] = a.perspective_correct ? q[k] / dn : w[k];
        if (WANT_V) {
            const float* __restrict__ ib = a.internal + (long long)b * S * S * C;
            const auto img = [&](int yy, int xx, int c) -> float { return ib[((long long)yy * S + xx) * C + c]; };
            float gx, gy;
            diff_stencil(img, up, y, x, S, S, C, (float)(2. / S), gx, gy);
#pragma unroll
            for (int k = 0; k < 3; k++) pos[3 * k] = w[k] * gx, pos[3 * k + 1] = w[k] * gy;
            if (a.perspective_correct) {
                // d out_c / d z_k = -(q_k / (z_k + 1e-10)) / Dn (a_kc - out_c)
                const float* __restrict__ ab = a.attributes + (long long)b * a.attr_batch_stride;
                long long r[3];
#pragma unroll
                for (int k = 0; k < 3; k++) r[k] = (long long)a.faces_attributes[(long long)fi * 3 + k] * C;
                float zs[3] = {0.f, 0.f, 0.f};
                for (int c = 0; c < C; c++) {
                    const float g = up(y, x, c), oc = img(y, x, c);
#pragma unroll
                    for (int k = 0; k < 3; k++) zs[k] += g * (ab[r[k] + c] - oc);
                }
                const float zq[3] = {f.z0 + 1e-10f, f.z1 + 1e-10f, f.z2 + 1e-10f};
#pragma unroll
                for (int k = 0; k < 3; k++) pos[3 * k + 2] = -(q[k] / zq[k]) / dn * zs[k];
            }
        }
    }
    // the lanes of one face, summed; each sum lands in a lane of its own and the lanes add together
    unsigned long long pend = __ballot(act);
    float* __restrict__ rb = rec + (long long)b * a.num_faces * 3 * R;
    while (pend) {
        const int leader = __builtin_ctzll(pend);
        const int key = __builtin_amdgcn_readlane(fi, leader);
        const bool mem = act && fi == key;
        pend &= ~__ballot(mem);
        float* __restrict__ rf = rb + (long long)key * 3 * R;
        if (WANT_V) {
            float mine = 0.f;
#pragma unroll
            for (int j = 0; j < 9; j++) {
                const float v = wave_sum(mem ? pos[j] : 0.f);
                if (lane == j) mine = v;
            }
            if (lane < 9 && mine != 0.f) unsafeAtomicAdd(rf + (lane / 3) * R + lane % 3, mine);
        }
        if (WANT_A) {
            for (int c0 = 0; c0 < C; c0 += AT_FLUSH) {
                const int n = min(AT_FLUSH, C - c0);
                float mine = 0.f;
                for (int j = 0; j < n; j++) {
                    const float g = mem ? up(y, x, c0 + j) : 0.f;
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        const float v = wave_sum(cf[k] * g);
                        if (lane == 3 * j + k) mine = v;
                    }
                }
                if (lane < 3 * n && mine != 0.f) unsafeAtomicAdd(rf + (lane % 3) * R + 3 + c0 + lane / 3, mine);
            }
        }
    }
}

// grad_vertices[b, v] = sum over the vertex's corners (CSR entries 3 f + k, in list order) of the records'
// position part
__global__ __launch_bounds__(AT_BLOCK) void k_attr_vertex_sum(const float* __restrict__ rec, const int32_t* __restrict__ off,
                                                             const int32_t* __restrict__ ent, float* __restrict__ gV, int F,
                                                             int V, int R, long long n) {
    const long long i = (long long)blockIdx.x * AT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int b = (int)(i / V), v = (int)(i % V);
    const float* __restrict__ base = rec + (long long)b * F * 3 * R;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int e = off[v]; e < off[v + 1]; e++) {
        const float* r = base + (long long)ent[e] * R;
        s0 += r[0], s1 += r[1], s2 += r[2];
    }
    gV[i * 3 + 0] = s0, gV[i * 3 + 1] = s1, gV[i * 3 + 2] = s2;
}

// grad_attributes[ba, r, c] = sum over the items of ba (every item when the table is shared, in item
// order) and the row's corners (in list order) of the records' channel c; lanes run along the channels
__global__ __launch_bounds__(AT_BLOCK) void k_attr_row_sum(const float* __restrict__ rec, const int32_t* __restrict__ off,
                                                          const int32_t* __restrict__ ent, float* __restrict__ gA, int B, int F,
                                                          int Va, int C, int shared, long long n) {
    const long long i = (long long)blockIdx.x * AT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const long long rc = i / C;
    const int r = (int)(rc % Va), ba = (int)(rc / Va);
    const int R = 3 + C;
    const int e0 = off[r], e1 = off[r + 1];
    const int b0 = shared ? 0 : ba, b1 = shared ? B : ba + 1;
    float sum = 0.f;
    for (int b = b0; b < b1; b++) {
        const float* __restrict__ base = rec + (long long)b * F * 3 * R + 3 + c;
        for (int e = e0; e < e1; e++) sum += base[(long long)ent[e] * R];
    }
    gA[i] = sum;
}

}  // namespace

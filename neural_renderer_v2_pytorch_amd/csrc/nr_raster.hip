// nr_raster.hip -- MI355X (gfx950 / CDNA4) differentiable mesh rasterizer.
//
// Hand-written HIP behind the C ABI of include/nr_raster.h.  Replaces the reference's CUDA
// extension (neural_renderer_torch/cuda/rasterize_cuda_kernel.cu) AND the torch glue around it in
// rasterize_core (neural_renderer_torch/rasterize.py:194-329), with the same results:
//   * face_index_map bit-exact: every pixel scans, in ascending face order, a superset of the faces
//     whose bounding box contains it, with the reference's float arithmetic unchanged
//     (rasterize_cuda_kernel.cu:82-149; no FMA contraction, IEEE division, double pixel centres);
//   * rgb / depth / silhouette values follow rasterize.py:80-153 operation for operation.
//
// Pipeline of one forward (3 launches: setup, raster, shade) -- see DESIGN.md for the data layout and rooflines:
//   k_face_setup     one block per (128 faces, item): gather the faces from vertices (rasterize.py:232),
//                    per-face screen bbox + face-level rejects, texture-uv gather, and the coarse-bin
//                    face bitmasks (32x32-pixel bins, bit f set when face f may touch the bin).
//   k_raster_fwd     one block per 32x32-pixel coarse bin: stages the bin's candidate faces in face
//                    order into LDS, each wave walks (ballot) the faces touching its pixels in order;
//                    writes the face-index map.
//   k_shade          one thread per output pixel: weights, texture, silhouette, depth, merged,
//                    flipped and 2x2-averaged into the [B, C, s, s] image.
//   backward         k_raster_bwd: one block per 32x16 pixels + 1-pixel halo: recomputes the internal
//                    image from fim, applies Differentiation.backward's stencil, and chains the
//                    coordinate / depth / texture gradients to vertices and textures with atomics.
//
// Source layout (one translation unit): nr_common.h (errors, profiling, geometry, exact division,
// per-pixel shading, XCD tile map), nr_fwd.h (setup + face-index raster), nr_shade.h (image epilogue,
// halo cache, standalone reference kernels), nr_bwd.h (backward), nr_camera.h (look_at / look +
// perspective), nr_projection.h (calibrated camera: K, R, t + distortion), nr_mesh_loss.h (Laplacian, cotangent
// Laplacian, flatten and edge-length regularizers), nr_arap.h (as-rigid-as-possible energy and the cotangent weights of a
// rest shape), nr_image_loss.h (squared-error, Huber and IoU image losses), nr_ssim_loss.h (SSIM image loss), nr_adam.h
// (multi-tensor Adam), nr_attributes.h (per-vertex attribute rendering), nr_point_loss.h (chamfer distance,
// nearest points and surface sampling), nr_point_mesh.h (point-to-surface distance), nr_face_point.h (face-to-scan distance),
// nr_skinning.h (forward kinematics and linear blend skinning), nr_rigid.h (rigid alignment and ICP), nr_host.h (workspace layouts, launch helpers, argument checks); this file holds the extern "C" ABI.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "nr_raster.h"


#pragma clang fp contract(off)

#include "nr_cull.h"
#include "nr_pixel.h"
#include "nr_common.h"
#include "nr_shade.h"
#include "nr_fwd.h"
#include "nr_bwd.h"
#include "nr_camera.h"
#include "nr_projection.h"
#include "nr_mesh_loss.h"
#include "nr_arap.h"
#include "nr_image_loss.h"
#include "nr_ssim_loss.h"
#include "nr_adam.h"
#include "nr_attributes.h"
#include "nr_point_loss.h"
#include "nr_point_mesh.h"
#include "nr_face_point.h"
#include "nr_skinning.h"
#include "nr_rigid.h"
#include "nr_host.h"


// self-test of the exact division shortcut (nr_selftest_division): q_fast = div_nr(a, b, rcp_nr(b)),
// q_ieee = a / b as the compiler lowers it
__global__ void k_selftest_div(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ qf,
                               float* __restrict__ qi, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = a[i], y = b[i];
    qf[i] = div_nr(x, y, rcp_nr(y));
    qi[i] = x / y;
}

// ==================================================================================================
extern "C" {

const char* nr_last_error(void) { return g_err.c_str(); }
int nr_version(void) { return NR_ABI_VERSION; }
size_t nr_raster_args_size(void) { return sizeof(NrRasterArgs); }

int nr_tile_order(int nx, int ny, int tile_w, int tile_h, uint16_t* out) {
    if (!out) return fail(NR_ERR_ARGS, "nr_tile_order: null output");
    if (!tile_order_entries(nx, ny, tile_w, tile_h, out))
        return fail(NR_ERR_ARGS, "nr_tile_order: %d x %d tiles of %d x %d pixels (1 to %d tiles, at most 256 a side)", nx, ny,
                    tile_w, tile_h, TILE_ORDER_MAX);
    return NR_OK;
}

int nr_num_channels(int draw_flags) {
    return ((draw_flags & NR_DRAW_RGB) ? 3 : 0) + ((draw_flags & NR_DRAW_SILHOUETTES) ? 1 : 0) +
           ((draw_flags & NR_DRAW_DEPTH) ? 1 : 0);
}

size_t nr_hot_acc_bytes(int num_hot) {
    if (num_hot <= 0) return 0;
    Cutter c;  // the windows' sums (k_raster_bwd finds the positions hot_sums_floats after them), then the positions
    c.take(hot_sums_floats(num_hot) * 4);
    c.take((size_t)num_hot * 8);
    return c.off;
}

size_t nr_workspace_bytes(int batch_size, int num_faces, int image_size) {
    return forward_layout(batch_size, num_faces, make_geom(num_faces, image_size)).total;
}

// A side stream per (host thread, device) for the split forward, with its fork / join events; created
// on first use outside a stream capture (null: no split for this call).  The thread's table releases
// them when the thread ends (a worker pool's recycled threads do not accumulate streams).  No
// synchronisation there: a synchronising call from an exiting thread would invalidate another thread's
// graph capture in global capture mode, so the code relies on hipStreamDestroy of a stream that may
// still have queued work neither waiting for that work nor dropping it.  HIP's documentation leaves
// that open (CUDA's promises it for cudaStreamDestroy): an assumption about the runtime, not a
// guarantee, and one no test exercises (the exiting-thread test's workers synchronise before they
// end).  The destroys themselves run in this thread's relaxed capture mode for the same reason.
// Errors are ignored (at process exit the runtime may be gone).
struct SideStream {
    hipStream_t s = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
};
struct SideStreamTable {
    SideStream tab[64];
    ~SideStreamTable() {
        bool any = false;
        for (const SideStream& x : tab) any = any || x.s || x.fork || x.join;
        if (!any) return;
        hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
        const bool exch = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess;
        for (SideStream& x : tab) {
            if (x.s) (void)hipStreamDestroy(x.s);
            if (x.fork) (void)hipEventDestroy(x.fork);
            if (x.join) (void)hipEventDestroy(x.join);
            x = SideStream{};
        }
        if (exch) (void)hipThreadExchangeStreamCaptureMode(&mode);
    }
};
constexpr int SPLIT_BUCKET = 10;  // deep bins: >= 512 candidates
constexpr int QS_CAP = 16;        // deep bins per list walked by quadrant blocks (a forward that does not split)
SideStream* side_stream(hipStream_t st) {
    static thread_local SideStreamTable table;
    SideStream* tab = table.tab;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    // the side stream lives on the current device: a caller's stream of another device gets no split
    hipDevice_t sdev = dev;
    if (st && hipStreamGetDevice(st, &sdev) != hipSuccess) return nullptr;
    if (sdev != dev) return nullptr;
    SideStream& x = tab[dev];
    if (!x.s) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
        if (hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&x.join, hipEventDisableTiming) != hipSuccess ||
            hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking) != hipSuccess) {
            if (x.fork) (void)hipEventDestroy(x.fork);
            if (x.join) (void)hipEventDestroy(x.join);
            x = SideStream{};
            return nullptr;
        }
    }
    return &x;
}

// 1024-thread blocks of k_raster_fwd resident at once on one XCD of the current device: two per CU
// (32 waves and 2 x 62.6 KB of LDS), the CUs dealt evenly over the 8 XCDs
static int deep_slots_per_xcd() {
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 64;
    if (!cached[dev]) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        __atomic_store_n(&cached[dev], 2 * max(cus / 8, 1), __ATOMIC_RELAXED);
    }
    return __atomic_load_n(&cached[dev], __ATOMIC_RELAXED);
}

// One k_raster_fwd launch: its instantiation (k_raster_fwd's template parameters, nr_fwd.h) and the part
// of a deep-first list it walks (ordered_bin: 0 every bin, 1 a split's deep prefix, 2 a split's rest,
// 3 every bin plus the quadrant blocks of the deepest)
struct FwdVariant {
    int ntf;     // NTF: block threads, 256 or 1024
    bool shade;  // SHADE: k_shade's work fused in
    int cc;      // CC: compile-time channels, MAXC or 4 (256 threads with SHADE only; 0: at run time)
    bool dq;     // DQ: the dealt-quarter walk (1024 threads only)
    int part;
};
// The forward's kernels by run-time choice: the setup with or without the gather from vertices, the
// eight k_raster_fwd instantiations the library holds, and the separate shading launch's by its lights
// (1) / backgrounds (2) feature mask.  (The compiler lays the instantiations out in the code object in
// the order these functions first name them.)
using SetupFn = decltype(&k_face_setup<true>);
static SetupFn setup_kernel(bool gather) { return gather ? k_face_setup<true> : k_face_setup<false>; }
using RasterFwdFn = decltype(&k_raster_fwd<1024, true>);
static RasterFwdFn raster_fwd_kernel(const FwdVariant& v) {
    if (v.shade && v.ntf == 1024 && !v.dq) return k_raster_fwd<1024, true>;
    if (v.shade && v.ntf == 256 && v.cc == MAXC) return k_raster_fwd<256, true, MAXC>;
    if (v.shade && v.ntf == 256) return v.cc == 4 ? k_raster_fwd<256, true, 4> : k_raster_fwd<256, true>;
    if (v.shade) return k_raster_fwd<1024, true, 0, true>;
    if (v.ntf == 256) return k_raster_fwd<256, false>;
    return v.dq ? k_raster_fwd<1024, false, 0, true> : k_raster_fwd<1024, false>;
}
using ShadeFn = decltype(&k_shade_px<0>);
static ShadeFn shade_kernel(bool per_pixel, int feat) {
    static const ShadeFn px[4] = {k_shade_px<0>, k_shade_px<1>, k_shade_px<2>, k_shade_px<3>};
    static const ShadeFn quad[4] = {k_shade<0>, k_shade<1>, k_shade<2>, k_shade<3>};
    return (per_pixel ? px : quad)[feat];
}

static int run_face_index(const float* vertices, const int32_t* faces_idx, float* face_records, int32_t* fim,
                          int B, int V, int F, int S, float near, float far, int draw_backside, float delta,
                          void* ws, size_t ws_bytes, hipStream_t st, const NrRasterArgs* ra, float* images,
                          TexPack pk, ZeroFill zf = ZeroFill{nullptr, 0}) {
    Geom g = make_geom(F, S);
    g.group = group_for(B, FWD_GROUP);
    g.B = B;
    const FwdLayout wl = forward_layout(B, F, g);
    int2* bbox = (int2*)((char*)ws + wl.bbox);
    uint32_t* mask = (uint32_t*)((char*)ws + wl.mask);
    uint8_t* bin_part = (uint8_t*)ws + wl.part;
    int* bin_order = (int*)((char*)ws + wl.order);
    if (B == 0) return NR_OK;
    // forward block size (k_raster_fwd notes): 256 threads when the grid alone fills the chip many
    // times over and the bins are shallow; 1024 when it does not, or when the bins are deep (F per bin
    // at the 32x32 bin granularity as the depth proxy)
    const long long blocks = (long long)g.nbins * B;
    const double faces_per_bin = (double)F / g.nbins;
    const int ntf = (blocks >= 8192 && faces_per_bin < 40.0) ? 256 : 1024;
    // deep bins (the car, the 50k torus): dispatch the bins deepest first (k_bin_order), from candidate
    // counts the setup adds up (its LDS bin-mask path); a list per XCD needs B % 8 == 0 or fits one block
    const long long order_list = (B % 8 == 0 ? B / 8 : B) * (long long)g.nbins;  // entries per k_bin_order block
    const bool ordered = F > 0 && ntf == 1024 && faces_per_bin >= 24.0 &&
                         (long long)g.nbins * (SETUP_FACES / 32) <= SETUP_LDS_WORDS && order_list <= ORDER_MAX_ENTRIES;
    // the setup's idle threads repack the textures when that takes them up to 32 texels each; with no
    // setup launch, or a texture too large for that, the repacking gets a launch of its own
    const long long setup_idle = (long long)((F + SETUP_FACES - 1) / SETUP_FACES) * B * (256 - SETUP_FACES);
    if (pk.out && (F == 0 || pk.n > 32 * setup_idle)) {
        ProfScope _p(P_TEXPACK, st, true);
        nr_launch(k_tex_pack, grid_1d(pk.n, 256), dim3(256), 0, st, pk);
        const int e = check_launch("k_tex_pack");
        if (e) return e;
        pk.out = nullptr;
    }
    int e;
    if (F == 0 && zf.p && !zero_async(zf.p, (size_t)zf.n16 * 16, st, &e)) return e;

    // k_shade's work fused into the forward's 256-thread variant (anti-aliasing, no lights or
    // backgrounds): the face-index map is not read back, and there is one launch fewer
    const Shade sh = ra ? make_shade(ra) : Shade{};
    // the deep-bin / small-grid 1024-thread variant shades too (its threads 0-255)
    const bool fuse = ra && ra->anti_aliasing && sh.nl == 0 && !sh.bg && vertices;
    // the split forward (below) when the batch is deep-first, fused and B % 8 == 0; otherwise a
    // deep-first forward reads its bins' mask words through sparse groups: the setup writes only the
    // (group, bin) pieces with candidates, and each forward block lists its bin's groups from the
    // setup's counts (for the 50k torus at 1024^2: 1024 bins x 1563 words of dense masks for ~10^4
    // non-empty pieces).  A split that finds no side stream falls back to the dense reads (the setup
    // wrote every piece)
    const int Bcap = B % 8 == 0 ? max(8, (B / 4 + 7) / 8 * 8) : 0;
    const bool want_split = ordered && fuse && B % 8 == 0 && Bcap <= B;
    const bool sg = ordered && !want_split && setup_groups(g) <= 1024;
    if (F > 0) {
        dim3 grid((F + SETUP_FACES - 1) / SETUP_FACES, B);
        const bool rgb = ra && (ra->draw_flags & NR_DRAW_RGB);
        const int uv_items = rgb ? (ra->vt_batch_stride ? B : 1) : 0;
        ProfScope _p(P_SETUP, st, true);
        const bool lit = rgb && ra->num_lights > 0;
        const size_t lds = (size_t)setup_lds_words(g.nbins) * 4;
        // gathering from vertices, or (no vertices, hence no ra: every texture argument is null) the caller's faces
        nr_launch(setup_kernel(vertices != nullptr), grid, dim3(256), lds, st, vertices, faces_idx,
                  face_records, V, F, S, draw_backside, bbox, mask, g.nbx, g.nbins, g.nwords,
                  rgb ? ra->vertices_textures : nullptr, rgb ? ra->vt_batch_stride : 0,
                  rgb ? ra->num_vertices_textures : 0, rgb ? ra->faces_textures : nullptr,
                  rgb ? ra->face_uv : nullptr, uv_items, lit ? ra->face_normals : nullptr, pk, zf,
                  ordered ? bin_part : nullptr, B % 8 == 0, sg ? 1 : 0);
        e = check_launch("k_face_setup");
        if (e) return e;
        if (lit && V > 0) {
            const long long nv = (long long)B * V;
            nr_launch(k_vertex_normals, grid_1d(nv, 256), dim3(256), 0, st, ra->face_normals,
                               ra->normal_offsets, ra->normal_faces, ra->vertex_normals, F, V, nv);
            e = check_launch("k_vertex_normals");
            if (e) return e;
        }
    }
    // split forward (deep-bin batches of B % 8 == 0 items, e.g. the car): the bins with >= 2^(SPLIT_BUCKET
    // - 1) candidates (a prefix of each deep-first list, at most Bcap / 8 * nbins of them) in the
    // 1024-thread variant on the caller's stream, the rest in the 256-thread variant on a side stream at
    // the same time: a shallow bin's 16 waves in the 1024-thread variant mostly wait for their block's
    // slowest wave, where the 256-thread variant deals its 16 8x8 blocks to 4 waves
    SideStream* side = want_split ? side_stream(st) : nullptr;
    // the deep launch takes at most 7/8 of one XCD's slots for 1024-thread blocks per list (two per CU,
    // by their waves and LDS), so every deep bin is dispatched at once: a deep block waiting for a slot
    // starves behind the rest launch's 256-thread blocks, which take every CU space that frees up (at
    // 75 deep bins per list the last ones started at 430 us of a 535 us car forward,
    // profiles/r05_v56_car_fwd_wave_phases.txt); the bins past the cap go to the rest launch.  Car
    // forward 0.49-0.50 -> 0.44 ms at 56 per list (48: the same; 40: 0.57 ms, the bins it leaves to the
    // 256-thread launch then end last; 64: 0.46-0.48 ms; no cap: 0.50 ms; same-box A/Bs, 3 runs each,
    // gpurun_out/e7, e9)
    const int deep_cap = min(Bcap / 8 * g.nbins, deep_slots_per_xcd() * 7 / 8);
    // a deep-first forward that does not split (e.g. one item, the 50k torus): each list's bins of
    // >= 512 candidates (up to QS_CAP of them) are walked by four blocks each, one per 16x16 quadrant
    // (ordered_bin part 3), so the deepest bins, which set the span while most of the chip idles, spread
    // over four CUs
    const bool qs = ordered && !side;
    const int lists = B % 8 == 0 ? 8 : 1;
    // each list's count of deep bins (k_bin_order): a deep-first forward either splits or walks quadrants
    int* split_cnt = ordered ? (int*)((char*)ws + wl.split_cnt) : nullptr;
    if (ordered) {
        nr_launch(k_bin_order, dim3(lists), dim3(1024), 0, st, bin_part, setup_groups(g), bin_order, B,
                           g.nbins, split_cnt, SPLIT_BUCKET, side ? deep_cap : QS_CAP);
        e = check_launch("k_bin_order");
        if (e) return e;
    }
    const int* order = ordered ? bin_order : nullptr;
    // per-bin foreground flags after the halo values (the backward skips background tiles)
    uint8_t* binfg = (ra && ra->halo) ? (uint8_t*)ra->halo + halo_layout(B, S, sh.C).flags : nullptr;
    // empty bins leave their -1 face ids unwritten (NrRasterArgs.face_index_sparse): with the fused
    // shading nothing else in this launch reads them, and the backward skips those tiles by the flags
    const int sparse = (ra && ra->face_index_sparse && fuse && binfg) ? 1 : 0;
    // The launches' variants, decided once; nr_last_launch reports the caller's-stream launch from the
    // same values.
    //   fwd:  on the caller's stream: the whole forward, or a split's deep prefix (part 1) in the plain
    //         1024-thread kernel (the dealt-quarter variant with its four-faces-per-step walk there
    //         instead: car forward 0.427 -> 0.434 ms, same-box A/B, run record w4b: the deep launch
    //         takes more of the rest's wave slots).  A deep-first forward that does not split (qs) runs
    //         the dealt-quarter kernel with the quadrant blocks (part 3).
    //   rest: a split's other bins (part 2) on the side stream, 256 threads.
    // cc256: the 256-thread fused kernel's compile-time channels: rgb + sil + depth, or rgba (the car)
    const int cc256 = sh.C == MAXC ? MAXC : (sh.draw == static_draw(4) ? 4 : 0);
    const FwdVariant fwd{ntf, fuse, fuse && ntf == 256 ? cc256 : 0, qs, side ? 1 : (qs ? 3 : 0)};
    const FwdVariant rest{256, true, cc256, false, 2};
    const dim3 bins(g.nbins, B);
    // (split: a grid of exactly the cap's blocks: every block past a list's deep prefix exits at once, but
    // each still needs a 1024-thread slot to be dispatched in; quadrants: 3 more blocks per deep bin)
    const dim3 fwd_grid = side ? dim3(8 * deep_cap)
                          : qs ? dim3((unsigned)((long long)g.nbins * B + 3 * QS_CAP * lists)) : bins;
    const int rs = vertices ? FACE_REC : 9;
    // the interleaved map's tile order (block_item_tile); the ordered forward reads its own lists
    const TileOrder& ord = tile_order(!order && g.group > 0, g, g.nbx, g.nby, COARSE, COARSE);
    const auto launch = [&](const FwdVariant& v, dim3 grid, hipStream_t s) {
        nr_launch(raster_fwd_kernel(v), grid, dim3(v.ntf), 0, s, face_records, rs, bbox, mask, F, g, near, far, delta,
                  fim, sh, v.shade ? images : nullptr, v.shade ? ra->halo : nullptr, binfg, order, sparse, split_cnt,
                  v.part, sg ? bin_part : nullptr, ord);
        return check_launch("k_raster_fwd");
    };
    g_last_fwd.store(LaunchRec{fwd.ntf, (fwd.shade ? NR_LAUNCH_FUSED_SHADE : 0) | (fwd.cc ? NR_LAUNCH_STATIC_CHANNELS : 0) |
                                            (order ? NR_LAUNCH_DEEP_FIRST : 0) | (side ? NR_LAUNCH_SPLIT : 0) |
                                            (fwd.dq ? NR_LAUNCH_DEALT_QUARTERS : 0) |
                                            (fwd.part == 3 ? NR_LAUNCH_QUADRANTS : 0)});
    {
        ProfScope _p(P_RASTER, st, side == nullptr);
        if (side) {
            // fork: the side stream waits for the setup and the order; join: the caller's stream waits
            // for the side stream's launch
            if (hipEventRecord(side->fork, st) != hipSuccess || hipStreamWaitEvent(side->s, side->fork, 0) != hipSuccess)
                return check_launch("hipEventRecord");
            e = launch(fwd, fwd_grid, st);
            if (e) return e;
            e = launch(rest, bins, side->s);
            if (e) return e;
            if (hipEventRecord(side->join, side->s) != hipSuccess || hipStreamWaitEvent(st, side->join, 0) != hipSuccess)
                return check_launch("hipEventRecord");
        } else {
            e = launch(fwd, fwd_grid, st);
        }
    }
    if (e || !ra || fuse) return e;
    // the separate shading launch: for a small grid k_shade_px, whose anti-aliased blocks cover 64
    // output pixels instead of 256
    const int s = ra->anti_aliasing ? S / 2 : S;
    const bool small = ((long long)s * s + 255) / 256 * B < 4096;
    const int per_block = small && ra->anti_aliasing ? 64 : 256;
    {
        ProfScope _p(P_SHADE, st, true);
        nr_launch(shade_kernel(small, (sh.nl ? 1 : 0) | (sh.bg ? 2 : 0)),
                  grid_1d((long long)s * s, per_block, B), dim3(256), 0, st, face_records, fim,
                  F, S, sh, ra->anti_aliasing, images, ra->halo);
    }
    return check_launch("k_shade");
}

int nr_face_index_map_forward_safe(const float* faces, int32_t* face_index, int batch_size, int num_faces,
                                   int image_size, float near, float far, int draw_backside, float eps,
                                   float depth_min_delta, void* workspace, size_t workspace_bytes, void* stream) {
    (void)eps;
    if (batch_size < 0 || num_faces < 0 || image_size <= 0 || image_size > 16384)
        return fail(NR_ERR_ARGS, "bad sizes B=%d F=%d S=%d", batch_size, num_faces, image_size);
    if (batch_size > 0 && (!face_index || (num_faces > 0 && !faces))) return fail(NR_ERR_ARGS, "null pointer");
    if (workspace_bytes < nr_workspace_bytes(batch_size, num_faces, image_size))
        return fail(NR_ERR_WORKSPACE, "workspace too small");
    return run_face_index(nullptr, nullptr, const_cast<float*>(faces), face_index, batch_size, 0, num_faces,
                          image_size, near, far, draw_backside, depth_min_delta, workspace, workspace_bytes,
                          (hipStream_t)stream, nullptr, nullptr, TexPack{});
}

int nr_compute_weight_map(const float* faces, const int32_t* face_index_map, float* weight_map, int batch_size,
                          int num_faces, int image_size, void* stream) {
    // the kernels' pixel centres are exact for S <= 16384 (nr_pixel.h), as in the other entry points
    if (batch_size < 0 || num_faces < 0 || image_size <= 0 || image_size > 16384)
        return fail(NR_ERR_ARGS, "bad sizes B=%d F=%d S=%d", batch_size, num_faces, image_size);
    const long long n = (long long)batch_size * image_size * image_size;
    if (n == 0) return NR_OK;
    nr_launch(k_weight_map, grid_1d(n, 256), dim3(256), 0, (hipStream_t)stream, faces,
                       face_index_map, weight_map, num_faces, image_size, n);
    return check_launch("k_weight_map");
}

int nr_mask_foreground_forward(const int32_t* face_index, const float* data_in, float* data_out, long long n, int dim,
                               void* stream) {
    if (n < 0 || dim < 0) return fail(NR_ERR_ARGS, "bad sizes");
    if (n == 0) return NR_OK;
    nr_launch(k_mask_fg, grid_1d(n, 256), dim3(256), 0, (hipStream_t)stream, face_index,
                       data_in, data_out, n, dim);
    return check_launch("k_mask_fg");
}

int nr_mask_foreground_backward(const int32_t* face_index, float* grad_in, const float* grad_out, long long n, int dim,
                                void* stream) {
    return nr_mask_foreground_forward(face_index, grad_out, grad_in, n, dim, stream);
}

int nr_differentiation_backward(const float* images, const float* grad, float* grad_xy, int batch_size, int height,
                                int width, int channels, void* stream) {
    if (batch_size < 0 || height <= 0 || width <= 0 || channels <= 0) return fail(NR_ERR_ARGS, "bad sizes");
    const long long n = (long long)batch_size * height * width;
    if (n == 0) return NR_OK;
    const float step = (float)(2. / height);
    nr_launch(k_diff_bwd, grid_1d(n, 256), dim3(256), 0, (hipStream_t)stream, images, grad,
                       grad_xy, height, width, channels, step, n);
    return check_launch("k_diff_bwd");
}

int nr_rasterize_forward(const NrRasterArgs* a, float* images, void* stream) {
    int e = validate_raster(a, true);
    if (e) return e;
    if (!images && a->batch_size > 0) return fail(NR_ERR_ARGS, "null images");
    TexPack pk{};
    if ((a->draw_flags & NR_DRAW_RGB) && a->textures_packed && a->batch_size > 0) {
        const int tex_items = a->tex_stride_b ? a->batch_size : 1;
        pk.tex = a->textures;
        pk.sb = a->tex_stride_b;
        pk.sc = (int)a->tex_stride_c;
        pk.sp = (int)a->tex_stride_p;
        pk.HW = a->tex_height * a->tex_width;
        pk.HWp = (int)packed_texels(a->tex_height, a->tex_width);
        pk.out = reinterpret_cast<float4*>(a->textures_packed);
        pk.n = (long long)tex_items * pk.HWp;
    }
    // the backward's accumulators, zeroed by the setup's idle threads (no memset launch in the backward)
    ZeroFill zf{nullptr, 0};
    if (a->bwd_workspace && a->bwd_workspace_bytes > 0) {
        if (((uintptr_t)a->bwd_workspace & 15) || (a->bwd_workspace_bytes & 15))
            return fail(NR_ERR_ARGS, "bwd_workspace must be 16-byte aligned and sized");
        zf.p = reinterpret_cast<float4*>(a->bwd_workspace);
        zf.n16 = (long long)(a->bwd_workspace_bytes / 16);
    }
    const int S = internal_size(a->anti_aliasing, a->image_size);
    return run_face_index(a->vertices, a->faces, a->face_records, a->face_index, a->batch_size, a->num_vertices,
                          a->num_faces, S, a->near, a->far, a->draw_backside, a->depth_min_delta, a->workspace,
                          a->workspace_bytes, (hipStream_t)stream, a, images, pk, zf);
}

size_t nr_texture_packed_bytes(int texture_items, int tex_height, int tex_width) {
    if (texture_items <= 0 || tex_height <= 0 || tex_width <= 0) return 0;
    return (size_t)texture_items * packed_texels(tex_height, tex_width) * 16;
}

size_t nr_halo_bytes(int batch_size, int image_size, int anti_aliasing, int draw_flags) {
    if (batch_size <= 0 || image_size <= 0) return 0;
    return halo_layout(batch_size, internal_size(anti_aliasing, image_size), nr_num_channels(draw_flags)).total;
}

size_t nr_backward_workspace_bytes(int batch_size, int num_faces, int num_vertices, int texture_items,
                                   int tex_height, int tex_width, int num_lights) {
    return backward_layout(batch_size, num_faces, num_vertices, texture_items, tex_height, tex_width, num_lights > 0).total;
}

int nr_rasterize_backward(const NrRasterArgs* a, const float* grad_images, float* grad_vertices, float* grad_textures,
                          void* workspace, size_t workspace_bytes, int workspace_zeroed, void* stream) {
    int e = validate_raster(a, false);
    if (e) return e;
    if (a->batch_size == 0) {
        // an empty batch still owes the caller its batch-shared gradient: a shared texture
        // (tex_stride_b == 0: one item) gets zeros; per-item textures and backgrounds have no items
        if ((a->draw_flags & NR_DRAW_RGB) && grad_textures && !a->tex_stride_b) {
            const size_t n = (size_t)3 * a->tex_height * a->tex_width * sizeof(float);
            if (n && !zero_async(grad_textures, n, (hipStream_t)stream, &e)) return e;
        }
        return NR_OK;
    }
    if (!grad_images || !grad_vertices) return fail(NR_ERR_ARGS, "null gradient buffers");
    if (a->num_faces > 0 && (!a->vertex_offsets || !a->vertex_faces))
        return fail(NR_ERR_ARGS, "missing vertex adjacency (vertex_offsets / vertex_faces)");
    const bool rgb = (a->draw_flags & NR_DRAW_RGB) && grad_textures;
    const bool lit = (a->draw_flags & NR_DRAW_RGB) && a->num_lights > 0;
    const int tex_items = rgb ? (a->tex_stride_b ? a->batch_size : 1) : 0;
    // texel indices of the backward's direct samples ride in a 32-bit field (nr_bwd.h POS_DIRECT)
    // (and a row at most DIRECT_OFF - 1 texels wide: the top-left index of a sample one row above the
    // texture, -W - 1 + x, must stay above -DIRECT_OFF to be encoded)
    if (rgb && ((long long)a->tex_height * a->tex_width > DIRECT_MAX_HW || a->tex_width >= DIRECT_OFF))
        return fail(NR_ERR_ARGS, "texture gradient: at most %d texels per texture and %d per row (got %d x %d)",
                    DIRECT_MAX_HW, DIRECT_OFF - 1, a->tex_height, a->tex_width);
    // shared texture windows into private copies (NrRasterArgs.face_hot): a texture and texture
    // coordinates shared by the batch
    // (the plain textured backward only: no lights, no backgrounds -- their instantiations have no
    // shared-window flush -- and rgb drawn)
    const bool hot = rgb && tex_items == 1 && a->face_hot && a->num_hot > 0 && !a->vt_batch_stride && !lit &&
                     !a->backgrounds;
    if (hot && (a->num_hot > NR_HOT_MAX || !a->hot_acc || ((uintptr_t)a->hot_acc & 15)))
        return fail(NR_ERR_ARGS, "face_hot: num_hot %d (at most %d) needs a 16-byte aligned hot_acc", a->num_hot, NR_HOT_MAX);
    const BwdLayout wl = backward_layout(a->batch_size, a->num_faces, a->num_vertices, tex_items, a->tex_height,
                                         a->tex_width, lit);
    if (wl.total > 0 && (!workspace || workspace_bytes < wl.total))
        return fail(NR_ERR_WORKSPACE, "backward workspace missing or too small");
    hipStream_t st = (hipStream_t)stream;
    const int S = internal_size(a->anti_aliasing, a->image_size);
    Geom g = make_geom(a->num_faces, S);
    const bool hot_texels = rgb && !a->tex_stride_b &&
                            (long long)a->tex_height * a->tex_width > BWD_HOT_TEXELS_PER_FACE * a->num_faces;
    g.group = group_for(a->batch_size, hot_texels ? BWD_GROUP_TEX : BWD_GROUP);
    const int HW = a->tex_height * a->tex_width;
    const int HWp = (int)packed_texels(a->tex_height, a->tex_width);
    char* w = (char*)workspace;
    float* gF = (float*)(w + wl.gF);
    float* g4 = rgb ? (float*)(w + wl.g4) : nullptr;
    float* gN = lit ? (float*)(w + wl.gN) : nullptr;
    float* gU = lit ? (float*)(w + wl.gU) : nullptr;
    // the accumulators before gU start at zero, unless the caller states, for this call, that the
    // forward zeroed them (NrRasterArgs.bwd_workspace)
    const bool prezeroed = workspace_zeroed != 0;
    if (prezeroed && wl.zero_bytes > 0 && (a->bwd_workspace != workspace || a->bwd_workspace_bytes < wl.zero_bytes))
        return fail(NR_ERR_ARGS, "workspace_zeroed = 1 needs args->bwd_workspace == workspace with at least %zu bytes "
                                 "(the buffer the forward zeroed)", wl.zero_bytes);
    if (wl.zero_bytes > 0 && !prezeroed && !zero_async(workspace, wl.zero_bytes, st, &e)) return e;
    if (hot) {
        // hot_acc starts at zero: the forward zeroed it when it lies inside the zeroed bwd_workspace
        const size_t hb = nr_hot_acc_bytes(a->num_hot);
        const char* hz = (const char*)a->hot_acc;
        const bool in_zeroed = prezeroed && hz >= (const char*)a->bwd_workspace &&
                               hz + hb <= (const char*)a->bwd_workspace + a->bwd_workspace_bytes;
        if (!in_zeroed && !zero_async(a->hot_acc, hb, st, &e)) return e;
    }
    BwdArgs ba;
    ba.face_records = a->face_records;
    ba.fim = a->face_index;
    ba.grad_images = grad_images;
    ba.grad_faces = gF;
    ba.grad_tex = g4;
    ba.halo = a->halo;
    ba.binfg = a->halo ? (const uint8_t*)a->halo + halo_layout(a->batch_size, S, nr_num_channels(a->draw_flags)).flags
                       : nullptr;
    ba.grad_normals = gN;
    ba.grad_bg = (a->draw_flags & NR_DRAW_RGB) && a->backgrounds ? a->grad_backgrounds : nullptr;
    ba.F = a->num_faces;
    ba.aa = a->anti_aliasing;
    ba.s = a->image_size;
    ba.HW = HW;
    ba.HWp = HWp;
    ba.step = (float)(2. / S);
    ba.inv_step = 1.f / ba.step;
    ba.step_pow2 = (S & (S - 1)) == 0;  // step = 2/S is then a power of two: x / step == x * (S / 2)
    ba.face_hot = hot ? a->face_hot : nullptr;
    ba.num_hot = hot ? a->num_hot : 0;
    ba.hot_acc = hot ? a->hot_acc : nullptr;
    Shade sh = make_shade(a);
    {
        ProfScope _p(P_BWD, st, !hot);
        const dim3 grid(((S + TW - 1) / TW) * ((S + BH - 1) / BH), a->batch_size);
        const bool silo = !(a->draw_flags & (NR_DRAW_RGB | NR_DRAW_DEPTH));  // lights / backgrounds need rgb
        switch ((lit ? 1 : 0) | (sh.bg ? 2 : 0) | (silo ? 4 : 0)) {
            case 0: launch_bwd<0>(grid, st, ba, g, sh); break;
            case 1: launch_bwd<1>(grid, st, ba, g, sh); break;
            case 2: launch_bwd<2>(grid, st, ba, g, sh); break;
            case 3: launch_bwd<3>(grid, st, ba, g, sh); break;
            default: launch_bwd<4>(grid, st, ba, g, sh); break;
        }
        e = check_launch("k_raster_bwd");
        if (e) return e;
        // the shared windows' private copies, summed (timed with k_raster_bwd, whose window flushes they
        // complete; bench.py counts their bytes there), before the texture-gradient output (k_vertex_grad
        // / k_tex_out) reads the accumulator
        if (hot) {
            nr_launch(k_hot_reduce, dim3((unsigned)a->num_hot), dim3(64), 0, st, a->hot_acc, a->num_hot, g4,
                               a->tex_width, a->tex_height);
            e = check_launch("k_hot_reduce");
            if (e) return e;
        }
    }
    const long long nv = (long long)a->batch_size * a->num_vertices;
    if (lit && nv > 0) {
        // lights: vertex-normal gradients -> face normals -> corner gradients (added into gF)
        nr_launch(k_vnormal_bwd, grid_1d(nv, 256), dim3(256), 0, st, gN, a->vertex_offsets,
                           a->vertex_faces, a->vertex_normals, gU, a->num_faces, a->num_vertices, nv);
        e = check_launch("k_vnormal_bwd");
        if (e) return e;
        const long long nf = (long long)a->batch_size * a->num_faces;
        if (nf > 0) {
            nr_launch(k_fnormal_bwd, grid_1d(nf, 256), dim3(256), 0, st, a->face_records,
                               a->faces, gU, gF, a->num_faces, a->num_vertices, nf);
            e = check_launch("k_fnormal_bwd");
            if (e) return e;
        }
    }
    TexOut to{};
    if (rgb) to = TexOut{g4, grad_textures, HW, HWp, (long long)tex_items * HW};
    // k_vertex_grad's blocks also carry the texture-gradient output when that is a few texels per
    // thread; otherwise (no vertices, or a large texture) it gets a launch of its own
    constexpr int VB = 256;  // small blocks: more of them in flight for this latency-bound gather
    // items on XCDs (k_vertex_grad): a multiple of 8 items
    const int xcd_items = a->batch_size % 8 == 0 && a->num_vertices > 0;
    const long long vblocks = xcd_items ? (long long)a->batch_size * ((a->num_vertices + VB - 1) / VB) : (nv + VB - 1) / VB;
    const long long vgrad_threads = vblocks * VB;
    // (up to 16 texels per thread: the car's texture-gradient output rides on its k_vertex_grad blocks,
    // 0.022 + 0.0135 -> 0.031 ms; at 8 it had a launch of its own; same-box A/B, gpurun_out/o28)
    const bool carry = nv > 0 && to.n <= 16 * vgrad_threads;
    if (nv > 0) {
        {
            ProfScope _p(P_VGRAD, st, true);
            nr_launch(k_vertex_grad, dim3((unsigned)vblocks), dim3(VB), 0, st, gF, a->vertex_offsets,
                               a->vertex_faces, grad_vertices, a->num_faces, a->num_vertices, nv, carry ? to : TexOut{},
                               xcd_items);
        }
        e = check_launch("k_vertex_grad");
        if (e) return e;
    }
    if (to.out && to.n > 0 && !carry) {
        {
            ProfScope _p(P_TEXOUT, st, true);
            nr_launch(k_tex_out, grid_1d(to.n, 256), dim3(256), 0, st, to);
        }
        e = check_launch("k_tex_out");
    }
    return e;
}

int nr_rasterize_backward_params(const NrRasterArgs* a, const float* grad_images, float* grad_vertices_textures,
                                 float* grad_lights, void* stream) {
    int e = validate_raster(a, false);
    if (e) return e;
    const bool rgb = (a->draw_flags & NR_DRAW_RGB) != 0;
    const bool uv = rgb && grad_vertices_textures, lgt = rgb && grad_lights && a->num_lights > 0;
    if ((grad_vertices_textures || grad_lights) && !rgb) return fail(NR_ERR_ARGS, "parameter gradients need NR_DRAW_RGB");
    if (a->face_index_sparse && (grad_vertices_textures || grad_lights))
        return fail(NR_ERR_ARGS, "parameter gradients read every face id: the forward must not use face_index_sparse");
    if (grad_lights && a->num_lights > 0 && !a->vertex_normals) return fail(NR_ERR_ARGS, "lights need vertex_normals");
    hipStream_t st = (hipStream_t)stream;
    const int B = a->batch_size;
    const long long gvt_bstride = (long long)a->num_vertices_textures * 2;
    if (uv) {
        const size_t n = (size_t)(a->vt_batch_stride ? B : 1) * gvt_bstride * sizeof(float);
        if (n && !zero_async(grad_vertices_textures, n, st, &e)) return e;
    }
    if (lgt) {
        const size_t n = (size_t)a->num_lights * B * NR_LIGHT_FLOATS * sizeof(float);
        if (n && !zero_async(grad_lights, n, st, &e)) return e;
    }
    if (B == 0 || a->num_faces == 0 || !(uv || lgt)) return NR_OK;
    if (!grad_images) return fail(NR_ERR_ARGS, "null grad_images");
    const int S = internal_size(a->anti_aliasing, a->image_size);
    BwdArgs ba = {};
    ba.face_records = a->face_records;
    ba.fim = a->face_index;
    ba.grad_images = grad_images;
    ba.F = a->num_faces;
    ba.aa = a->anti_aliasing;
    ba.s = a->image_size;
    const Shade sh = make_shade(a);  // the lights shade (cw) the uv gradient even without light gradients
    const dim3 grid = grid_1d((long long)S * S, 256, B);
    auto kernel = k_param_bwd<true, true>;  // <UV, LGT>: at least one of the two is wanted here
    if (!lgt) kernel = k_param_bwd<true, false>;
    if (!uv) kernel = k_param_bwd<false, true>;
    nr_launch(kernel, grid, dim3(256), 0, st, ba, sh, S, a->faces_textures, grad_vertices_textures, gvt_bstride, grad_lights);
    return check_launch("k_param_bwd");
}

static int validate_camera(const NrCameraArgs* c) {
    if (!c) return fail(NR_ERR_ARGS, "null camera args");
    if (c->batch_size < 0 || c->num_vertices < 0) return fail(NR_ERR_ARGS, "bad sizes B=%d V=%d", c->batch_size, c->num_vertices);
    if (c->mode != NR_CAMERA_NONE && c->mode != NR_CAMERA_LOOK_AT && c->mode != NR_CAMERA_LOOK) return fail(NR_ERR_ARGS, "bad camera mode %d", c->mode);
    if ((long long)c->batch_size * c->num_vertices > 0 && !c->vertices) return fail(NR_ERR_ARGS, "null vertices");
    if (c->mode != NR_CAMERA_NONE && c->batch_size > 0 && !c->eye) return fail(NR_ERR_ARGS, "null eye");
    return NR_OK;
}

size_t nr_camera_workspace_bytes(int batch_size) { return batch_size > 0 ? align_up((size_t)batch_size * 12 * 4) : 0; }

int nr_camera_forward(const NrCameraArgs* c, float* out, void* stream) {
    int e = validate_camera(c);
    if (e) return e;
    const long long n = (long long)c->batch_size * c->num_vertices;
    if (n == 0) return NR_OK;
    if (!out) return fail(NR_ERR_ARGS, "null output");
    nr_launch(k_camera_fwd, grid_1d(n, 256), dim3(256), 0, (hipStream_t)stream, *c, out);
    return check_launch("k_camera_fwd");
}

int nr_camera_backward(const NrCameraArgs* c, const float* grad_out, float* grad_vertices, float* grad_eye,
                       void* workspace, size_t workspace_bytes, void* stream) {
    int e = validate_camera(c);
    if (e) return e;
    hipStream_t st = (hipStream_t)stream;
    const bool want_eye = grad_eye && c->mode != NR_CAMERA_NONE;
    const int neye = c->eye_batch_stride ? c->batch_size : 1;
    if (grad_eye && !want_eye) {  // no eye in the transform: zero gradient
        if (!zero_async(grad_eye, (size_t)neye * 3 * 4, st, &e)) return e;
        grad_eye = nullptr;
    }
    const long long nv = (long long)(c->v_batch_stride ? c->batch_size : 1) * c->num_vertices;
    if (c->batch_size == 0) {
        if (grad_vertices && nv > 0 && !zero_async(grad_vertices, (size_t)nv * 12, st, &e)) return e;
        if (want_eye && !zero_async(grad_eye, (size_t)neye * 12, st, &e)) return e;
        return NR_OK;
    }
    if (!grad_out && (grad_vertices || want_eye)) return fail(NR_ERR_ARGS, "null grad_out");
    float* acc = nullptr;
    if (want_eye) {
        if (!workspace || workspace_bytes < nr_camera_workspace_bytes(c->batch_size))
            return fail(NR_ERR_WORKSPACE, "camera workspace missing or too small");
        acc = (float*)workspace;
        if (!zero_async(acc, (size_t)c->batch_size * 12 * 4, st, &e)) return e;
    }
    if ((grad_vertices || acc) && nv > 0) {
        nr_launch(k_camera_bwd, grid_1d(nv, 256), dim3(256), 0, st, *c, grad_out, grad_vertices, acc);
        e = check_launch("k_camera_bwd");
        if (e) return e;
    }
    if (want_eye) {
        if (nv == 0 && !zero_async(acc, (size_t)c->batch_size * 12 * 4, st, &e)) return e;
        nr_launch(k_camera_eye, grid_1d(neye, 64), dim3(64), 0, st, *c, acc, grad_eye);
        e = check_launch("k_camera_eye");
    }
    return e;
}

size_t nr_projection_args_size(void) { return sizeof(NrProjectionArgs); }

static int proj_blocks(int num_vertices) { return (int)(((long long)num_vertices + PROJ_BLOCK - 1) / PROJ_BLOCK); }

static int validate_projection(const NrProjectionArgs* p) {
    if (!p) return fail(NR_ERR_ARGS, "null projection args");
    if (p->batch_size < 0 || p->num_vertices < 0) return fail(NR_ERR_ARGS, "bad sizes B=%d V=%d", p->batch_size, p->num_vertices);
    if (p->v_batch_stride < 0 || p->k_batch_stride < 0 || p->r_batch_stride < 0 || p->t_batch_stride < 0 ||
        p->dist_batch_stride < 0)
        return fail(NR_ERR_ARGS, "negative batch stride");
    if (p->batch_size == 0 || p->num_vertices == 0) return NR_OK;
    if (!p->vertices) return fail(NR_ERR_ARGS, "null vertices");
    if (!p->K || !p->R || !p->t) return fail(NR_ERR_ARGS, "null K, R or t");
    if (!(p->orig_size > 0.f) || !(p->orig_size < INFINITY)) return fail(NR_ERR_ARGS, "bad orig_size %g", (double)p->orig_size);
    if ((long long)p->batch_size * proj_blocks(p->num_vertices) > INT_MAX)
        return fail(NR_ERR_ARGS, "too many vertices B=%d V=%d", p->batch_size, p->num_vertices);
    return NR_OK;
}

size_t nr_projection_workspace_bytes(int batch_size, int num_vertices) {
    if (batch_size <= 0 || num_vertices <= 0) return 0;
    return align_up((size_t)batch_size * proj_blocks(num_vertices) * PROJ_SLOT * 4);
}

int nr_projection_forward(const NrProjectionArgs* p, float* out, void* stream) {
    int e = validate_projection(p);
    if (e) return e;
    if (p->batch_size == 0 || p->num_vertices == 0) return NR_OK;
    if (!out) return fail(NR_ERR_ARGS, "null output");
    const int nblk = proj_blocks(p->num_vertices);
    nr_launch(k_proj_fwd, dim3((unsigned)(p->batch_size * nblk)), dim3(PROJ_BLOCK), 0, (hipStream_t)stream, *p, nblk, out);
    return check_launch("k_proj_fwd");
}

int nr_projection_backward(const NrProjectionArgs* p, const float* grad_out, float* grad_vertices, float* grad_K,
                           float* grad_R, float* grad_t, float* grad_dist, void* workspace, size_t workspace_bytes,
                           void* stream) {
    int e = validate_projection(p);
    if (e) return e;
    hipStream_t st = (hipStream_t)stream;
    const int B = p->batch_size, V = p->num_vertices;
    if (B == 0 || V == 0) {  // nothing projected: zero gradients
        const struct { float* g; size_t n; } fill[5] = {
            {grad_vertices, (size_t)(p->v_batch_stride ? B : 1) * V * 3}, {grad_K, (size_t)(p->k_batch_stride ? B : 1) * 9},
            {grad_R, (size_t)(p->r_batch_stride ? B : 1) * 9},           {grad_t, (size_t)(p->t_batch_stride ? B : 1) * 3},
            {grad_dist, (size_t)(p->dist_batch_stride ? B : 1) * 5}};
        for (const auto& f : fill)
            if (f.g && f.n && !zero_async(f.g, f.n * 4, st, &e)) return e;
        return NR_OK;
    }
    const bool params = grad_K || grad_R || grad_t || grad_dist;
    if (!grad_vertices && !params) return NR_OK;
    if (!grad_out) return fail(NR_ERR_ARGS, "null grad_out");
    if (params && (!workspace || workspace_bytes < nr_projection_workspace_bytes(B, V)))
        return fail(NR_ERR_WORKSPACE, "projection workspace missing or too small");
    const int nblk = proj_blocks(V);
    float* slab = params ? (float*)workspace : nullptr;
    nr_launch(k_proj_bwd, dim3((unsigned)((p->v_batch_stride ? B : 1) * nblk)), dim3(PROJ_BLOCK), 0, st, *p, nblk, grad_out,
              grad_vertices, slab);
    e = check_launch("k_proj_bwd");
    if (e || !params) return e;
    const bool per_item = (grad_K && p->k_batch_stride) || (grad_R && p->r_batch_stride) || (grad_t && p->t_batch_stride) ||
                          (grad_dist && p->dist_batch_stride);
    nr_launch(k_proj_params, dim3((unsigned)(per_item ? B : 1)), dim3(PROJ_BLOCK), 0, st, *p, nblk, slab, grad_K, grad_R, grad_t,
              grad_dist);
    return check_launch("k_proj_params");
}

// ---- mesh regularizers (nr_mesh_loss.h) ----
static long long ml_blocks(int count) { return ((long long)count + ML_BLOCK - 1) / ML_BLOCK; }

static int validate_mesh_loss(int B, int V, int E2) {
    if (B < 0 || V < 0 || E2 < 0) return fail(NR_ERR_ARGS, "bad sizes B=%d V=%d E2=%d", B, V, E2);
    if (E2 > INT_MAX / 4) return fail(NR_ERR_ARGS, "too many edges E2=%d (4 * E2 must stay below 2^31)", E2);
    if ((long long)B * ml_blocks(V) > INT_MAX || (long long)B * ml_blocks(E2) > INT_MAX)
        return fail(NR_ERR_ARGS, "too many vertices or edges B=%d V=%d E2=%d", B, V, E2);
    return NR_OK;
}

size_t nr_mesh_loss_workspace_bytes(int batch_size, int count) {
    if (batch_size <= 0 || count <= 0) return 0;
    return align_up((size_t)batch_size * (size_t)ml_blocks(count) * 4);
}

int nr_laplacian_forward(const float* vertices, const int32_t* nbr_offsets, const int32_t* nbr_index, int batch_size,
                         int num_vertices, float* delta, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
    const int B = batch_size, V = num_vertices;
    int e = validate_mesh_loss(B, V, 0);
    if (e) return e;
    if (B == 0) return NR_OK;
    if (!loss) return fail(NR_ERR_ARGS, "null loss");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (int)ml_blocks(V);
    if (V > 0) {
        if (!vertices || !nbr_offsets) return fail(NR_ERR_ARGS, "null vertices or nbr_offsets");
        if (!workspace || workspace_bytes < nr_mesh_loss_workspace_bytes(B, V))
            return fail(NR_ERR_WORKSPACE, "mesh loss workspace missing or too small");
        nr_launch(k_lap_fwd, dim3((unsigned)(B * nblk)), dim3(ML_BLOCK), 0, st, vertices, nbr_offsets, nbr_index, V, nblk, delta,
                  (float*)workspace);
        e = check_launch("k_lap_fwd");
        if (e) return e;
    }
    nr_launch(k_mesh_loss_sum, dim3((unsigned)B), dim3(ML_BLOCK), 0, st, (const float*)workspace, nblk, loss);
    return check_launch("k_mesh_loss_sum");
}

int nr_laplacian_backward(const float* delta, const int32_t* nbr_offsets, const int32_t* nbr_index, const float* grad_loss,
                          int batch_size, int num_vertices, float* grad_vertices, void* stream) {
    const int B = batch_size, V = num_vertices;
    int e = validate_mesh_loss(B, V, 0);
    if (e) return e;
    if (B == 0 || V == 0) return NR_OK;
    if (!delta || !nbr_offsets || !grad_loss || !grad_vertices) return fail(NR_ERR_ARGS, "null pointer");
    const int nblk = (int)ml_blocks(V);
    nr_launch(k_lap_bwd, dim3((unsigned)(B * nblk)), dim3(ML_BLOCK), 0, (hipStream_t)stream, delta, nbr_offsets, nbr_index,
              grad_loss, V, nblk, grad_vertices);
    return check_launch("k_lap_bwd");
}

int nr_flatten_forward(const float* vertices, const int32_t* edges, int batch_size, int num_vertices, int num_edges, float eps,
                       float* records, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
    const int B = batch_size, V = num_vertices, E2 = num_edges;
    int e = validate_mesh_loss(B, V, E2);
    if (e) return e;
    if (B == 0) return NR_OK;
    if (!loss) return fail(NR_ERR_ARGS, "null loss");
    if (!(eps >= 0.f) || !(eps < INFINITY)) return fail(NR_ERR_ARGS, "bad eps %g", (double)eps);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (int)ml_blocks(E2);
    if (E2 > 0) {
        if (V == 0 || !vertices || !edges) return fail(NR_ERR_ARGS, "edges without vertices");
        if (!workspace || workspace_bytes < nr_mesh_loss_workspace_bytes(B, E2))
            return fail(NR_ERR_WORKSPACE, "mesh loss workspace missing or too small");
        const auto kernel = records ? k_flat_fwd<true> : k_flat_fwd<false>;
        nr_launch(kernel, dim3((unsigned)(B * nblk)), dim3(ML_BLOCK), 0, st, vertices, edges, V, E2, nblk, eps, records,
                  (float*)workspace);
        e = check_launch("k_flat_fwd");
        if (e) return e;
    }
    nr_launch(k_mesh_loss_sum, dim3((unsigned)B), dim3(ML_BLOCK), 0, st, (const float*)workspace, nblk, loss);
    return check_launch("k_mesh_loss_sum");
}

int nr_flatten_backward(const float* records, const int32_t* edge_offsets, const int32_t* edge_slots, const float* grad_loss,
                        int batch_size, int num_vertices, int num_edges, float* grad_vertices, void* stream) {
    const int B = batch_size, V = num_vertices, E2 = num_edges;
    int e = validate_mesh_loss(B, V, E2);
    if (e) return e;
    if (B == 0 || V == 0) return NR_OK;
    if (!edge_offsets || !grad_loss || !grad_vertices) return fail(NR_ERR_ARGS, "null pointer");
    if (E2 > 0 && (!edge_slots || !records)) return fail(NR_ERR_ARGS, "null records or edge_slots");
    const int nblk = (int)ml_blocks(V);
    nr_launch(k_flat_bwd_gather, dim3((unsigned)(B * nblk)), dim3(ML_BLOCK), 0, (hipStream_t)stream, records, edge_offsets,
              edge_slots, grad_loss, V, E2, nblk, grad_vertices);
    return check_launch("k_flat_bwd_gather");
}

int nr_edge_length_forward(const float* vertices, const int32_t* nbr_offsets, const int32_t* nbr_index, int batch_size,
                           int num_vertices, float target_length, float* loss, void* workspace, size_t workspace_bytes,
                           void* stream) {
    const int B = batch_size, V = num_vertices;
    int e = validate_mesh_loss(B, V, 0);
    if (e) return e;
    if (B == 0) return NR_OK;
    if (!loss) return fail(NR_ERR_ARGS, "null loss");
    if (!(target_length >= 0.f) || !(target_length < INFINITY))
        return fail(NR_ERR_ARGS, "bad target_length %g", (double)target_length);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (int)ml_blocks(V);
    if (V > 0) {
        if (!vertices || !nbr_offsets) return fail(NR_ERR_ARGS, "null vertices or nbr_offsets");
        if (!workspace || workspace_bytes < nr_mesh_loss_workspace_bytes(B, V))
            return fail(NR_ERR_WORKSPACE, "mesh loss workspace missing or too small");
        nr_launch(k_edge_fwd, dim3((unsigned)(B * nblk)), dim3(ML_BLOCK), 0, st, vertices, nbr_offsets, nbr_index, V, nblk,
                  target_length, (float*)workspace);
        e = check_launch("k_edge_fwd");
        if (e) return e;
    }
    nr_launch(k_mesh_loss_sum, dim3((unsigned)B), dim3(ML_BLOCK), 0, st, (const float*)workspace, nblk, loss);
    return check_launch("k_mesh_loss_sum");
}

int nr_edge_length_backward(const float* vertices, const int32_t* nbr_offsets, const int32_t* nbr_index, const float* grad_loss,
                            int batch_size, int num_vertices, float target_length, float* grad_vertices, void* stream) {
    const int B = batch_size, V = num_vertices;
    int e = validate_mesh_loss(B, V, 0);
    if (e) return e;
    if (!(target_length >= 0.f) || !(target_length < INFINITY))
        return fail(NR_ERR_ARGS, "bad target_length %g", (double)target_length);
    if (B == 0 || V == 0) return NR_OK;
    if (!vertices || !nbr_offsets || !grad_loss || !grad_vertices) return fail(NR_ERR_ARGS, "null pointer");
    const int nblk = (int)ml_blocks(V);
    nr_launch(k_edge_bwd, dim3((unsigned)(B * nblk)), dim3(ML_BLOCK), 0, (hipStream_t)stream, vertices, nbr_offsets, nbr_index,
              grad_loss, V, nblk, target_length, grad_vertices);
    return check_launch("k_edge_bwd");
}

// num_neighbours: the entries of the neighbour CSR, below 2^31 as an int
static int validate_cot_laplacian(int B, int V, int F, int nnz) {
    if (F < 0 || nnz < 0) return fail(NR_ERR_ARGS, "bad sizes F=%d num_neighbours=%d", F, nnz);
    int e = validate_mesh_loss(B, V, 0);
    if (e) return e;
    if (F > INT_MAX / 3) return fail(NR_ERR_ARGS, "too many faces F=%d (3 * F must stay below 2^31)", F);
    if ((long long)B * ml_blocks(F) > INT_MAX) return fail(NR_ERR_ARGS, "too many faces B=%d F=%d", B, F);
    return NR_OK;
}

size_t nr_cot_laplacian_workspace_bytes(int batch_size, int num_vertices, int num_faces) {
    if (batch_size <= 0 || num_vertices <= 0 || num_faces < 0 || num_faces > INT_MAX / 3) return 0;
    return cot_layout(batch_size, num_vertices, num_faces).total;
}

int nr_cot_laplacian_forward(const float* vertices, const int32_t* faces, const int32_t* nbr_offsets, const int32_t* nbr_index,
                             const int32_t* nbr_corner_offsets, const int32_t* nbr_corners, int batch_size, int num_vertices,
                             int num_faces, int num_neighbours, float eps, float* delta, float* w, float* winv, float* loss,
                             void* workspace, size_t workspace_bytes, void* stream) {
    const int B = batch_size, V = num_vertices, F = num_faces, nnz = num_neighbours;
    int e = validate_cot_laplacian(B, V, F, nnz);
    if (e) return e;
    if (B == 0) return NR_OK;
    if (!loss) return fail(NR_ERR_ARGS, "null loss");
    if (!(eps >= 0.f) || !(eps < INFINITY)) return fail(NR_ERR_ARGS, "bad eps %g", (double)eps);
    if (V == 0 && (F > 0 || nnz > 0)) return fail(NR_ERR_ARGS, "faces or neighbours without vertices");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (int)ml_blocks(V);
    float* partial = nullptr;
    if (V > 0) {
        if (!vertices || !nbr_offsets) return fail(NR_ERR_ARGS, "null vertices or nbr_offsets");
        if (nnz > 0 && (!nbr_index || !nbr_corner_offsets || !nbr_corners || !faces || F == 0))
            return fail(NR_ERR_ARGS, "neighbours without nbr_index, corner lists or faces");
        if (F > 0 && !faces) return fail(NR_ERR_ARGS, "null faces");
        const CotLayout lay = cot_layout(B, V, F);
        if (!workspace || workspace_bytes < lay.total)
            return fail(NR_ERR_WORKSPACE, "cotangent Laplacian workspace missing or too small");
        partial = (float*)((char*)workspace + lay.partial);
        float* cot = (float*)((char*)workspace + lay.cot);
        if (F > 0) {
            const int fblk = (int)ml_blocks(F);
            nr_launch(k_cot_face, dim3((unsigned)(B * fblk)), dim3(ML_BLOCK), 0, st, vertices, faces, V, F, fblk, eps, cot);
            e = check_launch("k_cot_face");
            if (e) return e;
        }
        nr_launch(k_cotlap_fwd, dim3((unsigned)(B * nblk)), dim3(ML_BLOCK), 0, st, vertices, nbr_offsets, nbr_index,
                  nbr_corner_offsets, nbr_corners, (const float*)cot, V, F, nnz, nblk, w, winv, delta, partial);
        e = check_launch("k_cotlap_fwd");
        if (e) return e;
    }
    nr_launch(k_mesh_loss_sum, dim3((unsigned)B), dim3(ML_BLOCK), 0, st, (const float*)partial, nblk, loss);
    return check_launch("k_mesh_loss_sum");
}

int nr_cot_laplacian_backward(const float* delta, const float* w, const float* winv, const int32_t* nbr_offsets,
                              const int32_t* nbr_index, const float* grad_loss, int batch_size, int num_vertices,
                              int num_neighbours, float* grad_vertices, void* stream) {
    const int B = batch_size, V = num_vertices, nnz = num_neighbours;
    int e = validate_cot_laplacian(B, V, 0, nnz);
    if (e) return e;
    if (B == 0 || V == 0) return NR_OK;
    if (!delta || !winv || !nbr_offsets || !grad_loss || !grad_vertices) return fail(NR_ERR_ARGS, "null pointer");
    if (nnz > 0 && (!w || !nbr_index)) return fail(NR_ERR_ARGS, "null w or nbr_index");
    const int nblk = (int)ml_blocks(V);
    nr_launch(k_cotlap_bwd, dim3((unsigned)(B * nblk)), dim3(ML_BLOCK), 0, (hipStream_t)stream, delta, w, winv, nbr_offsets,
              nbr_index, grad_loss, V, nnz, nblk, grad_vertices);
    return check_launch("k_cotlap_bwd");
}

// ---- as-rigid-as-possible energy (nr_arap.h) ----
size_t nr_cot_weights_workspace_bytes(int batch_size, int num_faces) {
    if (batch_size <= 0 || num_faces <= 0 || num_faces > INT_MAX / 3) return 0;
    return align_up((size_t)batch_size * num_faces * 3 * 4);
}

int nr_cot_weights(const float* vertices, const int32_t* faces, const int32_t* nbr_corner_offsets, const int32_t* nbr_corners,
                   int batch_size, int num_vertices, int num_faces, int num_neighbours, float eps, float* w, void* workspace,
                   size_t workspace_bytes, void* stream) {
    const int B = batch_size, V = num_vertices, F = num_faces, nnz = num_neighbours;
    int e = validate_cot_laplacian(B, V, F, nnz);
    if (e) return e;
    if ((long long)B * ml_blocks(nnz) > INT_MAX) return fail(NR_ERR_ARGS, "too many neighbours B=%d num_neighbours=%d", B, nnz);
    if (!(eps >= 0.f) || !(eps < INFINITY)) return fail(NR_ERR_ARGS, "bad eps %g", (double)eps);
    if (B == 0 || nnz == 0) return NR_OK;
    if (V == 0 || F == 0) return fail(NR_ERR_ARGS, "neighbours without vertices or faces");
    if (!vertices || !faces || !nbr_corner_offsets || !nbr_corners || !w) return fail(NR_ERR_ARGS, "null pointer");
    if (!workspace || workspace_bytes < nr_cot_weights_workspace_bytes(B, F))
        return fail(NR_ERR_WORKSPACE, "cotangent weights workspace missing or too small");
    hipStream_t st = (hipStream_t)stream;
    float* cot = (float*)workspace;
    const int fblk = (int)ml_blocks(F), eblk = (int)ml_blocks(nnz);
    nr_launch(k_cot_face, dim3((unsigned)(B * fblk)), dim3(ML_BLOCK), 0, st, vertices, faces, V, F, fblk, eps, cot);
    e = check_launch("k_cot_face");
    if (e) return e;
    nr_launch(k_cot_entry, dim3((unsigned)(B * eblk)), dim3(ML_BLOCK), 0, st, nbr_corner_offsets, nbr_corners, (const float*)cot, F,
              nnz, eblk, w);
    return check_launch("k_cot_entry");
}

// an item stride is 0 (shared by the items) or the item's own size
static int validate_arap(int B, int V, int nnz, long long rest_bs, const float* w, long long w_bs) {
    if (nnz < 0) return fail(NR_ERR_ARGS, "bad size num_neighbours=%d", nnz);
    int e = validate_mesh_loss(B, V, 0);
    if (e) return e;
    if (rest_bs != 0 && rest_bs != (long long)V * 3)
        return fail(NR_ERR_ARGS, "rest_batch_stride %lld is neither 0 nor 3 V = %lld", rest_bs, (long long)V * 3);
    if (w && w_bs != 0 && w_bs != (long long)nnz)
        return fail(NR_ERR_ARGS, "w_batch_stride %lld is neither 0 nor num_neighbours = %d", w_bs, nnz);
    return NR_OK;
}

size_t nr_arap_workspace_bytes(int batch_size, int num_vertices) { return nr_mesh_loss_workspace_bytes(batch_size, num_vertices); }

int nr_arap_forward(const float* vertices, const float* rest, long long rest_batch_stride, const float* w, long long w_batch_stride,
                    const int32_t* nbr_offsets, const int32_t* nbr_index, int batch_size, int num_vertices, int num_neighbours,
                    float* rotations, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
    const int B = batch_size, V = num_vertices, nnz = num_neighbours;
    int e = validate_arap(B, V, nnz, rest_batch_stride, w, w_batch_stride);
    if (e) return e;
    if (B == 0) return NR_OK;
    if (!loss) return fail(NR_ERR_ARGS, "null loss");
    if (V == 0 && nnz > 0) return fail(NR_ERR_ARGS, "neighbours without vertices");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (int)ml_blocks(V);
    if (V > 0) {
        if (!vertices || !rest || !nbr_offsets) return fail(NR_ERR_ARGS, "null vertices, rest or nbr_offsets");
        if (nnz > 0 && !nbr_index) return fail(NR_ERR_ARGS, "neighbours without nbr_index");
        if (((uintptr_t)rotations & 15) != 0) return fail(NR_ERR_ARGS, "rotations must be 16-byte aligned");
        if (!workspace || workspace_bytes < nr_arap_workspace_bytes(B, V))
            return fail(NR_ERR_WORKSPACE, "arap workspace missing or too small");
        nr_launch(k_arap_fwd, dim3((unsigned)(B * nblk)), dim3(ML_BLOCK), 0, st, vertices, rest, rest_batch_stride, w, w_batch_stride,
                  nbr_offsets, nbr_index, V, nblk, (float4*)rotations, (float*)workspace);
        e = check_launch("k_arap_fwd");
        if (e) return e;
    }
    nr_launch(k_mesh_loss_sum, dim3((unsigned)B), dim3(ML_BLOCK), 0, st, (const float*)workspace, nblk, loss);
    return check_launch("k_mesh_loss_sum");
}

int nr_arap_backward(const float* vertices, const float* rest, long long rest_batch_stride, const float* w, long long w_batch_stride,
                     const float* rotations, const int32_t* nbr_offsets, const int32_t* nbr_index, const float* grad_loss,
                     int batch_size, int num_vertices, int num_neighbours, float* grad_vertices, void* stream) {
    const int B = batch_size, V = num_vertices, nnz = num_neighbours;
    int e = validate_arap(B, V, nnz, rest_batch_stride, w, w_batch_stride);
    if (e) return e;
    if (B == 0 || V == 0) return NR_OK;
    if (!vertices || !rest || !rotations || !nbr_offsets || !grad_loss || !grad_vertices) return fail(NR_ERR_ARGS, "null pointer");
    if (nnz > 0 && !nbr_index) return fail(NR_ERR_ARGS, "neighbours without nbr_index");
    if (((uintptr_t)rotations & 15) != 0) return fail(NR_ERR_ARGS, "rotations must be 16-byte aligned");
    const int nblk = (int)ml_blocks(V);
    nr_launch(k_arap_bwd, dim3((unsigned)(B * nblk)), dim3(ML_BLOCK), 0, (hipStream_t)stream, vertices, rest, rest_batch_stride, w,
              w_batch_stride, (const float4*)rotations, nbr_offsets, nbr_index, grad_loss, V, nblk, grad_vertices);
    return check_launch("k_arap_bwd");
}

// ---- articulated meshes (nr_skinning.h) ----
static int validate_pose(int B, int J, int L, long long joints_bstride) {
    if (B < 0) return fail(NR_ERR_ARGS, "bad batch size B=%d", B);
    if (J < 1 || J > NR_SKIN_MAX_JOINTS) return fail(NR_ERR_ARGS, "bad joint count J=%d (1 to %d)", J, NR_SKIN_MAX_JOINTS);
    if (L < 1 || L > J) return fail(NR_ERR_ARGS, "bad level count L=%d for J=%d joints", L, J);
    if (joints_bstride != 0 && joints_bstride != (long long)J * 3)
        return fail(NR_ERR_ARGS, "joints_batch_stride %lld is neither 0 nor 3 J = %d", joints_bstride, J * 3);
    return NR_OK;
}

int nr_pose_transforms_forward(const float* pose, int pose_is_matrix, const float* joints, long long joints_batch_stride,
                               const int32_t* parents, const int32_t* level_offsets, const int32_t* level_joints, int batch_size,
                               int num_joints, int num_levels, float* transforms, float* posed_joints, void* stream) {
    const int B = batch_size, J = num_joints, L = num_levels;
    int e = validate_pose(B, J, L, joints_batch_stride);
    if (e) return e;
    if (!pose || !joints || !parents || !level_offsets || !level_joints) return fail(NR_ERR_ARGS, "null pose, joints or skeleton");
    if (!transforms || !posed_joints) return fail(NR_ERR_ARGS, "null transforms or posed_joints");
    if (B == 0) return NR_OK;
    nr_launch(k_pose_fwd, dim3((unsigned)B), dim3(SK_BLOCK), 0, (hipStream_t)stream, pose, pose_is_matrix ? 1 : 0, joints,
              joints_batch_stride, parents, level_offsets, level_joints, J, L, transforms, posed_joints);
    return check_launch("k_pose_fwd");
}

int nr_pose_transforms_backward(const float* pose, int pose_is_matrix, const float* joints, long long joints_batch_stride,
                                const int32_t* parents, const int32_t* level_offsets, const int32_t* level_joints,
                                const int32_t* child_offsets, const int32_t* children, const float* transforms,
                                const float* grad_transforms, const float* grad_posed_joints, int batch_size, int num_joints,
                                int num_levels, float* grad_pose, float* grad_joints, void* stream) {
    const int B = batch_size, J = num_joints, L = num_levels;
    int e = validate_pose(B, J, L, joints_batch_stride);
    if (e) return e;
    if (!pose || !joints || !parents || !level_offsets || !level_joints) return fail(NR_ERR_ARGS, "null pose, joints or skeleton");
    // children may be NULL: a forest of roots alone has no child, and the kernel reads the list only inside a row
    if (!child_offsets) return fail(NR_ERR_ARGS, "null child_offsets");
    if (!transforms) return fail(NR_ERR_ARGS, "null transforms");
    if (!grad_pose && !grad_joints) return fail(NR_ERR_ARGS, "no gradient requested");
    if (B == 0) return NR_OK;
    nr_launch(k_pose_bwd, dim3((unsigned)B), dim3(SK_BLOCK), 0, (hipStream_t)stream, pose, pose_is_matrix ? 1 : 0, joints,
              joints_batch_stride, parents, level_offsets, level_joints, child_offsets, children, transforms, grad_transforms,
              grad_posed_joints, J, L, grad_pose, grad_joints);
    return check_launch("k_pose_bwd");
}

static int validate_skin(int B, int V, int J, int K, long long v_bstride) {
    if (B < 0 || V < 0) return fail(NR_ERR_ARGS, "bad sizes B=%d V=%d", B, V);
    if (B > 65535) return fail(NR_ERR_ARGS, "too many items B=%d (at most 65535)", B);
    if (J < 1 || J > NR_SKIN_MAX_JOINTS) return fail(NR_ERR_ARGS, "bad joint count J=%d (1 to %d)", J, NR_SKIN_MAX_JOINTS);
    if (K < 1 || K > NR_SKIN_MAX_INFLUENCES)
        return fail(NR_ERR_ARGS, "bad influence count K=%d (1 to %d)", K, NR_SKIN_MAX_INFLUENCES);
    if (V > INT_MAX / NR_SKIN_MAX_INFLUENCES) return fail(NR_ERR_ARGS, "too many vertices V=%d (8 V must stay below 2^31)", V);
    if (v_bstride != 0 && v_bstride != (long long)V * 3)
        return fail(NR_ERR_ARGS, "vertices_batch_stride %lld is neither 0 nor 3 V = %lld", v_bstride, (long long)V * 3);
    return NR_OK;
}

size_t nr_skin_workspace_bytes(int batch_size, int num_chunks) {
    if (batch_size <= 0 || num_chunks <= 0) return 0;
    return skin_layout(batch_size, num_chunks).total;
}

int nr_skin_forward(const float* vertices, long long vertices_batch_stride, const float* transforms, const float* weights,
                    const int32_t* indices, int batch_size, int num_vertices, int num_joints, int num_influences, float* out,
                    void* stream) {
    const int B = batch_size, V = num_vertices, J = num_joints, K = num_influences;
    int e = validate_skin(B, V, J, K, vertices_batch_stride);
    if (e) return e;
    if (B == 0 || V == 0) return NR_OK;
    if (!vertices || !transforms || !weights || !indices || !out) return fail(NR_ERR_ARGS, "null pointer");
    nr_launch(k_skin_fwd, grid_1d(V, SK_BLOCK, B), dim3(SK_BLOCK), 0, (hipStream_t)stream, vertices, vertices_batch_stride,
              transforms, weights, indices, V, J, K, out);
    return check_launch("k_skin_fwd");
}

int nr_skin_backward(const float* vertices, long long vertices_batch_stride, const float* transforms, const float* weights,
                     const int32_t* indices, const float* grad_out, const int32_t* entry_vertex, const int32_t* entry_slot,
                     const int32_t* chunk_begin, const int32_t* chunk_end, const int32_t* joint_chunk_offsets, int batch_size,
                     int num_vertices, int num_joints, int num_influences, int num_chunks, float* grad_vertices,
                     float* grad_transforms, float* grad_weights, void* workspace, size_t workspace_bytes, void* stream) {
    const int B = batch_size, V = num_vertices, J = num_joints, K = num_influences, NC = num_chunks;
    int e = validate_skin(B, V, J, K, vertices_batch_stride);
    if (e) return e;
    if (NC < 0) return fail(NR_ERR_ARGS, "bad chunk count %d", NC);
    if (!grad_vertices && !grad_transforms && !grad_weights) return fail(NR_ERR_ARGS, "no gradient requested");
    if (V > 0 && (!vertices || !transforms || !weights || !indices || !grad_out)) return fail(NR_ERR_ARGS, "null pointer");
    if (grad_transforms) {
        if (!joint_chunk_offsets) return fail(NR_ERR_ARGS, "grad_transforms without joint_chunk_offsets");
        if (NC > 0 && (V == 0 || !entry_vertex || !entry_slot || !chunk_begin || !chunk_end))
            return fail(NR_ERR_ARGS, "chunks without vertices, the joint CSR or the chunk table");
        if (B > 0 && NC > 0 && (!workspace || workspace_bytes < skin_layout(B, NC).total))
            return fail(NR_ERR_WORKSPACE, "skinning workspace missing or too small");
    }
    hipStream_t st = (hipStream_t)stream;
    const bool shared = vertices_batch_stride == 0;
    if (B == 0) {  // the sums over an empty batch
        if (V > 0 && grad_weights && !zero_async(grad_weights, (size_t)V * K * 4, st, &e)) return e;
        if (V > 0 && grad_vertices && shared && !zero_async(grad_vertices, (size_t)V * 3 * 4, st, &e)) return e;
        return NR_OK;
    }
    if (V > 0 && (grad_vertices || grad_weights)) {
        if (grad_weights || shared) {
            nr_launch(k_skin_bwd_vertices<true>, grid_1d(V, SK_BLOCK), dim3(SK_BLOCK), 0, st, vertices, vertices_batch_stride,
                      transforms, weights, indices, grad_out, B, V, J, K, grad_vertices, grad_weights);
        } else {
            nr_launch(k_skin_bwd_vertices<false>, grid_1d(V, SK_BLOCK, B), dim3(SK_BLOCK), 0, st, vertices,
                      vertices_batch_stride, transforms, weights, indices, grad_out, B, V, J, K, grad_vertices, grad_weights);
        }
        e = check_launch("k_skin_bwd_vertices");
        if (e) return e;
    }
    if (grad_transforms) {
        float* partial = NC > 0 ? (float*)((char*)workspace + skin_layout(B, NC).partial) : nullptr;
        if (NC > 0) {
            nr_launch(k_skin_bwd_transforms, dim3((unsigned)NC, (unsigned)B), dim3(SK_BLOCK), 0, st, vertices,
                      vertices_batch_stride, weights, grad_out, entry_vertex, entry_slot, chunk_begin, chunk_end, V, K, partial);
            e = check_launch("k_skin_bwd_transforms");
            if (e) return e;
        }
        const long long n = (long long)B * J * 12;
        nr_launch(k_skin_sum, grid_1d(n, SK_BLOCK), dim3(SK_BLOCK), 0, st, (const float*)partial, joint_chunk_offsets, n, J, NC,
                  grad_transforms);
        return check_launch("k_skin_sum");
    }
    return NR_OK;
}

// ---- point losses (nr_point_loss.h) ----
static int validate_chamfer(int B, int N, int M, int directions) {
    if (B < 0) return fail(NR_ERR_ARGS, "bad batch size B=%d", B);
    if (N <= 0 || M <= 0) return fail(NR_ERR_ARGS, "empty point set N=%d M=%d (both must be at least 1)", N, M);
    if (directions < 1 || directions > 3) return fail(NR_ERR_ARGS, "bad directions %d (1 x_to_y, 2 y_to_x, 3 both)", directions);
    if (B > 65535) return fail(NR_ERR_ARGS, "too many items B=%d (at most 65535)", B);
    if ((long long)B * (N > M ? N : M) > INT_MAX - 4096) return fail(NR_ERR_ARGS, "too many points B=%d N=%d M=%d", B, N, M);
    return NR_OK;
}

size_t nr_chamfer_workspace_bytes(int batch_size, int num_x, int num_y, int directions) {
    if (batch_size <= 0 || num_x <= 0 || num_y <= 0) return 0;
    return ((directions & NR_CHAMFER_X_TO_Y) ? chamfer_layout(batch_size, num_x, num_y).total : 0) +
           ((directions & NR_CHAMFER_Y_TO_X) ? chamfer_layout(batch_size, num_y, num_x).total : 0);
}

// The split path's tail, shared by every nearest-neighbour launch: a query's nsplit partials to the final arrays
// (k_chamfer_combine).  One range wrote there itself.
static int combine_split(const float* part_d2, const int32_t* part_index, int B, int nq, int nsplit, float* dist2, int32_t* index,
                         hipStream_t st) {
    if (nsplit == 1) return NR_OK;
    nr_launch(k_chamfer_combine, grid_1d(nq, PL_BLOCK, B), dim3(PL_BLOCK), 0, st, part_d2, part_index, nq, nsplit, dist2, index);
    return check_launch("k_chamfer_combine");
}

int nr_chamfer_forward(const float* x, const float* y, long long y_batch_stride, int batch_size, int num_x, int num_y,
                       int directions, int32_t* index_xy, int32_t* index_yx, float* dist2_xy, float* dist2_yx, float* loss,
                       void* workspace, size_t workspace_bytes, void* stream) {
    const int B = batch_size, N = num_x, M = num_y;
    int e = validate_chamfer(B, N, M, directions);
    if (e) return e;
    if (y_batch_stride < 0) return fail(NR_ERR_ARGS, "negative y batch stride");
    if (B == 0) return NR_OK;
    if (!x || !y) return fail(NR_ERR_ARGS, "null x or y");
    const bool xy = directions & NR_CHAMFER_X_TO_Y, yx = directions & NR_CHAMFER_Y_TO_X;
    if ((xy && !index_xy) || (yx && !index_yx)) return fail(NR_ERR_ARGS, "null index output of a requested direction");
    if (!loss && !(xy && dist2_xy) && !(yx && dist2_yx)) return fail(NR_ERR_ARGS, "null loss and no dist2 output");
    if (!workspace || workspace_bytes < nr_chamfer_workspace_bytes(B, N, M, directions))
        return fail(NR_ERR_ARGS, "chamfer workspace missing or too small");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    PlDir d[2] = {};
    float* fin_d[2] = {nullptr, nullptr};
    int32_t* fin_j[2] = {nullptr, nullptr};
    int nd = 0, flags = 0;
    for (int k = 0; k < 2; k++) {
        if (!(k == 0 ? xy : yx)) continue;
        const int nq = k == 0 ? N : M, nt = k == 0 ? M : N;
        const ChamferLayout wl = chamfer_layout(B, nq, nt);
        const SplitPlan p = wl.plan;
        PlDir& r = d[nd];
        r.q = k == 0 ? x : y, r.t = k == 0 ? y : x;
        r.q_stride = k == 0 ? (long long)N * 3 : y_batch_stride;
        r.t_stride = k == 0 ? y_batch_stride : (long long)N * 3;
        r.nq = nq, r.nt = nt, r.nqb = p.nqb, r.nsplit = p.nsplit;
        float* user = k == 0 ? dist2_xy : dist2_yx;
        fin_d[nd] = user ? user : (float*)(ws + wl.minima);
        fin_j[nd] = k == 0 ? index_xy : index_yx;
        if (p.nsplit > 1) {
            r.dist2 = (float*)(ws + wl.part_d2), r.index = (int32_t*)(ws + wl.part_j);
            flags |= k == 0 ? NR_LAUNCH_SPLIT_X_TO_Y : NR_LAUNCH_SPLIT_Y_TO_X;
        } else {
            r.dist2 = fin_d[nd], r.index = fin_j[nd];
        }
        ws += wl.total;
        nd++;
    }
    const int blocks0 = d[0].nqb * d[0].nsplit, blocks1 = nd > 1 ? d[1].nqb * d[1].nsplit : 0;
    if (nd == 1) d[1] = d[0];
    nr_launch(k_chamfer_nn, dim3((unsigned)(blocks0 + blocks1), (unsigned)B), dim3(PL_BLOCK), 0, st, d[0], d[1], blocks0);
    g_last_chamfer.store(LaunchRec{PL_BLOCK, flags});
    e = check_launch("k_chamfer_nn");
    if (e) return e;
    for (int k = 0; k < nd; k++) {
        e = combine_split(d[k].dist2, d[k].index, B, d[k].nq, d[k].nsplit, fin_d[k], fin_j[k], st);
        if (e) return e;
    }
    if (!loss) return NR_OK;
    const float* sxy = xy ? fin_d[0] : nullptr;
    const float* syx = yx ? fin_d[xy ? 1 : 0] : nullptr;
    nr_launch(k_chamfer_sum, dim3((unsigned)B), dim3(PL_WIDE), 0, st, sxy, N, syx, M, loss);
    return check_launch("k_chamfer_sum");
}

int nr_chamfer_backward(const float* x, const float* y, long long y_batch_stride, const int32_t* index_xy, const int32_t* index_yx,
                        const float* grad_loss, int batch_size, int num_x, int num_y, int directions, float* grad_x, float* grad_y,
                        void* stream) {
    const int B = batch_size, N = num_x, M = num_y;
    int e = validate_chamfer(B, N, M, directions);
    if (e) return e;
    if (y_batch_stride < 0) return fail(NR_ERR_ARGS, "negative y batch stride");
    if (B == 0 || (!grad_x && !grad_y)) return NR_OK;
    if (!x || !y || !grad_loss) return fail(NR_ERR_ARGS, "null x, y or grad_loss");
    const bool xy = directions & NR_CHAMFER_X_TO_Y, yx = directions & NR_CHAMFER_Y_TO_X;
    if ((xy && !index_xy) || (yx && !index_yx)) return fail(NR_ERR_ARGS, "null index array of a requested direction");
    PlSide s[2] = {};
    int ns = 0;
    if (grad_x) {
        PlSide& r = s[ns++];
        r.p = x, r.o = y, r.p_stride = (long long)N * 3, r.o_stride = y_batch_stride, r.np = N, r.no = M;
        r.own = xy ? index_xy : nullptr, r.other = yx ? index_yx : nullptr, r.grad = grad_x;
        r.nblk = (N + 63) / 64;
    }
    if (grad_y) {
        PlSide& r = s[ns++];
        r.p = y, r.o = x, r.p_stride = y_batch_stride, r.o_stride = (long long)N * 3, r.np = M, r.no = N;
        r.own = yx ? index_yx : nullptr, r.other = xy ? index_xy : nullptr, r.grad = grad_y;
        r.nblk = (M + 63) / 64;
    }
    const int blocks0 = s[0].nblk, blocks1 = ns > 1 ? s[1].nblk : 0;
    if (ns == 1) s[1] = s[0];
    nr_launch(k_chamfer_bwd, dim3((unsigned)(blocks0 + blocks1), (unsigned)B), dim3(PL_BWD_BLOCK), 0, (hipStream_t)stream, s[0], s[1],
              blocks0, grad_loss);
    return check_launch("k_chamfer_bwd");
}

static int validate_sample_points(int B, int V, int F, int S) {
    if (B < 0 || V < 0) return fail(NR_ERR_ARGS, "bad sizes B=%d V=%d", B, V);
    if (S <= 0) return fail(NR_ERR_ARGS, "no samples S=%d (must be at least 1)", S);
    if (F <= 0 || V == 0) return fail(NR_ERR_ARGS, "no faces to sample F=%d V=%d", F, V);
    if ((long long)B * S > INT_MAX || (long long)B * F > INT_MAX || (long long)B * V > INT_MAX / 3)
        return fail(NR_ERR_ARGS, "too many samples, faces or vertices B=%d S=%d F=%d V=%d", B, S, F, V);
    return NR_OK;
}

size_t nr_sample_points_workspace_bytes(int batch_size, int num_faces) {
    if (batch_size <= 0 || num_faces <= 0) return 0;
    return align_up((size_t)batch_size * num_faces * 4);
}

int nr_sample_points_forward(const float* vertices, const int32_t* faces, const float* u, int batch_size, int num_vertices,
                             int num_faces, int num_samples, float* points, int32_t* face, float* weights, void* workspace,
                             size_t workspace_bytes, void* stream) {
    const int B = batch_size, V = num_vertices, F = num_faces, S = num_samples;
    int e = validate_sample_points(B, V, F, S);
    if (e) return e;
    if (B == 0) return NR_OK;
    if (!vertices || !faces || !u || !points || !face || !weights) return fail(NR_ERR_ARGS, "null pointer");
    if (!workspace || workspace_bytes < nr_sample_points_workspace_bytes(B, F))
        return fail(NR_ERR_ARGS, "sample_points workspace missing or too small");
    hipStream_t st = (hipStream_t)stream;
    nr_launch(k_sample_scan, dim3((unsigned)B), dim3(PL_WIDE), 0, st, vertices, faces, V, F, (float*)workspace);
    e = check_launch("k_sample_scan");
    if (e) return e;
    const long long n = (long long)B * S;
    nr_launch(k_sample_points, grid_1d(n, PL_BLOCK), dim3(PL_BLOCK), 0, st, vertices, faces, u,
              (const float*)workspace, V, F, S, n, points, face, weights);
    return check_launch("k_sample_points");
}

int nr_sample_points_backward(const int32_t* faces, const int32_t* face, const float* weights, const float* grad_points,
                              int batch_size, int num_vertices, int num_faces, int num_samples, float* grad_vertices, void* stream) {
    const int B = batch_size, V = num_vertices, F = num_faces, S = num_samples;
    int e = validate_sample_points(B, V, F, S);
    if (e) return e;
    if (B == 0) return NR_OK;
    if (!faces || !face || !weights || !grad_points || !grad_vertices) return fail(NR_ERR_ARGS, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (!zero_async(grad_vertices, (size_t)B * V * 3 * 4, st, &e)) return e;
    const long long n = (long long)B * S;
    nr_launch(k_sample_points_bwd, grid_1d(n, PL_BLOCK), dim3(PL_BLOCK), 0, st, faces, face, weights,
              grad_points, V, S, n, grad_vertices);
    return check_launch("k_sample_points_bwd");
}

// ---- rigid registration (nr_rigid.h) ----
static int validate_rigid(int B, int N, int M, long long y_bs, const float* w, long long w_bs) {
    if (B < 0) return fail(NR_ERR_ARGS, "bad batch size B=%d", B);
    if (N <= 0 || M <= 0) return fail(NR_ERR_ARGS, "empty point set N=%d M=%d (both must be at least 1)", N, M);
    if (B > 65535) return fail(NR_ERR_ARGS, "too many items B=%d (at most 65535)", B);
    if ((long long)B * (N > M ? N : M) > INT_MAX - 4096) return fail(NR_ERR_ARGS, "too many points B=%d N=%d M=%d", B, N, M);
    if (y_bs != 0 && y_bs != (long long)M * 3)
        return fail(NR_ERR_ARGS, "y_batch_stride %lld is neither 0 nor 3 * %d", y_bs, M);
    if (w && w_bs != 0 && w_bs != (long long)N) return fail(NR_ERR_ARGS, "w_batch_stride %lld is neither 0 nor N = %d", w_bs, N);
    return NR_OK;
}

size_t nr_rigid_workspace_bytes(int batch_size, int num_points) {
    if (batch_size <= 0 || num_points <= 0) return 0;
    return rigid_layout(batch_size, num_points).total;
}

// Passes (a), (b) and (c) of nr_rigid.h on the pairs p: the solve of rigid_align and of one ICP update.
static int rigid_solve(const RgPairs& p, int B, const RigidLayout& wl, char* ws, int scale, int keep, const RgOut& out, hipStream_t st) {
    float* part_a = (float*)(ws + wl.sums);
    float* part_b = (float*)(ws + wl.moments);
    const dim3 grid((unsigned)wl.nchunk, (unsigned)B);
    nr_launch(k_rigid_sums, grid, dim3(RG_BLOCK), 0, st, p, wl.nchunk, part_a);
    int e = check_launch("k_rigid_sums");
    if (e) return e;
    nr_launch(k_rigid_moments, grid, dim3(RG_BLOCK), 0, st, p, wl.nchunk, (const float*)part_a, part_b);
    e = check_launch("k_rigid_moments");
    if (e) return e;
    nr_launch(k_rigid_solve, dim3((unsigned)B), dim3(RG_BLOCK), 0, st, p, wl.nchunk, (const float*)part_a, (const float*)part_b, scale,
              keep, 0, out);
    return check_launch("k_rigid_solve");
}

int nr_rigid_align_forward(const float* x, const float* y, long long y_batch_stride, const float* w, long long w_batch_stride,
                           int batch_size, int num_points, int scale, float* R, float* t, float* s, float* condition, float* record,
                           void* workspace, size_t workspace_bytes, void* stream) {
    const int B = batch_size, N = num_points;
    int e = validate_rigid(B, N, N, y_batch_stride, w, w_batch_stride);
    if (e) return e;
    if (B == 0) return NR_OK;
    if (!x || !y || !R || !t || !s) return fail(NR_ERR_ARGS, "null x, y, R, t or s");
    const RigidLayout wl = rigid_layout(B, N);
    if (!workspace || workspace_bytes < wl.total) return fail(NR_ERR_WORKSPACE, "rigid_align workspace missing or too small");
    RgPairs p = {};
    p.x = x, p.y = y, p.w = w, p.y_stride = y_batch_stride, p.w_stride = w_batch_stride, p.max_d2 = INFINITY, p.N = N;
    RgOut out = {};
    out.R = R, out.t = t, out.s = s, out.condition = condition, out.record = record;
    return rigid_solve(p, B, wl, (char*)workspace, scale != 0, 0, out, (hipStream_t)stream);
}

int nr_rigid_align_backward(const float* x, const float* y, long long y_batch_stride, const float* w, long long w_batch_stride,
                            const float* record, const float* grad_R, const float* grad_t, const float* grad_s, int batch_size,
                            int num_points, int scale, float* grad_x, float* grad_y, void* workspace, size_t workspace_bytes,
                            void* stream) {
    const int B = batch_size, N = num_points;
    int e = validate_rigid(B, N, N, y_batch_stride, w, w_batch_stride);
    if (e) return e;
    if (B == 0 || (!grad_x && !grad_y)) return NR_OK;
    if (!x || !y || !record) return fail(NR_ERR_ARGS, "null x, y or record");
    if (!workspace || workspace_bytes < rigid_layout(B, N).total)
        return fail(NR_ERR_WORKSPACE, "rigid_align workspace missing or too small");
    hipStream_t st = (hipStream_t)stream;
    float* gitem = (float*)workspace;
    nr_launch(k_rigid_bwd_item, grid_1d(B, RG_BLOCK), dim3(RG_BLOCK), 0, st, record, grad_R, grad_t, grad_s, B, scale != 0, gitem);
    e = check_launch("k_rigid_bwd_item");
    if (e) return e;
    RgPairs p = {};
    p.x = x, p.y = y, p.w = w, p.y_stride = y_batch_stride, p.w_stride = w_batch_stride, p.max_d2 = INFINITY, p.N = N;
    nr_launch(k_rigid_bwd_points, grid_1d(N, RG_BLOCK, B), dim3(RG_BLOCK), 0, st, p, record, (const float*)gitem, grad_x, grad_y);
    return check_launch("k_rigid_bwd_points");
}

size_t nr_icp_workspace_bytes(int batch_size, int num_x, int num_y) {
    if (batch_size <= 0 || num_x <= 0 || num_y <= 0) return 0;
    return icp_layout(batch_size, num_x, num_y).total;
}

int nr_icp(const float* x, const float* y, long long y_batch_stride, int batch_size, int num_x, int num_y, int iterations, int scale,
           float max_distance, float* transform, float* rmse, int32_t* index, float* dist2, void* workspace, size_t workspace_bytes,
           void* stream) {
    const int B = batch_size, N = num_x, M = num_y;
    int e = validate_rigid(B, N, M, y_batch_stride, nullptr, 0);
    if (e) return e;
    if (iterations < 0) return fail(NR_ERR_ARGS, "negative iterations %d", iterations);
    if (max_distance != max_distance) return fail(NR_ERR_ARGS, "max_distance is NaN");
    if (B == 0) return NR_OK;
    if (!x || !y || !transform || !rmse || !index || !dist2) return fail(NR_ERR_ARGS, "null pointer");
    const IcpLayout wl = icp_layout(B, N, M);
    if (!workspace || workspace_bytes < wl.total) return fail(NR_ERR_WORKSPACE, "icp workspace missing or too small");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const SplitPlan plan = wl.plan;
    IcpDir d = {};
    d.x = x, d.y = y, d.transform = transform, d.y_stride = y_batch_stride, d.nq = N, d.nt = M, d.nsplit = plan.nsplit;
    d.dist2 = plan.nsplit > 1 ? (float*)(ws + wl.part_d2) : dist2;
    d.index = plan.nsplit > 1 ? (int32_t*)(ws + wl.part_j) : index;
    RgPairs p = {};
    p.x = x, p.y = y, p.index = index, p.dist2 = dist2, p.y_stride = y_batch_stride, p.N = N;
    p.max_d2 = max_distance < 0.f ? INFINITY : max_distance * max_distance;
    for (int k = 0; k <= iterations; k++) {
        nr_launch(k_icp_nn, dim3((unsigned)(plan.nqb * plan.nsplit), (unsigned)B), dim3(PL_BLOCK), 0, st, d);
        g_last_icp.store(LaunchRec{PL_BLOCK, plan.nsplit > 1 ? NR_LAUNCH_SPLIT_TARGETS : 0});
        e = check_launch("k_icp_nn");
        if (e) return e;
        e = combine_split(d.dist2, d.index, B, N, plan.nsplit, dist2, index, st);
        if (e) return e;
        RgOut out = {};
        out.rmse = rmse + k, out.rmse_stride = iterations + 1;
        if (k < iterations) {
            out.transform = transform;
            e = rigid_solve(p, B, wl.rigid, ws, scale != 0, 1, out, st);
            if (e) return e;
        } else {  // the evaluation pass: rmse alone
            float* part_a = (float*)(ws + wl.rigid.sums);
            nr_launch(k_rigid_sums, dim3((unsigned)wl.rigid.nchunk, (unsigned)B), dim3(RG_BLOCK), 0, st, p, wl.rigid.nchunk, part_a);
            e = check_launch("k_rigid_sums");
            if (e) return e;
            nr_launch(k_rigid_solve, dim3((unsigned)B), dim3(RG_BLOCK), 0, st, p, wl.rigid.nchunk, (const float*)part_a,
                      (const float*)nullptr, 0, 1, 1, out);
            e = check_launch("k_rigid_solve");
            if (e) return e;
        }
    }
    return NR_OK;
}

// ---- point-to-surface and face-to-scan distance (nr_point_mesh.h, nr_face_point.h): one path, a PairDir each ----
// What every forward and backward of a direction starts with: the sizes and the stride; then, with nothing to
// do (B == 0, or nothing wanted), NR_OK and *go false: no pointer is needed; then the three inputs.
static int pair_begin(const PairDir& dir, int B, int N, int V, int F, long long points_batch_stride, bool wanted, const void* points,
                      const void* vertices, const void* faces, bool* go) {
    *go = false;
    if (B < 0) return fail(NR_ERR_ARGS, "bad batch size B=%d", B);
    if (N <= 0 || F <= 0 || V <= 0) return fail(NR_ERR_ARGS, "empty input N=%d F=%d V=%d (each must be at least 1)", N, F, V);
    if (B > 65535) return fail(NR_ERR_ARGS, "too many items B=%d (at most 65535)", B);
    if ((long long)B * dir.queries(N, F) > INT_MAX - 4096 || (long long)B * dir.targets(N, F) > INT_MAX ||
        (long long)B * V > INT_MAX / 3)
        return fail(NR_ERR_ARGS, "too many points, faces or vertices B=%d N=%d F=%d V=%d", B, N, F, V);
    if (points_batch_stride < 0) return fail(NR_ERR_ARGS, "negative points batch stride");
    if (B == 0 || !wanted) return NR_OK;
    if (!points || !vertices || !faces) return fail(NR_ERR_ARGS, "null points, vertices or faces");
    *go = true;
    return NR_OK;
}

static size_t pair_workspace_bytes(const PairDir& dir, int B, int N, int F) {
    return B <= 0 || N <= 0 || F <= 0 ? 0 : pair_layout(dir, B, N, F).total;
}

// records, the direction's nearest-neighbour loop, the combine of a split launch, the finish, the loss
static int pair_forward(const PairDir& dir, const float* points, long long points_batch_stride, const float* vertices,
                        const int32_t* faces, int B, int N, int V, int F, float* dist2, int32_t* index, float* weights, float* loss,
                        void* workspace, size_t workspace_bytes, void* stream) {
    bool go;
    int e = pair_begin(dir, B, N, V, F, points_batch_stride, true, points, vertices, faces, &go);
    if (e || !go) return e;
    if (!dist2 && !index && !weights && !loss) return fail(NR_ERR_ARGS, "no output asked for");
    const PairLayout wl = pair_layout(dir, B, N, F);
    if (!workspace || workspace_bytes < wl.total) return fail(NR_ERR_ARGS, "%s workspace missing or too small", dir.name);
    hipStream_t st = (hipStream_t)stream;
    const SplitPlan p = wl.plan;
    const int nq = dir.queries(N, F);
    char* ws = (char*)workspace;
    float* records = (float*)(ws + wl.records);
    int32_t* nearest = (int32_t*)(ws + wl.nearest);
    float* loop_d2 = (float*)(ws + wl.loop_d2);
    float* fin_d2 = dist2 ? dist2 : (float*)(ws + wl.fin_d2);
    nr_launch(k_point_face_records, grid_1d(F, PL_BLOCK, B), dim3(PL_BLOCK), 0, st, vertices, faces, V, F, records);
    e = check_launch("k_point_face_records");
    if (e) return e;
    PairArgs d;
    d.points = points, d.p_stride = points_batch_stride, d.records = records, d.N = N, d.F = F, d.nsplit = p.nsplit;
    if (p.nsplit > 1) {
        d.dist2 = (float*)(ws + wl.part_d2), d.index = (int32_t*)(ws + wl.part_index);
    } else {
        d.dist2 = loop_d2, d.index = nearest;
    }
    nr_launch(dir.nn, dim3((unsigned)(p.nqb * p.nsplit), (unsigned)B), dim3(PL_BLOCK), 0, st, d);
    dir.slot->store(LaunchRec{PL_BLOCK, p.nsplit > 1 ? dir.split_flag : 0});
    e = check_launch(dir.nn_name);
    if (e) return e;
    e = combine_split(d.dist2, d.index, B, nq, p.nsplit, loop_d2, nearest, st);
    if (e) return e;
    const bool need_d2 = dist2 || loss;
    nr_launch(dir.finish, grid_1d(nq, PL_BLOCK, B), dim3(PL_BLOCK), 0, st, points, points_batch_stride, vertices, faces,
              (const int32_t*)nearest, N, V, F, need_d2 ? fin_d2 : (float*)nullptr, index, weights);
    e = check_launch(dir.finish_name);
    if (e || !loss) return e;
    nr_launch(k_chamfer_sum, dim3((unsigned)B), dim3(PL_WIDE), 0, st, (const float*)fin_d2, nq, (const float*)nullptr, 0, loss);
    return check_launch("k_chamfer_sum");
}

size_t nr_point_mesh_workspace_bytes(int batch_size, int num_points, int num_faces) {
    return pair_workspace_bytes(POINT_FACE, batch_size, num_points, num_faces);
}

int nr_point_mesh_forward(const float* points, long long points_batch_stride, const float* vertices, const int32_t* faces,
                          int batch_size, int num_points, int num_vertices, int num_faces, float* dist2, int32_t* face,
                          float* weights, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
    return pair_forward(POINT_FACE, points, points_batch_stride, vertices, faces, batch_size, num_points, num_vertices, num_faces,
                        dist2, face, weights, loss, workspace, workspace_bytes, stream);
}

int nr_point_mesh_backward(const float* points, long long points_batch_stride, const float* vertices, const int32_t* faces,
                           const int32_t* face, const float* weights, const float* grad_loss, int batch_size, int num_points,
                           int num_vertices, int num_faces, float* grad_points, float* grad_vertices, void* stream) {
    const int B = batch_size, N = num_points, V = num_vertices, F = num_faces;
    bool go;
    int e = pair_begin(POINT_FACE, B, N, V, F, points_batch_stride, grad_points || grad_vertices, points, vertices, faces, &go);
    if (e || !go) return e;
    if (!face || !weights || !grad_loss) return fail(NR_ERR_ARGS, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (grad_vertices && !zero_async(grad_vertices, (size_t)B * V * 3 * 4, st, &e)) return e;
    nr_launch(k_point_mesh_bwd, grid_1d(N, PL_BLOCK, B), dim3(PL_BLOCK), 0, st, points,
              points_batch_stride, vertices, faces, face, weights, grad_loss, N, V, grad_points, grad_vertices);
    return check_launch("k_point_mesh_bwd");
}

size_t nr_face_point_workspace_bytes(int batch_size, int num_points, int num_faces) {
    return pair_workspace_bytes(FACE_POINT, batch_size, num_points, num_faces);
}

int nr_face_point_forward(const float* points, long long points_batch_stride, const float* vertices, const int32_t* faces,
                          int batch_size, int num_points, int num_vertices, int num_faces, float* dist2, int32_t* point,
                          float* weights, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
    return pair_forward(FACE_POINT, points, points_batch_stride, vertices, faces, batch_size, num_points, num_vertices, num_faces,
                        dist2, point, weights, loss, workspace, workspace_bytes, stream);
}

int nr_face_point_backward(const float* points, long long points_batch_stride, const float* vertices, const int32_t* faces,
                           const int32_t* corner_offsets, const int32_t* corner_index, const int32_t* point, const float* weights,
                           const float* grad_loss, int batch_size, int num_points, int num_vertices, int num_faces,
                           float* grad_points, float* grad_vertices, void* stream) {
    const int B = batch_size, N = num_points, V = num_vertices, F = num_faces;
    bool go;
    int e = pair_begin(FACE_POINT, B, N, V, F, points_batch_stride, grad_points || grad_vertices, points, vertices, faces, &go);
    if (e || !go) return e;
    if (!point || !weights || !grad_loss) return fail(NR_ERR_ARGS, "null pointer");
    if (grad_vertices && (!corner_offsets || !corner_index)) return fail(NR_ERR_ARGS, "grad_vertices needs the corner CSR lists");
    hipStream_t st = (hipStream_t)stream;
    if (grad_vertices) {
        nr_launch(k_face_point_bwd_vertices, grid_1d(V, PL_BLOCK, B), dim3(PL_BLOCK), 0, st, points, points_batch_stride, vertices,
                  faces, corner_offsets, corner_index, point, weights, grad_loss, V, F, grad_vertices);
        e = check_launch("k_face_point_bwd_vertices");
        if (e) return e;
    }
    if (!grad_points) return NR_OK;
    if (!zero_async(grad_points, (size_t)B * N * 3 * 4, st, &e)) return e;
    nr_launch(k_face_point_bwd_points, grid_1d(F, PL_BLOCK, B), dim3(PL_BLOCK), 0, st, points, points_batch_stride, vertices,
              faces, point, weights, grad_loss, N, V, F, grad_points);
    return check_launch("k_face_point_bwd_points");
}

// ---- image losses (nr_image_loss.h) ----
static long long il_chunks(int n) { return ((long long)n + IL_CHUNK - 1) / IL_CHUNK; }

static int validate_image_loss(int B, int N) {
    if (B < 0 || N < 0) return fail(NR_ERR_ARGS, "bad sizes B=%d N=%d", B, N);
    if (N > INT_MAX - IL_CHUNK || (long long)B * il_chunks(N) > INT_MAX) return fail(NR_ERR_ARGS, "too many elements B=%d N=%d", B, N);
    return NR_OK;
}

// every item base p + b * stride, b < B, on 16 bytes
static bool il_aligned(const void* p, long long stride, int B) { return ((uintptr_t)p & 15) == 0 && (B == 1 || (stride & 3) == 0); }

size_t nr_image_loss_workspace_bytes(int batch_size, int item_elems) {
    if (batch_size <= 0 || item_elems <= 0) return 0;
    return align_up((size_t)batch_size * (size_t)il_chunks(item_elems) * 2 * 4);
}

// The checked kernel arguments of both pointwise entry points, and the instantiation: vec (VW = 4) and wm.
static int pointwise_args(const float* images, long long istride, const float* targets, long long tstride, const float* weights,
                          long long wstride, int period, int kind, float delta, int B, int N, const float* grad_images,
                          ILPointwise* a, bool* vec, int* wm) {
    if (!images || !targets) return fail(NR_ERR_ARGS, "null images or targets");
    if (istride < 0 || tstride < 0 || wstride < 0) return fail(NR_ERR_ARGS, "negative item stride");
    if (kind != NR_LOSS_SQUARED && kind != NR_LOSS_HUBER) return fail(NR_ERR_ARGS, "bad kind %d", kind);
    if (kind == NR_LOSS_HUBER && !(delta > 0.f && delta < INFINITY)) return fail(NR_ERR_ARGS, "bad delta %g", (double)delta);
    if (weights && (period <= 0 || N % period != 0)) return fail(NR_ERR_ARGS, "the weight period %d must divide N=%d", period, N);
    *vec = il_aligned(images, istride, B) && il_aligned(targets, tstride, B) && (!grad_images || il_aligned(grad_images, N, B));
    *wm = !weights ? IL_W_NONE : (*vec && il_aligned(weights, wstride, B) && period % 4 == 0) ? IL_W_VECTOR : IL_W_SCALAR;
    *a = ILPointwise{images, targets, weights, istride, tstride, wstride, weights ? period : 1,
                     weights ? (IL_BLOCK * 4) % period : 0, delta, N, (int)il_chunks(N)};
    return NR_OK;
}

int nr_pointwise_loss_forward(const float* images, long long image_stride, const float* targets, long long target_stride,
                              const float* weights, long long weight_stride, int weight_period, int kind, float delta,
                              int batch_size, int item_elems, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
    const int B = batch_size, N = item_elems;
    int e = validate_image_loss(B, N);
    if (e) return e;
    if (B == 0) return NR_OK;
    if (!loss) return fail(NR_ERR_ARGS, "null loss");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        if (!zero_async(loss, (size_t)B * 4, st, &e)) return e;
        return NR_OK;
    }
    ILPointwise a;
    bool vec;
    int wm;
    e = pointwise_args(images, image_stride, targets, target_stride, weights, weight_stride, weight_period, kind, delta, B, N,
                       nullptr, &a, &vec, &wm);
    if (e) return e;
    if (!workspace || workspace_bytes < nr_image_loss_workspace_bytes(B, N))
        return fail(NR_ERR_WORKSPACE, "image loss workspace missing or too small");
    launch_pointwise(a, vec, wm, kind == NR_LOSS_HUBER, B, st, nullptr, (float*)workspace);
    e = check_launch("k_pointwise_fwd");
    if (e) return e;
    nr_launch(k_mesh_loss_sum, dim3((unsigned)B), dim3(ML_BLOCK), 0, st, (const float*)workspace, a.nchunk, loss);
    return check_launch("k_mesh_loss_sum");
}

int nr_pointwise_loss_backward(const float* images, long long image_stride, const float* targets, long long target_stride,
                               const float* weights, long long weight_stride, int weight_period, int kind, float delta,
                               int batch_size, int item_elems, const float* grad_loss, float* grad_images, void* stream) {
    const int B = batch_size, N = item_elems;
    int e = validate_image_loss(B, N);
    if (e) return e;
    if (B == 0 || N == 0) return NR_OK;
    if (!grad_loss || !grad_images) return fail(NR_ERR_ARGS, "null grad_loss or grad_images");
    ILPointwise a;
    bool vec;
    int wm;
    e = pointwise_args(images, image_stride, targets, target_stride, weights, weight_stride, weight_period, kind, delta, B, N,
                       grad_images, &a, &vec, &wm);
    if (e) return e;
    launch_pointwise(a, vec, wm, kind == NR_LOSS_HUBER, B, (hipStream_t)stream, grad_loss, grad_images);
    return check_launch("k_pointwise_bwd");
}

int nr_iou_loss_forward(const float* images, long long image_stride, const float* targets, long long target_stride, float eps,
                        int batch_size, int item_elems, float* loss, float* sums, void* workspace, size_t workspace_bytes,
                        void* stream) {
    const int B = batch_size, N = item_elems;
    int e = validate_image_loss(B, N);
    if (e) return e;
    if (B == 0) return NR_OK;
    if (!loss || !sums) return fail(NR_ERR_ARGS, "null loss or sums");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        const float one = 1.f - 0.f / (0.f + eps);  // 1, or NaN with eps == 0 as the formula has it
        int bits;
        memcpy(&bits, &one, 4);
        if (!zero_async(sums, (size_t)B * 8, st, &e)) return e;
        if (hipMemsetD32Async((hipDeviceptr_t)loss, bits, (size_t)B, st) != hipSuccess) return check_launch("hipMemsetAsync");
        return NR_OK;
    }
    if (!images || !targets) return fail(NR_ERR_ARGS, "null images or targets");
    if (image_stride < 0 || target_stride < 0) return fail(NR_ERR_ARGS, "negative item stride");
    if (!workspace || workspace_bytes < nr_image_loss_workspace_bytes(B, N))
        return fail(NR_ERR_WORKSPACE, "image loss workspace missing or too small");
    const int nchunk = (int)il_chunks(N);
    const dim3 grid((unsigned)(B * nchunk));
    const bool vec = il_aligned(images, image_stride, B) && il_aligned(targets, target_stride, B);
    nr_launch(vec ? k_iou_fwd<4> : k_iou_fwd<1>, grid, dim3(IL_BLOCK), 0, st, images, image_stride, targets, target_stride, N, nchunk,
              (float*)workspace);
    e = check_launch("k_iou_fwd");
    if (e) return e;
    nr_launch(k_iou_finish, dim3((unsigned)B), dim3(IL_BLOCK), 0, st, (const float*)workspace, nchunk, eps, sums, loss);
    return check_launch("k_iou_finish");
}

int nr_iou_loss_backward(const float* targets, long long target_stride, const float* sums, float eps, int batch_size,
                         int item_elems, const float* grad_loss, float* grad_images, void* stream) {
    const int B = batch_size, N = item_elems;
    int e = validate_image_loss(B, N);
    if (e) return e;
    if (B == 0 || N == 0) return NR_OK;
    if (!targets || !sums || !grad_loss || !grad_images) return fail(NR_ERR_ARGS, "null pointer");
    if (target_stride < 0) return fail(NR_ERR_ARGS, "negative item stride");
    const int nchunk = (int)il_chunks(N);
    const dim3 grid((unsigned)(B * nchunk));
    hipStream_t st = (hipStream_t)stream;
    const bool vec = il_aligned(targets, target_stride, B) && il_aligned(grad_images, N, B);
    nr_launch(vec ? k_iou_bwd<4> : k_iou_bwd<1>, grid, dim3(IL_BLOCK), 0, st, targets, target_stride, sums, grad_loss, eps, N, nchunk,
              grad_images);
    return check_launch("k_iou_bwd");
}

// ---- SSIM loss (nr_ssim_loss.h) ----
struct SSGeom {
    int R = 0, MH = 0, MW = 0;          // window radius, the SSIM map
    long long N = 0;                    // C H W
    long long ftiles = 0, btiles = 0;   // tiles per channel: of the map (forward), of the image (backward)
};

static long long ss_tiles(int h, int w) { return (((long long)h + SS_TILE - 1) / SS_TILE) * (((long long)w + SS_TILE - 1) / SS_TILE); }

// Sizes, window and padding of every SSIM entry point; g->N == 0 or B == 0: nothing to launch.
static int validate_ssim(int B, int C, int H, int W, int window_size, int padding, SSGeom* g) {
    if (B < 0 || C < 0 || H < 0 || W < 0) return fail(NR_ERR_ARGS, "bad sizes B=%d C=%d H=%d W=%d", B, C, H, W);
    if (window_size < 3 || window_size > 2 * SS_MAX_R + 1 || window_size % 2 == 0)
        return fail(NR_ERR_ARGS, "bad window size %d (odd, 3 to %d)", window_size, 2 * SS_MAX_R + 1);
    if (padding != NR_SSIM_SAME && padding != NR_SSIM_VALID) return fail(NR_ERR_ARGS, "bad padding %d", padding);
    g->R = window_size / 2;
    const long long hw = (long long)H * W;
    if (hw > INT_MAX || hw * C > INT_MAX) return fail(NR_ERR_ARGS, "too many elements C=%d H=%d W=%d", C, H, W);
    g->N = hw * C;
    if (B == 0 || g->N == 0) return NR_OK;
    g->MH = padding == NR_SSIM_VALID ? H - 2 * g->R : H, g->MW = padding == NR_SSIM_VALID ? W - 2 * g->R : W;
    if (g->MH < 1 || g->MW < 1)
        return fail(NR_ERR_ARGS, "a %d x %d image has no 'valid' window of %d", H, W, window_size);
    g->ftiles = ss_tiles(g->MH, g->MW), g->btiles = ss_tiles(H, W);
    if ((long long)B * C > INT_MAX || (long long)B * C * g->btiles > INT_MAX)
        return fail(NR_ERR_ARGS, "too many tiles B=%d C=%d H=%d W=%d", B, C, H, W);
    return NR_OK;
}

static int ssim_args(const float* images, long long istride, const float* targets, long long tstride, int B, int C, int H, int W,
                     const SSGeom& g, const float* window, float c1, float c2, int padding, SSArgs* a) {
    if (!images || !targets || !window) return fail(NR_ERR_ARGS, "null images, targets or window");
    if (istride < 0 || tstride < 0) return fail(NR_ERR_ARGS, "negative item stride");
    if (!(c1 >= 0.f && c1 < INFINITY && c2 >= 0.f && c2 < INFINITY)) return fail(NR_ERR_ARGS, "bad constants c1=%g c2=%g", (double)c1, (double)c2);
    *a = SSArgs{images, targets, istride, tstride, B, C, H, W, g.MH, g.MW, padding == NR_SSIM_SAME ? g.R : 0, 0, 0, c1, c2, {}};
    for (int k = 0; k <= 2 * g.R; k++) {
        if (!(fabsf(window[k]) < INFINITY)) return fail(NR_ERR_ARGS, "window weight %d is not finite", k);
        a->g[k] = ss_f2{window[k], window[k]};
    }
    return NR_OK;
}

size_t nr_ssim_loss_workspace_bytes(int batch_size, int channels, int height, int width, int window_size, int padding) {
    SSGeom g;
    if (validate_ssim(batch_size, channels, height, width, window_size, padding, &g) || batch_size == 0 || g.N == 0) return 0;
    return align_up((size_t)batch_size * (size_t)channels * (size_t)g.ftiles * 4);
}

int nr_ssim_loss_forward(const float* images, long long image_stride, const float* targets, long long target_stride,
                         int batch_size, int channels, int height, int width, int window_size, const float* window, float c1,
                         float c2, int padding, float* loss, float* saved, void* workspace, size_t workspace_bytes, void* stream) {
    const int B = batch_size, C = channels, H = height, W = width;
    SSGeom g;
    int e = validate_ssim(B, C, H, W, window_size, padding, &g);
    if (e) return e;
    if (B == 0) return NR_OK;
    if (!loss) return fail(NR_ERR_ARGS, "null loss");
    hipStream_t st = (hipStream_t)stream;
    if (g.N == 0) {
        if (!zero_async(loss, (size_t)B * 4, st, &e)) return e;
        return NR_OK;
    }
    SSArgs a;
    e = ssim_args(images, image_stride, targets, target_stride, B, C, H, W, g, window, c1, c2, padding, &a);
    if (e) return e;
    if (!workspace || workspace_bytes < nr_ssim_loss_workspace_bytes(B, C, H, W, window_size, padding))
        return fail(NR_ERR_WORKSPACE, "ssim loss workspace missing or too small");
    a.ntx = (g.MW + SS_TILE - 1) / SS_TILE, a.nty = (g.MH + SS_TILE - 1) / SS_TILE;
    const int nblk = (int)(C * g.ftiles);
    const dim3 grid((unsigned)(B * nblk));
    if (saved) ss_launch_fwd<true>(g.R, a, grid, st, (float*)workspace, saved);
    else ss_launch_fwd<false>(g.R, a, grid, st, (float*)workspace, nullptr);
    e = check_launch("k_ssim_fwd");
    if (e) return e;
    nr_launch(k_ssim_finish, dim3((unsigned)B), dim3(SS_BLOCK), 0, st, (const float*)workspace, nblk,
              (float)((long long)C * g.MH * g.MW), loss);
    return check_launch("k_ssim_finish");
}

int nr_ssim_loss_backward(const float* images, long long image_stride, const float* targets, long long target_stride,
                          const float* saved, int batch_size, int channels, int height, int width, int window_size,
                          const float* window, int padding, const float* grad_loss, float* grad_images, void* stream) {
    const int B = batch_size, C = channels, H = height, W = width;
    SSGeom g;
    int e = validate_ssim(B, C, H, W, window_size, padding, &g);
    if (e) return e;
    if (B == 0 || g.N == 0) return NR_OK;
    if (!saved || !grad_loss || !grad_images) return fail(NR_ERR_ARGS, "null saved, grad_loss or grad_images");
    SSArgs a;
    e = ssim_args(images, image_stride, targets, target_stride, B, C, H, W, g, window, 0.f, 0.f, padding, &a);
    if (e) return e;
    a.ntx = (W + SS_TILE - 1) / SS_TILE, a.nty = (H + SS_TILE - 1) / SS_TILE;
    const dim3 grid((unsigned)(B * C * g.btiles));
    ss_launch_bwd(g.R, a, grid, (hipStream_t)stream, saved, grad_loss, (float)((long long)C * g.MH * g.MW), grad_images);
    return check_launch("k_ssim_bwd");
}

// ---- optimiser (nr_adam.h) ----
size_t nr_adam_args_size(void) { return sizeof(NrAdamArgs); }

size_t nr_adam_scratch_bytes(int num_tensors) {
    if (num_tensors <= 0) return 0;
    return align_up((size_t)num_tensors * 2 * 4);
}

int nr_adam_step(const NrAdamArgs* args, void* stream) {
    if (!args) return fail(NR_ERR_ARGS, "null adam args");
    const int n = args->num_tensors;
    if (n < 0 || n > args->tensors_capacity) return fail(NR_ERR_ARGS, "bad tensor count %d (the array holds %d)", n, args->tensors_capacity);
    if (n == 0) return NR_OK;
    if (!args->tensors) return fail(NR_ERR_ARGS, "null tensor array");
    if (!(args->beta1 >= 0.0 && args->beta1 < 1.0) || !(args->beta2 >= 0.0 && args->beta2 < 1.0))
        return fail(NR_ERR_ARGS, "bad betas (%g, %g): need 0 <= beta < 1", args->beta1, args->beta2);
    if (!(args->eps >= 0.0) || !(args->eps < INFINITY)) return fail(NR_ERR_ARGS, "bad eps %g", args->eps);
    if (!isfinite(args->lr)) return fail(NR_ERR_ARGS, "bad lr %g", args->lr);
    for (int i = 0; i < n; i++) {
        const NrAdamTensor& t = args->tensors[i];
        if (t.numel < 0 || t.numel > (long long)INT_MAX - AD_CHUNK) return fail(NR_ERR_ARGS, "tensor %d: bad numel %lld", i, t.numel);
        if (t.numel > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq || !t.step))
            return fail(NR_ERR_ARGS, "tensor %d: null param, grad, exp_avg, exp_avg_sq or step", i);
        if (!isfinite(t.lr_scale)) return fail(NR_ERR_ARGS, "tensor %d: bad lr_scale %g", i, t.lr_scale);
    }
    if (!args->scratch || args->scratch_bytes < nr_adam_scratch_bytes(n))
        return fail(NR_ERR_WORKSPACE, "adam factor scratch missing or too small");
    hipStream_t st = (hipStream_t)stream;
    for (int base = 0; base < n; base += NR_ADAM_MAX_TENSORS) {
        const int cnt = min(n - base, (int)NR_ADAM_MAX_TENSORS);
        AdamTick tick = {};
        AdamLaunch up = {};
        long long blocks = 0;
        for (int i = 0; i < cnt; i++) {
            const NrAdamTensor& t = args->tensors[base + i];
            if (t.step) {
                tick.step[tick.n] = t.step, tick.lr_scale[tick.n] = t.lr_scale, tick.slot[tick.n] = base + i;
                tick.n++;
            }
            if (t.numel == 0) continue;
            const bool vec = (((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq) & 15) == 0;
            up.t[up.n] = AdamDesc{t.param, t.grad, t.exp_avg, t.exp_avg_sq, (int)t.numel, vec ? 1 : 0, base + i, 0};
            up.start[up.n] = (int)blocks;
            blocks += (t.numel + AD_CHUNK - 1) / AD_CHUNK;
            up.n++;
        }
        if (blocks > INT_MAX) return fail(NR_ERR_ARGS, "too many elements in one launch (%lld blocks)", blocks);
        for (int i = up.n; i <= NR_ADAM_MAX_TENSORS; i++) up.start[i] = (int)blocks;
        if (tick.n > 0) {
            tick.lr = args->lr, tick.beta1 = args->beta1, tick.beta2 = args->beta2;
            tick.lr_device = args->lr_device, tick.factors = (float*)args->scratch;
            nr_launch(k_adam_tick, dim3(1), dim3(64), 0, st, tick);
            int e = check_launch("k_adam_tick");
            if (e) return e;
        }
        if (blocks > 0) {
            up.c1 = (float)(1.0 - args->beta1), up.c2 = (float)(1.0 - args->beta2), up.eps = (float)args->eps;
            up.factors = (const float*)args->scratch;
            nr_launch(args->skip_zero_grad ? k_adam_update<true> : k_adam_update<false>, dim3((unsigned)blocks), dim3(AD_BLOCK), 0, st, up);
            int e = check_launch("k_adam_update");
            if (e) return e;
        }
    }
    return NR_OK;
}

// ---- vertex attributes (nr_attributes.h) ----
size_t nr_attribute_args_size(void) { return sizeof(NrAttributeArgs); }

static int validate_attributes(const NrAttributeArgs* a) {
    if (!a) return fail(NR_ERR_ARGS, "null attribute args");
    if (a->batch_size < 0 || a->num_faces < 0 || a->num_vertices < 0 || a->num_attributes < 0 || a->image_size <= 0)
        return fail(NR_ERR_ARGS, "bad sizes B=%d F=%d V=%d Va=%d s=%d", a->batch_size, a->num_faces, a->num_vertices,
                    a->num_attributes, a->image_size);
    if (a->image_size > 16384 || internal_size(a->anti_aliasing, a->image_size) > 16384)
        return fail(NR_ERR_ARGS, "image too large (s=%d)", a->image_size);
    if (a->num_channels < 1 || a->num_channels > NR_ATTR_MAX_CHANNELS)
        return fail(NR_ERR_ARGS, "bad channel count %d (1 .. %d)", a->num_channels, (int)NR_ATTR_MAX_CHANNELS);
    if (a->batch_size > 65535) return fail(NR_ERR_ARGS, "too many items B=%d (at most 65535)", a->batch_size);
    if (a->attr_batch_stride < 0) return fail(NR_ERR_ARGS, "negative attribute batch stride");
    if ((long long)a->batch_size * a->num_vertices > INT_MAX || (long long)a->batch_size * a->num_attributes * a->num_channels > INT_MAX)
        return fail(NR_ERR_ARGS, "too many vertices or attribute rows B=%d V=%d Va=%d", a->batch_size, a->num_vertices, a->num_attributes);
    if (a->batch_size > 0 && a->num_faces > 0 && a->num_vertices > 0) {
        if (!a->face_index || !a->face_records) return fail(NR_ERR_ARGS, "null face_index or face_records");
        if (!a->faces_attributes || !a->attributes || a->num_attributes == 0)
            return fail(NR_ERR_ARGS, "null or empty attributes / faces_attributes");
    }
    return NR_OK;
}

static bool attributes_empty(const NrAttributeArgs* a) { return a->batch_size == 0 || a->num_faces == 0 || a->num_vertices == 0; }

int nr_attributes_forward(const NrAttributeArgs* a, float* images, void* stream) {
    int e = validate_attributes(a);
    if (e) return e;
    if (a->batch_size == 0) return NR_OK;
    if (!images) return fail(NR_ERR_ARGS, "null images");
    hipStream_t st = (hipStream_t)stream;
    const int s = a->image_size, S = internal_size(a->anti_aliasing, s), C = a->num_channels;
    if (attributes_empty(a)) {  // nothing drawn: background everywhere
        if (!zero_async(images, (size_t)a->batch_size * C * s * s * 4, st, &e)) return e;
        if (a->internal && !zero_async(a->internal, (size_t)a->batch_size * S * S * C * 4, st, &e)) return e;
        return NR_OK;
    }
    nr_launch(a->anti_aliasing ? k_attr_fwd<true> : k_attr_fwd<false>, grid_1d((long long)s * s, AT_BLOCK, a->batch_size),
              dim3(AT_BLOCK), 0, st, *a, S, images);
    return check_launch("k_attr_fwd");
}

size_t nr_attributes_backward_workspace_bytes(int batch_size, int num_faces, int num_channels) {
    if (batch_size <= 0 || num_faces <= 0 || num_channels <= 0) return 0;
    return align_up((size_t)batch_size * num_faces * 3 * (3 + (size_t)num_channels) * 4);
}

int nr_attributes_backward(const NrAttributeArgs* a, const float* grad_images, float* grad_vertices, float* grad_attributes,
                           const int32_t* vertex_offsets, const int32_t* vertex_faces, const int32_t* attr_offsets,
                           const int32_t* attr_faces, void* workspace, size_t workspace_bytes, void* stream) {
    int e = validate_attributes(a);
    if (e) return e;
    hipStream_t st = (hipStream_t)stream;
    const int B = a->batch_size, F = a->num_faces, V = a->num_vertices, Va = a->num_attributes, C = a->num_channels;
    const int Ba = a->attr_batch_stride ? B : 1;
    const size_t nv = (size_t)B * V * 3, na = (size_t)Ba * Va * C;
    if (attributes_empty(a)) {  // nothing drawn: zero gradients
        if (grad_vertices && nv && !zero_async(grad_vertices, nv * 4, st, &e)) return e;
        if (grad_attributes && na && !zero_async(grad_attributes, na * 4, st, &e)) return e;
        return NR_OK;
    }
    if (!grad_vertices && !grad_attributes) return NR_OK;
    if (!grad_images) return fail(NR_ERR_ARGS, "null grad_images");
    if (grad_vertices && (!a->internal || !vertex_offsets || !vertex_faces))
        return fail(NR_ERR_ARGS, "grad_vertices needs the forward's internal image and the vertex CSR");
    if (grad_attributes && (!attr_offsets || !attr_faces)) return fail(NR_ERR_ARGS, "grad_attributes needs the attribute CSR");
    const size_t need = nr_attributes_backward_workspace_bytes(B, F, C);
    if (!workspace || workspace_bytes < need) return fail(NR_ERR_WORKSPACE, "attribute backward workspace missing or too small");
    if (!zero_async(workspace, need, st, &e)) return e;
    float* rec = (float*)workspace;
    const int S = internal_size(a->anti_aliasing, a->image_size);
    const dim3 grid((unsigned)(((S + TW - 1) / TW) * ((S + TH - 1) / TH)), (unsigned)B);
    auto kernel = k_attr_bwd<true, true>;  // <GV, GA>: at least one of the two is wanted here
    if (!grad_attributes) kernel = k_attr_bwd<true, false>;
    if (!grad_vertices) kernel = k_attr_bwd<false, true>;
    nr_launch(kernel, grid, dim3(AT_BLOCK), 0, st, *a, S, grad_images, rec);
    e = check_launch("k_attr_bwd");
    if (e) return e;
    if (grad_vertices) {
        const long long n = (long long)B * V;
        nr_launch(k_attr_vertex_sum, grid_1d(n, AT_BLOCK), dim3(AT_BLOCK), 0, st, (const float*)rec,
                  vertex_offsets, vertex_faces, grad_vertices, F, V, 3 + C, n);
        e = check_launch("k_attr_vertex_sum");
        if (e) return e;
    }
    if (grad_attributes) {
        const long long n = (long long)na;
        nr_launch(k_attr_row_sum, grid_1d(n, AT_BLOCK), dim3(AT_BLOCK), 0, st, (const float*)rec,
                  attr_offsets, attr_faces, grad_attributes, B, F, Va, C, a->attr_batch_stride ? 0 : 1, n);
        e = check_launch("k_attr_row_sum");
    }
    return e;
}

int nr_selftest_division(const float* a, const float* b, float* q_fast, float* q_ieee, long long n, void* stream) {
    if (n < 0 || (n > 0 && (!a || !b || !q_fast || !q_ieee))) return fail(NR_ERR_ARGS, "bad arguments");
    if (n == 0) return NR_OK;
    nr_launch(k_selftest_div, grid_1d(n, 256), dim3(256), 0, (hipStream_t)stream, a, b,
                       q_fast, q_ieee, n);
    return check_launch("k_selftest_div");
}

#ifdef NR_FWD_TIMING
// timing builds only: the fused forward's per-wave phase timestamps (g_fwd_t)
__attribute__((visibility("default"))) int nr_debug_fwd_timing(unsigned long long* out, size_t n) {
    if (n > (size_t)NR_FTIMING_MAX) n = NR_FTIMING_MAX;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fwd_t), n * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(NR_ERR_LAUNCH, "hipMemcpyFromSymbol failed");
    return NR_OK;
}
#endif
#ifdef NR_COUNT_DIRECT
__attribute__((visibility("default"))) int nr_debug_counts(unsigned long long* out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ncount), 4 * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(NR_ERR_LAUNCH, "hipMemcpyFromSymbol failed");
    return NR_OK;
}
#endif
#ifdef NR_BWD_TIMING
// timing builds only: the backward's per-wave phase timestamps (g_bwd_t), n entries to host memory
__attribute__((visibility("default"))) int nr_debug_bwd_timing(unsigned long long* out, size_t n) {
    if (n > (size_t)NR_TIMING_MAX) n = NR_TIMING_MAX;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bwd_t), n * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(NR_ERR_LAUNCH, "hipMemcpyFromSymbol failed");
    return NR_OK;
}
#endif

int nr_last_launch(const char* kernel, int* block_threads, int* flags) {
    if (!kernel || !block_threads || !flags) return fail(NR_ERR_ARGS, "null argument");
    const LaunchSlot* slot = strcmp(kernel, "k_raster_fwd") == 0 ? &g_last_fwd
                             : strcmp(kernel, "k_raster_bwd") == 0 ? &g_last_bwd
                             : strcmp(kernel, "k_chamfer_nn") == 0 ? &g_last_chamfer
                             : strcmp(kernel, "k_point_face_nn") == 0 ? &g_last_point_mesh
                             : strcmp(kernel, "k_face_point_nn") == 0 ? &g_last_face_point
                             : strcmp(kernel, "k_icp_nn") == 0 ? &g_last_icp : nullptr;
    if (!slot) return fail(NR_ERR_ARGS, "nr_last_launch: unknown kernel name %s", kernel);
    const LaunchRec r = slot->load();
    if (!r.threads) return fail(NR_ERR_ARGS, "nr_last_launch: no %s launch recorded in this process", kernel);
    *block_threads = r.threads;
    *flags = r.flags;
    return NR_OK;
}

int nr_profile_enable(int on) {
    if (on && !g_prof) {
        for (int k = 0; k < P_N; k++)
            for (int r = 0; r < PROF_RING; r++)
                for (int j = 0; j < 2; j++)
                    if (hipEventCreate(&g_prof_ev[k][r][j]) != hipSuccess) return fail(NR_ERR_LAUNCH, "hipEventCreate failed");
    } else if (!on && g_prof) {
        for (int k = 0; k < P_N; k++)
            for (int r = 0; r < PROF_RING; r++)
                for (int j = 0; j < 2; j++) (void)hipEventDestroy(g_prof_ev[k][r][j]);
    }
    // (re)enabling starts a new measurement: the ring's recorded launches are forgotten
    for (int k = 0; k < P_N; k++) g_prof_n[k] = 0;
    g_prof = on != 0;
    return NR_OK;
}

#ifdef NR_COUNT_TESTS
int nr_count_read(unsigned long long* out4, int reset) {
    if (!out4) return fail(NR_ERR_ARGS, "null argument");
    if (hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_fwd_count), 4 * sizeof(unsigned long long)) != hipSuccess)
        return fail(NR_ERR_LAUNCH, "nr_count_read: hipMemcpyFromSymbol failed");
    if (reset) {
        const unsigned long long z[4] = {0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_fwd_count), z, sizeof(z)) != hipSuccess)
            return fail(NR_ERR_LAUNCH, "nr_count_read: hipMemcpyToSymbol failed");
    }
    return NR_OK;
}
#endif

int nr_profile_read(const char* kernel, float* ms) {
    if (!kernel || !ms) return fail(NR_ERR_ARGS, "null argument");
    for (int k = 0; k < P_N; k++) {
        if (strcmp(kernel, kProfNames[k]) != 0) continue;
        if (!g_prof || g_prof_n[k] == 0) return fail(NR_ERR_ARGS, "%s: no profiled launch recorded", kernel);
        const int n = g_prof_n[k] < PROF_RING ? g_prof_n[k] : PROF_RING;
        double sum = 0.0;
        for (int r = 0; r < n; r++) {
            float e = 0.f;
            if (hipEventElapsedTime(&e, g_prof_ev[k][r][0], g_prof_ev[k][r][1]) != hipSuccess)
                return fail(NR_ERR_LAUNCH, "%s: hipEventElapsedTime failed", kernel);
            sum += e;
        }
        *ms = (float)(sum / n);
        return NR_OK;
    }
    return fail(NR_ERR_ARGS, "unknown kernel name %s", kernel);
}

}  // extern "C"

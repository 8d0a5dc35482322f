// nr_host.h -- host-side helpers: launch grids, workspace layouts, split plan, argument validation and Shade construction
// Part of nr_raster.hip (one translation unit); see that file and DESIGN.md.
#pragma once

#pragma clang fp contract(off)

namespace {

// the raster the kernels work on: twice the output's side with anti-aliasing
int internal_size(int anti_aliasing, int image_size) { return anti_aliasing ? 2 * image_size : image_size; }

// texels of one packed RGBA texture (textures_packed, the backward's g4): H * W rounded up to four
size_t packed_texels(int H, int W) { return ((size_t)H * W + 3) & ~size_t(3); }

// one thread per element: blocks of `block` threads over n elements, by `items` in y
dim3 grid_1d(long long n, int block, int items = 1) { return dim3((unsigned)((n + block - 1) / block), (unsigned)items); }

// hipMemsetAsync to zero; on failure *e takes the status the entry point returns
bool zero_async(void* p, size_t bytes, hipStream_t st, int* e) {
    if (hipMemsetAsync(p, 0, bytes, st) == hipSuccess) return true;
    *e = check_launch("hipMemsetAsync");
    return false;
}

// ---- tile order of the interleaved forward launch (TileOrder, block_item_tile) ----
// The nx x ny tiles of tile_w x tile_h pixels by squared pixel distance of the tile's centre from the
// raster's centre, ties by row, then column: an integer sort of (dx^2 + dy^2, ty, tx), dx = (2 tx + 1
// - nx) tile_w and dy = (2 ty + 1 - ny) tile_h (twice the distance; pixels, so tiles that are not
// square order correctly).  out: nx ny entries tx | ty << 8.  False when the raster has more
// than TILE_ORDER_MAX tiles or a coordinate does not fit its 8 bits.
bool tile_order_entries(int nx, int ny, int tile_w, int tile_h, uint16_t* out) {
    if (nx < 1 || ny < 1 || tile_w < 1 || tile_h < 1 || nx > 256 || ny > 256 || nx * ny > TILE_ORDER_MAX) return false;
    struct Key {
        long long d2;
        int ty, tx;
    };
    std::vector<Key> keys;
    keys.reserve((size_t)nx * ny);
    for (int ty = 0; ty < ny; ty++) {
        for (int tx = 0; tx < nx; tx++) {
            const long long dx = (long long)(2 * tx + 1 - nx) * tile_w, dy = (long long)(2 * ty + 1 - ny) * tile_h;
            keys.push_back(Key{dx * dx + dy * dy, ty, tx});
        }
    }
    std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) {
        return a.d2 != b.d2 ? a.d2 < b.d2 : (a.ty != b.ty ? a.ty < b.ty : a.tx < b.tx);
    });
    for (size_t t = 0; t < keys.size(); t++) out[t] = (uint16_t)(keys[t].tx | (keys[t].ty << 8));
    return true;
}
// The table of a launch over nx x ny tiles: built once per geometry and kept for the life of the
// process (a handful of rasters; map nodes do not move).  Sets g.table.  wanted = false (group 0, the
// ordered forward) and rasters past the cap get an empty table and
// g.table = 0: the arithmetic order.
const TileOrder& tile_order(bool wanted, Geom& g, int nx, int ny, int tile_w, int tile_h) {
    static const TileOrder none{};
    g.table = 0;
    if (!wanted || nx > 256 || ny > 256 || nx * ny > TILE_ORDER_MAX) return none;
    static std::mutex mu;
    static std::map<std::array<int, 4>, TileOrder> cache;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find({nx, ny, tile_w, tile_h});
    if (it == cache.end()) {
        TileOrder o{};
        uint16_t e[TILE_ORDER_MAX];
        if (!tile_order_entries(nx, ny, tile_w, tile_h, e)) return none;
        for (int t = 0; t < nx * ny; t++) o.w[t >> 1] |= (uint32_t)e[t] << ((t & 1) * 16);
        it = cache.emplace(std::array<int, 4>{nx, ny, tile_w, tile_h}, o).first;
    }
    g.table = 1;
    return it->second;
}

// ---- workspace layouts ----
// A workspace is cut once: every piece starts where the one before it ended, rounded up to 256 bytes.
// Each *_layout below lists its pieces' byte offsets in order, then the total (a braced list is evaluated
// left to right); the nr_*_bytes functions return that total, and the entry points test the caller's size
// against it and point into the buffer by the offsets.
struct Cutter {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off += align_up(bytes);
        return at;
    }
    size_t take_if(bool wanted, size_t bytes) { return wanted ? take(bytes) : off; }
};

// forward: [bbox int2 B*F][mask u32 B*nbins*nwords][per-face-group bin candidate counts u8
// B*groups*nbins][bin order i32 B*nbins][split counts: one i32 per list, at most 8 lists] (the last three:
// deep-bin dispatch order, run_face_index; groups = the setup's face groups of SETUP_FACES)
struct FwdLayout {
    size_t bbox, mask, part, order, split_cnt, total;
};
FwdLayout forward_layout(int B, int F, const Geom& g) {
    Cutter c;
    return {c.take((size_t)B * F * sizeof(int2)), c.take((size_t)B * g.nbins * g.nwords * 4),
            c.take((size_t)B * setup_groups(g) * g.nbins), c.take((size_t)B * g.nbins * 4), c.take(8 * sizeof(int)), c.off};
}

// backward: [gF: B F 9 face-corner floats][g4: Bt HWp RGBA texel rows][lights: gN: B F 9][gU: B V 3];
// the first zero_bytes start at zero (one memset, or the forward's setup zeroed them:
// NrRasterArgs.bwd_workspace): everything before gU, which k_vnormal_bwd writes in full
struct BwdLayout {
    size_t gF, g4, gN, zero_bytes, gU, total;
};
BwdLayout backward_layout(int B, int F, int V, int tex_items, int tex_height, int tex_width, bool lit) {
    Cutter c;
    return {c.take((size_t)B * F * 9 * 4), c.take_if(tex_items > 0, (size_t)tex_items * packed_texels(tex_height, tex_width) * 16),
            c.take_if(lit, (size_t)B * F * 9 * 4), c.off, c.take_if(lit, (size_t)B * V * 3 * 4), c.off};
}

// halo cache (nr_shade.h): the B items' halo values, then one byte per (item, 32x32 bin), nonzero when the
// bin has a foreground pixel (written by the forward, read by the backward to skip background tiles)
struct HaloLayout {
    size_t flags, total;
};
HaloLayout halo_layout(int B, int S, int C) {
    const size_t flags = (size_t)((long long)B * halo_item_floats(S, C) * 4);
    return {flags, flags + (((size_t)B * make_geom(0, S).nbins + 3) & ~size_t(3))};
}

// cotangent Laplacian forward (nr_mesh_loss.h): the per-block partial sums [B][blocks of ML_BLOCK vertices],
// then the half-cotangents [B][3 F] the face pass leaves for the vertex pass
struct CotLayout {
    size_t partial, cot, total;
};
CotLayout cot_layout(int B, int V, int F) {
    Cutter c;
    return {c.take((size_t)B * (((size_t)V + ML_BLOCK - 1) / ML_BLOCK) * 4), c.take((size_t)B * F * 3 * 4), c.off};
}

// skinning backward (nr_skinning.h): the chunk partials [B][num_chunks][12] k_skin_bwd_transforms leaves for
// k_skin_sum
struct SkinLayout {
    size_t partial, total;
};
SkinLayout skin_layout(int B, int num_chunks) {
    Cutter c;
    return {c.take((size_t)B * num_chunks * 12 * 4), c.off};
}

// How a nearest-neighbour launch (a chamfer direction: PL_*, a PairDir: PM_* or FP_*) is cut: query blocks per
// item, and target ranges per query block (more than one -- the split path -- while the launch has fewer
// than split_blocks blocks and every range still holds at least a full tile of targets: few queries against
// many targets would otherwise leave most of the chip idle).  Results do not depend on the cut.
struct SplitPlan {
    int nqb, nsplit;
};
SplitPlan split_plan(int B, int nq, int nt, int qblock, int tile, int split_blocks) {
    SplitPlan p;
    p.nqb = (int)(((long long)nq + qblock - 1) / qblock);
    const long long have = (long long)B * p.nqb;
    const long long want = (split_blocks + have - 1) / have, most = nt / tile;
    p.nsplit = (int)(want < most ? want : most);
    if (p.nsplit < 1) p.nsplit = 1;
    return p;
}

// one chamfer direction: the per-query minima [B, nq] and, on the split path, the partial d2 and j
// [B, nsplit, nq] each
struct ChamferLayout {
    SplitPlan plan;
    size_t minima, part_d2, part_j, total;
};
ChamferLayout chamfer_layout(int B, int nq, int nt) {
    const SplitPlan p = split_plan(B, nq, nt, PL_QBLOCK, PL_TILE, PL_SPLIT_BLOCKS);
    const size_t part = (size_t)B * p.nsplit * nq * 4;
    Cutter c;
    return {p, c.take((size_t)B * nq * 4), c.take_if(p.nsplit > 1, part), c.take_if(p.nsplit > 1, part), c.off};
}

// rigid_align (nr_rigid.h): pass (a)'s partial sums [B][chunks][RG_SUMS], then pass (b)'s [B][chunks][RG_MOM], a chunk
// being RG_CHUNK points.  The backward keeps its per-item gradients [B][RG_GRAD] at the start of the same buffer
// (never larger: a chunk's two partials are RG_SUMS + RG_MOM >= RG_GRAD floats).
struct RigidLayout {
    int nchunk;
    size_t sums, moments, total;
};
RigidLayout rigid_layout(int B, int N) {
    const int nchunk = (int)(((long long)N + RG_CHUNK - 1) / RG_CHUNK);
    Cutter c;
    return {nchunk, c.take((size_t)B * nchunk * RG_SUMS * 4), c.take((size_t)B * nchunk * RG_MOM * 4), c.off};
}
static_assert(RG_SUMS + RG_MOM >= RG_GRAD, "the backward's gradients fit the forward's workspace");

// icp: rigid_align's two pieces for the N queries, then on the split path of k_icp_nn the partial d2 and j
// [B, nsplit, N] each
struct IcpLayout {
    SplitPlan plan;
    RigidLayout rigid;
    size_t part_d2, part_j, total;
};
IcpLayout icp_layout(int B, int N, int M) {
    const SplitPlan p = split_plan(B, N, M, PL_QBLOCK, PL_TILE, PL_SPLIT_BLOCKS);
    const RigidLayout r = rigid_layout(B, N);
    const size_t part = (size_t)B * p.nsplit * N * 4;
    Cutter c;
    c.off = r.total;
    return {p, r, c.take_if(p.nsplit > 1, part), c.take_if(p.nsplit > 1, part), c.off};
}

// The two directions of the point / mesh distance, which share one host path (nr_raster.hip): point -> face (for
// every point its nearest face, nr_point_mesh.h) and face -> point (for every face its nearest point,
// nr_face_point.h).  Everything that tells them apart on the host is stated here.
struct PairDir {
    bool face_query;                   // the queries are the F faces and the targets the N points; else the reverse
    int qblock, tile, split_blocks;    // the nearest-neighbour launch's split plan
    int split_flag;                    // NR_LAUNCH_* of a split launch
    LaunchSlot* slot;                  // what nr_last_launch reads
    decltype(&k_point_face_nn) nn;     // the nearest-neighbour loop
    decltype(&k_pair_finish<false>) finish;
    const char *nn_name, *finish_name, *name;  // the two kernels as check_launch reports them; the direction in messages
    int queries(int N, int F) const { return face_query ? F : N; }
    int targets(int N, int F) const { return face_query ? N : F; }
};
const PairDir POINT_FACE = {false, PM_QBLOCK, PM_TILE, PM_SPLIT_BLOCKS, NR_LAUNCH_SPLIT_FACES, &g_last_point_mesh,
                            k_point_face_nn, k_pair_finish<false>, "k_point_face_nn", "k_point_face_finish", "point_mesh"};
const PairDir FACE_POINT = {true, FP_FBLOCK, FP_TILE, FP_SPLIT_BLOCKS, NR_LAUNCH_SPLIT_POINTS, &g_last_face_point,
                            k_face_point_nn, k_pair_finish<true>, "k_face_point_nn", "k_face_point_finish", "face_point"};

// either direction, nq its queries per item: records [B, F, PM_REC], the nearest target [B, nq], the loop's and
// the finish's dist2 [B, nq] each, and on the split path the partial d2 and index [B, nsplit, nq] each
struct PairLayout {
    SplitPlan plan;
    size_t records, nearest, loop_d2, fin_d2, part_d2, part_index, total;
};
PairLayout pair_layout(const PairDir& dir, int B, int N, int F) {
    const SplitPlan p = split_plan(B, dir.queries(N, F), dir.targets(N, F), dir.qblock, dir.tile, dir.split_blocks);
    const size_t bq = (size_t)B * dir.queries(N, F) * 4, part = bq * p.nsplit;
    Cutter c;
    return {p, c.take((size_t)B * F * PM_REC * 4), c.take(bq), c.take(bq), c.take(bq), c.take_if(p.nsplit > 1, part),
            c.take_if(p.nsplit > 1, part), c.off};
}

int validate_raster(const NrRasterArgs* a, bool need_workspace) {
    if (!a) return fail(NR_ERR_ARGS, "null args");
    if (a->batch_size < 0 || a->num_faces < 0 || a->num_vertices < 0 || a->image_size <= 0)
        return fail(NR_ERR_ARGS, "bad sizes B=%d F=%d V=%d s=%d", a->batch_size, a->num_faces, a->num_vertices,
                    a->image_size);
    const int S = internal_size(a->anti_aliasing, a->image_size);
    if (S > 16384) return fail(NR_ERR_ARGS, "image too large (%d internal pixels per side)", S);
    if (nr_num_channels(a->draw_flags) == 0) return fail(NR_ERR_ARGS, "nothing to draw");
    if (a->batch_size > 0 && a->num_faces > 0 && (!a->vertices || !a->faces || !a->face_records))
        return fail(NR_ERR_ARGS, "null vertices/faces/face_records");
    if (a->batch_size > 0 && !a->face_index) return fail(NR_ERR_ARGS, "null face_index");
    if (a->draw_flags & NR_DRAW_RGB) {
        if (!a->vertices_textures || !a->faces_textures || !a->textures || !a->face_uv)
            return fail(NR_ERR_ARGS, "rgb requested without textures");
        if (a->tex_height <= 0 || a->tex_width <= 0) return fail(NR_ERR_ARGS, "bad texture size");
        if (a->num_lights < 0) return fail(NR_ERR_ARGS, "negative light count");
        if (a->num_lights > 0 && (!a->lights || !a->vertex_normals || !a->face_normals || !a->normal_offsets ||
                                  !a->normal_faces))
            return fail(NR_ERR_ARGS, "lights need lights / face_normals / vertex_normals / normal CSR buffers");
        const long long span = 2 * std::llabs(a->tex_stride_c) +
                               ((long long)a->tex_height * a->tex_width - 1) * std::llabs(a->tex_stride_p) + 1;
        if (span >= (1ll << 31)) return fail(NR_ERR_ARGS, "texture item spans 2^31 elements or more");
    }
    const size_t need = forward_layout(a->batch_size, a->num_faces, make_geom(a->num_faces, S)).total;
    if (need_workspace && need > 0 && (!a->workspace || a->workspace_bytes < need))
        return fail(NR_ERR_WORKSPACE, "workspace missing or too small");
    return NR_OK;
}

Shade make_shade(const NrRasterArgs* a) {
    Shade sh;
    sh.draw = a->draw_flags;
    sh.C = nr_num_channels(a->draw_flags);
    sh.eps = a->eps;
    sh.tv.tex = a->textures;
    sh.tv.sb = a->tex_stride_b;
    sh.tv.sc = (int)a->tex_stride_c;
    sh.tv.sp = (int)a->tex_stride_p;
    sh.tv.H = a->tex_height;
    sh.tv.W = a->tex_width;
    sh.tv.t4 = reinterpret_cast<const float4*>(a->textures_packed);
    sh.tv.HWp = (int)packed_texels(a->tex_height, a->tex_width);
    sh.face_uv = a->face_uv;
    sh.uv_bstride = a->vt_batch_stride ? (long long)a->num_faces * 8 : 0;
    const bool rgb = (a->draw_flags & NR_DRAW_RGB) != 0;
    sh.nl = rgb ? a->num_lights : 0;
    sh.B = a->batch_size;
    sh.V = a->num_vertices;
    sh.lights = a->lights;
    sh.vnorm = a->vertex_normals;
    sh.fidx = a->faces;
    sh.bg = rgb ? a->backgrounds : nullptr;
    sh.bg_sb = a->bg_stride_b;
    sh.bg_sc = (int)a->bg_stride_c;
    sh.bg_sy = (int)a->bg_stride_y;
    return sh;
}

}  // namespace

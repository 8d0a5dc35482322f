/*
 * nr_raster.h -- C ABI of the MI355X (gfx950) rasterizer library libnr_raster.so.
 *
 * Plain pointers (device memory), sizes and a hipStream_t passed as void*.  No torch types.
 * Every entry point is asynchronous on `stream`, returns 0 on success and a nonzero
 * NR_ERR_* code on failure, with a message in nr_last_error() (thread-local).  The library never
 * allocates device memory: callers pass every output and the scratch workspace.
 *
 * Reference interfaces replaced (paths relative to /root/reference):
 *   pybind11 module neural_renderer_torch.cuda.rasterize_cuda  (cuda/rasterize_cuda.cpp:93-99)
 *     face_index_map_forward_safe  (.cpp:55-65 -> rasterize_cuda_kernel.cu:362-390, kernel :52-153)
 *                                   -> nr_face_index_map_forward_safe
 *     compute_weight_map_c         (.cpp:81-90 -> .cu:420-443, kernel :246-308)
 *                                   -> nr_compute_weight_map
 *     mask_foreground_forward      (.cpp:35-43 -> .cu:312-335)  -> nr_mask_foreground_forward
 *     mask_foreground_backward     (.cpp:45-53 -> .cu:337-359)  -> nr_mask_foreground_backward
 *     face_index_map_forward_unsafe (.cpp:67-79) -- dead code in the reference (its z-buffer
 *                                   update is commented out, .cu:236-240); not provided.
 *   python-level stages that had no native code in the reference, fused here:
 *     rasterize_core forward (rasterize.py:194-329: gather, face index, weight, coordinate, depth,
 *       texture and silhouette maps, channel merge, flip, 2x2 anti-aliasing)
 *                                   -> nr_rasterize_forward
 *     its autograd backward (Differentiation.backward differentiation.py:12-36, MaskForeground,
 *       to_map index backward, face gather backward)      -> nr_rasterize_backward
 *     Differentiation.backward on its own (differentiation.py:12-36)
 *                                   -> nr_differentiation_backward
 */
#ifndef NR_RASTER_H_
#define NR_RASTER_H_

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define NR_API __attribute__((visibility("default")))
#else
#define NR_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

enum {
    NR_OK = 0,
    NR_ERR_ARGS = 1,    /* invalid sizes / null pointers */
    NR_ERR_LAUNCH = 2,  /* a HIP launch failed */
    NR_ERR_WORKSPACE = 3 /* workspace too small */
};

/* Draw flags for nr_rasterize_forward / nr_rasterize_backward (RasterizeHyperparam.draw_*). */
enum { NR_DRAW_RGB = 1, NR_DRAW_SILHOUETTES = 2, NR_DRAW_DEPTH = 4 };

NR_API const char* nr_last_error(void);
NR_API int nr_version(void);
/* sizeof(NrRasterArgs), for bindings to check their mirror of the struct */
NR_API size_t nr_raster_args_size(void);

/* ABI version of this header: 6 (NrRasterArgs.face_hot / num_hot / hot_acc, nr_hot_acc_bytes; 5:
 * NrRasterArgs.face_index_sparse; 4: nr_last_launch; 3: workspace_zeroed of nr_rasterize_backward).
 * Bindings check it, and nr_raster_args_size(), before the first call. */
#define NR_ABI_VERSION 6

/* Scratch bytes needed by the face-index map for B items, F faces, S x S internal pixels
 * (per-face screen bounding boxes + coarse-bin face bitmasks). */
NR_API size_t nr_workspace_bytes(int batch_size, int num_faces, int image_size);

/* rasterize.py:27-38 / rasterize_cuda_kernel.cu:52-153.
 * faces: [B, F, 3, 3] f32 (screen x, y and depth z of each corner), face_index: [B, S, S] int32
 * (fully written; -1 = background).  Same arguments and meaning as the reference binding;
 * `eps` is accepted and unused exactly as in the reference kernel. */
NR_API int nr_face_index_map_forward_safe(const float* faces, int32_t* face_index, int batch_size, int num_faces,
                                   int image_size, float near, float far, int draw_backside, float eps,
                                   float depth_min_delta, void* workspace, size_t workspace_bytes,
                                   void* stream);

/* rasterize.py:67-77 / .cu:246-308.  weight_map: [B, S, S, 3] f32; background pixels are written
 * with 0 (the reference relies on a caller-zeroed buffer; here every element is written). */
NR_API int nr_compute_weight_map(const float* faces, const int32_t* face_index_map, float* weight_map,
                          int batch_size, int num_faces, int image_size, void* stream);

/* .cu:7-49: copy `dim` floats per pixel where face_index >= 0 (n = number of pixels). */
NR_API int nr_mask_foreground_forward(const int32_t* face_index, const float* data_in, float* data_out,
                               long long n, int dim, void* stream);
NR_API int nr_mask_foreground_backward(const int32_t* face_index, float* grad_in, const float* grad_out,
                                long long n, int dim, void* stream);

/* differentiation.py:12-36: grad_xy[B, H, W, 2] (x first) from the saved images[B, H, W, C] and
 * the incoming gradient grad[B, H, W, C]; step = 2 / H as in the reference. */
NR_API int nr_differentiation_backward(const float* images, const float* grad, float* grad_xy, int batch_size,
                                int height, int width, int channels, void* stream);

/* Arguments of the fused rasterize_core.  All pointers are device pointers; f32 unless noted.
 * Strides are in elements; a batch stride of 0 means "shared by every item" (a torch.expand). */
typedef struct NrRasterArgs {
    int batch_size;          /* B */
    int num_vertices;        /* V */
    int num_faces;           /* F */
    int image_size;          /* s: output size (RasterizeHyperparam.image_size) */
    int anti_aliasing;       /* internal S = 2s when set */
    int draw_backside;
    int draw_flags;          /* NR_DRAW_* */
    float near, far, eps;    /* eps: texture-coordinate clamp (RasterizeHyperparam.eps) */
    float depth_min_delta;   /* 1e-4 in the reference (rasterize.py:35) */
    const float* vertices;   /* [B, V, 3] contiguous, screen space (after look_at + perspective) */
    const int32_t* faces;    /* [F, 3] vertex indices, shared by every item */
    /* textures (only with NR_DRAW_RGB) */
    const float* vertices_textures; /* [Bvt, Vt, 2]; item stride vt_batch_stride (0 = shared) */
    long long vt_batch_stride;
    int num_vertices_textures;
    const int32_t* faces_textures;  /* [F, 3] */
    const float* textures;          /* [Bt, 3, H, W] with the strides below; (h, w) row-contiguous.
                                       Texture coordinates must stay inside the texture (within one
                                       texel past its edge, whose bilinear weight is 0), as the
                                       reference's to_map indexing requires (it raises IndexError);
                                       H and W below 2^23 (24-bit texel index arithmetic). */
    long long tex_stride_b, tex_stride_c, tex_stride_p; /* p = flat texel index h * W + w */
    int tex_height, tex_width;
    /* saved state, written by forward, read by backward */
    float* face_records;     /* [B, F, 16]: gathered faces (rasterize.py:232) + per-face reciprocals/flags */
    float* face_uv;          /* [Buv, F, 8] with Buv = (vt_batch_stride ? B : 1); only with RGB */
    int32_t* face_index;     /* [B, S, S] */
    void* workspace;         /* forward scratch, nr_workspace_bytes(B, F, S) */
    size_t workspace_bytes;
    /* backward only: CSR adjacency vertex -> face corners, built once per faces tensor.
     * vertex_faces[vertex_offsets[v] .. vertex_offsets[v+1]) lists 3 f + k for every faces[f, k] == v. */
    const int32_t* vertex_offsets; /* [V + 1] */
    const int32_t* vertex_faces;   /* [3 F] */
    /* optional halo cache, nr_halo_bytes() bytes (the tile-border image values, then one byte per
     * 32x32 bin and item: "the bin has a foreground pixel", which lets the backward skip background
     * tiles): when set, the forward stores the internal-image
     * values of the backward's tile borders there and the backward reads them instead of shading
     * its tile halos again; NULL = backward re-shades (same results). */
    float* halo;
    /* lights (rasterize.py:252-283, lights.py:4-39), only with NR_DRAW_RGB.  lights holds
     * [num_lights][B][NR_LIGHT_FLOATS] records in list order: kind (NR_LIGHT_*), backside, colour
     * r g b, then direction x y z (directional) or alpha (specular, slot 5).  The smooth normal
     * map (rasterize.py:162-190) needs: */
    int num_lights;
    const float* lights;
    float* face_normals;             /* [B, F, 3] scratch (forward) */
    float* vertex_normals;           /* [B, V, 4]: normalised normal + norm; written by the forward,
                                        read by the backward */
    const int32_t* normal_offsets;   /* [V + 1] CSR vertex -> its distinct faces (the reference's */
    const int32_t* normal_faces;     /*          one-hot [F, V] matrix, rasterize.py:173-179)     */
    /* backgrounds, only with NR_DRAW_RGB: [B, 3, S, S] at the internal size (x stride 1); the rgb of
     * background pixels is backgrounds[b, c, S-1-y, S-1-x] (the blend of
     * neural_renderer_chainer/rasterize.py:574-577; the torch blend_backgrounds raises) */
    const float* backgrounds;
    long long bg_stride_b, bg_stride_c, bg_stride_y;
    float* grad_backgrounds;         /* backward output [B, 3, S, S] contiguous, fully written; or NULL */
    /* optional, only with NR_DRAW_RGB: nr_texture_packed_bytes() of scratch that the forward fills
     * with the texels as RGBA rows [Bt, ceil4(H*W), 4] (Bt = tex_stride_b ? B : 1) and the forward and
     * backward then sample (one 16-B load per bilinear corner); kept by the caller from the forward
     * to the backward.  NULL = sample `textures` directly (same results). */
    float* textures_packed;
    /* optional, read by nr_rasterize_forward only: the backward's workspace
     * (nr_backward_workspace_bytes), allocated before the forward.  The forward zeroes its first
     * bwd_workspace_bytes bytes (the backward's accumulators) from the face-setup launch; the caller
     * may then pass workspace_zeroed = 1 to the ONE nr_rasterize_backward call that uses this
     * workspace next (after a backward its accumulators are no longer zero).  NULL = nothing zeroed. */
    void* bwd_workspace;
    size_t bwd_workspace_bytes;
    /* 1 = the caller reads face_index only inside the 32x32 bins that hold candidate faces (the
     * backward with a halo cache reads no other entry; a bin without candidates is -1 throughout): the
     * fused forward then leaves those bins' -1 entries unwritten (64 % of the headline's face-index
     * map).  Honoured only with the halo cache and the fused shading; nr_rasterize_backward_params
     * (which reads every entry) refuses such a forward state.  0 = face_index fully written. */
    int face_index_sparse;
    /* optional, backward only (NR_DRAW_RGB, a texture and texture coordinates shared by the batch):
     * texture windows that many faces share -- every face of an OBJ's flat-colour material samples
     * one 2x2 atlas patch (load_obj.py:84-94), so every wave that renders such a material would add
     * its window into the same texels.  face_hot[f] in [0, num_hot) names the shared window of face f
     * (faces with identical texture-coordinate triples share it), -1 for the rest; the backward then
     * adds those faces' window sums into one of NR_HOT_COPIES private copies per hot window in
     * hot_acc (nr_hot_acc_bytes(num_hot) bytes; zero at the start, like the backward's accumulators:
     * zeroed by the forward when it lies inside bwd_workspace, otherwise by nr_rasterize_backward
     * unless workspace_zeroed) and sums the copies into the texture gradient after its main kernel.
     * num_hot <= NR_HOT_MAX.  NULL / 0 = every window adds into the texture gradient directly (same
     * results up to the order of float additions). */
    const int32_t* face_hot;
    int num_hot;
    float* hot_acc;
} NrRasterArgs;

enum { NR_HOT_MAX = 256, NR_HOT_COPIES = 32 };
/* bytes of NrRasterArgs.hot_acc for num_hot shared windows */
NR_API size_t nr_hot_acc_bytes(int num_hot);

enum { NR_LIGHT_AMBIENT = 0, NR_LIGHT_DIRECTIONAL = 1, NR_LIGHT_SPECULAR = 2, NR_LIGHT_FLOATS = 8 };

/* Channels in output order: rgb (3), silhouettes (1), depth (1) -- those enabled by draw_flags. */
NR_API int nr_num_channels(int draw_flags);

/* rasterize.py:194-329 (without lights / backgrounds): images [B, C, s, s] contiguous.  Ordered on
 * `stream`; a deep-bin batch (B % 8 == 0) forks part of the forward onto the library's side stream and
 * joins it back with events before returning (NR_LAUNCH_SPLIT). */
NR_API int nr_rasterize_forward(const NrRasterArgs* args, float* images, void* stream);

/* Bytes of NrRasterArgs.textures_packed for texture_items textures of H x W texels. */
NR_API size_t nr_texture_packed_bytes(int texture_items, int tex_height, int tex_width);

/* Bytes of NrRasterArgs.halo for B items at output size s (internal 2s with anti-aliasing). */
NR_API size_t nr_halo_bytes(int batch_size, int image_size, int anti_aliasing, int draw_flags);

/* Scratch bytes of nr_rasterize_backward: per-face gradient records [B, F, 9], the texture
 * gradient accumulator [texture_items, H*W rounded up to 4, 4], and with lights the per-face
 * vertex-normal gradients [B, F, 9] and per-vertex normal gradients [B, V, 3]. */
NR_API size_t nr_backward_workspace_bytes(int batch_size, int num_faces, int num_vertices, int texture_items,
                                          int tex_height, int tex_width, int num_lights);

/* Backward of nr_rasterize_forward for upstream grad_images [B, C, s, s] (contiguous), given the
 * state the forward saved in `args`.  Writes grad_vertices [B, V, 3] and, with NR_DRAW_RGB and
 * grad_textures != NULL, grad_textures [Bt, 3, H, W] contiguous with Bt = (tex_stride_b ? B : 1)
 * (the batch total when the textures are shared).  Needs args->vertex_offsets/vertex_faces.
 * workspace_zeroed: per call, 1 when the caller guarantees the workspace's accumulators are zero
 * (the forward zeroed them through NrRasterArgs.bwd_workspace and no backward has used it since):
 * the backward then skips its own zero fill; 0 = the backward zero-fills (always correct).  With 1,
 * args->bwd_workspace must be `workspace` and args->bwd_workspace_bytes must cover the accumulators
 * (NR_ERR_ARGS otherwise).  A second backward over the same forward state must pass 0.  A texture
 * gradient takes at most 2^25 texels per texture and rows of at most 2^22 - 1 texels (NR_ERR_ARGS). */
NR_API int nr_rasterize_backward(const NrRasterArgs* args, const float* grad_images, float* grad_vertices,
                                 float* grad_textures, void* workspace, size_t workspace_bytes, int workspace_zeroed,
                                 void* stream);

/* The gradients that only the rgb channels carry and nr_rasterize_backward does not produce, for the
 * same forward state and upstream grad_images:
 *   grad_vertices_textures [Bvt, Vt, 2] (Bvt = vt_batch_stride ? B : 1; the batch total when shared):
 *     autograd of sample_textures' uv interpolation and clamps (rasterize.py:111-121) and of the
 *     faces_textures gather (rasterize.py:246);
 *   grad_lights [num_lights, B, NR_LIGHT_FLOATS], laid out like NrRasterArgs.lights: colour at 2..4,
 *     direction at 5..7 (directional) or exponent alpha at 5 (specular), zero elsewhere: autograd of
 *     the light loop (rasterize.py:252-283).
 * Either may be NULL; those given are fully written (zeroed, then accumulated).  Needs NR_DRAW_RGB. */
NR_API int nr_rasterize_backward_params(const NrRasterArgs* args, const float* grad_images,
                                        float* grad_vertices_textures, float* grad_lights, void* stream);

/* Camera prologue of Renderer.transform_vertices (renderer.py:27-38): look_at (look_at.py:5-44, with
 * the default at = (0, 0, 0) / up = (0, 1, 0) or the given ones) and/or perspective
 * (perspective.py:4-18), fused.  Cross products are per item (the reference's dim-less torch.cross
 * mixes items at B == 3, SURVEY section 8a hazards). */
/* NR_CAMERA_LOOK (look.py:5-30): the camera looks along a fixed direction, carried in `at` (z_u = at);
 * the axes then do not depend on the eye, whose gradient is the translation term alone. */
enum { NR_CAMERA_NONE = 0, NR_CAMERA_LOOK_AT = 1, NR_CAMERA_LOOK = 2 };
typedef struct NrCameraArgs {
    int batch_size;            /* B */
    int num_vertices;          /* V */
    const float* vertices;     /* [B, V, 3] world space; v_batch_stride 0 = one mesh for every item */
    long long v_batch_stride;
    const float* eye;          /* [B, 3] viewpoints; eye_batch_stride 0 = one eye for every item */
    long long eye_batch_stride;
    int mode;                  /* NR_CAMERA_* */
    float at[3], up[3];        /* at: the point looked at (LOOK_AT) or the viewing direction (LOOK) */
    int perspective;          /* apply x / z / width, y / z / width */
    float width;               /* tan(angle / 180 * 3.1416) in f32, as perspective.py:10-13 computes it */
} NrCameraArgs;

/* out [B, V, 3] contiguous. */
NR_API int nr_camera_forward(const NrCameraArgs* args, float* out, void* stream);
/* Scratch bytes of nr_camera_backward (per-item eye-gradient sums). */
NR_API size_t nr_camera_workspace_bytes(int batch_size);
/* grad_out [B, V, 3] -> grad_vertices [Bv, V, 3] (Bv = v_batch_stride ? B : 1, the item sum for a
 * shared mesh) and grad_eye [Be, 3] (Be = eye_batch_stride ? B : 1); either may be NULL, those
 * given are fully written. */
NR_API int nr_camera_backward(const NrCameraArgs* args, const float* grad_out, float* grad_vertices,
                              float* grad_eye, void* workspace, size_t workspace_bytes, void* stream);

/* Calibrated camera (projection.py): per vertex v of item b
 *   p = R v + t = (x, y, z);  x' = x / (z + eps), y' = y / (z + eps), r2 = x'^2 + y'^2
 *   rad = 1 + k1 r2 + k2 r2^2 + k3 r2^3
 *   x'' = x' rad + 2 p1 x' y' + p2 (r2 + 2 x'^2);  y'' = y' rad + p1 (r2 + 2 y'^2) + 2 p2 x' y'
 *   u = K00 x'' + K01 y'' + K02;  v = K10 x'' + K11 y'' + K12          (row 2 of K is not read)
 *   out = (2 (u - S/2) / S, 2 ((S - v) - S/2) / S, z)                  with S = orig_size
 * dist holds (k1, k2, p1, p2, k3) per item, in OpenCV's order.  Batch strides are in elements; 0 = the
 * one record is shared by every item. */
typedef struct NrProjectionArgs {
    int batch_size;            /* B */
    int num_vertices;          /* V */
    const float* vertices;     /* [B, V, 3] world space; v_batch_stride 0 = one mesh for every item */
    long long v_batch_stride;
    const float* K;            /* [B, 3, 3] row-major intrinsics */
    long long k_batch_stride;
    const float* R;            /* [B, 3, 3] row-major rotation */
    long long r_batch_stride;
    const float* t;            /* [B, 3] translation */
    long long t_batch_stride;
    const float* dist;         /* [B, 5] distortion coefficients, or NULL = zeros */
    long long dist_batch_stride;
    float orig_size;           /* S */
    float eps;
} NrProjectionArgs;

/* sizeof(NrProjectionArgs), for bindings to check their mirror of the struct */
NR_API size_t nr_projection_args_size(void);
/* out [B, V, 3] contiguous. */
NR_API int nr_projection_forward(const NrProjectionArgs* args, float* out, void* stream);
/* Scratch bytes of nr_projection_backward when a parameter gradient is asked for: the per-block partial
 * sums [B][ceil(V / 256)][24] (no zero fill needed; every entry read is written first). */
NR_API size_t nr_projection_workspace_bytes(int batch_size, int num_vertices);
/* grad_out [B, V, 3] -> grad_vertices [Bv, V, 3], grad_K [Bk, 3, 3] (row 2 zero), grad_R [Br, 3, 3],
 * grad_t [Bt, 3], grad_dist [Bd, 5], each with Bx = (its batch stride ? B : 1), the item sum when shared.
 * Any of them may be NULL; those given are fully written (zeros when B == 0 or V == 0).  The parameter
 * gradients are summed in a fixed order without atomics: bitwise reproducible from run to run.  The
 * workspace is needed only with a parameter gradient. */
NR_API int nr_projection_backward(const NrProjectionArgs* args, const float* grad_out, float* grad_vertices,
                                  float* grad_K, float* grad_R, float* grad_t, float* grad_dist,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* Mesh regularizers (mesh_loss.py), for vertices [B, V, 3] contiguous and a topology shared by every item.
 * No float atomics: losses and gradients are bitwise reproducible from run to run.
 *
 * Laplacian: N(i) = the distinct vertices sharing a face edge with i, as the CSR nbr_offsets [V + 1] /
 * nbr_index (ascending per vertex; symmetric: j in N(i) <=> i in N(j)).
 *   delta_i = v_i - (1 / |N(i)|) sum_{j in N(i)} v_j   (0 when N(i) is empty);   loss_b = sum_i |delta_i|^2
 *   grad v_i = 2 g_b (delta_i - sum_{j in N(i)} delta_j / |N(j)|)
 * Flatten: edges [E2, 4] int32 rows (v0, v1, v2, v3), one per undirected edge v0 < v1 with exactly two
 * incident faces, v2 / v3 their opposite vertices (16-byte aligned).  Per row, with a = v1 - v0,
 * b1 = v2 - v0, b2 = v3 - v0:
 *   c_k = b_k - a (a . b_k) / (|a|^2 + eps);  cos = (c_1 . c_2) / (sqrt(|c_1|^2 + eps) sqrt(|c_2|^2 + eps))
 *   loss_b = sum_rows (cos + 1)^2
 * edge_offsets [V + 1] / edge_slots [4 E2]: CSR vertex -> the entries 4 e + k with edges[e, k] == vertex,
 * ascending.
 * Limits: 4 E2 < 2^31; B * ceil(V / 256) and B * ceil(E2 / 256) <= INT_MAX (NR_ERR_ARGS otherwise).  The
 * topology arrays are trusted: every vertex index in them must be below V, every slot below 4 E2.
 *
 * Scratch bytes of a forward: the per-block partial sums [B][ceil(count / 256)], count = V (Laplacian) or
 * E2 (flatten); no zero fill needed. */
NR_API size_t nr_mesh_loss_workspace_bytes(int batch_size, int count);
/* loss [B], fully written (0 when V == 0).  delta [B, V, 3] (what the backward reads) or NULL. */
NR_API int nr_laplacian_forward(const float* vertices, const int32_t* nbr_offsets, const int32_t* nbr_index,
                                int batch_size, int num_vertices, float* delta, float* loss, void* workspace,
                                size_t workspace_bytes, void* stream);
/* grad_loss [B] -> grad_vertices [B, V, 3], fully written, from the forward's delta. */
NR_API int nr_laplacian_backward(const float* delta, const int32_t* nbr_offsets, const int32_t* nbr_index,
                                 const float* grad_loss, int batch_size, int num_vertices, float* grad_vertices,
                                 void* stream);
/* loss [B], fully written (0 when E2 == 0).  records [B, E2, 12] (what the backward reads) or NULL: each
 * row's gradient to its four vertices (d loss_row / d v0..v3), 16-byte aligned. */
NR_API int nr_flatten_forward(const float* vertices, const int32_t* edges, int batch_size, int num_vertices,
                              int num_edges, float eps, float* records, float* loss, void* workspace,
                              size_t workspace_bytes, void* stream);
/* grad_loss [B] -> grad_vertices [B, V, 3], fully written: each vertex sums the forward's records of its
 * slots in ascending order. */
NR_API int nr_flatten_backward(const float* records, const int32_t* edge_offsets, const int32_t* edge_slots,
                               const float* grad_loss, int batch_size, int num_vertices, int num_edges,
                               float* grad_vertices, void* stream);

/* Two more regularizers on the same neighbour CSR and the same conventions.  Faces with a repeated vertex
 * index are ignored by both (the CSR holds no edge of theirs).
 *
 * Edge length: E = the distinct undirected edges {i, j} of the faces -- the pairs j in N(i), j > i;
 * boundary and non-manifold edges count once each.  With len_ij = |v_i - v_j| and L = target_length >= 0:
 *   loss_b = sum_{ {i,j} in E } (len_ij - L)^2
 *   grad v_i = 2 g_b sum_{j in N(i)} (len_ij - L) / len_ij * (v_i - v_j)
 * An edge with len_ij == 0 contributes L^2 to the loss and nothing to the gradient.  The backward
 * recomputes from the vertices; the workspace is nr_mesh_loss_workspace_bytes(B, V).
 *
 * Cotangent Laplacian: for corner k of face f (faces [F, 3] int32), a and b the edge vectors leaving it,
 *   c_{f,k} = 0.5 (a . b) / sqrt(|a x b|^2 + eps)
 * Corner (f, k) is opposite the edge of the face's two other corners.  Every entry e = (i, j) of the
 * neighbour CSR lists its opposite corners 3 f + k, ascending, in nbr_corners [nbr_corner_offsets[e] ..
 * nbr_corner_offsets[e + 1]) (nbr_corner_offsets [nnz + 1], nnz = num_neighbours = nbr_offsets[V]); the
 * entries (i, j) and (j, i) hold the same list.  A boundary edge has one corner, a manifold edge two.
 *   w_ij = max(0, sum of c_{f,k} over the list of (i, j), in list order)      (so w_ij == w_ji bit for bit)
 *   W_i  = sum_{j in N(i)} w_ij  (CSR order);   ok_i = W_i > NR_COT_MIN_WEIGHT
 *   delta_i = ok_i ? v_i - (sum_j w_ij v_j) / W_i : 0;   loss_b = sum_i |delta_i|^2
 * The clamp keeps the weighted mean a convex combination where both opposite angles are obtuse.  The
 * weights are constants of the backward (no gradient flows through them):
 *   grad v_k = 2 g_b (delta_k - sum_{i in N(k)} w_ki Winv_i delta_i),   Winv_i = ok_i ? 1 / W_i : 0
 * Limits: those above with E2 = 0, and B * ceil(F / 256) <= INT_MAX, 3 F < 2^31.  The corner lists are
 * trusted: every corner below 3 F and of a face without a repeated index. */
#define NR_COT_MIN_WEIGHT 1e-6f
/* loss [B], fully written (0 when V == 0). */
NR_API int nr_edge_length_forward(const float* vertices, const int32_t* nbr_offsets, const int32_t* nbr_index,
                                  int batch_size, int num_vertices, float target_length, float* loss,
                                  void* workspace, size_t workspace_bytes, void* stream);
/* grad_loss [B] -> grad_vertices [B, V, 3], fully written, from the forward's vertices. */
NR_API int nr_edge_length_backward(const float* vertices, const int32_t* nbr_offsets, const int32_t* nbr_index,
                                   const float* grad_loss, int batch_size, int num_vertices, float target_length,
                                   float* grad_vertices, void* stream);
/* Scratch bytes of nr_cot_laplacian_forward: the per-block partial sums [B][ceil(V / 256)], then the
 * half-cotangents [B][3 F]; no zero fill needed. */
NR_API size_t nr_cot_laplacian_workspace_bytes(int batch_size, int num_vertices, int num_faces);
/* loss [B], fully written (0 when V == 0).  What the backward reads, each fully written or NULL:
 * delta [B, V, 3], w [B, nnz] (the weight of every CSR entry) and winv [B, V]. */
NR_API int nr_cot_laplacian_forward(const float* vertices, const int32_t* faces, const int32_t* nbr_offsets,
                                    const int32_t* nbr_index, const int32_t* nbr_corner_offsets,
                                    const int32_t* nbr_corners, int batch_size, int num_vertices, int num_faces,
                                    int num_neighbours, float eps, float* delta, float* w, float* winv, float* loss,
                                    void* workspace, size_t workspace_bytes, void* stream);
/* grad_loss [B] -> grad_vertices [B, V, 3], fully written, from the forward's delta, w and winv. */
NR_API int nr_cot_laplacian_backward(const float* delta, const float* w, const float* winv,
                                     const int32_t* nbr_offsets, const int32_t* nbr_index, const float* grad_loss,
                                     int batch_size, int num_vertices, int num_neighbours, float* grad_vertices,
                                     void* stream);

/* As-rigid-as-possible (ARAP) energy (mesh_loss.py: arap_loss), on the same neighbour CSR and the same
 * conventions: how far the deformed vertices q [B, V, 3] are from being, around every vertex, a rotated copy
 * of the rest shape p.  p and the entry weights w are read at an item stride each, 0 when the items share
 * them (else 3 V and nnz).  With e_ij = p_i - p_j and d_ij = q_i - q_j:
 *   S_i  = sum_{j in N(i)} w_ij e_ij d_ij^T   (3 x 3, the neighbours in CSR order)
 *   R_i  = the rotation (det +1) that maximises tr(R S_i): with S = U Sigma V^T it is
 *          V diag(1, 1, det(V U^T)) U^T.  S_i = 0 gives R_i = I.  Where the maximiser is not unique (the two
 *          largest eigenvalues of Horn's 4 x 4 matrix meet: sigma_2 + det sigma_3 = 0) any maximiser is
 *          returned; every output stays finite.
 *   loss_b = sum_i sum_{j in N(i)} w_ij |d_ij - R_i e_ij|^2
 * The rotations are constants of the backward; they maximise, so by the envelope theorem this is the exact
 * gradient wherever the maximiser is unique:
 *   grad q_i = 2 g_b sum_{j in N(i)} w_ij (2 d_ij - (R_i + R_j) e_ij)           (needs w_ij == w_ji)
 * Neither p nor w takes a gradient.  w == NULL is the weight 1 for every entry.  A rotation is stored as the
 * unit quaternion (w, x, y, z), rotations [B, V, 4], 16-byte aligned; it is found per vertex in registers as
 * the top eigenvector of Horn's symmetric 4 x 4 matrix by cyclic Jacobi sweeps.
 * Limits: those of the Laplacian (NR_ERR_ARGS otherwise, and for an item stride that is neither 0 nor the
 * item's size).
 *
 * The cotangent weights of the cotangent Laplacian as an output of their own, so that they can be taken from
 * a rest shape once: w [B, nnz], w_ij = max(0, sum of c_{f,k} over the corner list of entry (i, j)), bit for
 * bit the weights nr_cot_laplacian_forward forms on the same vertices (w_ij == w_ji bit for bit).  Limits:
 * the cotangent Laplacian's, and B * ceil(nnz / 256) <= INT_MAX.
 * Scratch bytes of nr_cot_weights: the half-cotangents [B][3 F]; no zero fill needed. */
NR_API size_t nr_cot_weights_workspace_bytes(int batch_size, int num_faces);
/* vertices [B, V, 3] -> w [B, nnz], fully written. */
NR_API int nr_cot_weights(const float* vertices, const int32_t* faces, const int32_t* nbr_corner_offsets,
                          const int32_t* nbr_corners, int batch_size, int num_vertices, int num_faces,
                          int num_neighbours, float eps, float* w, void* workspace, size_t workspace_bytes,
                          void* stream);
/* Scratch bytes of nr_arap_forward: the per-block partial sums [B][ceil(V / 256)]; no zero fill needed. */
NR_API size_t nr_arap_workspace_bytes(int batch_size, int num_vertices);
/* loss [B], fully written (0 when V == 0).  rotations [B, V, 4] (what the backward reads), fully written, or
 * NULL. */
NR_API int nr_arap_forward(const float* vertices, const float* rest, long long rest_batch_stride, const float* w,
                           long long w_batch_stride, const int32_t* nbr_offsets, const int32_t* nbr_index,
                           int batch_size, int num_vertices, int num_neighbours, float* rotations, float* loss,
                           void* workspace, size_t workspace_bytes, void* stream);
/* grad_loss [B] -> grad_vertices [B, V, 3], fully written, from the forward's inputs and rotations. */
NR_API int nr_arap_backward(const float* vertices, const float* rest, long long rest_batch_stride, const float* w,
                            long long w_batch_stride, const float* rotations, const int32_t* nbr_offsets,
                            const int32_t* nbr_index, const float* grad_loss, int batch_size, int num_vertices,
                            int num_neighbours, float* grad_vertices, void* stream);

/* Articulated meshes (skinning.py): forward kinematics of a joint tree, then linear blend skinning.  A
 * transform is 12 floats, row-major 3 x 4: [R | t].  No float atomics anywhere: every output and gradient is
 * bitwise reproducible from run to run, and an item's results do not depend on the batch it is in.
 *
 * Skeleton: parents [J] int32, -1 a root (several allowed), else a joint index; joints need not be listed
 * parents-first.  The host passes the joints sorted by depth -- level_joints [J], ascending within a level,
 * level l being level_joints[level_offsets[l] .. level_offsets[l + 1]), level_offsets [L + 1] -- and the children
 * CSR, child_offsets [J + 1] and children, ascending.  These arrays are trusted (topology.py builds them).
 *
 * Rotation: pose [B, J, 3] axis-angle (pose_is_matrix == 0) or [B, J, 3, 3] matrices, used as given.  For an
 * axis-angle r with t2 = |r|^2, K = skew(r):  R = I + a K + b K^2,  a = sin t / t,  b = (1 - cos t) / t^2; where
 * t2 < NR_RODRIGUES_SERIES, a = 1 - t2/6 + t2^2/120 and b = 1/2 - t2/24 + t2^2/720 (R and its gradient are
 * defined at r = 0).
 *
 * Chain: c_j = joints[b or shared, j] (joints_batch_stride 0 or 3 J), p the parent of j:
 *   root: G_j.R = R_j, G_j.t = c_j;   else: G_j.R = G_p.R R_j,  G_j.t = G_p.t + G_p.R (c_j - c_p)
 *   posed_joints[b, j] = G_j.t;   transforms[b, j] = [G_j.R | G_j.t - G_j.R c_j]
 * (a transform takes a rest-pose point to its posed place).
 *
 * Skinning: out[b, v] = sum_k w[v, k] (A.R x + A.t),  A = transforms[b, indices[v, k]],  x = vertices[b or
 * shared, v] (vertices_batch_stride 0 or 3 V); weights and indices are [V, K], 1 <= K <= NR_SKIN_MAX_INFLUENCES,
 * the weights used as given (not normalised).  A slot of weight 0 is padding; its index must still be in
 * [0, J) (trusted).  The gradient to the transforms sums, per joint, over the slots of non-zero weight that
 * name it: the joint CSR lists them by (vertex, slot) -- entry_vertex and entry_slot -- and the chunk table cuts
 * each joint's row into runs of at most NR_SKIN_CHUNK entries: chunk c is the entries [chunk_begin[c],
 * chunk_end[c]), and joint j owns the chunks [joint_chunk_offsets[j], joint_chunk_offsets[j + 1]), ascending.
 *
 * Limits (NR_ERR_ARGS otherwise): 1 <= J <= NR_SKIN_MAX_JOINTS for every call; for the nr_skin_* calls also
 * 1 <= K <= NR_SKIN_MAX_INFLUENCES, B <= 65535 (an item is a grid row there) and 8 V < 2^31.  Pointers need the
 * alignment of their element type only.  children may be NULL when no joint has a parent. */
#define NR_SKIN_MAX_JOINTS 256
#define NR_SKIN_MAX_INFLUENCES 8
#define NR_SKIN_CHUNK 256
#define NR_RODRIGUES_SERIES 1e-4f
/* transforms [B, J, 3, 4] and posed_joints [B, J, 3], both fully written.  One block per item, one thread per
 * joint, one barrier per level. */
NR_API int nr_pose_transforms_forward(const float* pose, int pose_is_matrix, const float* joints,
                                      long long joints_batch_stride, const int32_t* parents,
                                      const int32_t* level_offsets, const int32_t* level_joints, int batch_size,
                                      int num_joints, int num_levels, float* transforms, float* posed_joints,
                                      void* stream);
/* grad_transforms [B, J, 3, 4] and grad_posed_joints [B, J, 3] (either may be NULL: zeros) -> grad_pose (the
 * pose's shape) and grad_joints [B, J, 3] (per item also for shared joints: the caller sums), each fully
 * written or NULL.  transforms are the forward's. */
NR_API int nr_pose_transforms_backward(const float* pose, int pose_is_matrix, const float* joints,
                                       long long joints_batch_stride, const int32_t* parents,
                                       const int32_t* level_offsets, const int32_t* level_joints,
                                       const int32_t* child_offsets, const int32_t* children,
                                       const float* transforms, const float* grad_transforms,
                                       const float* grad_posed_joints, int batch_size, int num_joints,
                                       int num_levels, float* grad_pose, float* grad_joints, void* stream);
/* Scratch bytes of nr_skin_backward's transform gradient: the chunk partials [B][num_chunks][12]; no zero fill
 * needed. */
NR_API size_t nr_skin_workspace_bytes(int batch_size, int num_chunks);
/* out [B, V, 3], fully written. */
NR_API int nr_skin_forward(const float* vertices, long long vertices_batch_stride, const float* transforms,
                           const float* weights, const int32_t* indices, int batch_size, int num_vertices,
                           int num_joints, int num_influences, float* out, void* stream);
/* grad_out [B, V, 3] -> grad_vertices ([B, V, 3], or [V, 3] for shared vertices: the sum over the items, in item
 * order), grad_transforms [B, J, 3, 4] (exact zeros for a joint without entries; needs the joint CSR, the chunk
 * table and the workspace) and grad_weights [V, K] (the sum over the items of g . (A x), for every slot); each
 * fully written or NULL. */
NR_API int nr_skin_backward(const float* vertices, long long vertices_batch_stride, const float* transforms,
                            const float* weights, const int32_t* indices, const float* grad_out,
                            const int32_t* entry_vertex, const int32_t* entry_slot, const int32_t* chunk_begin,
                            const int32_t* chunk_end, const int32_t* joint_chunk_offsets, int batch_size,
                            int num_vertices, int num_joints, int num_influences, int num_chunks,
                            float* grad_vertices, float* grad_transforms, float* grad_weights, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Image losses (image_loss.py): per-item reductions of images [B, N] float32, item b being the N
 * contiguous floats at images + b * image_stride (strides in elements, >= 0).  targets: item b at
 * targets + b * target_stride, 0 = one target shared by every item.  No float atomics: losses and
 * gradients are bitwise reproducible from run to run.
 *
 * Pointwise (kind = NR_LOSS_SQUARED or NR_LOSS_HUBER), d_i = x_i - t_i:
 *   loss_b = sum_i w_i h(d_i),   h(d) = d^2   (squared; no 1/2)
 *                                h(d) = d^2 / 2 if |d| < delta, else delta (|d| - delta / 2)   (Huber; 0 < delta < inf)
 *   grad x_i = g_b w_i h'(d_i),  h'(d) = 2 d  (squared);  d if |d| < delta, else delta sign(d)  (Huber)
 * weights: NULL (w_i = 1), or w_i = weights[b * weight_stride + i % weight_period] with weight_period >= 1
 * dividing N: N for full weights, H W for a pixel mask shared by the channels; weight_stride 0 = shared.
 * IoU of silhouettes p against t:
 *   I_b = sum_i p_i t_i,  U_b = sum_i (p_i + t_i - p_i t_i),  loss_b = 1 - I_b / (U_b + eps)
 *   grad p_i = -g_b (t_i (U_b + eps) - I_b (1 - t_i)) / (U_b + eps)^2
 *
 * Each launch takes 16-byte loads and stores when every item base of images, targets (and grad_images)
 * is 16-byte aligned, and vector weight loads when the weights' bases are too and weight_period is a
 * multiple of 4; an N that is no multiple of 4 ends in scalar accesses; any other layout runs scalar.
 * Limits: N <= INT_MAX - 4096 and B * ceil(N / 4096) <= INT_MAX (NR_ERR_ARGS otherwise).  With B == 0 or
 * N == 0 no kernel is launched and every output is still fully written (fills on the stream).
 *
 * Scratch bytes of a forward: the per-block partial sums [B][ceil(N / 4096)][2]; no zero fill needed. */
enum { NR_LOSS_SQUARED = 0, NR_LOSS_HUBER = 1 };
NR_API size_t nr_image_loss_workspace_bytes(int batch_size, int item_elems);
/* loss [B], fully written (0 when N == 0). */
NR_API int nr_pointwise_loss_forward(const float* images, long long image_stride, const float* targets,
                                     long long target_stride, const float* weights, long long weight_stride,
                                     int weight_period, int kind, float delta, int batch_size, int item_elems,
                                     float* loss, void* workspace, size_t workspace_bytes, void* stream);
/* grad_loss [B] -> grad_images [B, N] contiguous, fully written; recomputed from the forward's inputs. */
NR_API int nr_pointwise_loss_backward(const float* images, long long image_stride, const float* targets,
                                      long long target_stride, const float* weights, long long weight_stride,
                                      int weight_period, int kind, float delta, int batch_size, int item_elems,
                                      const float* grad_loss, float* grad_images, void* stream);
/* loss [B] and sums [B, 2] = (I_b, U_b), both fully written (N == 0: sums 0, loss 1 - 0 / (0 + eps)). */
NR_API int nr_iou_loss_forward(const float* images, long long image_stride, const float* targets,
                               long long target_stride, float eps, int batch_size, int item_elems, float* loss,
                               float* sums, void* workspace, size_t workspace_bytes, void* stream);
/* grad_loss [B] -> grad_images [B, N] contiguous, fully written, from the forward's sums and the targets
 * (the gradient does not depend on p_i, so the silhouettes are not an argument). */
NR_API int nr_iou_loss_backward(const float* targets, long long target_stride, const float* sums, float eps,
                                int batch_size, int item_elems, const float* grad_loss, float* grad_images,
                                void* stream);

/* SSIM loss (image_loss.py ssim_loss; Wang et al. 2004): images [B, C, H, W] float32, item b being the
 * C H W contiguous floats at images + b * image_stride; targets the same at target_stride (0 = shared).
 * window: HOST array of window_size float32 weights g, window_size = 2R + 1 odd in 3..11 (read during the
 * call, passed to the kernels by value); G = g (x) g, applied per channel.  padding NR_SSIM_SAME: zeros
 * R pixels around the image, the map is H' x W' = H x W; NR_SSIM_VALID: no padding, H' x W' =
 * (H - 2R) x (W - 2R), which must be at least 1 x 1.  Per map pixel, with x the image and t the target:
 *   mu1 = G*x   mu2 = G*t   s11 = G*x^2 - mu1^2   s22 = G*t^2 - mu2^2   s12 = G*(x t) - mu1 mu2
 *   n1 = 2 mu1 mu2 + c1   n2 = 2 s12 + c2   d1 = mu1^2 + mu2^2 + c1   d2 = s11 + s22 + c2
 *   S = n1 n2 / (d1 d2)          loss_b = 1 - (sum of S over the item's C H' W' map pixels) / (C H' W')
 * No variance clamp.  The forward with saved != NULL also writes three maps, saved [3][B][C][H'][W']:
 *   Bm = -S / d2 (= dS / d G*x^2)      Cm = 2 n1 / (d1 d2) (= dS / d G*(x t))
 *   A  = 2 mu2 n2 / (d1 d2) - 2 mu1 S / d1 - 2 mu1 Bm - mu2 Cm (= dS / d mu1)
 * which with the inputs are all the backward reads (the maps zero outside H' x W', 'valid' maps sitting R
 * pixels inside the image):
 *   grad x(p) = -(g_b / (C H' W')) ((G*A)(p) + 2 x(p) (G*Bm)(p) + t(p) (G*Cm)(p))
 * One block per 32 x 32 tile of one channel stages the tile and its R-pixel halo in LDS and filters rows,
 * then columns; the filter taps are fused multiply-adds.  No float atomics: bitwise reproducible.
 * Limits: C H W <= INT_MAX, B C ceil(H / 32) ceil(W / 32) <= INT_MAX (NR_ERR_ARGS otherwise).  With B == 0
 * nothing is written; with C H W == 0 the losses are 0 (a fill on the stream) and no kernel is launched.
 *
 * Scratch bytes of a forward: the per-tile partial sums [B][C][tiles of the map]; no zero fill needed
 * (0 for sizes the entry points reject). */
enum { NR_SSIM_SAME = 0, NR_SSIM_VALID = 1 };
NR_API size_t nr_ssim_loss_workspace_bytes(int batch_size, int channels, int height, int width, int window_size,
                                           int padding);
/* loss [B], fully written; saved NULL (no gradient wanted) or [3][B][C][H'][W'], fully written. */
NR_API int nr_ssim_loss_forward(const float* images, long long image_stride, const float* targets,
                                long long target_stride, int batch_size, int channels, int height, int width,
                                int window_size, const float* window, float c1, float c2, int padding, float* loss,
                                float* saved, void* workspace, size_t workspace_bytes, void* stream);
/* grad_loss [B] -> grad_images [B, C H W] contiguous, fully written, from the forward's saved maps. */
NR_API int nr_ssim_loss_backward(const float* images, long long image_stride, const float* targets,
                                 long long target_stride, const float* saved, int batch_size, int channels,
                                 int height, int width, int window_size, const float* window, int padding,
                                 const float* grad_loss, float* grad_images, void* stream);

/* Optimiser (optimizers.py): Adam over a list of float32 tensors, with the two rules of the reference's
 * optimizers.py:1-37: an element whose gradient is zero is left alone (skip_zero_grad), and each tensor
 * scales the rate by its own lr_scale (the reference's param.lr).  One call advances every listed
 * tensor's step and updates it, NR_ADAM_MAX_TENSORS tensors per launch pair (k_adam_tick, k_adam_update).
 *
 * Per tensor, with t = its step after the increment (step: one float32 on the device, as
 * torch.optim.Adam(capturable=True) keeps it):
 *   c1 = (float)(1 - beta1)      c2 = (float)(1 - beta2)             (from the double arguments)
 *   step_size = (float)(lr * lr_scale / (1 - beta1^t))               (computed in double)
 *   inv_sqrt_bc2 = (float)(1 / sqrt(1 - beta2^t))                    (computed in double)
 * and per element, in float32, in this order, with no contraction:
 *   if skip_zero_grad and g == 0: leave p, m, v as they are          (both zeros count; NaN does not)
 *   m = m + c1 * (g - m)
 *   v = v + c2 * (g * g - v);   v = v < 0 ? 0 : v                    (the reference's clamp, optimizers.py:25)
 *   p = p - step_size * (m / (sqrt(v) * inv_sqrt_bc2 + eps))
 * Without skip_zero_grad and with lr_scale = 1 this is torch.optim.Adam's rule (amsgrad = False, no weight
 * decay, maximize = False) up to rounding.  With skip_zero_grad the step still advances per tensor and a
 * skipped element's moments do not decay (lazy Adam).
 *
 * lr: the host double, or, with lr_device non-null, the float32 read from the device by the tick kernel (a
 * schedule can change it between replays of a captured step); lr must be finite either way.  The factor
 * scratch holds (step_size, inv_sqrt_bc2) per listed tensor, in list order, written by the tick kernel of
 * this call: it belongs to the caller, needs no fill, and must not be shared by calls that may overlap.
 * A tensor takes 16-byte accesses when param, grad, exp_avg and exp_avg_sq are all 16-byte aligned and
 * lane-consecutive scalar accesses otherwise, with bitwise identical results.  The listed tensors must not
 * overlap each other, and no two may share a step.  A tensor with numel == 0 takes no blocks (its step,
 * when given, still advances).
 * Checked before any launch (NR_ERR_ARGS): 0 <= num_tensors <= tensors_capacity (the length of the host
 * array), non-null param / grad / exp_avg / exp_avg_sq / step for every tensor with numel > 0,
 * 0 <= numel <= INT_MAX - NR_ADAM_CHUNK, finite lr and lr_scale, 0 <= beta1, beta2 < 1, eps >= 0; a missing
 * or short scratch is NR_ERR_WORKSPACE.  Never synchronises with the host. */
enum { NR_ADAM_MAX_TENSORS = 24, NR_ADAM_CHUNK = 4096 /* elements of one tensor per block */ };
typedef struct NrAdamTensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    float* step;
    long long numel;
    double lr_scale;
} NrAdamTensor;
typedef struct NrAdamArgs {
    int num_tensors;
    int tensors_capacity;
    const NrAdamTensor* tensors; /* host array */
    double lr, beta1, beta2, eps;
    const float* lr_device;
    int skip_zero_grad;
    void* scratch;
    size_t scratch_bytes;
} NrAdamArgs;
NR_API size_t nr_adam_args_size(void);
NR_API size_t nr_adam_scratch_bytes(int num_tensors);
NR_API int nr_adam_step(const NrAdamArgs* args, void* stream);

/* Vertex attributes (attributes.py): any per-vertex table [Va, C] rendered as an image [B, C, s, s], in
 * place of rgb_map in rasterize_core (rasterize.py:227-329).  The caller first runs nr_rasterize_forward
 * with NR_DRAW_SILHOUETTES alone, face_index_sparse = 0 and no halo, and hands its face_index [B, S, S]
 * and face_records [B, F, 16] over (S = 2 s with anti-aliasing, else s).  Per foreground pixel of face f
 * with the weights w_k of compute_weight_map, corner depths z_k and corner rows a_k = attributes[b,
 * faces_attributes[f, k]]:
 *   linear:               out_c = sum_k w_k a_kc                                    (rasterize.py:185-187)
 *   perspective-correct:  q_k = w_k / (z_k + 1e-10),  Dn = sum_k (q_k + 1e-10),
 *                         out_c = (sum_k q_k a_kc) / Dn                             (rasterize.py:113-119)
 * no clamp; background pixels 0.  The image is the internal one [B, S, S, C] permuted to [B, C, S, S],
 * flipped along both image axes and, with anti-aliasing, averaged over 2x2 (rasterize.py:315-328).
 * Backward, for the internal-pixel upstream g_c and the soft gradient (gx, gy) of Differentiation.backward
 * (differentiation.py:12-36) on the internal image:
 *   d a_kc: w_k g_c (linear), (q_k / Dn) g_c (perspective-correct)
 *   d vertex (x, y): w_k (gx, gy);   d vertex z: -(q_k / (z_k + 1e-10)) / Dn sum_c g_c (a_kc - out_c)
 *   (perspective-correct; 0 in the linear mode), added at vertex faces[f, k] and row faces_attributes[f, k].
 * The sums over a wave's pixels use float atomics into per-face-corner records: gradients agree from run
 * to run up to the order of float additions; the sums over the records keep a fixed order.
 * Limits: 1 <= C <= NR_ATTR_MAX_CHANNELS, S <= 16384, B <= 65535 (NR_ERR_ARGS otherwise).  The index arrays
 * are trusted: face_index below F, faces_attributes below Va, CSR entries below 3 F.  With B, F or V equal
 * to 0 no kernel is launched and every output is still fully written (fills on the stream). */
enum { NR_ATTR_MAX_CHANNELS = 64 };
typedef struct NrAttributeArgs {
    int batch_size;               /* B */
    int num_faces;                /* F */
    int num_vertices;             /* V */
    int num_attributes;           /* Va: rows of the attribute table */
    int num_channels;             /* C */
    int image_size;               /* s */
    int anti_aliasing;            /* internal S = 2 s when set */
    int perspective_correct;
    const int32_t* face_index;    /* [B, S, S], fully written by the forward (-1 = background) */
    const float* face_records;    /* [B, F, 16] */
    const int32_t* faces;         /* [F, 3] vertex indices (the layout the vertex CSR was built from; not read) */
    const int32_t* faces_attributes; /* [F, 3] attribute row indices */
    const float* attributes;      /* [Ba, Va, C], item stride attr_batch_stride in elements; 0 = shared, Ba = 1 */
    long long attr_batch_stride;
    float* internal;              /* the internal image [B, S, S, C]: written by the forward when non-null,
                                     read by the backward for grad_vertices; or NULL */
} NrAttributeArgs;
/* sizeof(NrAttributeArgs), for bindings to check their mirror of the struct */
NR_API size_t nr_attribute_args_size(void);
/* images [B, C, s, s] contiguous, fully written; args->internal too when non-null. */
NR_API int nr_attributes_forward(const NrAttributeArgs* args, float* images, void* stream);
/* Scratch bytes of nr_attributes_backward: the per-face-corner records [B, F, 3, 3 + C] (zero-filled by
 * the call). */
NR_API size_t nr_attributes_backward_workspace_bytes(int batch_size, int num_faces, int num_channels);
/* grad_images [B, C, s, s] contiguous -> grad_vertices [B, V, 3] and grad_attributes [Ba, Va, C] with
 * Ba = attr_batch_stride ? B : 1 (the item sum for a shared table).  Either may be NULL; each one given is
 * fully written.  grad_vertices needs args->internal (the forward's) and the vertex CSR: vertex_faces[
 * vertex_offsets[v] .. vertex_offsets[v + 1]) lists 3 f + k for every faces[f, k] == v; grad_attributes
 * needs the same lists of faces_attributes over the Va rows (attr_offsets [Va + 1], attr_faces [3 F]).
 * A missing or short workspace is NR_ERR_WORKSPACE. */
NR_API int nr_attributes_backward(const NrAttributeArgs* args, const float* grad_images, float* grad_vertices,
                                  float* grad_attributes, const int32_t* vertex_offsets, const int32_t* vertex_faces,
                                  const int32_t* attr_offsets, const int32_t* attr_faces, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* Point losses (point_loss.py; no reference counterpart): nearest neighbours and the chamfer distance
 * between two point sets, and area-weighted surface sampling of a mesh.
 *
 * Chamfer: x [B, N, 3] contiguous, y [B, M, 3] with the item stride y_batch_stride in elements (0: one
 * [M, 3] set shared by every item), directions = NR_CHAMFER_X_TO_Y | NR_CHAMFER_Y_TO_X.  The squared
 * distance is fma(dz, dz, fma(dy, dy, dx dx)) of the float32 coordinate differences (never the
 * |x|^2 + |y|^2 - 2 x.y expansion); the nearest neighbour is the lowest index among exact ties.
 *   index_xy [B, N]: nearest y of every x;   index_yx [B, M]: nearest x of every y
 *   loss_b = (1/N) sum_i |x_i - y_{index_xy[i]}|^2 + (1/M) sum_j |x_{index_yx[j]} - y_j|^2   (the requested terms)
 * Backward, the indices held constant:
 *   grad x_i = g_b [(2/N) (x_i - y_{index_xy[i]}) + (2/M) sum_{j: index_yx[j] = i} (x_i - y_j)],
 *   grad y_j the same with the roles exchanged.
 * No float atomics, every sum in one fixed order: bitwise reproducible.  The gathered sum of a point scans
 * the other set's index array: eight equal ranges, each in ascending order, added in range order.
 * Checked before any launch (NR_ERR_ARGS, also for a missing or short workspace): N, M >= 1, B <= 65535,
 * B * max(N, M) <= INT_MAX - 4096, directions in 1..3, non-null pointers of what the directions need.  With B == 0
 * nothing is launched. */
enum { NR_CHAMFER_X_TO_Y = 1, NR_CHAMFER_Y_TO_X = 2 };
/* Scratch bytes of nr_chamfer_forward (the per-point minima and, where the targets are split over several
 * blocks, their partial (d2, j) pairs); 0 when a size is not positive. */
NR_API size_t nr_chamfer_workspace_bytes(int batch_size, int num_x, int num_y, int directions);
/* Writes the index array of every requested direction; dist2_xy [B, N] / dist2_yx [B, M] (the per-point
 * squared distances) and loss [B] when non-null (one of them must be). */
NR_API int nr_chamfer_forward(const float* x, const float* y, long long y_batch_stride, int batch_size, int num_x,
                              int num_y, int directions, int32_t* index_xy, int32_t* index_yx, float* dist2_xy,
                              float* dist2_yx, float* loss, void* workspace, size_t workspace_bytes, void* stream);
/* grad_loss [B] -> grad_x [B, N, 3], grad_y [B, M, 3] (dense, also for a shared y); either may be NULL, each
 * one given is fully written.  The index arrays are the forward's (trusted: every entry inside the other set). */
NR_API int nr_chamfer_backward(const float* x, const float* y, long long y_batch_stride, const int32_t* index_xy,
                               const int32_t* index_yx, const float* grad_loss, int batch_size, int num_x, int num_y,
                               int directions, float* grad_x, float* grad_y, void* stream);
/* Surface sampling: vertices [B, V, 3], faces [F, 3] (trusted: below V), u [B, S, 3] in [0, 1).  Per item,
 * a_f = |(v1 - v0) x (v2 - v0)| / 2, c_f = the float32 inclusive prefix sum of a up to the latest face of
 * positive area at or before f; sample s takes the smallest f with c_f > u_s0 c_{F-1} (if rounding leaves
 * none: the last face of positive area), so a face of zero area is never taken; an item whose total area
 * is 0 takes face F - 1.  weights = (1 - r, r (1 - u_s2), r u_s2) with r = sqrt(u_s1); point = the weighted
 * sum of the face's corners.  Outputs points [B, S, 3], face [B, S], weights [B, S, 3], all fully written.
 * Backward: grad_vertices [B, V, 3] (zero-filled by the call) += weights * grad_points at the corners,
 * with float atomics (agrees from run to run up to the order of float additions).
 * Checked before any launch (NR_ERR_ARGS, also for a missing or short workspace): S, F, V >= 1, B * S,
 * B * F and 3 B V <= INT_MAX, non-null pointers. */
NR_API size_t nr_sample_points_workspace_bytes(int batch_size, int num_faces);
NR_API int nr_sample_points_forward(const float* vertices, const int32_t* faces, const float* u, int batch_size,
                                    int num_vertices, int num_faces, int num_samples, float* points, int32_t* face,
                                    float* weights, void* workspace, size_t workspace_bytes, void* stream);
NR_API int nr_sample_points_backward(const int32_t* faces, const int32_t* face, const float* weights,
                                     const float* grad_points, int batch_size, int num_vertices, int num_faces,
                                     int num_samples, float* grad_vertices, void* stream);

/* Point-to-surface distance (point_loss.py point_mesh_distance / closest_points_on_mesh; no reference
 * counterpart): points [B, N, 3] with the item stride points_batch_stride in elements (0: one [N, 3] set
 * shared by every item), vertices [B, V, 3] contiguous, faces [F, 3] (trusted: below V).  With T_f the
 * triangle f as a closed set:
 *   face[b, i]    = argmin_f dist^2(p_i, T_f), the lowest f among exact float32 ties
 *   weights[b, i] = the barycentric weights of the closest point of that face over its three corners:
 *                   c_i = w_0 v[faces[f, 0]] + w_1 v[faces[f, 1]] + w_2 v[faces[f, 2]]
 *   dist2[b, i]   = |p_i - c_i|^2, the sum of the squared coordinate differences to that closest point
 *   loss_b        = (1/N) sum_i dist2[b, i]   (one fixed order)
 * The face is chosen by a float32 distance (the least of the distances to the three edges and, where the
 * projection falls inside, to the plane); the closest point on the chosen face is then formed in float64
 * from the float32 inputs, and its weights and squared distance are rounded to float32 once.  Every weight is finite, in [0, 1], and the three
 * sum to 1 within 1e-6.
 * A degenerate face (a repeated index, or a float32 cross product (b - a) x (c - a) of exactly zero:
 * coincident or exactly collinear corners) is the segment between its two most distant corners (the first
 * of the edges ab, ac, bc among equally long ones), a point when all three coincide (weights 1, 0, 0); the
 * weight of the unused corner is 0.  Near-degenerate faces get no special promise.
 * Backward, face and weights held constant (by the envelope theorem the exact gradient of the squared
 * distance wherever the closest face is unique):
 *   grad p_i = g_b (2/N) (p_i - c_i)
 *   grad v_j = -g_b (2/N) sum over (i, k) with faces[face_i, k] == j of w_ik (p_i - c_i)
 * dist2, face, weights, loss and grad_points are bitwise reproducible (no float atomics, every sum in one
 * fixed order, the same whether or not the faces were split over several blocks); grad_vertices is
 * scattered with float atomics and agrees from run to run up to the order of float additions.
 * Checked before any launch (NR_ERR_ARGS, also for a missing or short workspace): N, F, V >= 1,
 * B <= 65535, B * N <= INT_MAX - 4096, B * F and 3 B V <= INT_MAX, non-null inputs.  With B == 0 nothing is
 * launched.  The saved face indices are inside [0, F) whatever the coordinates hold (NaN included). */
NR_API size_t nr_point_mesh_workspace_bytes(int batch_size, int num_points, int num_faces);
/* dist2 [B, N], face [B, N], weights [B, N, 3], loss [B]: each may be NULL (not all four); each one given
 * is fully written. */
NR_API int nr_point_mesh_forward(const float* points, long long points_batch_stride, const float* vertices,
                                 const int32_t* faces, int batch_size, int num_points, int num_vertices,
                                 int num_faces, float* dist2, int32_t* face, float* weights, float* loss,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* grad_loss [B] -> grad_points [B, N, 3] (dense, also for shared points), grad_vertices [B, V, 3]
 * (zero-filled by the call); either may be NULL.  face and weights are the forward's (trusted). */
NR_API int nr_point_mesh_backward(const float* points, long long points_batch_stride, const float* vertices,
                                  const int32_t* faces, const int32_t* face, const float* weights,
                                  const float* grad_loss, int batch_size, int num_points, int num_vertices,
                                  int num_faces, float* grad_points, float* grad_vertices, void* stream);

/* Face-to-scan distance (point_loss.py mesh_point_distance / closest_points_to_faces; no reference
 * counterpart): the opposite direction of the point-to-surface distance above, with the same arguments:
 * points [B, N, 3] with the item stride points_batch_stride in elements (0: one [N, 3] set shared by every
 * item, read in place), vertices [B, V, 3] contiguous, faces [F, 3] (trusted: below V).  With T_f the
 * triangle f as a closed set:
 *   point[b, f]   = argmin_i dist^2(p_i, T_f), the lowest i among exact float32 ties
 *   weights[b, f] = the barycentric weights of the closest point c_f of T_f to p_point[b, f]
 *   dist2[b, f]   = |p_point[b, f] - c_f|^2
 *   loss_b        = (1/F) sum_f dist2[b, f]   (one fixed order)
 * Every face counts.  The point is chosen by the float32 pair distance of the point-to-surface loop (the
 * same operations in the same order); the closest point on the face is then formed in float64 from the
 * float32 inputs, and its weights and squared distance are rounded to float32 once.  Degenerate faces follow
 * the rules stated above (a segment between the two most distant corners, or a point).
 * Backward, point and weights held constant:
 *   grad v_j = -g_b (2/F) sum over (f, k) with faces[f, k] == j of w_fk (p_point(f) - c_f)
 *   grad p_i =  g_b (2/F) sum over f with point(f) == i of (p_i - c_f)
 * corner_offsets [V + 1] and corner_index [3 F] are the CSR lists vertex -> its corners 3 f + k, ascending
 * (trusted); grad_vertices is gathered over them in that order without atomics.  dist2, point, weights,
 * loss and grad_vertices are bitwise reproducible (every sum in one fixed order, the same whether or not the
 * points were split over several blocks); grad_points is scattered with float atomics (many faces share a
 * nearest point) and agrees from run to run up to the order of float additions.
 * Checked before any launch (NR_ERR_ARGS, also for a missing or short workspace): N, F, V >= 1,
 * B <= 65535, B * F <= INT_MAX - 4096, B * N and 3 B V <= INT_MAX, a non-negative stride, non-null inputs, at
 * least one output.  With B == 0 nothing is launched (the sizes are checked first: B == 0 with N, F or V
 * below 1 is still NR_ERR_ARGS, as in the point-to-surface calls).  The saved point indices are inside [0, N)
 * whatever the coordinates hold (NaN included). */
NR_API size_t nr_face_point_workspace_bytes(int batch_size, int num_points, int num_faces);
/* dist2 [B, F], point [B, F], weights [B, F, 3], loss [B]: each may be NULL (not all four); each one given
 * is fully written. */
NR_API int nr_face_point_forward(const float* points, long long points_batch_stride, const float* vertices,
                                 const int32_t* faces, int batch_size, int num_points, int num_vertices,
                                 int num_faces, float* dist2, int32_t* point, float* weights, float* loss,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* grad_loss [B] -> grad_points [B, N, 3] (dense, also for shared points; zero-filled by the call),
 * grad_vertices [B, V, 3] (fully written, zeros for a vertex without a face); either may be NULL (the CSR
 * lists are needed for grad_vertices only).  point and weights are the forward's (trusted). */
NR_API int nr_face_point_backward(const float* points, long long points_batch_stride, const float* vertices,
                                  const int32_t* faces, const int32_t* corner_offsets, const int32_t* corner_index,
                                  const int32_t* point, const float* weights, const float* grad_loss,
                                  int batch_size, int num_points, int num_vertices, int num_faces,
                                  float* grad_points, float* grad_vertices, void* stream);

/* Rigid registration (rigid.py; no reference counterpart): the closed-form weighted similarity between
 * corresponding points, and point-to-point ICP built on it.
 *
 * rigid_align: x [B, N, 3] contiguous, y [B, N, 3] at the item stride y_batch_stride in elements (0: one
 * [N, 3] set shared by every item), weights w [B, N] at the item stride w_batch_stride (0: shared), non-negative
 * and used as given, or NULL: the weight 1.  Minimises sum_i w_i |s R x_i + t - y_i|^2 over proper rotations R
 * (det +1, never a reflection), t, and s when `scale` is set (else s = 1):
 *   W    = sum w,   xbar = sum w x / W,   ybar = sum w y / W
 *   A    = sum w (y - ybar) (x - xbar)^T                 (3 x 3, row-major)
 *   var  = sum w |x - xbar|^2
 *   R    = argmax tr(R^T A)                              (Horn's quaternion method, nr_arap.h's Jacobi sweeps)
 *   s    = tr(R^T A) / var   with scale,  1 without
 *   t    = ybar - s R xbar
 *   condition = (s2 + d s3) / s1 of A's singular values s1 >= s2 >= s3, d = sign det A: (l1 - l2) / (l1 + l2) of
 *          the two largest eigenvalues of Horn's 4 x 4 matrix.  Near 0 the rotation is not determined.
 * Corner cases, all finite: W == 0 gives R = I, t = 0, s = 1, condition = 0;  A == 0 (N = 1, coincident points)
 * gives R = I and condition = 0;  var == 0 gives s = 1;  where the maximiser is not unique (collinear points,
 * N = 2) any maximiser is returned, orthonormal with det +1.
 * The sums are never raw second moments: the centroids are summed relative to the item's first pair, and A and
 * var from centred points, so a cloud far from the origin loses nothing.
 * Backward, from the gradients gR [B, 9], gt [B, 3], gs [B] of the outputs (any may be NULL: zero), closed form:
 *   through t:  g_ybar = gt,  g_xbar = -s R^T gt,  G = gR - s gt xbar^T,  g_s = gs - gt . (R xbar)
 *   through s:  g_tau = g_s / var,  g_var = -g_s s / var            (scale set and var > 0; else both 0)
 *   through R:  P = R^T A (symmetric), K = tr(P) I - P, a perturbation dA turns R by dR = R [omega]x with
 *               K omega = axial(R^T dA - dA^T R); so with m = axial(R^T G - G^T R) and u = K^{-1} m (adjugate),
 *               gA = g_tau R + R [u]x.  K's smallest eigenvalue is s2 + d s3: where condition <=
 *               NR_RIGID_MIN_CONDITION the rotation passes no gradient (u = 0).
 *   grad x_n = w_n (gA^T (y_n - ybar) + 2 g_var (x_n - xbar) + g_xbar / W)
 *   grad y_n = w_n (gA (x_n - xbar) + g_ybar / W)                   (the centring terms cancel)
 * The weights take no gradient.  No float atomics, every sum in one fixed order: all outputs and gradients are
 * bitwise reproducible, and an item's results do not depend on its batch.
 *
 * icp: x [B, N, 3] onto y [B, M, 3] (item stride y_batch_stride, 0: shared), exactly `iterations` updates, no
 * early exit and nothing read back by the host.  `transform` [B, 13] = (R [9] row-major, t [3], s) per item is
 * the start on entry and the result on return.  Pass k = 0 .. iterations - 1: index_i = the nearest y of
 * s R x_i + t (fma(dz, dz, fma(dy, dy, dx dx)), the lowest index among exact ties), dist2_i its squared distance;
 * w_i = 1, or 0 where dist2_i > max_distance^2 (max_distance < 0: no rejection); then (R, t, s) =
 * rigid_align(x, y[index], w) of the original x -- left as it was when no pair is kept.  A last pass writes index
 * and dist2 under the returned transform.  rmse [B, iterations + 1]: entry k = sqrt(sum w dist2 / sum w) of pass k,
 * 0 when no pair is kept.
 *
 * Checked before any launch (NR_ERR_ARGS; NR_ERR_WORKSPACE for a missing or short workspace): N, M >= 1,
 * iterations >= 0, B <= 65535, B * max(N, M) <= INT_MAX - 4096, item strides 0 or the item's size, non-null
 * pointers.  With B == 0 nothing is launched. */
#define NR_RIGID_MIN_CONDITION 1e-6f
enum { NR_RIGID_RECORD_FLOATS = 32, NR_RIGID_TRANSFORM_FLOATS = 13 };
/* Scratch bytes of nr_rigid_align_forward and _backward (the per-chunk partial sums of 1024 points; the backward
 * uses the first 64 B bytes); no zero fill needed; 0 when a size is not positive. */
NR_API size_t nr_rigid_workspace_bytes(int batch_size, int num_points);
/* R [B, 9], t [B, 3], s [B], condition [B], record [B, NR_RIGID_RECORD_FLOATS] (what the backward reads), all
 * fully written; condition and record may be NULL. */
NR_API int nr_rigid_align_forward(const float* x, const float* y, long long y_batch_stride, const float* w,
                                  long long w_batch_stride, int batch_size, int num_points, int scale, float* R,
                                  float* t, float* s, float* condition, float* record, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* grad_x [B, N, 3], grad_y [B, N, 3] (dense, also for a shared y); either may be NULL, each one given is fully
 * written.  x, y, w and scale are the forward's. */
NR_API int nr_rigid_align_backward(const float* x, const float* y, long long y_batch_stride, const float* w,
                                   long long w_batch_stride, const float* record, const float* grad_R,
                                   const float* grad_t, const float* grad_s, int batch_size, int num_points, int scale,
                                   float* grad_x, float* grad_y, void* workspace, size_t workspace_bytes,
                                   void* stream);
/* Scratch bytes of nr_icp (the partial sums, and where the targets are split over several blocks their partial
 * (d2, j) pairs); no zero fill needed; 0 when a size is not positive. */
NR_API size_t nr_icp_workspace_bytes(int batch_size, int num_x, int num_y);
/* transform [B, 13] in and out; rmse [B, iterations + 1], index [B, N], dist2 [B, N] fully written. */
NR_API int nr_icp(const float* x, const float* y, long long y_batch_stride, int batch_size, int num_x, int num_y,
                  int iterations, int scale, float max_distance, float* transform, float* rmse, int32_t* index,
                  float* dist2, void* workspace, size_t workspace_bytes, void* stream);

/* Diagnostics (no reference counterpart): the kernels replace some IEEE divisions by a shortened
 * form of the compiler's own division sequence inside a guarded operand range (DESIGN.md,
 * "Numerics").  This runs both forms on n operand pairs so tests can check they agree bit for bit. */
NR_API int nr_selftest_division(const float* a, const float* b, float* q_fast, float* q_ieee, long long n,
                                void* stream);

/* Measurement hook (bench.py's roofline leg; no reference counterpart).  With profiling on, the
 * library brackets each launch of its kernels with a pair of HIP events recorded on the launch
 * stream; nr_profile_read gives the mean duration in ms of the launches of `kernel` ("k_face_setup",
 * "k_raster_fwd", "k_shade", "k_raster_bwd", "k_vertex_grad", "k_tex_out", "k_tex_pack") recorded
 * since profiling was last enabled (up to the last 64), once the stream has been synchronised;
 * nr_profile_enable(1) while on starts a new measurement.  Process-wide state, meant for a single
 * measuring thread. */
NR_API int nr_profile_enable(int on);
NR_API int nr_profile_read(const char* kernel, float* ms);

/* Launch record (no reference counterpart; the tests use it to assert which kernel variant ran).
 * For the most recent launch of `kernel` ("k_raster_fwd", "k_raster_bwd", or "k_chamfer_nn" / "k_point_face_nn" / "k_face_point_nn" / "k_icp_nn": 256 threads) in this process
 * (process-wide, like the profiling hook; torch issues a backward from its autograd thread): block_threads = threads per block (k_raster_fwd: 256 = four 16x16 quadrants per
 * 32x32 bin, 1024 = one wave per 8x8 block; k_raster_bwd: 256 = 2 pixels per lane, 512 = 1 pixel
 * per lane) and flags = NR_LAUNCH_* bits.  NR_ERR_ARGS when none was recorded. */
enum { NR_LAUNCH_FUSED_SHADE = 1, NR_LAUNCH_STATIC_CHANNELS = 2, NR_LAUNCH_TWO_PX_PER_LANE = 4,
       NR_LAUNCH_DEEP_FIRST = 8 /* k_raster_fwd: bins dispatched deepest first (k_bin_order) */,
       NR_LAUNCH_SPLIT = 16 /* k_raster_fwd: deep bins at 1024 threads, the rest at 256 on a side stream */,
       NR_LAUNCH_HOT_WINDOWS = 32 /* k_raster_bwd: shared texture windows into private copies (face_hot) */,
       NR_LAUNCH_DEALT_QUARTERS = 64 /* k_raster_fwd: deep bins' 4x4 quarters dealt to the waves (not split) */,
       NR_LAUNCH_QUADRANTS = 128 /* k_raster_fwd: deep bins walked by four blocks, one per 16x16 quadrant (not split) */,
       /* k_raster_bwd: the feature instantiation (none of the three: the plain path) */
       NR_LAUNCH_LIGHTS = 256, NR_LAUNCH_BACKGROUNDS = 512, NR_LAUNCH_SIL_ONLY = 1024,
       /* k_chamfer_nn: the direction's targets were split over several blocks and combined */
       NR_LAUNCH_SPLIT_X_TO_Y = 2048, NR_LAUNCH_SPLIT_Y_TO_X = 4096,
       /* k_point_face_nn: the faces were split over several blocks and combined */
       NR_LAUNCH_SPLIT_FACES = 8192,
       /* k_face_point_nn: the points were split over several blocks and combined */
       NR_LAUNCH_SPLIT_POINTS = 16384,
       /* k_icp_nn: the targets were split over several blocks and combined */
       NR_LAUNCH_SPLIT_TARGETS = 32768 };
NR_API int nr_last_launch(const char* kernel, int* block_threads, int* flags);

/* Dispatch order of a raster launch's tiles (no reference counterpart; host only, for tests and the
 * timing tools).  With the items interleaved in groups (a batch that is a multiple of 8) the raster
 * kernels hand out an item's nx x ny tiles of tile_w x tile_h pixels nearest the raster centre first:
 * sorted by (dx^2 + dy^2, ty, tx) with dx = (2 tx + 1 - nx) tile_w and dy = (2 ty + 1 - ny) tile_h,
 * in integers.  out[t] = tx | ty << 8 of rank t, nx * ny entries (k_raster_fwd: 32 x 32 bins;
 * k_raster_bwd: 32 x 16 tiles).  NR_ERR_ARGS above 1024 tiles or 256 tiles a side: such a raster keeps
 * the arithmetic order, rows from the middle row outwards and each row from its middle outwards. */
NR_API int nr_tile_order(int nx, int ny, int tile_w, int tile_h, uint16_t* out);

#ifdef NR_COUNT_TESTS
/* Face-test counters, in the diagnostic build compiled with -DNR_COUNT_TESTS only
 * (_lib/libnr_raster_count.so, bench.py's face-test rate; SURVEY 8d's secondary bound, the reference's
 * brute force doing B*S^2*F tests per call, rasterize_cuda_kernel.cu:82-149).  Since the last reset,
 * out[0] = (pixel, face) pass tests the forward's walks evaluated (64 per face a wave walks over an 8x8
 * block, 16 over a 4x4 quarter), out[1] = faces walked (wave level), out[2] = deferred commit batches
 * (the division chain, run by a whole wave), out[3] = walks (8x8 blocks or quarters walked).  reset != 0
 * zeroes them after the read (device-wide counters: call with the device idle). */
NR_API int nr_count_read(unsigned long long* out4, int reset);
#endif

#ifdef __cplusplus
}
#endif
#endif /* NR_RASTER_H_ */

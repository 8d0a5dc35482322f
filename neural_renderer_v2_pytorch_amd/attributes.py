"""Per-vertex attribute rendering: any per-vertex tensor [B, V, C] -- vertex colours, normals, positions,
part labels, learned features -- drawn as an image [B, C, s, s], with gradients to the attributes and,
through the reference's soft rasterization gradient, to the vertices.

The definition is rasterize_core (reference rasterize.py:227-329) with one new map in place of rgb_map.
At the internal size S (2 s with anti-aliasing, else s), for a foreground pixel of face f with the weights
w_k of compute_weight_map (no gradient, as in the reference), corner depths z_k and corner attributes
a_kc = attributes[b, faces_attributes[f, k], c]:

  perspective_correct=False:  out_c = sum_k w_k a_kc                          (the normal map's form, rasterize.py:185-187)
  perspective_correct=True:   q_k = w_k / (z_k + 1e-10),  Dn = sum_k (q_k + 1e-10),
                              out_c = (sum_k q_k a_kc) / Dn                   (the uv interpolation, rasterize.py:113-119)

No clamp; background pixels are 0.  Then images = differentiation(attribute_map, coordinate_map) (identity
forward; backward the upstream gradient to the attribute map and the neighbour-difference estimate of
differentiation.py:12-36 to the coordinate map), permuted to [B, C, S, S], flipped along both image axes
and, with anti-aliasing, averaged over 2x2.

A channel of ones renders the silhouette: the linear mode gives sum_k w_k, which is 1 up to rounding, so an
alpha channel that carries the renderer's own edge gradients needs no extra flag -- append a column of
ones to the attributes and pass perspective_correct=False.

rasterize_attributes is the fused path (HIP: nr_attributes_forward / nr_attributes_backward after a
silhouette-only nr_rasterize_forward, include/nr_raster.h); rasterize_attributes_torch the same composition
from the Level-1 bindings and torch ops (the baseline of tools/bench_attributes.py);
attributes_from_maps_torch the interpolation alone as torch ops on any device and dtype (the reference of
the tests)."""
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .topology import faces_i32, vertex_adjacency
from .rasterize_param import RasterizeHyperparam

NR_ATTR_MAX_CHANNELS = _lib.NR_ATTR_MAX_CHANNELS


# ---- the torch composition ----
def _gather_faces(data, face_index_map):
    """data [B or 1, F, ...] -> [B, S, S, ...]: the visible face's entry per pixel, 0 on the background."""
    B, S = face_index_map.shape[0], face_index_map.shape[1]
    fg = face_index_map >= 0
    idx = face_index_map.clamp(min=0).long().reshape(B, -1)
    if data.shape[0] != B:
        data = data.expand((B,) + tuple(data.shape[1:]))
    rows = torch.arange(B, device=idx.device)[:, None].expand_as(idx)
    out = data[rows, idx].reshape((B, S, S) + tuple(data.shape[2:]))
    mask = fg.reshape((B, S, S) + (1,) * (data.ndim - 2))
    return torch.where(mask, out, torch.zeros((), dtype=out.dtype, device=out.device))


def attributes_from_maps_torch(face_index_map, weight_map, faces_v, faces_a, perspective_correct=True):
    """The interpolation as plain torch ops: face_index_map [B, S, S] (int, -1 = background), weight_map
    [B, S, S, 3], faces_v [B, F, 3, 3] (screen x, y, depth per corner), faces_a [B or 1, F, 3, C] ->
    [B, S, S, C].  Any device and dtype; differentiates to faces_a and faces_v (only the depths enter, in
    the perspective-correct mode; the weights are constants)."""
    a = _gather_faces(faces_a, face_index_map)                        # [B, S, S, 3, C]
    w = weight_map
    if perspective_correct:
        z = _gather_faces(faces_v[:, :, :, 2], face_index_map)        # [B, S, S, 3]
        q = w / (z + 1e-10)
        dn = (q + 1e-10).sum(-1)
        out = (q[..., None] * a).sum(-2) / dn[..., None]
    else:
        out = (w[..., None] * a).sum(-2)
    fg = (face_index_map >= 0)[..., None]
    return torch.where(fg, out, torch.zeros((), dtype=out.dtype, device=out.device))


def _flip_pool(images, anti_aliasing):
    """[B, S, S, C] -> [B, C, s, s]: rasterize.py:315-328."""
    images = torch.flip(images.permute((0, 3, 1, 2)), dims=(2, 3))
    if anti_aliasing:
        images = (images[:, :, 0::2, 0::2] + images[:, :, 1::2, 0::2] + images[:, :, 0::2, 1::2] +
                  images[:, :, 1::2, 1::2]) / 4.
    return images


class _Call:
    """The checked arguments of one call."""
    __slots__ = ("vertices", "attributes", "faces", "faces_attributes", "B", "V", "F", "Va", "C", "shared", "s", "S",
                 "aa", "backside", "near", "far", "pc")


def _prepare(vertices, faces, attributes, hyperparams, faces_attributes, perspective_correct):
    if not torch.is_tensor(vertices) or vertices.ndim != 3 or vertices.shape[2] != 3:
        raise ValueError("vertices must be a [B, V, 3] tensor")
    if not torch.is_tensor(attributes) or attributes.ndim not in (2, 3):
        raise ValueError("attributes must be a [B, Va, C], [1, Va, C] or [Va, C] tensor")
    c = _Call()
    c.B, c.V = vertices.shape[0], vertices.shape[1]
    c.Va, c.C = attributes.shape[-2], attributes.shape[-1]
    if not 1 <= c.C <= NR_ATTR_MAX_CHANNELS:
        raise ValueError("attributes have %d channels; 1 to %d are supported" % (c.C, NR_ATTR_MAX_CHANNELS))
    if attributes.ndim == 3 and attributes.shape[0] not in (1, c.B):
        raise ValueError("attributes batch must be 1 or %d, got %d" % (c.B, attributes.shape[0]))
    hp = hyperparams if hyperparams is not None else RasterizeHyperparam()
    c.s = int(hp.image_size)
    c.aa = bool(hp.anti_aliasing)
    c.S = c.s * (2 if c.aa else 1)
    c.backside = bool(hp.draw_backside)
    c.near, c.far = float(hp.near), float(hp.far)
    c.pc = bool(perspective_correct)
    dev = vertices.device
    c.faces = faces_i32(faces, dev, c.V, "faces")
    c.F = c.faces.shape[0]
    if faces_attributes is None:
        c.faces_attributes = c.faces if c.Va == c.V else faces_i32(faces, dev, c.Va, "faces (as faces_attributes)")
    else:
        c.faces_attributes = faces_i32(faces_attributes, dev, c.Va, "faces_attributes")
        if c.faces_attributes.shape[0] != c.F:
            raise ValueError("faces_attributes must have one row per face (%d), got %d" % (c.F, c.faces_attributes.shape[0]))
    _lib.require_gpu(vertices, attributes)
    if attributes.device != dev:
        raise ValueError("attributes must be on the vertices' device")
    v = vertices if (vertices.dtype == torch.float32 and vertices.is_contiguous()) else vertices.float().contiguous()
    at = attributes if attributes.dtype == torch.float32 else attributes.float()
    # a table shared by the batch ([Va, C], [1, Va, C] or a batch-expanded view) is read at stride 0 and never
    # expanded; the Function gets its one item, so autograd returns the gradient once, summed over the items
    if at.ndim == 3 and at.shape[0] > 1 and at.stride(0) == 0 and at.requires_grad and at.grad_fn is None:
        at = at.contiguous()  # an expanded view that is itself the leaf takes one gradient per item
    c.shared = at.ndim == 2 or at.shape[0] == 1 or at.stride(0) == 0
    if c.shared and at.ndim == 3 and at.shape[0] != 1:
        at = at[:1]
    if not at.is_contiguous():
        at = at.contiguous()
    c.vertices, c.attributes = v, at
    return c


class RasterizeAttributes(torch.autograd.Function):
    """vertices [B, V, 3], attributes [B, Va, C] or the one item of a shared table -> images [B, C, s, s].
    Saves the face-index map and the face records, and the internal image [B, S, S, C] only when the
    vertices take a gradient (ctx.internal_bytes: its size, 0 when it was not kept)."""

    @staticmethod
    def forward(ctx, vertices, attributes, call):
        c = call
        dev = vertices.device
        L = _lib.lib()
        images = torch.empty((c.B, c.C, c.s, c.s), dtype=torch.float32, device=dev)
        ctx.call = c
        ctx.attr_shape = attributes.shape
        ctx.internal_bytes = 0
        ctx.state = None
        if c.B == 0:
            return images
        want_v, want_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        fim = torch.empty((c.B, c.S, c.S), dtype=torch.int32, device=dev)
        frec = torch.empty((c.B, max(c.F, 1), 16), dtype=torch.float32, device=dev)
        sil = torch.empty((c.B, 1, c.s, c.s), dtype=torch.float32, device=dev)
        ws = torch.empty(max(L.nr_workspace_bytes(c.B, c.F, c.S), 256), dtype=torch.uint8, device=dev)
        r = _lib.NrRasterArgs()
        r.batch_size, r.num_vertices, r.num_faces, r.image_size = c.B, c.V, c.F, c.s
        r.anti_aliasing, r.draw_backside, r.draw_flags = int(c.aa), int(c.backside), _lib.NR_DRAW_SILHOUETTES
        r.near, r.far, r.eps, r.depth_min_delta = c.near, c.far, 1e-5, 1e-4
        r.vertices, r.faces = vertices.data_ptr(), c.faces.data_ptr()
        r.face_records, r.face_index = frec.data_ptr(), fim.data_ptr()
        r.workspace, r.workspace_bytes = ws.data_ptr(), ws.numel()
        r.face_index_sparse = 0
        internal = torch.empty((c.B, c.S, c.S, c.C), dtype=torch.float32, device=dev) if want_v else None
        a = _lib.NrAttributeArgs()
        a.batch_size, a.num_faces, a.num_vertices, a.num_attributes, a.num_channels = c.B, c.F, c.V, c.Va, c.C
        a.image_size, a.anti_aliasing, a.perspective_correct = c.s, int(c.aa), int(c.pc)
        a.face_index, a.face_records = fim.data_ptr(), frec.data_ptr()
        a.faces, a.faces_attributes = c.faces.data_ptr(), c.faces_attributes.data_ptr()
        a.attributes = attributes.data_ptr()
        a.attr_batch_stride = 0 if c.shared else c.Va * c.C
        a.internal = internal.data_ptr() if internal is not None else None
        stream = _lib.stream_of(vertices)
        with _lib.on_device(dev):
            _lib.check(L.nr_rasterize_forward(r, sil.data_ptr(), stream), "nr_rasterize_forward")
            _lib.check(L.nr_attributes_forward(a, images.data_ptr(), stream), "nr_attributes_forward")
        if want_v or want_a:
            # the CSR lists of the backward's second level, built once per index tensor (a host copy on the
            # first sight of a tensor; cached, so steady-state steps never synchronise)
            vadj = vertex_adjacency(c.faces, c.V) if want_v else None
            aadj = vertex_adjacency(c.faces_attributes, c.Va) if want_a else None
            ctx.save_for_backward(attributes)  # read again by the perspective-correct depth gradient
            ctx.state = (a, fim, frec, internal, vadj, aadj)
            ctx.internal_bytes = internal.numel() * 4 if internal is not None else 0
            ctx.face_index_map = fim  # [B, S, S] int32, kept for the backward anyway (the tests read it)
        return images

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_images):
        c = ctx.call
        want_v, want_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if grad_images is None or not (want_v or want_a):
            return None, None, None
        dev = grad_images.device
        gv = torch.empty((c.B, c.V, 3), dtype=torch.float32, device=dev) if want_v else None
        ga = torch.empty(tuple(ctx.attr_shape), dtype=torch.float32, device=dev) if want_a else None
        if c.B == 0:
            if ga is not None:
                ga.zero_()
            return gv, ga, None
        a, fim, frec, internal, vadj, aadj = ctx.state
        L = _lib.lib()
        g = grad_images.to(torch.float32).contiguous()
        nbytes = L.nr_attributes_backward_workspace_bytes(c.B, c.F, c.C)
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.nr_attributes_backward(a, g.data_ptr(), _lib.ptr(gv), _lib.ptr(ga),
                                                _lib.ptr(vadj[0]) if vadj else None, _lib.ptr(vadj[1]) if vadj else None,
                                                _lib.ptr(aadj[0]) if aadj else None, _lib.ptr(aadj[1]) if aadj else None,
                                                ws.data_ptr(), ws.numel(), _lib.stream_of(g)), "nr_attributes_backward")
        return gv, ga, None


def rasterize_attributes(vertices, faces, attributes, hyperparams=None, faces_attributes=None, perspective_correct=True):
    """Render per-vertex attributes: [B, C, s, s] float32 (the module docstring has the definition).

    vertices   [B, V, 3] float32 on the GPU, in screen space, as rasterize_* takes them
    faces      [F, 3] vertex indices
    attributes [B, Va, C], or shared by the batch as [1, Va, C], [Va, C] or a batch-expanded view: a shared
               table is read at stride 0, never expanded in memory, and its gradient is the sum over the batch.
               1 <= C <= NR_ATTR_MAX_CHANNELS = 64 (a design limit of the kernels' run-time channel loop);
               ValueError outside it
    hyperparams a RasterizeHyperparam: image_size, near, far, anti_aliasing and draw_backside are read, the
               draw_* flags ignored; None = the defaults
    faces_attributes [F, 3] rows of the attribute table per face corner, default `faces` (then Va = V); given
               separately it indexes a table of its own length Va, as faces_textures indexes
               vertices_textures: face-varying data such as OBJ normals
    perspective_correct  the interpolation mode

    One autograd Function; no host synchronisation and no .cpu() in the steady state (the index checks and
    the backward's CSR lists are cached per index tensor), so a step can be captured in a HIP graph.  It
    keeps the face-index map and the face records for the backward, and the internal image [B, S, S, C] only
    when the vertices take a gradient: 4 B S^2 C bytes, 201 MB at B = 64, 256^2 with anti-aliasing, C = 3.
    Gradients by float atomics: equal from run to run up to the order of additions.  CPU tensors raise (no
    CPU fallback; rasterize_attributes_torch's pieces serve there)."""
    c = _prepare(vertices, faces, attributes, hyperparams, faces_attributes, perspective_correct)
    v, at = c.vertices, c.attributes
    c.vertices = c.attributes = None  # the Function keeps `c`: the index tensors, not the inputs
    return RasterizeAttributes.apply(v, at, c)


def rasterize_attributes_torch(vertices, faces, attributes, hyperparams=None, faces_attributes=None,
                               perspective_correct=True):
    """The same composition on the GPU from the Level-1 bindings (rasterize_cuda: face-index and weight
    maps), attributes_from_maps_torch, nr.differentiation, flip and pool: what the reference's rasterize_core
    would run with an attribute map in place of rgb_map.  Same arguments and result as rasterize_attributes."""
    from . import rasterize_cuda
    from .differentiation import differentiation
    c = _prepare(vertices, faces, attributes, hyperparams, faces_attributes, perspective_correct)
    v, at = c.vertices, c.attributes
    if at.ndim == 2:
        at = at[None]
    faces_v = v[:, c.faces.long()]                                    # [B, F, 3, 3]
    faces_a = at[:, c.faces_attributes.long()]                        # [B or 1, F, 3, C]
    fv = faces_v.detach().contiguous()
    fim = torch.empty(c.B * c.S * c.S, dtype=torch.int32, device=v.device)
    rasterize_cuda.face_index_map_forward_safe(fv, fim, c.F, c.S, c.near, c.far, int(c.backside), 1e-8, 1e-4)
    wm = torch.zeros((c.B * c.S * c.S, 3), dtype=torch.float32, device=v.device)
    rasterize_cuda.compute_weight_map_c(fv, fim, wm, c.F, c.S)
    fim = fim.reshape(c.B, c.S, c.S)
    wm = wm.reshape(c.B, c.S, c.S, 3)
    amap = attributes_from_maps_torch(fim, wm, faces_v, faces_a, c.pc)
    coord = (_gather_faces(faces_v[:, :, :, :2], fim) * wm[..., None]).sum(-2)
    return _flip_pool(differentiation(amap, coord), c.aa)

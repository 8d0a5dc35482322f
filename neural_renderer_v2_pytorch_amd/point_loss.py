"""3-D point supervision for the optimisation loop around the renderer: the chamfer distance between two
point sets, the nearest-neighbour query under it, area-weighted sampling of points on a mesh, and the
distance from a point set to the surface of a mesh and from the faces of a mesh to a point set.  Each is a
fused HIP launch sequence (nr_chamfer_* / nr_sample_points_* / nr_point_mesh_* / nr_face_point_*,
include/nr_raster.h) for float32 GPU tensors and a torch composition
(chamfer_distance_torch / nearest_points_torch / sample_points_torch / point_mesh_distance_torch /
closest_points_on_mesh_torch / mesh_point_distance_torch / closest_points_to_faces_torch) for every other
device and dtype.  The compositions are the tests' reference and the baseline of
tools/bench_point_loss.py.

Chamfer distance, for x [B, N, 3] and y [B, M, 3] (or one [M, 3] set shared by the items):

    loss_b = (1/N) sum_i min_j |x_i - y_j|^2  +  (1/M) sum_j min_i |x_i - y_j|^2

The squared distance is the float32 sum of the squared coordinate differences (never the
|x|^2 + |y|^2 - 2 x.y expansion, which loses the small distances that matter near convergence); the
nearest neighbour is the lowest index among exact ties.  The gradient treats the nearest index as a
constant: x_i takes g_b (2/N) (x_i - y_nn(i)) from its own term and g_b (2/M) sum_{j: nn(j) = i} (x_i - y_j)
from the points of y that chose it; y takes the symmetric pair.  The fused forward saves only the two
int32 index arrays; the backward reads x and y again.

Determinism: the fused chamfer path uses no float atomics.  The loss is a fixed-order sum of the
per-point minima, and the backward gathers the incoming terms of a point by scanning the other set's
saved index array, staged through LDS: eight equal ranges, one per wave, each walked in ascending order
and added in range order (one integer compare per pair; no inverse list is built).  Losses and gradients
are bitwise identical from run to run.  The sampling backward scatters to the vertices with float
atomics, as the attribute backward does: its vertex gradient agrees from run to run up to the order of
float additions.

Point-to-surface distance, for points p [B, N, 3] (or one [N, 3] set shared by the items), vertices
[B, V, 3] and faces [F, 3], with T_f the triangle f as a closed set:

    loss_b = (1/N) sum_i min_f dist^2(p_i, T_f)

The closest face is the lowest index among exact float32 ties; a degenerate face (a repeated index,
coincident or exactly collinear corners) is the segment between its two most distant corners, or a
point.  The fused forward chooses the face with a float32 distance, then forms the closest point on it
in float64 and saves the face and the barycentric weights; the gradient holds both constant, which by
the envelope theorem is the exact gradient of the squared distance wherever the closest face is unique.
Determinism: dist2, face, weights, the loss and the gradient of the points are bitwise reproducible from
run to run (no float atomics, fixed-order sums, the same whether or not the faces were split over several
blocks); the gradient of the vertices is scattered with float atomics and agrees up to the order of float
additions, like the sampling backward.

Face-to-scan distance, the opposite direction with the same inputs:

    loss_b = (1/F) sum_f min_i dist^2(p_i, T_f)

Every face counts; the nearest point is the lowest index among exact float32 ties of the same float32 pair
distance, and a degenerate face follows the same rule.  The fused forward (nr_face_point_*) chooses the point,
forms the face's closest point to it in float64 and saves the point and the weights; the gradient holds both
constant.  Determinism: dist2, point, weights, the loss and the gradient of the vertices (a gather over each
vertex's corners in ascending order, no atomics) are bitwise reproducible, the same whether or not the points
were split over several blocks; the gradient of the points is scattered with float atomics (many faces share a
nearest point) and agrees up to the order of float additions.

No call synchronises with the host in the steady state (a faces tensor is range-checked once and
cached, as everywhere else; the first mesh_point_distance forward that needs the vertex gradient also builds
the vertex -> corner lists of its faces tensor on the host, a device-to-host copy, and caches them), so a
step can be captured in a HIP graph once an eager step has run."""
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .mesh_loss import _finish
from .topology import faces_i32, vertex_adjacency

CHAMFER_TILE = _lib.NR_CHAMFER_TILE  # targets the nearest-neighbour kernel stages in LDS at a time
_DIRECTIONS = {"both": _lib.NR_CHAMFER_X_TO_Y | _lib.NR_CHAMFER_Y_TO_X, "x_to_y": _lib.NR_CHAMFER_X_TO_Y,
               "y_to_x": _lib.NR_CHAMFER_Y_TO_X}
_CHUNK_ELEMS = 1 << 24  # difference-tensor elements the compositions build at a time
_CHUNK_PAIRS = 1 << 20  # point-face pairs the point-mesh composition tests at a time (some twenty [pairs, 3] temporaries)
POINT_MESH_TILE, POINT_MESH_QBLOCK = _lib.NR_POINT_MESH_TILE, _lib.NR_POINT_MESH_QBLOCK  # faces per LDS tile, queries per block
FACE_POINT_TILE, FACE_POINT_FBLOCK = _lib.NR_FACE_POINT_TILE, _lib.NR_FACE_POINT_FBLOCK  # points per LDS tile, faces per block


def _directions(directions):
    if directions not in _DIRECTIONS:
        raise ValueError("directions must be 'both', 'x_to_y' or 'y_to_x', got %r" % (directions,))
    return _DIRECTIONS[directions]


def _prepare_sets(x, y):
    """x as [B, N, 3], y as [B, M, 3] or a shared [M, 3], and whether x was a single [N, 3] set."""
    for name, t in (("x", x), ("y", y)):
        if not torch.is_tensor(t) or t.ndim not in (2, 3) or t.shape[-1] != 3:
            raise ValueError("%s must be a [B, %s, 3] or [%s, 3] tensor" % (name, "NM"[name == "y"], "NM"[name == "y"]))
    single = x.ndim == 2
    if single:
        if y.ndim != 2:
            raise ValueError("a single [N, 3] x takes a single [M, 3] y, got y of shape %s" % (tuple(y.shape),))
        x = x[None]
    elif y.ndim == 3 and y.shape[0] != x.shape[0]:
        raise ValueError("batch sizes differ: x has %d items, y has %d" % (x.shape[0], y.shape[0]))
    if x.shape[1] == 0 or y.shape[-2] == 0:
        raise ValueError("empty point set: N = %d, M = %d (both must be at least 1)" % (x.shape[1], y.shape[-2]))
    return x, y, single


def _fused(*tensors):
    dev = tensors[0].device if torch.is_tensor(tensors[0]) else None
    return all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.device == dev for t in tensors)


# ---- the torch compositions: reference of the tests, baseline of tools/bench_point_loss.py ----
def _nearest_torch(x, y):
    """dist2 [B, N] and int64 index [B, N] of the nearest y of every x (x [B, N, 3], y [B, M, 3] or [M, 3]):
    the direct difference form and torch.min (the first of equal minima), chunked over N."""
    yb = y if y.ndim == 3 else y[None]
    B, N, M = x.shape[0], x.shape[1], yb.shape[1]
    step = max(1, _CHUNK_ELEMS // (3 * M * B))
    dist2, index = [], []
    for i in range(0, N, step):
        diff = x[:, i:i + step, None, :] - yb[:, None, :, :]
        d, j = (diff * diff).sum(-1).min(dim=2)
        dist2.append(d)
        index.append(j)
    return torch.cat(dist2, 1), torch.cat(index, 1)


def nearest_points_torch(x, y):
    """nearest_points as torch ops; any device and floating dtype (dist2 in that dtype)."""
    xb, y, single = _prepare_sets(x, y)
    with torch.no_grad():
        d, j = _nearest_torch(xb, y)
    j = j.to(torch.int32)
    return (d[0], j[0]) if single else (d, j)


def chamfer_distance_torch(x, y, directions="both", average=False):
    """The chamfer distance as torch ops: the nearest indices from the direct difference form (held
    constant), then a gather and a mean; any device and floating dtype."""
    dirs = _directions(directions)
    xb, y, single = _prepare_sets(x, y)
    B = xb.shape[0]
    yb = y if y.ndim == 3 else y[None].expand(B, -1, -1)
    loss = 0.
    if dirs & _lib.NR_CHAMFER_X_TO_Y:
        with torch.no_grad():
            j = _nearest_torch(xb, yb)[1]
        d = xb - yb.gather(1, j[..., None].expand(-1, -1, 3))
        loss = loss + (d * d).sum(-1).mean(1)
    if dirs & _lib.NR_CHAMFER_Y_TO_X:
        with torch.no_grad():
            i = _nearest_torch(yb, xb)[1]
        d = xb.gather(1, i[..., None].expand(-1, -1, 3)) - yb
        loss = loss + (d * d).sum(-1).mean(1)
    return _finish(loss, single, average)


def _face_cdf(v, f):
    """[B, F]: the inclusive prefix sum of the face areas up to the latest face of positive area at or
    before f, so that a face of zero area repeats its predecessor exactly whatever order cumsum added in."""
    tri = v[:, f]
    area = 0.5 * torch.linalg.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], dim=-1).norm(dim=-1)
    c = torch.cumsum(area, 1)
    return torch.cummax(torch.where(area > 0, c, torch.zeros_like(c)), 1)[0]


def _prepare_mesh(vertices, faces, num_samples, u, generator):
    if not torch.is_tensor(vertices) or vertices.ndim not in (2, 3) or vertices.shape[-1] != 3:
        raise ValueError("vertices must be a [B, V, 3] or [V, 3] tensor")
    single = vertices.ndim == 2
    v = vertices[None] if single else vertices
    B, V, S = v.shape[0], v.shape[1], int(num_samples)
    if S < 1:
        raise ValueError("num_samples must be at least 1, got %d" % S)
    f = faces_i32(faces, v.device, V, "faces")
    if f.shape[0] == 0:
        raise ValueError("sample_points needs at least one face")
    if u is None:
        u = torch.rand((B, S, 3), device=v.device, dtype=v.dtype, generator=generator)
    else:
        if not torch.is_tensor(u) or tuple(u.shape) not in ((B, S, 3),) + (((S, 3),) if single else ()):
            raise ValueError("u must be [B, S, 3] = [%d, %d, 3], got %s" % (B, S, tuple(getattr(u, "shape", ()))))
        u = u.reshape(B, S, 3).to(device=v.device, dtype=v.dtype)
    return v, f, u, single


def _sample_result(points, face, weights, single, return_faces):
    if single:
        points, face, weights = points[0], face[0], weights[0]
    return (points, face, weights) if return_faces else points


def sample_points_torch(vertices, faces, num_samples, u=None, generator=None, return_faces=False):
    """sample_points as torch ops (cumsum, searchsorted(right=True), gather, whose backward is the
    index_add_ of weights times the upstream gradient); any device and floating dtype."""
    v, f, u, single = _prepare_mesh(vertices, faces, num_samples, u, generator)
    fl = f.long()
    F = fl.shape[0]
    with torch.no_grad():
        c = _face_cdf(v, fl)
        total = c[:, -1:]
        face = torch.searchsorted(c, (u[..., 0] * total).contiguous(), right=True)
        # u0 * total rounded up to the total: the last face of positive area (F - 1 when there is none)
        last = torch.where(total > 0, torch.searchsorted(c, total.contiguous(), right=False), torch.full_like(face[:, :1], F - 1))
        face = torch.where(face >= F, last.expand_as(face), face)
        r = torch.sqrt(u[..., 1])
        weights = torch.stack([1 - r, r * (1 - u[..., 2]), r * u[..., 2]], -1)
    corners = fl[face]  # [B, S, 3]
    points = sum(weights[..., k, None] * v.gather(1, corners[..., k, None].expand(-1, -1, 3)) for k in range(3))
    return _sample_result(points, face.to(torch.int32), weights, single, return_faces)


# ---- the fused path ----
def _chamfer_launch(x, y, dirs, want_dist2, want_loss):
    """x [B, N, 3] contiguous; y [M, 3] contiguous (shared), a batch-expanded view of one, or [B, M, 3]
    contiguous.  Returns (loss, index_xy, index_yx, dist2_xy), each None when not asked for."""
    B, N, M = x.shape[0], x.shape[1], y.shape[-2]
    dev = x.device
    L = _lib.lib()
    xy, yx = dirs & _lib.NR_CHAMFER_X_TO_Y, dirs & _lib.NR_CHAMFER_Y_TO_X
    index_xy = torch.empty((B, N), dtype=torch.int32, device=dev) if xy else None
    index_yx = torch.empty((B, M), dtype=torch.int32, device=dev) if yx else None
    dist2 = torch.empty((B, N), dtype=torch.float32, device=dev) if want_dist2 else None
    loss = torch.empty(B, dtype=torch.float32, device=dev) if want_loss else None
    ws = torch.empty(L.nr_chamfer_workspace_bytes(B, N, M, dirs), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(L.nr_chamfer_forward(_lib.ptr(x), _lib.ptr(y), _y_stride(y), B, N, M, dirs, _lib.ptr(index_xy), _lib.ptr(index_yx),
                                        _lib.ptr(dist2), None, _lib.ptr(loss), _lib.ptr(ws), ws.numel(), _lib.stream_of(x)),
                   "nr_chamfer_forward")
    return loss, index_xy, index_yx, dist2


def _y_stride(y):
    return 0 if y.ndim == 2 or y.stride(0) == 0 else y.shape[1] * 3


def _dense_y(y):
    """y as the kernels read it: a shared [M, 3] set or a batch-expanded view of one is read in place with
    an item stride of 0; anything else is made contiguous."""
    if y.ndim == 3 and y.stride(0) == 0 and y.stride(1) == 3 and y.stride(2) == 1:
        return y
    return y.contiguous()


class ChamferFunction(torch.autograd.Function):
    """x [B, N, 3] float32 contiguous on the GPU, y as _dense_y gives it -> loss [B]; saves the nearest
    index arrays of the requested directions (and x and y themselves, which the backward reads again)."""

    @staticmethod
    def forward(ctx, x, y, dirs):
        loss, index_xy, index_yx, _ = _chamfer_launch(x, y, dirs, False, True)
        ctx.dirs = dirs
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(x, y, index_xy, index_yx)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_y):
            return None, None, None
        x, y, index_xy, index_yx = ctx.saved_tensors
        B, N, M = x.shape[0], x.shape[1], y.shape[-2]
        if need_y and y.ndim == 2:
            raise RuntimeError("a shared y that takes a gradient must be passed batch-expanded")
        g = grad_loss.to(torch.float32).contiguous()
        gx = torch.empty_like(x) if need_x else None
        gy = torch.empty((B, M, 3), dtype=torch.float32, device=x.device) if need_y else None
        with _lib.on_device(x.device):
            _lib.check(_lib.lib().nr_chamfer_backward(_lib.ptr(x), _lib.ptr(y), _y_stride(y), _lib.ptr(index_xy), _lib.ptr(index_yx),
                                                      _lib.ptr(g), B, N, M, ctx.dirs, _lib.ptr(gx), _lib.ptr(gy),
                                                      _lib.stream_of(x)), "nr_chamfer_backward")
        return gx, gy, None


def chamfer_distance(x, y, directions="both", average=False):
    """(1/N) sum_i min_j |x_i - y_j|^2 + (1/M) sum_j min_i |x_i - y_j|^2 per item: [B] for x [B, N, 3], a
    0-dim tensor for [N, 3] or with average=True (the mean over the items).  y is [B, M, 3], or [M, 3]: alone
    with a single x, shared by every item of a batched one (read in place; expanded only when it takes a
    gradient, so that torch's expand backward sums the items).  directions='x_to_y' / 'y_to_x' keeps the
    first / second term only.  An empty set raises ValueError; the inputs are taken to be finite.
    float32 GPU tensors run the fused kernels; everything else chamfer_distance_torch.  The gradient
    reaches x and, if it requires one, y; the nearest indices are constants (module docstring)."""
    if not _fused(x, y):
        return chamfer_distance_torch(x, y, directions, average)
    dirs = _directions(directions)
    xb, y, single = _prepare_sets(x, y)
    if y.ndim == 2 and y.requires_grad and torch.is_grad_enabled():
        y = y[None].expand(xb.shape[0], -1, -1)
    return _finish(ChamferFunction.apply(xb.contiguous(), _dense_y(y), dirs), single, average)


def nearest_points(x, y):
    """For every point of x [B, N, 3] (or [N, 3]) its nearest point of y ([B, M, 3], or [M, 3] alone or
    shared): (dist2 [B, N] float32 squared distances, index [B, N] int32, the lowest index among exact
    ties).  The chamfer kernel in one direction; both results are detached.  For a loss with custom
    weighting gather y by `index` in torch (y.gather(1, index.long()[..., None].expand(-1, -1, 3))) and form
    the differences there: the gradient then follows torch's own gather."""
    if not _fused(x, y):
        return nearest_points_torch(x, y)
    xb, y, single = _prepare_sets(x, y)
    with torch.no_grad():
        _, index, _, dist2 = _chamfer_launch(xb.detach().contiguous(), _dense_y(y.detach()), _lib.NR_CHAMFER_X_TO_Y, True, False)
    return (dist2[0], index[0]) if single else (dist2, index)


class SamplePointsFunction(torch.autograd.Function):
    """vertices [B, V, 3] float32 contiguous on the GPU, faces [F, 3] int32, u [B, S, 3] -> points, face,
    weights; the backward needs face and weights alone."""

    @staticmethod
    def forward(ctx, vertices, faces, u):
        B, V, F, S = vertices.shape[0], vertices.shape[1], faces.shape[0], u.shape[1]
        dev = vertices.device
        L = _lib.lib()
        points = torch.empty((B, S, 3), dtype=torch.float32, device=dev)
        face = torch.empty((B, S), dtype=torch.int32, device=dev)
        weights = torch.empty((B, S, 3), dtype=torch.float32, device=dev)
        ws = torch.empty(L.nr_sample_points_workspace_bytes(B, F), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.nr_sample_points_forward(_lib.ptr(vertices), _lib.ptr(faces), _lib.ptr(u), B, V, F, S, _lib.ptr(points),
                                                  _lib.ptr(face), _lib.ptr(weights), _lib.ptr(ws), ws.numel(),
                                                  _lib.stream_of(vertices)), "nr_sample_points_forward")
        ctx.num_vertices = V
        ctx.mark_non_differentiable(face, weights)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(faces, face, weights)
        return points, face, weights

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_points, _grad_face, _grad_weights):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        faces, face, weights = ctx.saved_tensors
        B, S, V = face.shape[0], face.shape[1], ctx.num_vertices
        g = grad_points.to(torch.float32).contiguous()
        gv = torch.empty((B, V, 3), dtype=torch.float32, device=g.device)
        with _lib.on_device(g.device):
            _lib.check(_lib.lib().nr_sample_points_backward(_lib.ptr(faces), _lib.ptr(face), _lib.ptr(weights), _lib.ptr(g), B, V,
                                                            faces.shape[0], S, _lib.ptr(gv), _lib.stream_of(g)),
                       "nr_sample_points_backward")
        return gv, None, None


def sample_points(vertices, faces, num_samples, u=None, generator=None, return_faces=False):
    """num_samples points on the surface of each mesh, faces weighted by area: points [B, S, 3] for
    vertices [B, V, 3] ([S, 3] for [V, 3]); with return_faces=True also face [B, S] int32 and weights
    [B, S, 3].  `faces` is [F, 3], shared by the items (out-of-range indices raise IndexError).  `u` is
    [B, S, 3] uniform in [0, 1); when absent it is drawn with torch.rand on the vertices' device from
    `generator`, so the sampling itself is a pure function of (vertices, faces, u).

    Per item, with a_f the face areas and c_f their inclusive float32 prefix sum: sample s takes the
    smallest f with c_f > u_s0 c_{F-1}, so a face of zero area (a repeated index among them) is never
    taken; with r = sqrt(u_s1) the weights over the face's corners are (1 - r, r (1 - u_s2), r u_s2) and the
    point is their weighted sum.  An item whose total area is 0 raises no error: its samples take face
    F - 1.  The gradient reaches the vertices through the weighted sum only (face choice and weights are
    constants).  float32 GPU vertices run the fused kernels, whose backward scatters with float atomics
    (module docstring); everything else sample_points_torch."""
    if not (_fused(vertices) and vertices.ndim in (2, 3)):
        return sample_points_torch(vertices, faces, num_samples, u, generator, return_faces)
    v, f, u, single = _prepare_mesh(vertices, faces, num_samples, u, generator)
    points, face, weights = SamplePointsFunction.apply(v.contiguous(), f, u.detach().contiguous())
    return _sample_result(points, face, weights, single, return_faces)


# ---- point-to-surface distance ----
def _prepare_point_mesh(points, vertices, faces):
    """points as [B, N, 3] or a shared [N, 3], vertices as [B, V, 3], faces as [F, 3] int32 on the vertices'
    device, and whether the mesh was a single [V, 3] one."""
    if not torch.is_tensor(points) or points.ndim not in (2, 3) or points.shape[-1] != 3:
        raise ValueError("points must be a [B, N, 3] or [N, 3] tensor")
    if not torch.is_tensor(vertices) or vertices.ndim not in (2, 3) or vertices.shape[-1] != 3:
        raise ValueError("vertices must be a [B, V, 3] or [V, 3] tensor")
    single = vertices.ndim == 2
    if single:
        if points.ndim != 2:
            raise ValueError("a single [V, 3] mesh takes a single [N, 3] point set, got points of shape %s" % (tuple(points.shape),))
        vertices = vertices[None]
    elif points.ndim == 3 and points.shape[0] != vertices.shape[0]:
        raise ValueError("batch sizes differ: points has %d items, vertices has %d" % (points.shape[0], vertices.shape[0]))
    f = faces_i32(faces, vertices.device, vertices.shape[1], "faces")
    if points.shape[-2] == 0 or f.shape[0] == 0:
        raise ValueError("empty input: N = %d, F = %d (both must be at least 1)" % (points.shape[-2], f.shape[0]))
    return points, vertices, f, single


def _point_triangle(p, a, b, c, degenerate, want_weights):
    """The closest point of the triangles (a, b, c) to the points p (all [..., 3], broadcast against each
    other; degenerate [...] bool): the squared distance, and with want_weights the barycentric weights
    [..., 3] instead.  The rule of csrc/nr_point_mesh.h: a regular face takes the plane's closest point
    where it falls inside, else the nearest of the edges ab, ac, bc (the first among equals); a degenerate
    one its longest edge (the first among equals), the third corner's weight 0."""
    ab, ac, bc, ap, bp = b - a, c - a, c - b, p - a, p - b

    def segment(r, e):
        ee = (e * e).sum(-1)
        live = ee > 0
        t = torch.where(live, (r * e).sum(-1) / torch.where(live, ee, torch.ones_like(ee)), torch.zeros_like(ee)).clamp(0, 1)
        d = r - t[..., None] * e
        return (d * d).sum(-1), t

    (e0, t0), (e1, t1), (e2, t2) = segment(ap, ab), segment(ap, ac), segment(bp, bc)
    d00, d01, d11 = (ab * ab).sum(-1), (ab * ac).sum(-1), (ac * ac).sum(-1)
    det = d00 * d11 - d01 * d01
    degenerate = degenerate | ~(det > 0)
    safe = torch.where(degenerate, torch.ones_like(det), det)
    d1, d2 = (ap * ab).sum(-1), (ap * ac).sum(-1)
    v, w = (d11 * d1 - d01 * d2) / safe, (d00 * d2 - d01 * d1) / safe
    inside = ~degenerate & (v >= 0) & (w >= 0) & (v + w <= 1)
    if not want_weights:
        d = ap - v[..., None] * ab - w[..., None] * ac
        return torch.where(inside, (d * d).sum(-1), torch.minimum(torch.minimum(e0, e1), e2))
    dbc = (bc * bc).sum(-1)
    first = torch.where(degenerate, (d00 >= d11) & (d00 >= dbc), (e0 <= e1) & (e0 <= e2))
    second = torch.where(degenerate, d11 >= dbc, e1 <= e2)
    zero = torch.zeros_like(t0)
    on_ab, on_ac, on_bc = torch.stack([1 - t0, t0, zero], -1), torch.stack([1 - t1, zero, t1], -1), torch.stack([zero, 1 - t2, t2], -1)
    edge = torch.where(first[..., None], on_ab, torch.where(second[..., None], on_ac, on_bc))
    return torch.where(inside[..., None], torch.stack([(1 - v - w).clamp(min=0), v, w], -1), edge)


def _mesh_corners(v, fl):
    """The corners [B, F, 3, 3] of the faces fl (int64) and which faces are degenerate [B, F]: a repeated index
    or an exactly zero cross product of the edges ab and ac."""
    tri = v[:, fl]
    n = torch.linalg.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], dim=-1)
    repeated = (fl[:, 0] == fl[:, 1]) | (fl[:, 0] == fl[:, 2]) | (fl[:, 1] == fl[:, 2])
    return tri, repeated[None] | (n == 0).all(-1)


def _nearest_face_torch(p, tri, degenerate):
    """int64 [B, N]: the nearest face of every point of p [B, N, 3] (torch.min: the first of equal minima),
    chunked over N."""
    B, N, F = p.shape[0], p.shape[1], tri.shape[1]
    step = max(1, _CHUNK_PAIRS // (F * B))
    a, b, c, deg = tri[:, None, :, 0], tri[:, None, :, 1], tri[:, None, :, 2], degenerate[:, None]
    return torch.cat([_point_triangle(p[:, i:i + step, None, :], a, b, c, deg, False).min(dim=2)[1] for i in range(0, N, step)], 1)


def _closest_torch(p, v, fl, face):
    """(dist2 [B, N], int64 face [B, N], weights [B, N, 3]) of p [B, N, 3] against the mesh; dist2 is
    differentiable in p and v, face (its own arg-min when None) and weights are constants."""
    with torch.no_grad():
        tri, degenerate = _mesh_corners(v, fl)
        if face is None:
            face = _nearest_face_torch(p, tri, degenerate)
        own = tri.gather(1, face[..., None, None].expand(-1, -1, 3, 3))
        weights = _point_triangle(p, own[:, :, 0], own[:, :, 1], own[:, :, 2], degenerate.gather(1, face), True)
    corners = fl[face]  # [B, N, 3]
    c = sum(weights[..., k, None] * v.gather(1, corners[..., k, None].expand(-1, -1, 3)) for k in range(3))
    d = p - c
    return (d * d).sum(-1), face, weights


def _expanded(points, B):
    return points if points.ndim == 3 else points[None].expand(B, -1, -1)


def closest_points_on_mesh_torch(points, vertices, faces):
    """closest_points_on_mesh as torch ops; any device and floating dtype (dist2 and weights in that dtype)."""
    p, v, f, single = _prepare_point_mesh(points, vertices, faces)
    with torch.no_grad():
        dist2, face, weights = _closest_torch(_expanded(p, v.shape[0]), v, f.long(), None)
    face = face.to(torch.int32)
    return (dist2[0], face[0], weights[0]) if single else (dist2, face, weights)


def point_mesh_distance_torch(points, vertices, faces, average=False, face=None):
    """point_mesh_distance as torch ops: the nearest face from a chunked [B, n, F] point-triangle test (held
    constant, as are the weights of the closest point), then a gather and a mean; any device and floating
    dtype.  With face [B, N] (or [N] for single inputs) given, that assignment replaces the arg-min: the
    closest point on the given face is still computed, differentiably."""
    p, v, f, single = _prepare_point_mesh(points, vertices, faces)
    B = v.shape[0]
    pb = _expanded(p, B)
    if face is not None:
        face = torch.as_tensor(face, device=v.device).long().reshape(B, pb.shape[1])
        if face.numel() and (int(face.min()) < 0 or int(face.max()) >= f.shape[0]):
            raise IndexError("face index out of range [0, %d)" % f.shape[0])
    dist2 = _closest_torch(pb, v, f.long(), face)[0]
    return _finish(dist2.mean(1), single, average)


def _points_stride(p):
    return 0 if p.ndim == 2 or p.stride(0) == 0 else p.shape[1] * 3


# The two directions of the fused path: the entry points' prefix (nr_<abi>_workspace_bytes / _forward / _backward,
# include/nr_raster.h) and whether the faces are the queries.  Everything below that differs between them reads
# it from here.
_POINT_FACE = ("nr_point_mesh", False)  # for every point its nearest face
_FACE_POINT = ("nr_face_point", True)   # for every face its nearest point


def _pair_launch(p, v, f, direction, want_loss):
    """p as _dense_y gives it, v [B, V, 3] contiguous, f [F, 3] int32 -> (loss or None, dist2, index, weights), a row
    per query: per point (index: its face) in _POINT_FACE, per face (index: its point) in _FACE_POINT."""
    abi, face_query = direction
    B, N, V, F = v.shape[0], p.shape[-2], v.shape[1], f.shape[0]
    Q = F if face_query else N
    dev = v.device
    L = _lib.lib()
    dist2 = torch.empty((B, Q), dtype=torch.float32, device=dev)
    index = torch.empty((B, Q), dtype=torch.int32, device=dev)
    weights = torch.empty((B, Q, 3), dtype=torch.float32, device=dev)
    loss = torch.empty(B, dtype=torch.float32, device=dev) if want_loss else None
    ws = torch.empty(getattr(L, abi + "_workspace_bytes")(B, N, F), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(getattr(L, abi + "_forward")(_lib.ptr(p), _points_stride(p), _lib.ptr(v), _lib.ptr(f), B, N, V, F, _lib.ptr(dist2),
                                                _lib.ptr(index), _lib.ptr(weights), _lib.ptr(loss), _lib.ptr(ws), ws.numel(),
                                                _lib.stream_of(v)), abi + "_forward")
    return loss, dist2, index, weights


class PairDistanceFunction(torch.autograd.Function):
    """points as _dense_y gives them, vertices [B, V, 3] float32 contiguous on the GPU, faces [F, 3] int32, a direction
    -> loss [B]; saves the chosen index and the weights (and the inputs, which the backward reads again).  The
    corner lists of _FACE_POINT's vertex gather are looked up in the forward (cached per faces tensor), so the
    backward does no host work."""

    @staticmethod
    def forward(ctx, points, vertices, faces, direction):
        loss, _, index, weights = _pair_launch(points, vertices, faces, direction, True)
        ctx.direction = direction
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(points, vertices, faces, index, weights)
            if direction[1]:
                ctx.corners = vertex_adjacency(faces, vertices.shape[1]) if ctx.needs_input_grad[1] else (None, None)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        need_p, need_v = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_p or need_v):
            return None, None, None, None
        abi, face_query = ctx.direction
        p, v, f, index, weights = ctx.saved_tensors
        B, N, V = v.shape[0], p.shape[-2], v.shape[1]
        if need_p and p.ndim == 2:
            raise RuntimeError("shared points that take a gradient must be passed batch-expanded")
        g = grad_loss.to(torch.float32).contiguous()
        gp = torch.empty((B, N, 3), dtype=torch.float32, device=v.device) if need_p else None
        gv = torch.empty_like(v) if need_v else None
        corners = [_lib.ptr(c) for c in ctx.corners] if face_query else []
        with _lib.on_device(v.device):
            _lib.check(getattr(_lib.lib(), abi + "_backward")(_lib.ptr(p), _points_stride(p), _lib.ptr(v), _lib.ptr(f), *corners,
                                                              _lib.ptr(index), _lib.ptr(weights), _lib.ptr(g), B, N, V, f.shape[0],
                                                              _lib.ptr(gp), _lib.ptr(gv), _lib.stream_of(v)), abi + "_backward")
        return gp, gv, None, None


def point_mesh_distance(points, vertices, faces, average=False):
    """(1/N) sum_i min_f dist^2(p_i, T_f) per item, T_f the triangle f as a closed set: the mean squared
    distance from the points to the surface.  [B] for vertices [B, V, 3], a 0-dim tensor for [V, 3] or with
    average=True (the mean over the items).  points is [B, N, 3], or [N, 3]: alone with a single mesh, shared
    by the items of a batched one (read in place; expanded only when it takes a gradient, so that torch's
    expand backward sums the items).  faces is [F, 3], shared (out-of-range indices raise IndexError).
    N = 0, F = 0 and differing batch sizes raise ValueError; the inputs are taken to be finite.

    The lowest face index wins among exact float32 ties.  A degenerate face (a repeated index, coincident
    or exactly collinear corners) counts as the segment between its two most distant corners, or a point.
    The gradient holds the face choice and the barycentric weights w of the closest point c_i constant:
    p_i takes g_b (2/N) (p_i - c_i), vertex j takes -g_b (2/N) sum w_ik (p_i - c_i) over the corners (i, k) that
    are j.  By the envelope theorem this is the exact gradient of the squared distance wherever the
    closest face is unique.  float32 GPU tensors run the fused kernels (nr_point_mesh_*); everything else
    point_mesh_distance_torch."""
    if not _fused(points, vertices):
        return point_mesh_distance_torch(points, vertices, faces, average)
    p, v, f, single = _prepare_point_mesh(points, vertices, faces)
    if p.ndim == 2 and p.requires_grad and torch.is_grad_enabled():
        p = p[None].expand(v.shape[0], -1, -1)
    return _finish(PairDistanceFunction.apply(_dense_y(p), v.contiguous(), f, _POINT_FACE), single, average)


def closest_points_on_mesh(points, vertices, faces):
    """For every point of points ([B, N, 3], or [N, 3] alone or shared) its closest point on the mesh:
    (dist2 [B, N] float32, face [B, N] int32: the closest face, the lowest index among exact ties,
    weights [B, N, 3] float32: the barycentric weights of the closest point over that face's corners, so
    that it is sum_k weights[..., k] * vertices[faces[face, k]]).  dist2 is the squared distance to exactly
    that point.  All three are detached; for a custom loss rebuild the closest point from face and weights
    in torch and let the gradient follow torch's own gather."""
    if not _fused(points, vertices):
        return closest_points_on_mesh_torch(points, vertices, faces)
    p, v, f, single = _prepare_point_mesh(points, vertices, faces)
    with torch.no_grad():
        _, dist2, face, weights = _pair_launch(_dense_y(p.detach()), v.detach().contiguous(), f, _POINT_FACE, False)
    return (dist2[0], face[0], weights[0]) if single else (dist2, face, weights)


# ---- face-to-scan distance ----
def _nearest_point_torch(p, tri, degenerate):
    """int64 [B, F]: the nearest point of p [B, N, 3] to every face (torch.min: the first of equal minima),
    chunked over F."""
    B, N, F = p.shape[0], p.shape[1], tri.shape[1]
    step = max(1, _CHUNK_PAIRS // (N * B))
    out = []
    for i in range(0, F, step):
        t, deg = tri[:, i:i + step, None], degenerate[:, i:i + step, None]
        out.append(_point_triangle(p[:, None, :, :], t[..., 0, :], t[..., 1, :], t[..., 2, :], deg, False).min(dim=2)[1])
    return torch.cat(out, 1)


def _closest_to_faces_torch(p, v, fl, point):
    """(dist2 [B, F], int64 point [B, F], weights [B, F, 3]) of the faces against p [B, N, 3]; dist2 is
    differentiable in p and v, point (its own arg-min when None) and weights are constants."""
    with torch.no_grad():
        tri, degenerate = _mesh_corners(v, fl)
        if point is None:
            point = _nearest_point_torch(p, tri, degenerate)
        own = p.gather(1, point[..., None].expand(-1, -1, 3))
        weights = _point_triangle(own, tri[:, :, 0], tri[:, :, 1], tri[:, :, 2], degenerate, True)
    c = sum(weights[..., k, None] * v[:, fl[:, k]] for k in range(3))
    d = p.gather(1, point[..., None].expand(-1, -1, 3)) - c
    return (d * d).sum(-1), point, weights


def closest_points_to_faces_torch(vertices, faces, points):
    """closest_points_to_faces as torch ops; any device and floating dtype (dist2 and weights in that dtype)."""
    p, v, f, single = _prepare_point_mesh(points, vertices, faces)
    with torch.no_grad():
        dist2, point, weights = _closest_to_faces_torch(_expanded(p, v.shape[0]), v, f.long(), None)
    point = point.to(torch.int32)
    return (dist2[0], point[0], weights[0]) if single else (dist2, point, weights)


def mesh_point_distance_torch(vertices, faces, points, average=False, point=None):
    """mesh_point_distance as torch ops: the nearest point of every face from a chunked [B, f, N] point-triangle
    test (held constant, as are the weights of the closest point), then a gather and a mean; any device and
    floating dtype.  With point [B, F] (or [F] for single inputs) given, that assignment replaces the arg-min:
    the closest point of the face to the given point is still computed, differentiably."""
    p, v, f, single = _prepare_point_mesh(points, vertices, faces)
    B = v.shape[0]
    pb = _expanded(p, B)
    if point is not None:
        point = torch.as_tensor(point, device=v.device).long().reshape(B, f.shape[0])
        if point.numel() and (int(point.min()) < 0 or int(point.max()) >= pb.shape[1]):
            raise IndexError("point index out of range [0, %d)" % pb.shape[1])
    dist2 = _closest_to_faces_torch(pb, v, f.long(), point)[0]
    return _finish(dist2.mean(1), single, average)


def mesh_point_distance(vertices, faces, points, average=False):
    """(1/F) sum_f min_i dist^2(p_i, T_f) per item, T_f the triangle f as a closed set: the mean over the faces of
    the squared distance from the face to its nearest point, the term that keeps a mesh from growing surface
    where a scan has no points (the face -> point half of a point-mesh face distance).  [B] for vertices
    [B, V, 3], a 0-dim tensor for [V, 3] or with average=True (the mean over the items).  points is [B, N, 3],
    or [N, 3]: alone with a single mesh, shared by the items of a batched one (read in place; expanded only
    when it takes a gradient, so that torch's expand backward sums the items).  faces is [F, 3], shared
    (out-of-range indices raise IndexError).  N = 0, F = 0 and differing batch sizes raise ValueError; the
    inputs are taken to be finite.

    Every face counts.  The lowest point index wins among exact float32 ties; the pair distance and the
    degenerate-face rule are point_mesh_distance's.  The gradient holds the point choice and the barycentric
    weights w of the closest point c_f constant: vertex j takes -g_b (2/F) sum w_fk (p - c_f) over the corners
    (f, k) that are j, point i takes g_b (2/F) sum (p_i - c_f) over the faces that chose it.  float32 GPU
    tensors run the fused kernels (nr_face_point_*): the loss and the vertex gradient are bitwise
    reproducible, the point gradient is scattered with float atomics (module docstring).  Everything else
    runs mesh_point_distance_torch."""
    if not _fused(vertices, points):
        return mesh_point_distance_torch(vertices, faces, points, average)
    p, v, f, single = _prepare_point_mesh(points, vertices, faces)
    if p.ndim == 2 and p.requires_grad and torch.is_grad_enabled():
        p = p[None].expand(v.shape[0], -1, -1)
    return _finish(PairDistanceFunction.apply(_dense_y(p), v.contiguous(), f, _FACE_POINT), single, average)


def closest_points_to_faces(vertices, faces, points):
    """For every face of the mesh its nearest point of points ([B, N, 3], or [N, 3] alone or shared): (dist2
    [B, F] float32, point [B, F] int32: the nearest point, the lowest index among exact ties, weights [B, F, 3]
    float32: the barycentric weights of the face's closest point to it over the face's corners).  dist2 is the
    squared distance between exactly those two.  All three are detached."""
    if not _fused(vertices, points):
        return closest_points_to_faces_torch(vertices, faces, points)
    p, v, f, single = _prepare_point_mesh(points, vertices, faces)
    with torch.no_grad():
        _, dist2, point, weights = _pair_launch(_dense_y(p.detach()), v.detach().contiguous(), f, _FACE_POINT, False)
    return (dist2[0], point[0], weights[0]) if single else (dist2, point, weights)


class _PointSetLoss(torch.nn.Module):
    """A distance between the mesh given to forward and an optional fixed point set held by the module (a buffer: it
    moves with .to()); forward(vertices, faces) uses it, forward(vertices, faces, points) the given points."""

    def __init__(self, points=None, average=False):
        super().__init__()
        self.register_buffer("points", None if points is None else torch.as_tensor(points).detach().clone())
        self.average = average

    def forward(self, vertices, faces, points=None):
        points = self.points if points is None else points
        if points is None:
            raise ValueError("%s needs points: pass them, or construct the module with a point set" % type(self).__name__)
        return self.distance(points, vertices, faces)


class MeshPointLoss(_PointSetLoss):
    """mesh_point_distance from the mesh given to forward to an optional fixed point set held by the module (a
    buffer: it moves with .to()); forward(vertices, faces) uses it, forward(vertices, faces, points) the given
    points."""

    def distance(self, points, vertices, faces):
        return mesh_point_distance(vertices, faces, points, self.average)


class PointMeshLoss(_PointSetLoss):
    """point_mesh_distance from an optional fixed point set held by the module (a buffer: it moves with
    .to()) to the mesh given to forward; forward(vertices, faces) uses it, forward(vertices, faces, points)
    the given points."""

    def distance(self, points, vertices, faces):
        return point_mesh_distance(points, vertices, faces, self.average)


class ChamferLoss(torch.nn.Module):
    """chamfer_distance against an optional fixed target held by the module (a buffer: it moves with
    .to()); forward(x) uses it, forward(x, y) the given y."""

    def __init__(self, target=None, directions="both", average=False):
        super().__init__()
        _directions(directions)
        self.register_buffer("target", None if target is None else torch.as_tensor(target).detach().clone())
        self.directions = directions
        self.average = average

    def forward(self, x, y=None):
        y = self.target if y is None else y
        if y is None:
            raise ValueError("ChamferLoss needs a target: pass y, or construct the module with one")
        return chamfer_distance(x, y, self.directions, self.average)

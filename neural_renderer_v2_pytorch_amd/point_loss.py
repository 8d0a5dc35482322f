"""3-D point supervision for the optimisation loop around the renderer: the chamfer distance between two
point sets, the nearest-neighbour query under it, and area-weighted sampling of points on a mesh.  Each
is a fused HIP launch sequence (nr_chamfer_* / nr_sample_points_*, include/nr_raster.h) for float32 GPU
tensors and a torch composition (chamfer_distance_torch / nearest_points_torch / sample_points_torch) for
every other device and dtype.  The compositions are the tests' reference and the baseline of
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

No call synchronises with the host in the steady state (a faces tensor is range-checked once and
cached, as everywhere else), so a step can be captured in a HIP graph."""
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .mesh_loss import _finish
from .topology import faces_i32

CHAMFER_TILE = _lib.NR_CHAMFER_TILE  # targets the nearest-neighbour kernel stages in LDS at a time
_DIRECTIONS = {"both": _lib.NR_CHAMFER_X_TO_Y | _lib.NR_CHAMFER_Y_TO_X, "x_to_y": _lib.NR_CHAMFER_X_TO_Y,
               "y_to_x": _lib.NR_CHAMFER_Y_TO_X}
_CHUNK_ELEMS = 1 << 24  # difference-tensor elements the compositions build at a time


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

"""Mesh regularizers for the optimisation loop around the renderer: the uniform Laplacian smoothness
loss and the dihedral 'flatten' loss, each one fused HIP launch pair forward and one launch backward
(nr_laplacian_* / nr_flatten_*, include/nr_raster.h) for float32 GPU vertices, and a torch composition
(laplacian_loss_torch / flatten_loss_torch) for every other device and dtype.

Definitions, for vertices [B, V, 3] and faces [F, 3] shared by every item.  Faces with a repeated
vertex index are ignored by both losses; duplicate faces count separately.

  Laplacian: N(i) = the distinct vertices that share a face edge with i,
             delta_i = v_i - mean_{j in N(i)} v_j (0 when N(i) is empty), loss_b = sum_i |delta_i|^2
             -- the dense row-normalised umbrella Laplacian |L v|^2, without the V x V matrix.
  Flatten:   over every undirected edge v0 < v1 with exactly two incident faces (boundary edges and
             edges with three or more faces contribute nothing), v2 / v3 the opposite vertices of the
             lower- / higher-numbered face:  a = v1 - v0, b_k = v_{k+1} - v0,
             c_k = b_k - a (a . b_k) / (|a|^2 + eps),
             cos = (c_1 . c_2) / (sqrt(|c_1|^2 + eps) sqrt(|c_2|^2 + eps)), loss_b = sum_edges (cos + 1)^2.

The topology (mesh_topology) is built on the host once per faces tensor and cached, so steady-state
calls issue no host synchronisation and a step can be captured in a HIP graph.  The fused kernels use
no float atomics: losses and gradients are bitwise identical from run to run."""
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .topology import MeshTopology, mesh_topology


def _prepare(vertices, faces):
    """vertices as [B, V, 3], whether the input was a single [V, 3] mesh, and the topology on its device."""
    if not torch.is_tensor(vertices) or vertices.ndim not in (2, 3) or vertices.shape[-1] != 3:
        raise ValueError("vertices must be a [B, V, 3] or [V, 3] tensor")
    single = vertices.ndim == 2
    v = vertices[None] if single else vertices
    V = v.shape[1]
    if isinstance(faces, MeshTopology):
        if faces.num_vertices != V:
            raise ValueError("the topology was built for %d vertices, got %d" % (faces.num_vertices, V))
        topo = faces.to(v.device)
    else:
        topo = mesh_topology(faces, V, v.device)
    return v, single, topo


def _finish(loss, single, average):
    if average:
        return loss.mean()
    return loss[0] if single else loss


def _fused(vertices):
    return torch.is_tensor(vertices) and vertices.is_cuda and vertices.dtype == torch.float32


# ---- the torch composition: reference of the tests, baseline of tools/bench_mesh_loss.py ----
def laplacian_loss_torch(vertices, faces, average=False):
    """The Laplacian loss as torch ops (index_select + index_add_ over the topology); any device and
    floating dtype.  `faces` is a faces tensor / array or a MeshTopology."""
    v, single, topo = _prepare(vertices, faces)
    rows, cols, deg, _ = topo.composition_index()
    total = torch.zeros_like(v).index_add_(1, rows, v.index_select(1, cols))
    n = deg.to(v.dtype)
    delta = (v - total / n.clamp(min=1)[None, :, None]) * (n > 0).to(v.dtype)[None, :, None]
    return _finish((delta * delta).sum((1, 2)), single, average)


def flatten_loss_torch(vertices, faces, eps=1e-6, average=False):
    """The flatten loss as torch ops (index_select over the edge rows); any device and floating dtype."""
    v, single, topo = _prepare(vertices, faces)
    e = topo.composition_index()[3]
    p0, p1, p2, p3 = (v.index_select(1, e[:, k]) for k in range(4))
    a, b1, b2 = p1 - p0, p2 - p0, p3 - p0
    la = (a * a).sum(-1, keepdim=True) + eps
    c1 = b1 - a * ((a * b1).sum(-1, keepdim=True) / la)
    c2 = b2 - a * ((a * b2).sum(-1, keepdim=True) / la)
    cos = (c1 * c2).sum(-1) / (torch.sqrt((c1 * c1).sum(-1) + eps) * torch.sqrt((c2 * c2).sum(-1) + eps))
    return _finish(((cos + 1) ** 2).sum(1), single, average)


# ---- the fused path ----
def _workspace(L, B, count, dev):
    return torch.empty(L.nr_mesh_loss_workspace_bytes(B, count), dtype=torch.uint8, device=dev)


class LaplacianFunction(torch.autograd.Function):
    """vertices [B, V, 3] float32 contiguous on the GPU -> loss [B]; the forward saves delta [B, V, 3]."""

    @staticmethod
    def forward(ctx, vertices, topo):
        B, V = vertices.shape[0], vertices.shape[1]
        dev = vertices.device
        L = _lib.lib()
        need = ctx.needs_input_grad[0]
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        delta = torch.empty_like(vertices) if need else None
        ws = _workspace(L, B, V, dev)
        with _lib.on_device(dev):
            _lib.check(L.nr_laplacian_forward(_lib.ptr(vertices), _lib.ptr(topo.nbr_offsets), _lib.ptr(topo.nbr_index), B, V,
                                              _lib.ptr(delta), _lib.ptr(loss), _lib.ptr(ws), ws.numel(),
                                              _lib.stream_of(vertices)), "nr_laplacian_forward")
        ctx.topo = topo
        if need:
            ctx.save_for_backward(delta)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None
        delta, = ctx.saved_tensors
        topo = ctx.topo
        g = grad_loss.to(torch.float32).contiguous()
        gv = torch.empty_like(delta)
        with _lib.on_device(delta.device):
            _lib.check(_lib.lib().nr_laplacian_backward(_lib.ptr(delta), _lib.ptr(topo.nbr_offsets), _lib.ptr(topo.nbr_index),
                                                        _lib.ptr(g), delta.shape[0], delta.shape[1], _lib.ptr(gv),
                                                        _lib.stream_of(delta)), "nr_laplacian_backward")
        return gv, None


class FlattenFunction(torch.autograd.Function):
    """vertices [B, V, 3] float32 contiguous on the GPU -> loss [B].  When a gradient is needed the forward
    also writes each edge's gradient to its four vertices as [B, E2, 12] records, which are all the
    backward's vertex gather reads (measured against recomputing the edges in the backward: DESIGN.md
    section 4)."""

    @staticmethod
    def forward(ctx, vertices, topo, eps):
        B, V, E2 = vertices.shape[0], vertices.shape[1], topo.num_edges
        dev = vertices.device
        L = _lib.lib()
        need = ctx.needs_input_grad[0]
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        records = torch.empty((B, E2, 12), dtype=torch.float32, device=dev) if need else None
        ws = _workspace(L, B, E2, dev)
        with _lib.on_device(dev):
            _lib.check(L.nr_flatten_forward(_lib.ptr(vertices), _lib.ptr(topo.edges), B, V, E2, eps, _lib.ptr(records),
                                            _lib.ptr(loss), _lib.ptr(ws), ws.numel(), _lib.stream_of(vertices)),
                       "nr_flatten_forward")
        ctx.topo, ctx.num_vertices = topo, V
        if need:
            ctx.save_for_backward(records)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        records, = ctx.saved_tensors
        topo, B, V = ctx.topo, records.shape[0], ctx.num_vertices
        g = grad_loss.to(torch.float32).contiguous()
        gv = torch.empty((B, V, 3), dtype=torch.float32, device=records.device)
        with _lib.on_device(records.device):
            _lib.check(_lib.lib().nr_flatten_backward(_lib.ptr(records), _lib.ptr(topo.edge_offsets), _lib.ptr(topo.edge_slots),
                                                      _lib.ptr(g), B, V, topo.num_edges, _lib.ptr(gv),
                                                      _lib.stream_of(records)), "nr_flatten_backward")
        return gv, None, None


def laplacian_loss(vertices, faces, average=False):
    """sum_i |v_i - mean of i's neighbours|^2 per item: [B] for vertices [B, V, 3], a 0-dim tensor for
    [V, 3] or with average=True (the mean over the items).  `faces` is [F, 3] (shared by the items) or a
    MeshTopology.  float32 GPU vertices run the fused kernels; everything else laplacian_loss_torch.
    The gradient reaches the vertices only; a batch-expanded mesh is made contiguous, so torch's own
    expand backward sums the items onto the base."""
    if not _fused(vertices):
        return laplacian_loss_torch(vertices, faces, average)
    v, single, topo = _prepare(vertices, faces)
    return _finish(LaplacianFunction.apply(v.contiguous(), topo), single, average)


def flatten_loss(vertices, faces, eps=1e-6, average=False):
    """sum over the two-face edges of (cos + 1)^2, cos the cosine between the two faces' in-plane
    directions away from the edge (-1 when flat): shapes, dispatch and gradient as laplacian_loss."""
    if not _fused(vertices):
        return flatten_loss_torch(vertices, faces, eps, average)
    v, single, topo = _prepare(vertices, faces)
    return _finish(FlattenFunction.apply(v.contiguous(), topo, float(eps)), single, average)


class LaplacianLoss(torch.nn.Module):
    """laplacian_loss with the topology of `faces` held by the module."""

    def __init__(self, faces, num_vertices, average=False):
        super().__init__()
        self.topology = mesh_topology(faces, num_vertices)
        self.average = average

    def forward(self, vertices):
        return laplacian_loss(vertices, self.topology, self.average)


class FlattenLoss(torch.nn.Module):
    """flatten_loss with the topology of `faces` held by the module."""

    def __init__(self, faces, num_vertices, eps=1e-6, average=False):
        super().__init__()
        self.topology = mesh_topology(faces, num_vertices)
        self.eps = eps
        self.average = average

    def forward(self, vertices):
        return flatten_loss(vertices, self.topology, self.eps, self.average)

"""Mesh regularizers for the optimisation loop around the renderer: the uniform Laplacian smoothness
loss, the dihedral 'flatten' loss, the edge-length loss and the cotangent-weighted Laplacian loss, each
a few fused HIP launches forward and one launch backward (nr_laplacian_* / nr_flatten_* /
nr_edge_length_* / nr_cot_laplacian_*, include/nr_raster.h) for float32 GPU vertices, and a torch
composition (*_loss_torch) for every other device and dtype.

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
  Edge length: over every distinct undirected edge {i, j} of the faces (boundary and non-manifold edges
             once each; MeshTopology.num_all_edges of them), loss_b = sum (|v_i - v_j| - target_length)^2.
             An edge of length 0 adds target_length^2 and takes no gradient.
  Cotangent Laplacian: c_{f,k} = 0.5 (a . b) / sqrt(|a x b|^2 + eps) at corner k of face f, a and b the
             edge vectors leaving it; w_ij = max(0, sum of c over the corners opposite edge {i, j});
             W_i = sum_{j in N(i)} w_ij; delta_i = v_i - (sum_j w_ij v_j) / W_i where W_i > COT_MIN_WEIGHT,
             else 0; loss_b = sum_i |delta_i|^2.  The clamp keeps the weighted mean a convex combination
             where both angles opposite an edge are obtuse.  The weights are constants of the backward:
             no gradient flows through them, in the fused path and in the composition alike.
  ARAP:      for deformed vertices q against a rest shape p ([V, 3] shared by the items, or [B, V, 3]), with
             e_ij = p_i - p_j, d_ij = q_i - q_j and entry weights w_ij == w_ji (the cotangent weights above
             taken on p, 1, or given):  S_i = sum_{j in N(i)} w_ij e_ij d_ij^T;  R_i = the rotation (det +1)
             maximising tr(R S_i) -- V diag(1, 1, det(V U^T)) U^T of S_i = U Sigma V^T, I where S_i = 0, any
             maximiser where it is not unique;  loss_b = sum_i sum_{j in N(i)} w_ij |d_ij - R_i e_ij|^2.
             The rotations are constants of the backward (they maximise: the envelope theorem makes that the
             exact gradient): grad q_i = 2 g_b sum_{j in N(i)} w_ij (2 d_ij - (R_i + R_j) e_ij).  Neither p
             nor the weights take a gradient (nr_arap_* / nr_cot_weights).

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


COT_MIN_WEIGHT = _lib.NR_COT_MIN_WEIGHT  # a vertex whose weights sum to no more has delta = 0


def edge_length_loss_torch(vertices, faces, target_length=0.0, average=False):
    """The edge-length loss as torch ops (index_select over the neighbour entries j > i); any device and
    floating dtype.  A `where` keeps the square root's gradient away from edges of length 0."""
    v, single, topo = _prepare(vertices, faces)
    i, j = topo.edge_index()
    d = v.index_select(1, i) - v.index_select(1, j)
    d2 = (d * d).sum(-1)
    zero = d2 == 0
    length = torch.where(zero, torch.zeros_like(d2), torch.sqrt(torch.where(zero, torch.ones_like(d2), d2)))
    return _finish(((length - target_length) ** 2).sum(1), single, average)


def cot_weights_torch(v, topo, eps=1e-12):
    """The clamped cotangent weight of every neighbour entry, [B, nnz], of vertices [B, V, 3]: computed
    without gradient (the weights are constants of the loss's backward)."""
    with torch.no_grad():
        f, entry, corners = topo.cot_composition_index()
        p = [v.index_select(1, f[:, k]) for k in range(3)]
        c = []
        for k in range(3):
            a, b = p[(k + 1) % 3] - p[k], p[(k + 2) % 3] - p[k]
            n = torch.linalg.cross(a, b)
            c.append(0.5 * (a * b).sum(-1) / torch.sqrt((n * n).sum(-1) + eps))
        c = torch.stack(c, -1).reshape(v.shape[0], -1)  # [B, 3 F]; corners of ignored faces are never selected
        w = torch.zeros((v.shape[0], topo.nbr_index.numel()), dtype=v.dtype, device=v.device)
        return w.index_add_(1, entry, c.index_select(1, corners)).clamp_(min=0)


def cot_laplacian_loss_torch(vertices, faces, eps=1e-12, average=False):
    """The cotangent Laplacian loss as torch ops; any device and floating dtype.  The weights carry no
    gradient."""
    v, single, topo = _prepare(vertices, faces)
    rows, cols = topo.composition_index()[:2]
    w = cot_weights_torch(v.detach(), topo, eps)
    W = torch.zeros(v.shape[:2], dtype=v.dtype, device=v.device).index_add_(1, rows, w)
    ok = W > COT_MIN_WEIGHT
    total = torch.zeros_like(v).index_add_(1, rows, w[:, :, None] * v.index_select(1, cols))
    delta = (v - total / torch.where(ok, W, torch.ones_like(W))[:, :, None]) * ok.to(v.dtype)[:, :, None]
    return _finish((delta * delta).sum((1, 2)), single, average)


def _arap_prepare(vertices, rest_vertices, faces, weights):
    """vertices as [B, V, 3], single, the topology, the rest shape as [1 or B, V, 3] (detached, the vertices'
    device and dtype) and `weights` checked: 'cotangent', 'uniform' or a tensor as [1 or B, nnz] (detached)."""
    v, single, topo = _prepare(vertices, faces)
    B, V = v.shape[0], v.shape[1]
    if not torch.is_tensor(rest_vertices) or rest_vertices.ndim not in (2, 3) or rest_vertices.shape[-1] != 3:
        raise ValueError("rest_vertices must be a [V, 3] or [B, V, 3] tensor")
    p = rest_vertices.detach().to(device=v.device, dtype=v.dtype)
    p = p[None] if p.ndim == 2 else p
    if p.shape[1] != V or p.shape[0] not in (1, B):
        raise ValueError("rest_vertices %s do not fit vertices %s" % (list(rest_vertices.shape), list(vertices.shape)))
    if torch.is_tensor(weights):
        nnz = topo.nbr_index.numel()
        w = weights.detach()
        if not w.is_floating_point() or w.ndim not in (1, 2) or w.shape[-1] != nnz:
            raise ValueError("weights must be a float tensor [nnz] or [B, nnz] with nnz = %d neighbour entries, got %s"
                             % (nnz, list(weights.shape)))
        w = w[None] if w.ndim == 1 else w
        if w.shape[0] not in (1, B):
            raise ValueError("weights %s do not fit vertices %s" % (list(weights.shape), list(vertices.shape)))
        weights = w.to(device=v.device, dtype=v.dtype)
    elif weights not in ("cotangent", "uniform"):
        raise ValueError("weights must be 'cotangent', 'uniform' or a tensor, got %r" % (weights,))
    return v, single, topo, p, weights


def _arap_rotations_torch(v, p, w, topo):
    """R [B, V, 3, 3] without gradient: per vertex the rotation maximising tr(R S), S = sum_j w e d^T, through
    torch.linalg.svd; S = 0 gives I."""
    with torch.no_grad():
        rows, cols = topo.composition_index()[:2]
        e = p.index_select(1, rows) - p.index_select(1, cols)
        d = v.index_select(1, rows) - v.index_select(1, cols)
        terms = (w[:, :, None] * e)[:, :, :, None] * d[:, :, None, :]
        S = torch.zeros(v.shape[:2] + (3, 3), dtype=v.dtype, device=v.device).index_add_(1, rows, terms)
        U, _, Vh = torch.linalg.svd(S)
        Vm, Ut = Vh.transpose(-1, -2), U.transpose(-1, -2)
        flip = torch.ones(v.shape[:2] + (3,), dtype=v.dtype, device=v.device)
        flip[..., 2] = torch.linalg.det(Vm @ Ut)
        R = (Vm * flip[..., None, :]) @ Ut
        zero = (S == 0).all(-1).all(-1)
        return torch.where(zero[..., None, None], torch.eye(3, dtype=v.dtype, device=v.device), R)


def _arap_weights_torch(p, topo, weights, eps):
    if torch.is_tensor(weights):
        return weights
    if weights == "uniform":
        return torch.ones((1, topo.nbr_index.numel()), dtype=p.dtype, device=p.device)
    return cot_weights_torch(p, topo, eps)


def arap_rotations_torch(vertices, rest_vertices, faces, weights="cotangent", eps=1e-12):
    """arap_rotations as torch ops (torch.linalg.svd per vertex); any device and floating dtype."""
    v, single, topo, p, weights = _arap_prepare(vertices, rest_vertices, faces, weights)
    R = _arap_rotations_torch(v.detach(), p, _arap_weights_torch(p, topo, weights, eps), topo)
    return R[0] if single else R


def arap_loss_torch(vertices, rest_vertices, faces, weights="cotangent", eps=1e-12, average=False):
    """The ARAP energy as torch ops; any device and floating dtype.  The rotations come from
    torch.linalg.svd under no_grad and are constants of the backward, as in the fused path; neither the rest
    shape nor the weights take a gradient."""
    v, single, topo, p, weights = _arap_prepare(vertices, rest_vertices, faces, weights)
    w = _arap_weights_torch(p, topo, weights, eps)
    R = _arap_rotations_torch(v.detach(), p, w, topo)
    rows, cols = topo.composition_index()[:2]
    e = p.index_select(1, rows) - p.index_select(1, cols)
    d = v.index_select(1, rows) - v.index_select(1, cols)
    r = d - (R.index_select(1, rows) @ e[..., None])[..., 0]
    return _finish((w * (r * r).sum(-1)).sum(1), single, average)


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


class EdgeLengthFunction(torch.autograd.Function):
    """vertices [B, V, 3] float32 contiguous on the GPU -> loss [B]; the backward recomputes from the saved
    vertices."""

    @staticmethod
    def forward(ctx, vertices, topo, target_length):
        B, V = vertices.shape[0], vertices.shape[1]
        dev = vertices.device
        L = _lib.lib()
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        ws = _workspace(L, B, V, dev)
        with _lib.on_device(dev):
            _lib.check(L.nr_edge_length_forward(_lib.ptr(vertices), _lib.ptr(topo.nbr_offsets), _lib.ptr(topo.nbr_index), B, V,
                                                target_length, _lib.ptr(loss), _lib.ptr(ws), ws.numel(),
                                                _lib.stream_of(vertices)), "nr_edge_length_forward")
        ctx.topo, ctx.target_length = topo, target_length
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(vertices)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        vertices, = ctx.saved_tensors
        topo = ctx.topo
        g = grad_loss.to(torch.float32).contiguous()
        gv = torch.empty_like(vertices)
        with _lib.on_device(vertices.device):
            _lib.check(_lib.lib().nr_edge_length_backward(_lib.ptr(vertices), _lib.ptr(topo.nbr_offsets), _lib.ptr(topo.nbr_index),
                                                          _lib.ptr(g), vertices.shape[0], vertices.shape[1], ctx.target_length,
                                                          _lib.ptr(gv), _lib.stream_of(vertices)), "nr_edge_length_backward")
        return gv, None, None


class CotLaplacianFunction(torch.autograd.Function):
    """vertices [B, V, 3] float32 contiguous on the GPU -> loss [B].  When a gradient is needed the forward
    saves delta [B, V, 3], the entry weights w [B, nnz] and winv [B, V]; the weights are constants of the
    backward."""

    @staticmethod
    def forward(ctx, vertices, topo, eps):
        B, V, F, nnz = vertices.shape[0], vertices.shape[1], topo.faces.shape[0], topo.nbr_index.numel()
        dev = vertices.device
        L = _lib.lib()
        need = ctx.needs_input_grad[0]
        corner_offsets, corners = topo.corner_csr()
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        delta = torch.empty_like(vertices) if need else None
        w = torch.empty((B, nnz), dtype=torch.float32, device=dev) if need else None
        winv = torch.empty((B, V), dtype=torch.float32, device=dev) if need else None
        ws = torch.empty(L.nr_cot_laplacian_workspace_bytes(B, V, F), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.nr_cot_laplacian_forward(_lib.ptr(vertices), _lib.ptr(topo.faces), _lib.ptr(topo.nbr_offsets),
                                                  _lib.ptr(topo.nbr_index), _lib.ptr(corner_offsets), _lib.ptr(corners), B, V, F,
                                                  nnz, eps, _lib.ptr(delta), _lib.ptr(w), _lib.ptr(winv), _lib.ptr(loss),
                                                  _lib.ptr(ws), ws.numel(), _lib.stream_of(vertices)),
                       "nr_cot_laplacian_forward")
        ctx.topo = topo
        if need:
            ctx.save_for_backward(delta, w, winv)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        delta, w, winv = ctx.saved_tensors
        topo = ctx.topo
        g = grad_loss.to(torch.float32).contiguous()
        gv = torch.empty_like(delta)
        with _lib.on_device(delta.device):
            _lib.check(_lib.lib().nr_cot_laplacian_backward(_lib.ptr(delta), _lib.ptr(w), _lib.ptr(winv),
                                                            _lib.ptr(topo.nbr_offsets), _lib.ptr(topo.nbr_index), _lib.ptr(g),
                                                            delta.shape[0], delta.shape[1], w.shape[1], _lib.ptr(gv),
                                                            _lib.stream_of(delta)), "nr_cot_laplacian_backward")
        return gv, None, None


def _item_stride(t):
    """The item stride in elements of a contiguous [1 or B, ...] tensor read per item: 0 when shared."""
    return 0 if t.shape[0] == 1 else t[0].numel()


class ArapFunction(torch.autograd.Function):
    """vertices [B, V, 3], rest [1 or B, V, 3], w [1 or B, nnz] or None (uniform), float32 contiguous on the
    GPU -> loss [B] and the rotations as unit quaternions [B, V, 4] (non-differentiable).  The backward reads
    the inputs and the quaternions; only the vertices take a gradient.  With rotations=False and no gradient
    needed the quaternions are not written."""

    @staticmethod
    def forward(ctx, vertices, rest, w, topo, rotations):
        B, V, nnz = vertices.shape[0], vertices.shape[1], topo.nbr_index.numel()
        dev = vertices.device
        L = _lib.lib()
        need = ctx.needs_input_grad[0]
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        quat = torch.empty((B, V, 4), dtype=torch.float32, device=dev) if need or rotations else None
        ws = torch.empty(L.nr_arap_workspace_bytes(B, V), dtype=torch.uint8, device=dev)
        ctx.strides = (_item_stride(rest), 0 if w is None else _item_stride(w))
        with _lib.on_device(dev):
            _lib.check(L.nr_arap_forward(_lib.ptr(vertices), _lib.ptr(rest), ctx.strides[0], _lib.ptr(w), ctx.strides[1],
                                         _lib.ptr(topo.nbr_offsets), _lib.ptr(topo.nbr_index), B, V, nnz, _lib.ptr(quat),
                                         _lib.ptr(loss), _lib.ptr(ws), ws.numel(), _lib.stream_of(vertices)), "nr_arap_forward")
        ctx.topo, ctx.uniform = topo, w is None
        if need:
            ctx.save_for_backward(vertices, rest, quat, *(() if w is None else (w,)))
        if quat is None:
            quat = loss.new_empty(0)
        ctx.mark_non_differentiable(quat)
        return loss, quat

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_quat):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        vertices, rest, quat = ctx.saved_tensors[:3]
        w = None if ctx.uniform else ctx.saved_tensors[3]
        topo = ctx.topo
        g = grad_loss.to(torch.float32).contiguous()
        gv = torch.empty_like(vertices)
        with _lib.on_device(vertices.device):
            _lib.check(_lib.lib().nr_arap_backward(_lib.ptr(vertices), _lib.ptr(rest), ctx.strides[0], _lib.ptr(w), ctx.strides[1],
                                                   _lib.ptr(quat), _lib.ptr(topo.nbr_offsets), _lib.ptr(topo.nbr_index),
                                                   _lib.ptr(g), vertices.shape[0], vertices.shape[1], topo.nbr_index.numel(),
                                                   _lib.ptr(gv), _lib.stream_of(vertices)), "nr_arap_backward")
        return gv, None, None, None, None


def _cot_weights_fused(v, topo, eps):
    """w [B, nnz] of float32 contiguous GPU vertices [B, V, 3]: nr_cot_weights."""
    B, V, F, nnz = v.shape[0], v.shape[1], topo.faces.shape[0] if topo.faces is not None else 0, topo.nbr_index.numel()
    w = torch.empty((B, nnz), dtype=torch.float32, device=v.device)
    if nnz == 0:
        return w
    corner_offsets, corners = topo.corner_csr()
    L = _lib.lib()
    ws = torch.empty(L.nr_cot_weights_workspace_bytes(B, F), dtype=torch.uint8, device=v.device)
    with _lib.on_device(v.device):
        _lib.check(L.nr_cot_weights(_lib.ptr(v), _lib.ptr(topo.faces), _lib.ptr(corner_offsets), _lib.ptr(corners), B, V, F, nnz,
                                    eps, _lib.ptr(w), _lib.ptr(ws), ws.numel(), _lib.stream_of(v)), "nr_cot_weights")
    return w


def cot_weights(vertices, faces, eps=1e-12):
    """The clamped cotangent weight w_ij = max(0, sum of the half-cotangents opposite edge {i, j}) of every
    entry of the neighbour CSR, [B, nnz] for vertices [B, V, 3] ([nnz] for [V, 3]), without gradient: the
    weights cot_laplacian_loss forms, bit for bit on the fused path, and w_ij == w_ji bit for bit.  float32 GPU
    vertices run the fused kernels; everything else cot_weights_torch.  `faces` is [F, 3] or a MeshTopology
    that knows its faces; the entries are in the order of its nbr_index."""
    v, single, topo = _prepare(vertices, faces)
    v = v.detach()
    w = _cot_weights_fused(v.contiguous(), topo, float(eps)) if _fused(v) else cot_weights_torch(v, topo, eps)
    return w[0] if single else w


def _arap_fused(v, p, weights, topo, eps, rotations):
    """(loss [B], quaternions [B, V, 4] or an empty tensor) of ArapFunction for checked inputs."""
    p = p.contiguous()
    if torch.is_tensor(weights):
        w = weights.contiguous()
    else:
        w = None if weights == "uniform" else _cot_weights_fused(p, topo, float(eps))
    return ArapFunction.apply(v.contiguous(), p, w, topo, rotations)


def arap_loss(vertices, rest_vertices, faces, weights="cotangent", eps=1e-12, average=False):
    """The as-rigid-as-possible energy of the deformed `vertices` against the rest shape `rest_vertices`
    ([V, 3], shared by the items, or [B, V, 3]): with e_ij = p_i - p_j and d_ij = q_i - q_j over the
    neighbour entries of `faces`,
        S_i = sum_j w_ij e_ij d_ij^T,  R_i = the rotation (det +1) maximising tr(R S_i)  (I where S_i = 0),
        loss_b = sum_i sum_{j in N(i)} w_ij |d_ij - R_i e_ij|^2.
    `weights`: 'cotangent' (cot_laplacian_loss's clamped weights, computed on the rest shape with `eps`),
    'uniform' (1), or a float tensor [nnz] or [B, nnz] in the order of MeshTopology.nbr_index, used as given:
    the caller guarantees w_ij == w_ji.  The rotations are constants of the backward -- they maximise, so the
    gradient is exact wherever the maximiser is unique -- and neither the rest shape nor the weights take a
    gradient: the gradient reaches `vertices` only.  Shapes, dispatch, `average` and batch-expanded
    vertices as laplacian_loss; float32 GPU vertices run the fused kernels, everything else arap_loss_torch.
    ArapLoss computes the weights of a fixed rest shape once."""
    if not _fused(vertices):
        return arap_loss_torch(vertices, rest_vertices, faces, weights, eps, average)
    v, single, topo, p, weights = _arap_prepare(vertices, rest_vertices, faces, weights)
    return _finish(_arap_fused(v, p, weights, topo, eps, False)[0], single, average)


def _quaternion_matrices(q):
    """Rotation matrices [..., 3, 3] of unit quaternions [..., 4] (w, x, y, z)."""
    w, x, y, z = q.unbind(-1)
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, -1).reshape(q.shape[:-1] + (3, 3))


def arap_rotations(vertices, rest_vertices, faces, weights="cotangent", eps=1e-12):
    """The best-fitting rotation R_i of every vertex neighbourhood of arap_loss, [B, V, 3, 3] ([V, 3, 3] for
    [V, 3] vertices), without gradient: R_i e_ij is the rest edge as the deformed mesh holds it.  Arguments
    and dispatch as arap_loss."""
    if not _fused(vertices):
        return arap_rotations_torch(vertices, rest_vertices, faces, weights, eps)
    v, single, topo, p, weights = _arap_prepare(vertices, rest_vertices, faces, weights)
    R = _quaternion_matrices(_arap_fused(v.detach(), p, weights, topo, eps, True)[1])
    return R[0] if single else R


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


def edge_length_loss(vertices, faces, target_length=0.0, average=False):
    """sum over the distinct undirected edges of (|v_i - v_j| - target_length)^2 per item (divide by
    MeshTopology.num_all_edges for the mean form); target_length is a float >= 0.  Shapes, dispatch and
    gradient as laplacian_loss; an edge of length 0 takes no gradient."""
    target_length = float(target_length)
    if not target_length >= 0.:
        raise ValueError("target_length must not be negative")
    if not _fused(vertices):
        return edge_length_loss_torch(vertices, faces, target_length, average)
    v, single, topo = _prepare(vertices, faces)
    return _finish(EdgeLengthFunction.apply(v.contiguous(), topo, target_length), single, average)


def cot_laplacian_loss(vertices, faces, eps=1e-12, average=False):
    """sum_i |v_i - the cotangent-weighted mean of i's neighbours|^2 per item, the weights clamped at 0
    per edge and a vertex whose weights sum to COT_MIN_WEIGHT or less left out (the module docstring has
    the formulas).  The weights are recomputed from the vertices at every call but are constants of the
    backward: no gradient flows through them.  Shapes, dispatch and gradient as laplacian_loss; a
    MeshTopology passed as `faces` must know its faces (mesh_topology builds such a one)."""
    if not _fused(vertices):
        return cot_laplacian_loss_torch(vertices, faces, eps, average)
    v, single, topo = _prepare(vertices, faces)
    return _finish(CotLaplacianFunction.apply(v.contiguous(), topo, float(eps)), single, average)


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


class EdgeLengthLoss(torch.nn.Module):
    """edge_length_loss with the topology of `faces` held by the module."""

    def __init__(self, faces, num_vertices, target_length=0.0, average=False):
        super().__init__()
        self.topology = mesh_topology(faces, num_vertices)
        self.target_length = target_length
        self.average = average

    def forward(self, vertices):
        return edge_length_loss(vertices, self.topology, self.target_length, self.average)


class CotLaplacianLoss(torch.nn.Module):
    """cot_laplacian_loss with the topology of `faces` held by the module."""

    def __init__(self, faces, num_vertices, eps=1e-12, average=False):
        super().__init__()
        self.topology = mesh_topology(faces, num_vertices)
        self.eps = eps
        self.average = average

    def forward(self, vertices):
        return cot_laplacian_loss(vertices, self.topology, self.eps, self.average)


class ArapLoss(torch.nn.Module):
    """arap_loss against a fixed rest shape: the module holds the topology of `faces`, keeps `rest_vertices`
    ([V, 3] or [B, V, 3]) as a buffer, and forms the weights ('cotangent' with `eps`, 'uniform' or a tensor,
    as arap_loss) once per device and dtype of the vertices it is called with, at the first such call."""

    def __init__(self, rest_vertices, faces, weights="cotangent", average=False, eps=1e-12):
        super().__init__()
        if not torch.is_tensor(rest_vertices) or rest_vertices.ndim not in (2, 3) or rest_vertices.shape[-1] != 3:
            raise ValueError("rest_vertices must be a [V, 3] or [B, V, 3] tensor")
        self.topology = mesh_topology(faces, rest_vertices.shape[-2])
        self.register_buffer("rest_vertices", rest_vertices.detach().clone())
        self.weights, self.eps, self.average = weights, eps, average
        self._held = {}  # (device, dtype) -> (the buffer's version, rest shape, weights) as arap_loss takes them

    def held(self, vertices):
        """The rest shape and the weights on the device and in the dtype of `vertices`."""
        key = (vertices.device, vertices.dtype)
        hit = self._held.get(key)
        if hit is None or hit[0] != (self.rest_vertices.data_ptr(), self.rest_vertices._version):
            p = self.rest_vertices.to(device=key[0], dtype=key[1])
            w = self.weights
            if torch.is_tensor(w):
                w = w.detach().to(device=key[0], dtype=key[1])
            elif w == "cotangent":
                w = cot_weights(p, self.topology, self.eps)
            hit = self._held[key] = ((self.rest_vertices.data_ptr(), self.rest_vertices._version), p, w)
        return hit[1], hit[2]

    def forward(self, vertices):
        p, w = self.held(vertices)
        return arap_loss(vertices, p, self.topology, w, self.eps, self.average)

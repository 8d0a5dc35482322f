"""Fused camera prologue: Renderer.transform_vertices (reference renderer.py:27-38) as one HIP
launch each way (nr_camera_forward / nr_camera_backward, include/nr_raster.h) -- look_at
(look_at.py:5-44) followed by perspective (perspective.py:4-18) -- instead of the ~15 torch
launches of the composed ops and their autograd graph.

Gradients reach the vertices and the viewpoints (example4's camera fit, examples_pytorch/
example4.py:30-33).  `look` (look.py) along one constant direction runs through the same kernels.
The standalone look_at / look / perspective / projection functions stay torch ops, like the
reference's; this module is what the Renderer runs for GPU tensors.

projection_transform is the calibrated camera (projection.py: K, R, t, OpenCV distortion) fused the
same way (nr_projection_forward / nr_projection_backward), with gradients to all five inputs."""
import math

import torch

from . import _lib


def _width(angle):
    """tan(angle / 180 * 3.1416) in float32, as perspective.py:10-13 computes it."""
    a = torch.as_tensor(angle, dtype=torch.float32).detach().cpu()
    return float(torch.tan(a / 180. * 3.1416))


class _Cam:
    __slots__ = ("B", "V", "look_at", "look", "perspective", "width", "at", "up")


def _args(cfg, vertices, eye):
    c = _lib.NrCameraArgs()
    c.batch_size, c.num_vertices = cfg.B, cfg.V
    c.vertices = vertices.data_ptr()
    c.v_batch_stride = 0 if vertices.shape[0] == 1 and cfg.B > 1 else cfg.V * 3
    if cfg.look_at:
        c.eye = eye.data_ptr()
        c.eye_batch_stride = 0 if eye.shape[0] == 1 else 3
        c.mode = _lib.NR_CAMERA_LOOK if cfg.look else _lib.NR_CAMERA_LOOK_AT
    else:
        c.mode = _lib.NR_CAMERA_NONE
    for j in range(3):
        c.at[j], c.up[j] = cfg.at[j], cfg.up[j]
    c.perspective = int(cfg.perspective)
    c.width = cfg.width
    return c


class CameraTransform(torch.autograd.Function):
    """vertices [1 or B, V, 3] (world), eye [1 or B, 3] -> projected vertices [B, V, 3]."""

    @staticmethod
    def forward(ctx, vertices, eye, cfg):
        out = torch.empty((cfg.B, cfg.V, 3), dtype=torch.float32, device=vertices.device)
        c = _args(cfg, vertices, eye)
        with torch.cuda.device(vertices.device):
            _lib.check(_lib.lib().nr_camera_forward(c, _lib.ptr(out), _lib.stream_of(vertices)), "nr_camera_forward")
        ctx.cfg = cfg
        ctx.save_for_backward(vertices, eye)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        vertices, eye = ctx.saved_tensors
        cfg = ctx.cfg
        grad_out = grad_out.contiguous()
        dev = vertices.device
        gv = torch.empty_like(vertices) if ctx.needs_input_grad[0] else None
        ge = torch.empty_like(eye) if (ctx.needs_input_grad[1] and cfg.look_at) else None
        L = _lib.lib()
        ws = torch.empty(L.nr_camera_workspace_bytes(cfg.B) if ge is not None else 0, dtype=torch.uint8, device=dev)
        c = _args(cfg, vertices, eye)
        with torch.cuda.device(dev):
            _lib.check(L.nr_camera_backward(c, _lib.ptr(grad_out), _lib.ptr(gv), _lib.ptr(ge), _lib.ptr(ws), ws.numel(),
                                            _lib.stream_of(vertices)), "nr_camera_backward")
        return gv, ge, None


def camera_transform(vertices, viewpoints=None, perspective=True, angle=30., at=None, up=None, direction=None):
    """look_at(vertices, viewpoints, at, up) (when viewpoints is given) then, with `perspective`,
    perspective(., angle): the result of the reference's composition, fused on the GPU.
    vertices [B, V, 3] (a batch-expanded view is read once); viewpoints [3], [1, 3] or [B, 3].
    With `direction` (one constant 3-vector, no gradient) the camera is look(vertices, viewpoints,
    direction, up) instead of look_at, and `at` is not used."""
    assert vertices.ndim == 3
    if direction is not None and viewpoints is None:
        raise ValueError("direction needs viewpoints")
    _lib.require_gpu(vertices)
    dev = vertices.device
    cfg = _Cam()
    cfg.B, cfg.V = vertices.shape[0], vertices.shape[1]
    v = vertices.float()
    if v.shape[0] > 1 and v.stride(0) == 0:
        v = v[:1]  # one mesh for every item: read once, gradient summed over the items
    v = v.contiguous()
    cfg.look_at = viewpoints is not None
    cfg.look = direction is not None
    cfg.perspective = bool(perspective)
    cfg.width = _width(angle) if perspective else 1.0
    cfg.at = [0., 0., 0.] if at is None else [float(x) for x in torch.as_tensor(at, dtype=torch.float32).reshape(3)]
    if cfg.look:  # NrCameraArgs.at carries the direction
        cfg.at = [float(x) for x in torch.as_tensor(direction, dtype=torch.float32).detach().reshape(3)]
    cfg.up = [0., 1., 0.] if up is None else [float(x) for x in torch.as_tensor(up, dtype=torch.float32).reshape(3)]
    if cfg.look_at:
        eye = viewpoints if torch.is_tensor(viewpoints) else torch.as_tensor(viewpoints, dtype=torch.float32)
        eye = eye.float().to(dev).reshape(-1, 3)
        if eye.shape[0] not in (1, cfg.B):
            raise AssertionError("viewpoints batch must be 1 or %d" % cfg.B)
        if eye.shape[0] > 1 and eye.stride(0) == 0:
            eye = eye[:1]
        eye = eye.contiguous()
    else:
        eye = torch.zeros((1, 3), dtype=torch.float32, device=dev)
    return CameraTransform.apply(v, eye, cfg)


def fusable(vertices, angle):
    """The fused path covers GPU float tensors whose viewing angle takes no gradient."""
    return (torch.is_tensor(vertices) and vertices.is_cuda and vertices.ndim == 3 and
            not (torch.is_tensor(angle) and angle.requires_grad) and
            (not torch.is_tensor(angle) or angle.numel() == 1) and not math.isnan(_width(angle)))


def look_fusable(direction):
    """The fused 'look' covers one constant direction: a 3-vector that takes no gradient."""
    if torch.is_tensor(direction):
        return direction.numel() == 3 and not direction.requires_grad
    try:
        return torch.as_tensor(direction, dtype=torch.float32).numel() == 3
    except (TypeError, ValueError, RuntimeError):
        return False


# ---- calibrated camera: projection.projection fused (nr_projection_forward / nr_projection_backward) ----
class _Proj:
    __slots__ = ("B", "V", "orig_size", "eps")


def _proj_args(cfg, vertices, K, R, t, dist):
    def stride(x, n):
        return 0 if x.shape[0] == 1 and cfg.B != 1 else n

    p = _lib.NrProjectionArgs()
    p.batch_size, p.num_vertices = cfg.B, cfg.V
    p.vertices, p.v_batch_stride = vertices.data_ptr(), stride(vertices, cfg.V * 3)
    p.K, p.k_batch_stride = K.data_ptr(), stride(K, 9)
    p.R, p.r_batch_stride = R.data_ptr(), stride(R, 9)
    p.t, p.t_batch_stride = t.data_ptr(), stride(t, 3)
    if dist is not None:
        p.dist, p.dist_batch_stride = dist.data_ptr(), stride(dist, 5)
    p.orig_size, p.eps = cfg.orig_size, cfg.eps
    return p


class ProjectionTransform(torch.autograd.Function):
    """vertices [1 or B, V, 3], K / R [1 or B, 3, 3], t [1 or B, 3], dist [1 or B, 5] or None
    -> projected vertices [B, V, 3].  A leading 1 (at B > 1) is shared by every item."""

    @staticmethod
    def forward(ctx, vertices, K, R, t, dist, cfg):
        out = torch.empty((cfg.B, cfg.V, 3), dtype=torch.float32, device=vertices.device)
        p = _proj_args(cfg, vertices, K, R, t, dist)
        with _lib.on_device(vertices.device):
            _lib.check(_lib.lib().nr_projection_forward(p, _lib.ptr(out), _lib.stream_of(vertices)),
                       "nr_projection_forward")
        ctx.cfg = cfg
        ctx.has_dist = dist is not None
        ctx.save_for_backward(*((vertices, K, R, t) + ((dist,) if dist is not None else ())))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        vertices, K, R, t = saved[:4]
        dist = saved[4] if ctx.has_dist else None
        cfg = ctx.cfg
        grad_out = grad_out.contiguous()
        dev = vertices.device
        need = ctx.needs_input_grad
        gv, gK, gR, gt = [torch.empty_like(x) if n else None for x, n in zip((vertices, K, R, t), need[:4])]
        gd = torch.empty_like(dist) if (need[4] and dist is not None) else None
        L = _lib.lib()
        params = any(g is not None for g in (gK, gR, gt, gd))
        ws = torch.empty(L.nr_projection_workspace_bytes(cfg.B, cfg.V) if params else 0, dtype=torch.uint8, device=dev)
        p = _proj_args(cfg, vertices, K, R, t, dist)
        with _lib.on_device(dev):
            _lib.check(L.nr_projection_backward(p, _lib.ptr(grad_out), _lib.ptr(gv), _lib.ptr(gK), _lib.ptr(gR), _lib.ptr(gt),
                                                _lib.ptr(gd), _lib.ptr(ws), ws.numel(), _lib.stream_of(vertices)),
                       "nr_projection_backward")
        return gv, gK, gR, gt, gd, None


def _proj_param(x, name, tail, B, dev):
    """x as a contiguous float32 [1 or B, *tail] tensor on dev; a batch-expanded view becomes its one
    record (autograd sums the items back through the slice of the expand)."""
    if not torch.is_tensor(x):
        x = torch.as_tensor(x, dtype=torch.float32)
    x = x.to(device=dev, dtype=torch.float32)
    if x.ndim == len(tail):
        x = x[None]
    if x.ndim == len(tail) + 1 and x.shape[0] > 1 and x.stride(0) == 0:
        x = x[:1]
    if tuple(x.shape[1:]) != tuple(tail) or x.shape[0] not in (1, B):
        raise ValueError("%s must be a [%d or 1, %s] tensor, got %s" % (name, B, ", ".join(map(str, tail)), list(x.shape)))
    return x.contiguous()


def projection_transform(vertices, K, R, t, dist_coeffs=None, orig_size=1024, eps=1e-9):
    """projection.projection(vertices, K, R, t, dist_coeffs, orig_size, eps) fused on the GPU: one HIP
    launch forward, two backward.  Gradients reach vertices, K, R, t and dist_coeffs (each only when it
    requires one).  A batch-expanded mesh is read once and receives the item sum; parameters with a
    leading dimension of 1, or batch-expanded, are shared by the items and receive the item sum.  The
    parameter gradients are summed in a fixed order (no atomics): the same bits on every run."""
    assert vertices.ndim == 3
    _lib.require_gpu(vertices)
    dev = vertices.device
    cfg = _Proj()
    cfg.B, cfg.V = vertices.shape[0], vertices.shape[1]
    cfg.orig_size, cfg.eps = float(orig_size), float(eps)
    if not cfg.orig_size > 0:
        raise ValueError("orig_size must be positive, got %r" % (orig_size,))
    v = vertices.float()
    if v.shape[0] > 1 and v.stride(0) == 0:
        v = v[:1]  # one mesh for every item: read once, gradient summed over the items
    v = v.contiguous()
    if torch.is_tensor(t) and t.ndim == 3 and t.shape[1:] == (1, 3):
        t = t[:, 0]
    K = _proj_param(K, "K", (3, 3), cfg.B, dev)
    R = _proj_param(R, "R", (3, 3), cfg.B, dev)
    t = _proj_param(t, "t", (3,), cfg.B, dev)
    dist = None if dist_coeffs is None else _proj_param(dist_coeffs, "dist_coeffs", (5,), cfg.B, dev)
    return ProjectionTransform.apply(v, K, R, t, dist, cfg)


def projection_fusable(vertices, K, R, t, dist_coeffs=None, orig_size=1024, eps=1e-9):
    """The fused projection covers float32 GPU vertices with scalar orig_size and eps that take no
    gradient (K, R, t and dist_coeffs are converted to float32 on the vertices' device)."""
    def const(x):
        return not (torch.is_tensor(x) and (x.requires_grad or x.numel() != 1))
    return (torch.is_tensor(vertices) and vertices.is_cuda and vertices.ndim == 3 and
            vertices.dtype == torch.float32 and
            all(x is not None for x in (K, R, t)) and const(orig_size) and const(eps))

"""Rigid registration of point sets: the frame a scan and a template share, found before the non-rigid terms
(point_mesh_distance, mesh_point_distance, arap_loss) are of any use.  Two functions, each a fused HIP launch
sequence (nr_rigid_align_* / nr_icp, include/nr_raster.h, csrc/nr_rigid.h) for float32 GPU tensors and a torch
composition (rigid_align_torch / icp_torch) for every other device and dtype; the compositions are the tests'
reference and the baseline of tools/bench_rigid.py.

rigid_align(x, y, weights, scale): the weighted least-squares similarity between corresponding points, the
minimiser of sum_i w_i |s R x_i + t - y_i|^2 over proper rotations R (det +1, never a reflection), t, and s when
scale=True (s = 1 otherwise):

    W = sum w,   xbar = sum w x / W,   ybar = sum w y / W
    A = sum w (y - ybar) (x - xbar)^T,   var = sum w |x - xbar|^2
    R = argmax tr(R^T A),   s = tr(R^T A) / var,   t = ybar - s R xbar

W == 0 gives R = I, t = 0, s = 1; A == 0 (one point, coincident points) gives R = I; var == 0 gives s = 1; where
the maximiser is not unique (collinear points, N = 2) any maximiser is returned, orthonormal with det +1.
Everything is finite in all of these.  condition = (s2 + d s3) / s1 of A's singular values, d = sign det A,
tells where the rotation is well determined: near 0 it is not.

The gradient reaches x and y from the gradients of R, t and s in closed form (no SVD, no iteration; the
formulas are in include/nr_raster.h).  Where condition <= NR_RIGID_MIN_CONDITION the rotation passes no
gradient and everything stays finite.  The weights take no gradient on the fused path: a call whose weights
require one runs the composition.  The fused path uses no float atomics and sums in fixed orders: R, t, s,
condition and both gradients are bitwise reproducible, and an item's results do not depend on its batch.

icp(x, y, iterations, ...): point-to-point ICP of x onto y.  Exactly `iterations` updates, no early exit and
no host synchronisation, so a call captures into a HIP graph.  Update k finds the nearest y of every
s R x_i + t (the lowest index among exact ties, as nearest_points) and sets (R, t, s) = rigid_align(x, y[index], w)
of the ORIGINAL x: the total transform is estimated directly, nothing is composed and no drift accumulates.
w_i = 1, or 0 where dist2_i > max_distance^2; an update that keeps no pair leaves the transform as it was.  A
last pass gives index and dist2 under the returned transform.  All outputs are detached: for gradients call
rigid_align on y[index].  Against a mesh surface, closest_points_on_mesh plus rigid_align composes the same
loop by hand."""
import collections

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .point_loss import _dense_y, _fused, _nearest_torch, _prepare_sets, _y_stride

NR_RIGID_MIN_CONDITION = _lib.NR_RIGID_MIN_CONDITION

ICPResult = collections.namedtuple("ICPResult", ["R", "t", "s", "rmse", "index", "dist2"])
ICPResult.__doc__ = """icp's result: R [B, 3, 3], t [B, 3], s [B] with y ~ s R x + t; rmse [B, iterations + 1], entry k the
root of the weighted mean squared nearest distance of pass k (0 where no pair was kept); index [B, N] int32 and
dist2 [B, N], the nearest y of every transformed x under the returned transform.  Unbatched for an [N, 3] x."""


def _prepare_pairs(x, y, weights):
    """x as [B, N, 3], y as [B, N, 3] or a shared [N, 3], weights as [B, N], a shared [N] or None, and whether x was
    a single [N, 3] set."""
    xb, y, single = _prepare_sets(x, y)
    B, N = xb.shape[0], xb.shape[1]
    if y.shape[-2] != N:
        raise ValueError("corresponding points: x has %d points, y has %d" % (N, y.shape[-2]))
    if weights is not None:
        if not torch.is_tensor(weights) or tuple(weights.shape) not in ((B, N), (N,)):
            raise ValueError("weights must be [B, N] = [%d, %d] or [N], got %s" % (B, N, tuple(getattr(weights, "shape", ()))))
    return xb, y, weights, single


def _result(out, single, return_condition):
    out = out if return_condition else out[:3]
    return tuple(o[0] for o in out) if single else tuple(out)


# ---- the torch composition: reference of the tests, baseline of tools/bench_rigid.py ----
def _align_torch(x, y, w, scale):
    """x, y [B, N, 3], w [B, N] -> R, t, s, condition."""
    B = x.shape[0]
    eye = torch.eye(3, dtype=x.dtype, device=x.device).expand(B, 3, 3)
    W = w.sum(1)
    any_w = W > 0
    Ws = torch.where(any_w, W, torch.ones_like(W))[:, None]
    # centred as the kernels centre: the sums relative to the first pair, so that coincident points centre to exact
    # zeros and a cloud far from the origin loses nothing
    dx, dy = x - x[:, :1], y - y[:, :1]
    cx, cy = (w[..., None] * dx).sum(1) / Ws, (w[..., None] * dy).sum(1) / Ws
    xc, yc = dx - cx[:, None], dy - cy[:, None]
    xbar, ybar = x[:, 0] + cx, y[:, 0] + cy
    A = torch.einsum("bn,bni,bnj->bij", w, yc, xc)
    var = (w * (xc * xc).sum(-1)).sum(1)
    flat = (A == 0).reshape(B, 9).all(1) | ~any_w
    U, S, Vh = torch.linalg.svd(torch.where(flat[:, None, None], eye, A))
    d = torch.sign(torch.linalg.det(U @ Vh))
    D = torch.stack([torch.ones_like(d), torch.ones_like(d), d], 1)
    R = torch.where(flat[:, None, None], eye, (U * D[:, None, :]) @ Vh)
    S = torch.where(flat[:, None], torch.zeros_like(S), S)
    top = torch.where(flat, torch.ones_like(W), S[:, 0])
    condition = torch.where(flat, torch.zeros_like(W), (S[:, 1] + d * S[:, 2]) / top)
    scaled = any_w & (var > 0) if scale else torch.zeros_like(any_w)
    s = torch.where(scaled, (S * D).sum(1) / torch.where(scaled, var, torch.ones_like(var)), torch.ones_like(W))
    t = ybar - s[:, None] * (R @ xbar[..., None])[..., 0]
    t = torch.where(any_w[:, None], t, torch.zeros_like(t))
    return R, t, s, condition


def rigid_align_torch(x, y, weights=None, scale=False, return_condition=False):
    """rigid_align as torch ops (centre, einsum, torch.linalg.svd, determinant fix), differentiable by autograd,
    the weights included; any device and floating dtype."""
    xb, y, w, single = _prepare_pairs(x, y, weights)
    B, N = xb.shape[0], xb.shape[1]
    yb = y if y.ndim == 3 else y[None].expand(B, -1, -1)
    w = torch.ones((B, N), dtype=xb.dtype, device=xb.device) if w is None else w.to(xb.dtype).expand(B, N)
    return _result(_align_torch(xb, yb, w, scale), single, return_condition)


# ---- the fused path ----
def _w_stride(w):
    return 0 if w.ndim == 1 else w.shape[1]


class RigidAlignFunction(torch.autograd.Function):
    """x [B, N, 3] float32 contiguous on the GPU, y as _dense_y gives it, w [B, N] or [N] contiguous or None ->
    R [B, 3, 3], t [B, 3], s [B], condition [B]; saves the inputs and the forward's per-item record."""

    @staticmethod
    def forward(ctx, x, y, w, scale):
        B, N = x.shape[0], x.shape[1]
        dev = x.device
        L = _lib.lib()
        R = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
        t = torch.empty((B, 3), dtype=torch.float32, device=dev)
        s = torch.empty(B, dtype=torch.float32, device=dev)
        condition = torch.empty(B, dtype=torch.float32, device=dev)
        record = torch.empty((B, _lib.NR_RIGID_RECORD_FLOATS), dtype=torch.float32, device=dev)
        ws = torch.empty(L.nr_rigid_workspace_bytes(B, N), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.nr_rigid_align_forward(_lib.ptr(x), _lib.ptr(y), _y_stride(y), _lib.ptr(w), 0 if w is None else _w_stride(w),
                                                B, N, int(scale), _lib.ptr(R), _lib.ptr(t), _lib.ptr(s), _lib.ptr(condition),
                                                _lib.ptr(record), _lib.ptr(ws), ws.numel(), _lib.stream_of(x)),
                       "nr_rigid_align_forward")
        ctx.scale = int(scale)
        ctx.mark_non_differentiable(condition)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(x, y, w, record)
        return R, t, s, condition

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_R, grad_t, grad_s, _grad_condition):
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_y):
            return None, None, None, None
        x, y, w, record = ctx.saved_tensors
        B, N = x.shape[0], x.shape[1]
        if need_y and y.ndim == 2:
            raise RuntimeError("a shared y that takes a gradient must be passed batch-expanded")
        gR, gt, gs = (None if g is None else g.to(torch.float32).contiguous() for g in (grad_R, grad_t, grad_s))
        gx = torch.empty_like(x) if need_x else None
        gy = torch.empty((B, N, 3), dtype=torch.float32, device=x.device) if need_y else None
        L = _lib.lib()
        ws = torch.empty(L.nr_rigid_workspace_bytes(B, N), dtype=torch.uint8, device=x.device)
        with _lib.on_device(x.device):
            _lib.check(L.nr_rigid_align_backward(_lib.ptr(x), _lib.ptr(y), _y_stride(y), _lib.ptr(w), 0 if w is None else _w_stride(w),
                                                 _lib.ptr(record), _lib.ptr(gR), _lib.ptr(gt), _lib.ptr(gs), B, N, ctx.scale,
                                                 _lib.ptr(gx), _lib.ptr(gy), _lib.ptr(ws), ws.numel(), _lib.stream_of(x)),
                       "nr_rigid_align_backward")
        return gx, gy, None, None


def rigid_align(x, y, weights=None, scale=False, return_condition=False):
    """The similarity (R, t, s) that takes x onto its corresponding points y in the weighted least-squares sense,
    y ~ s R x + t: R [B, 3, 3] a proper rotation, t [B, 3], s [B] (1 unless scale=True), for x [B, N, 3]; unbatched
    for [N, 3].  y is [B, N, 3], or [N, 3]: alone with a single x, shared by every item of a batched one (read in
    place; expanded only when it takes a gradient, so that torch's expand backward sums the items).  weights are
    [B, N] or [N], non-negative and used as given, or None.  With return_condition=True a fourth output,
    condition [B] (module docstring; detached).  N = 0 and differing sizes raise ValueError; the inputs are taken to
    be finite.  The corner cases (no weight, coincident or collinear points) are the module docstring's.
    float32 GPU tensors whose weights take no gradient run the fused kernels; everything else
    rigid_align_torch.  The gradient reaches x and, if it requires one, y."""
    if not _fused(x, y) or (weights is not None and (not _fused(x, weights) or (weights.requires_grad and torch.is_grad_enabled()))):
        return rigid_align_torch(x, y, weights, scale, return_condition)
    xb, y, w, single = _prepare_pairs(x, y, weights)
    if y.ndim == 2 and y.requires_grad and torch.is_grad_enabled():
        y = y[None].expand(xb.shape[0], -1, -1)
    out = RigidAlignFunction.apply(xb.contiguous(), _dense_y(y), None if w is None else w.detach().contiguous(), bool(scale))
    return _result(out, single, return_condition)


# ---- ICP ----
def _prepare_icp(x, y, iterations, max_distance, init):
    xb, y, single = _prepare_sets(x, y)
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("iterations must be at least 0, got %d" % iterations)
    if max_distance is not None:
        max_distance = float(max_distance)
        if not max_distance >= 0:
            raise ValueError("max_distance must be non-negative, got %r" % (max_distance,))
    B, dev, dt = xb.shape[0], xb.device, xb.dtype
    if init is None:
        R = torch.eye(3, dtype=dt, device=dev).expand(B, 3, 3)
        t, s = torch.zeros((B, 3), dtype=dt, device=dev), torch.ones(B, dtype=dt, device=dev)
    else:
        try:
            R, t, s = (torch.as_tensor(v, dtype=dt, device=dev).detach() for v in init)
            R, t, s = R.expand(B, 3, 3), t.expand(B, 3), s.expand(B)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError("init must be (R [B, 3, 3], t [B, 3], s [B]) or their unbatched forms") from None
    return xb, y, single, iterations, max_distance, (R, t, s)


def _icp_result(R, t, s, rmse, index, dist2, single):
    out = (R, t, s, rmse, index, dist2)
    return ICPResult(*(o[0] for o in out)) if single else ICPResult(*out)


def icp_torch(x, y, iterations=20, scale=False, max_distance=None, init=None):
    """icp as torch ops: nearest_points_torch's chunked search, a gather and rigid_align_torch per update; any device
    and floating dtype, the same outputs (detached)."""
    xb, y, single, iterations, max_distance, (R, t, s) = _prepare_icp(x, y, iterations, max_distance, init)
    with torch.no_grad():
        xb = xb.detach()
        B = xb.shape[0]
        yb = (y if y.ndim == 3 else y[None].expand(B, -1, -1)).detach()
        rmse = []
        for k in range(iterations + 1):
            q = s[:, None, None] * (xb @ R.transpose(1, 2)) + t[:, None]
            dist2, index = _nearest_torch(q, yb)
            w = torch.ones_like(dist2) if max_distance is None else (~(dist2 > max_distance * max_distance)).to(dist2.dtype)
            W = w.sum(1)
            kept = W > 0
            rmse.append(torch.where(kept, torch.sqrt((w * dist2).sum(1) / torch.where(kept, W, torch.ones_like(W))), torch.zeros_like(W)))
            if k == iterations:
                break
            Rn, tn, sn, _ = _align_torch(xb, yb.gather(1, index[..., None].expand(-1, -1, 3)), w, scale)
            R, t, s = torch.where(kept[:, None, None], Rn, R), torch.where(kept[:, None], tn, t), torch.where(kept, sn, s)
    return _icp_result(R, t, s, torch.stack(rmse, 1), index.to(torch.int32), dist2, single)


def icp(x, y, iterations=20, scale=False, max_distance=None, init=None):
    """Point-to-point ICP of x [B, N, 3] (or [N, 3]) onto y ([B, M, 3], or [M, 3] alone or shared): an ICPResult
    (R, t, s, rmse, index, dist2) with y ~ s R x + t.  Exactly `iterations` updates (module docstring), each the
    nearest y of every transformed x, then rigid_align of the original x onto them; scale=True also estimates s.
    max_distance drops the pairs farther apart than that from the update (the usual rejection for partial
    overlap); an update that keeps none leaves the transform as it was.  init = (R, t, s) is the start, the
    identity by default.  rmse [B, iterations + 1] is the convergence history; index [B, N] int32 and dist2 [B, N]
    belong to the returned transform.  iterations=0 returns init and that one evaluation.

    No gradient: every output is detached, like nearest_points; for one, call rigid_align(x, y[index]).  N = 0,
    M = 0, iterations < 0, differing batch sizes and a negative max_distance raise ValueError.  float32 GPU
    tensors run the fused kernels (nr_icp), with no host synchronisation; everything else icp_torch."""
    if not _fused(x, y):
        return icp_torch(x, y, iterations, scale, max_distance, init)
    xb, y, single, iterations, max_distance, (R, t, s) = _prepare_icp(x, y, iterations, max_distance, init)
    B, N, M = xb.shape[0], xb.shape[1], y.shape[-2]
    dev = xb.device
    L = _lib.lib()
    with torch.no_grad():
        xb, y = xb.detach().contiguous(), _dense_y(y.detach())
        transform = torch.cat([R.reshape(B, 9), t, s[:, None]], 1).contiguous()
        rmse = torch.empty((B, iterations + 1), dtype=torch.float32, device=dev)
        index = torch.empty((B, N), dtype=torch.int32, device=dev)
        dist2 = torch.empty((B, N), dtype=torch.float32, device=dev)
        ws = torch.empty(L.nr_icp_workspace_bytes(B, N, M), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.nr_icp(_lib.ptr(xb), _lib.ptr(y), _y_stride(y), B, N, M, iterations, int(bool(scale)),
                                -1. if max_distance is None else max_distance, _lib.ptr(transform), _lib.ptr(rmse), _lib.ptr(index),
                                _lib.ptr(dist2), _lib.ptr(ws), ws.numel(), _lib.stream_of(xb)), "nr_icp")
        R, t, s = transform[:, :9].reshape(B, 3, 3), transform[:, 9:12], transform[:, 12]
    return _icp_result(R, t, s, rmse, index, dist2, single)

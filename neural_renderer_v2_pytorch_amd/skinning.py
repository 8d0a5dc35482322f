"""Articulated meshes: forward kinematics of a joint tree (pose_transforms) and linear blend skinning
(skin_vertices), each one fused HIP launch forward (nr_pose_transforms_* / nr_skin_*, include/nr_raster.h) for
float32 GPU tensors, and a torch composition (*_torch) for every other device and dtype.  With them a rigged
model -- a body, a hand, an animal, any mesh with a skeleton and skinning weights -- is fitted to silhouettes,
keypoints or a scan with every operation of the step a fused kernel; Skinning holds a rig as a module.

Definitions (the compositions and the kernels both follow them):

  Skeleton.  parents [J] integers: -1 marks a root (several are allowed), any other value is a joint index in
             [0, J).  A cycle or an index out of range is a ValueError; J <= NR_SKIN_MAX_JOINTS = 256.  Joints
             need not be listed parents-first.
  Rotation.  pose is [B, J, 3] axis-angle or [B, J, 3, 3] matrices (used as given, not orthonormalised).  For an
             axis-angle r:  t2 = |r|^2, K = skew(r), R = I + a K + b K^2, a = sin(t) / t, b = (1 - cos t) / t^2 with
             t = sqrt(t2); where t2 < NR_RODRIGUES_SERIES = 1e-4, a = 1 - t2/6 + t2^2/120 and
             b = 1/2 - t2/24 + t2^2/720 (the truncation error at the switch is about 2e-16).  R and its gradient
             are defined at r = 0, and nothing depends on an eps inside a norm.
  Chain.     c_j is the rest position of joint j: joints [J, 3] (shared) or [B, J, 3].  d_j = c_j - c_parent(j),
             for a root d_j = c_j.  World rotation G_j.R = G_p.R R_j (root: R_j), world translation
             G_j.t = G_p.t + G_p.R d_j (root: d_j).  posed_joints[b, j] = G_j.t, and
             transforms[b, j] = [G_j.R | G_j.t - G_j.R c_j], [B, J, 3, 4] row-major: it takes a rest-pose point to
             its posed place.
  Skinning.  out[b, v] = sum_k w[v, k] (A.R x + A.t) with A = transforms[b, idx[v, k]] and x = vertices[b or
             shared, v]; K <= NR_SKIN_MAX_INFLUENCES = 8.  Weights are used as given, not normalised.  A slot of
             weight 0 is padding (its index must still be in range); a vertex whose weights are all 0 maps to 0.

Learned weights.  The host-built SkinBinding (topology.py) holds the structure the transform gradient walks: which
slots have a non-zero weight, per joint.  It is looked up by the (storage, version) of the weights tensor, so it is
rebuilt -- one device-to-host copy -- only after the tensor was edited in place (an optimiser's step), and a
steady-state call with fixed weights is one key and one lookup.  The weight *values* the kernels read never come
from that snapshot when the caller's tensor is a leaf being learned: [V, K] weights are passed to the kernels as
they are (the caller's own storage), and a dense [V, J] matrix that requires grad is gathered into [V, K] by torch
ops at every call, so its gradient is scattered back to [V, J] by autograd, on the kept (non-zero) slots only.  A
SkinBinding passed as `weights` is a constant: its own values are used and take no gradient.

What misses the cache.  The lookup needs the same storage at the same version, so it serves leaves.  Weights that
are computed every step -- softmax(logits), a normalised or masked copy -- are a new tensor each time: every call
then pays the device-to-host copy and the host-side rebuild (a synchronisation, so such a step cannot be captured
in a HIP graph), and the cache keeps its last 8 such tensors alive.  The same holds for a weights tensor passed
with indices that are not a tensor (an array or a list is never cached): keep the indices a tensor.  Such weights
are correct, only slower per step than a leaf; the torch composition skin_vertices_torch needs no binding at all.

The fused kernels use no float atomics: outputs and gradients are bitwise identical from run to run, and an
item's results do not depend on the batch it is in."""
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .topology import Skeleton, SkinBinding, skeleton, skin_binding

NR_SKIN_MAX_JOINTS, NR_SKIN_MAX_INFLUENCES = _lib.NR_SKIN_MAX_JOINTS, _lib.NR_SKIN_MAX_INFLUENCES
NR_SKIN_CHUNK, NR_RODRIGUES_SERIES = _lib.NR_SKIN_CHUNK, _lib.NR_RODRIGUES_SERIES


# ---- the torch composition: reference of the tests, baseline of tools/bench_skinning.py ----
def rodrigues_torch(r):
    """Rotation matrices [..., 3, 3] of axis-angle vectors r [..., 3] as torch ops; any device and floating
    dtype.  Both branches run on values safe for them (`where` before and after), so neither poisons the
    other's gradient, and the gradient at r = 0 is the series'."""
    if not torch.is_tensor(r) or r.shape[-1:] != (3,):
        raise ValueError("r must be a [..., 3] tensor")
    t2 = (r * r).sum(-1)
    small = t2 < NR_RODRIGUES_SERIES
    big = torch.where(small, torch.ones_like(t2), t2)
    t = torch.sqrt(big)
    half = torch.sin(0.5 * t)
    a_closed, b_closed = torch.sin(t) / t, 2 * half * half / big
    s = torch.where(small, t2, torch.zeros_like(t2))
    a = torch.where(small, 1 - s / 6 + s * s / 120, a_closed)[..., None]
    b = torch.where(small, 0.5 - s / 24 + s * s / 720, b_closed)[..., None]
    x, y, z = r.unbind(-1)
    xx, yy, zz = x * x, y * y, z * z
    zero = torch.zeros_like(x)
    K = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1)
    K2 = torch.stack([-(yy + zz), x * y, x * z, x * y, -(xx + zz), y * z, x * z, y * z, -(xx + yy)], -1)
    eye = torch.eye(3, dtype=r.dtype, device=r.device).reshape(9)
    return (eye + a * K + b * K2).reshape(r.shape[:-1] + (3, 3))


def _check_pose(pose, joints, skel):
    """(B, whether the pose is matrices, whether the joints are shared)."""
    J = skel.num_joints
    if not torch.is_tensor(pose) or pose.ndim not in (3, 4) or tuple(pose.shape[1:]) not in ((J, 3), (J, 3, 3)):
        raise ValueError("pose must be [B, %d, 3] axis-angle or [B, %d, 3, 3] matrices, got %s"
                         % (J, J, list(pose.shape) if torch.is_tensor(pose) else type(pose).__name__))
    B = pose.shape[0]
    if not torch.is_tensor(joints) or tuple(joints.shape) not in ((J, 3), (B, J, 3)):
        raise ValueError("joints must be [%d, 3] or [%d, %d, 3], got %s"
                         % (J, B, J, list(joints.shape) if torch.is_tensor(joints) else type(joints).__name__))
    return B, pose.ndim == 4, joints.ndim == 2


def pose_transforms_torch(pose, joints, parents):
    """pose_transforms as torch ops -- a Python loop over the joints, parents first -- on any device and floating
    dtype: the reference of the tests and what a user writes without this module."""
    skel = skeleton(parents)
    B, is_matrix, _ = _check_pose(pose, joints, skel)
    R = pose if is_matrix else rodrigues_torch(pose)
    c = (joints[None].expand(B, -1, -1) if joints.ndim == 2 else joints).to(R.dtype)
    GR, Gt = [None] * skel.num_joints, [None] * skel.num_joints
    for j in skel.order:
        p = skel.parent_list[j]
        if p < 0:
            GR[j], Gt[j] = R[:, j], c[:, j]
        else:
            GR[j] = GR[p] @ R[:, j]
            Gt[j] = Gt[p] + (GR[p] @ (c[:, j] - c[:, p])[..., None])[..., 0]
    GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)
    At = Gt - (GR @ c[..., None])[..., 0]
    return torch.cat([GR, At[..., None]], -1), Gt


def _check_skin(vertices, transforms):
    """(B, V, J, whether the vertices are shared)."""
    if not torch.is_tensor(transforms) or transforms.ndim != 4 or tuple(transforms.shape[2:]) != (3, 4):
        raise ValueError("transforms must be a [B, J, 3, 4] tensor")
    B, J = transforms.shape[0], transforms.shape[1]
    if not torch.is_tensor(vertices) or vertices.ndim not in (2, 3) or vertices.shape[-1] != 3 or (
            vertices.ndim == 3 and vertices.shape[0] != B):
        raise ValueError("vertices must be [V, 3] or [%d, V, 3]" % B)
    return B, vertices.shape[-2], J, vertices.ndim == 2


def _check_weights(weights, indices, V, J):
    if isinstance(weights, SkinBinding):
        if indices is not None:
            raise ValueError("a SkinBinding carries its own indices")
        if weights.num_vertices != V or weights.num_joints != J:
            raise ValueError("the binding was built for %d vertices and %d joints, got %d and %d"
                             % (weights.num_vertices, weights.num_joints, V, J))
        return
    if not torch.is_tensor(weights) or weights.ndim != 2 or weights.shape[0] != V:
        raise ValueError("weights must be [%d, J] dense, [%d, K] with indices, or a SkinBinding" % (V, V))
    if indices is None:
        if weights.shape[1] != J:
            raise ValueError("dense weights must be [%d, %d], got %s" % (V, J, list(weights.shape)))
    elif not torch.is_tensor(indices) or indices.shape != weights.shape or indices.dtype.is_floating_point:
        raise ValueError("indices must be an integer tensor of the weights' shape %s" % list(weights.shape))


def skin_vertices_torch(vertices, transforms, weights, indices=None):
    """skin_vertices as torch ops on any device and floating dtype.  Dense [V, J] weights blend the transforms
    first (einsum 'vj,bjrc->bvrc': the [B, V, 3, 4] intermediate a user writes today); [V, K] weights with indices,
    or a SkinBinding, transform the vertex by each influence and blend the points."""
    B, V, J, shared = _check_skin(vertices, transforms)
    _check_weights(weights, indices, V, J)
    x = (vertices[None].expand(B, -1, -1) if shared else vertices).to(transforms.dtype)
    if isinstance(weights, SkinBinding):
        weights = weights.to(transforms.device)
        weights, indices = weights.weights, weights.indices
    w = weights.to(transforms.dtype)
    if indices is None:
        T = torch.einsum('vj,bjrc->bvrc', w, transforms)
        return (T[..., :3] @ x[..., None])[..., 0] + T[..., 3]
    idx = indices.long()
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= J):
        raise ValueError("indices out of range [0, %d)" % J)
    A = transforms[:, idx]  # [B, V, K, 3, 4]
    p = (A[..., :3] @ x[:, :, None, :, None])[..., 0] + A[..., 3]
    return (w[None, :, :, None] * p).sum(2)


# ---- the fused path ----
def _fused(*tensors):
    return all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors)


class PoseFunction(torch.autograd.Function):
    """pose [B, J, 3] or [B, J, 3, 3] and joints [J, 3] or [B, J, 3], float32 contiguous on the GPU ->
    transforms [B, J, 3, 4], posed_joints [B, J, 3].  The backward reads G.R from the saved transforms."""

    @staticmethod
    def forward(ctx, pose, joints, skel):
        B, J = pose.shape[0], skel.num_joints
        dev = pose.device
        transforms = torch.empty((B, J, 3, 4), dtype=torch.float32, device=dev)
        posed = torch.empty((B, J, 3), dtype=torch.float32, device=dev)
        stride = 0 if joints.ndim == 2 else J * 3
        with _lib.on_device(dev):
            _lib.check(_lib.lib().nr_pose_transforms_forward(
                _lib.ptr(pose), int(pose.ndim == 4), _lib.ptr(joints), stride, _lib.ptr(skel.parents),
                _lib.ptr(skel.level_offsets), _lib.ptr(skel.level_joints), B, J, skel.num_levels, _lib.ptr(transforms),
                _lib.ptr(posed), _lib.stream_of(pose)), "nr_pose_transforms_forward")
        ctx.skel = skel
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(pose, joints, transforms)
        return transforms, posed

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_transforms, grad_posed):
        need_pose, need_joints = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_pose or need_joints):
            return None, None, None
        pose, joints, transforms = ctx.saved_tensors
        skel, B, J = ctx.skel, pose.shape[0], ctx.skel.num_joints
        gA = None if grad_transforms is None else grad_transforms.to(torch.float32).contiguous()
        gP = None if grad_posed is None else grad_posed.to(torch.float32).contiguous()
        grad_pose = torch.empty_like(pose) if need_pose else None
        grad_joints = torch.empty((B, J, 3), dtype=torch.float32, device=pose.device) if need_joints else None
        stride = 0 if joints.ndim == 2 else J * 3
        with _lib.on_device(pose.device):
            _lib.check(_lib.lib().nr_pose_transforms_backward(
                _lib.ptr(pose), int(pose.ndim == 4), _lib.ptr(joints), stride, _lib.ptr(skel.parents),
                _lib.ptr(skel.level_offsets), _lib.ptr(skel.level_joints), _lib.ptr(skel.child_offsets),
                _lib.ptr(skel.children), _lib.ptr(transforms), _lib.ptr(gA), _lib.ptr(gP), B, J, skel.num_levels,
                _lib.ptr(grad_pose), _lib.ptr(grad_joints), _lib.stream_of(pose)), "nr_pose_transforms_backward")
        if need_joints and joints.ndim == 2:
            grad_joints = grad_joints.sum(0)  # shared joints take the sum over the items
        return grad_pose, grad_joints, None


class SkinFunction(torch.autograd.Function):
    """vertices [V, 3] or [B, V, 3], transforms [B, J, 3, 4], weights [V, K], float32 contiguous on the GPU ->
    out [B, V, 3]; `binding` gives the indices and, for the transform gradient, the joint CSR and its chunks."""

    @staticmethod
    def forward(ctx, vertices, transforms, weights, binding):
        B, J = transforms.shape[0], transforms.shape[1]
        V, K = weights.shape
        dev = transforms.device
        out = torch.empty((B, V, 3), dtype=torch.float32, device=dev)
        stride = 0 if vertices.ndim == 2 else V * 3
        with _lib.on_device(dev):
            _lib.check(_lib.lib().nr_skin_forward(_lib.ptr(vertices), stride, _lib.ptr(transforms), _lib.ptr(weights),
                                                  _lib.ptr(binding.indices), B, V, J, K, _lib.ptr(out),
                                                  _lib.stream_of(transforms)), "nr_skin_forward")
        ctx.binding = binding
        if any(ctx.needs_input_grad[:3]):
            ctx.save_for_backward(vertices, transforms, weights)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        need = ctx.needs_input_grad
        if not any(need[:3]):
            return None, None, None, None
        vertices, transforms, weights = ctx.saved_tensors
        bind = ctx.binding
        B, J = transforms.shape[0], transforms.shape[1]
        V, K = weights.shape
        dev = transforms.device
        L = _lib.lib()
        g = grad_out.to(torch.float32).contiguous()
        gv = torch.empty_like(vertices) if need[0] else None
        gt = torch.empty_like(transforms) if need[1] else None
        gw = torch.empty_like(weights) if need[2] else None
        ws = torch.empty(L.nr_skin_workspace_bytes(B, bind.num_chunks), dtype=torch.uint8, device=dev) if need[1] else None
        stride = 0 if vertices.ndim == 2 else V * 3
        with _lib.on_device(dev):
            _lib.check(L.nr_skin_backward(
                _lib.ptr(vertices), stride, _lib.ptr(transforms), _lib.ptr(weights), _lib.ptr(bind.indices), _lib.ptr(g),
                _lib.ptr(bind.entry_vertex), _lib.ptr(bind.entry_slot), _lib.ptr(bind.chunk_begin), _lib.ptr(bind.chunk_end),
                _lib.ptr(bind.joint_chunk_offsets), B, V, J, K, bind.num_chunks, _lib.ptr(gv), _lib.ptr(gt), _lib.ptr(gw),
                _lib.ptr(ws), 0 if ws is None else ws.numel(), _lib.stream_of(transforms)), "nr_skin_backward")
        return gv, gt, gw, None


def pose_transforms(pose, joints, parents):
    """(transforms [B, J, 3, 4], posed_joints [B, J, 3]) of pose [B, J, 3] (axis-angle) or [B, J, 3, 3]
    (matrices), rest joints [J, 3] (shared) or [B, J, 3] and `parents`: a [J] integer tensor, array or list, or a
    Skeleton (the module docstring has the formulas).  Gradients go to the pose (either form) and to the joints;
    shared joints take the sum over the items.  float32 GPU pose and joints run the fused kernels; everything
    else pose_transforms_torch.  Non-contiguous inputs are made contiguous."""
    if not _fused(pose, joints):
        return pose_transforms_torch(pose, joints, parents)
    skel = skeleton(parents, pose.device)
    _check_pose(pose, joints, skel)
    return PoseFunction.apply(pose.contiguous(), joints.contiguous(), skel)


def skin_vertices(vertices, transforms, weights, indices=None):
    """out [B, V, 3]: every vertex blended through the transforms [B, J, 3, 4] of the joints that influence it.
    vertices are [V, 3] (shared by the items) or [B, V, 3]; weights are dense [V, J] (indices None), [V, K] with
    integer indices [V, K], or a SkinBinding (skin_binding builds one; a module holds it).  Gradients go to the
    vertices (shared vertices take the sum over the items), to the transforms and, where they require grad, to the
    weights (the sum over the items; a dense matrix takes it on its non-zero entries only -- see the module
    docstring on learned weights).  float32 GPU vertices and transforms run the fused kernels; everything else
    skin_vertices_torch.  Non-contiguous inputs are made contiguous."""
    if not _fused(vertices, transforms):
        return skin_vertices_torch(vertices, transforms, weights, indices)
    B, V, J, _ = _check_skin(vertices, transforms)
    _check_weights(weights, indices, V, J)
    dev = transforms.device
    if isinstance(weights, SkinBinding):
        bind = weights.to(dev)
        w = bind.weights
    else:
        bind = skin_binding(weights, indices, J, dev)
        if indices is not None:
            w = weights.to(device=dev, dtype=torch.float32)  # the caller's own values, live
        elif weights.requires_grad:
            index, kept = bind.gather_index()
            w = weights.to(device=dev, dtype=torch.float32).gather(1, index) * kept
        else:
            w = bind.weights  # built from this very version of the tensor
    return SkinFunction.apply(vertices.contiguous(), transforms.contiguous(), w.contiguous(), bind)


class Skinning(torch.nn.Module):
    """A rig held by a module: rest joints [J, 3], `parents` and the skinning weights (dense [V, J], or [V, K]
    with indices, or a SkinBinding).  forward(pose, vertices) -> (posed_vertices [B, V, 3], posed_joints
    [B, J, 3]) for pose [B, J, 3] or [B, J, 3, 3] and rest vertices [V, 3] or [B, V, 3].  The joints are a buffer
    (they follow .to()); pass `joints=` to forward to pose from other ones (a joint regressor's output)."""

    def __init__(self, joints, parents, weights, indices=None):
        super().__init__()
        joints = torch.as_tensor(joints)
        self.skeleton = skeleton(parents)
        if joints.ndim != 2 or tuple(joints.shape) != (self.skeleton.num_joints, 3):
            raise ValueError("joints must be [%d, 3]" % self.skeleton.num_joints)
        self.register_buffer("joints", joints.detach().clone())
        self.binding = skin_binding(weights, indices, self.skeleton.num_joints)
        if self.binding.num_joints != self.skeleton.num_joints:
            raise ValueError("the weights name %d joints, the skeleton has %d" % (self.binding.num_joints, self.skeleton.num_joints))

    def forward(self, pose, vertices, joints=None):
        transforms, posed_joints = pose_transforms(pose, self.joints if joints is None else joints, self.skeleton)
        return skin_vertices(vertices, transforms, self.binding), posed_joints

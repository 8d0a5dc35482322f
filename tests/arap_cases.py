"""Inputs and float64 references shared by test_arap_loss.py and test_gpu_arap_loss.py.

Meshes and batch sizes are test_gpu_mesh_loss.CASES'.  The rest shape is the case's mesh un-jittered; the
deformed shape of item b is that mesh rotated by 0.7 rad about a seeded random axis, twisted by 0.8 z rad
about z, plus Gaussian noise of 0.01 x the rest shape's coordinate std.  Seeds are
test_gpu_mesh_regularizers': sum(map(ord, name)) for the vertices, that + 1 for the upstream gradient."""
import functools
import math

import numpy as np
import torch

import neural_renderer_v2_pytorch_amd as nr
from test_gpu_mesh_loss import CASES

MIN_CONDITION = 1e-3  # the cap every comparison asserts on its float64 reference: (s2 + det s3) / s1 per vertex
WEIGHTS = ("cotangent", "uniform", "tensor")


def axis_rotation(axis, angle):
    """The 3 x 3 rotation by `angle` rad about `axis` (Rodrigues), float64 numpy."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0., -a[2], a[1]], [a[2], 0., -a[0]], [-a[1], a[0], 0.]])
    return np.eye(3) + math.sin(angle) * K + (1. - math.cos(angle)) * (K @ K)


def deform(v, B, seed):
    """[B, V, 3] float64: per item v rotated by 0.7 rad about a random axis, twisted by 0.8 z rad about z, plus
    N(0, 0.01 std(v)) noise, all drawn from RandomState(seed)."""
    rng = np.random.RandomState(seed)
    v = np.asarray(v, np.float64)
    out = np.empty((B,) + v.shape)
    for b in range(B):
        x = v @ axis_rotation(rng.normal(size=3), 0.7).T
        t = 0.8 * x[:, 2]
        c, s = np.cos(t), np.sin(t)
        x = np.stack([c * x[:, 0] - s * x[:, 1], s * x[:, 0] + c * x[:, 1], x[:, 2]], 1)
        out[b] = x + rng.normal(0., 0.01 * v.std(), v.shape)
    return out


def symmetric_weights(topo, seed):
    """A float64 weight in [0.5, 1.5) per neighbour entry, the same for (i, j) and (j, i)."""
    rows, cols = (t.cpu().numpy() for t in topo.composition_index()[:2])
    key = np.minimum(rows, cols) * max(topo.num_vertices, 1) + np.maximum(rows, cols)
    uniq, inverse = np.unique(key, return_inverse=True)
    return torch.as_tensor(np.random.RandomState(seed).uniform(0.5, 1.5, uniq.shape[0])[inverse.reshape(-1)])


def condition(q, p, f, w):
    """(s2 + det(V U^T) s3) / s1 of every vertex's S = U diag(s) V^T, [B, V] float64, infinity where s1 == 0: half
    the gap between the two largest eigenvalues of Horn's matrix over s1, which is what makes the best rotation
    unique.  q [B, V, 3], p [1 or B, V, 3], w [1 or B, nnz], float64."""
    topo = nr.mesh_topology(f, q.shape[1])
    rows, cols = topo.composition_index()[:2]
    e, d = p[:, rows] - p[:, cols], q[:, rows] - q[:, cols]
    S = torch.zeros(q.shape[:2] + (3, 3), dtype=q.dtype).index_add_(1, rows, (w[:, :, None] * e)[:, :, :, None] * d[:, :, None, :])
    U, s, Vh = torch.linalg.svd(S)
    det = torch.linalg.det(Vh.transpose(-1, -2) @ U.transpose(-1, -2))
    return torch.where(s[..., 0] > 0, (s[..., 1] + det * s[..., 2]) / s[..., 0].clamp(min=1e-300), torch.full_like(det, math.inf))


def reference(q, p, f, weights, g=None):
    """The float64 composition on CPU tensors: a dict of the loss, the vertex gradient for the upstream gradient
    g (ones when None), the rotations, the weights as [1 or B, nnz] and condition()."""
    topo = nr.mesh_topology(f, q.shape[-2])
    y = q.clone().requires_grad_(True)
    out = nr.arap_loss_torch(y, p, f, weights)
    out.backward(torch.ones_like(out) if g is None else g)
    qb, pb = (q[None] if q.ndim == 2 else q), (p[None] if p.ndim == 2 else p)
    if torch.is_tensor(weights):
        w = weights[None] if weights.ndim == 1 else weights
    elif weights == "uniform":
        w = torch.ones((1, topo.nbr_index.numel()), dtype=q.dtype)
    else:
        w = nr.cot_weights_torch(pb, topo)
    return {"loss": out.detach(), "grad": y.grad, "R": nr.arap_rotations_torch(q, p, f, weights), "w": w,
            "condition": condition(qb, pb, f, w)}


def assert_conditioned(ref, what):
    """A condition on the inputs, not a measurement: a failure means the inputs changed, not the kernel."""
    worst = float(ref["condition"].min()) if ref["condition"].numel() else math.inf
    assert worst >= MIN_CONDITION, "%s: the inputs' worst (s2 + det s3) / s1 is %g" % (what, worst)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Float64 CPU tensors: the rest mesh [V, 3], the deformed vertices [B, V, 3], faces (numpy), the upstream
    gradient [B]."""
    mesh, B, _ = CASES[name]
    v, f = mesh()
    seed = sum(map(ord, name))
    p = torch.as_tensor(np.asarray(v, np.float64))
    q = torch.as_tensor(deform(v, B, seed))
    g = torch.as_tensor(np.random.RandomState(seed + 1).normal(size=B))
    return p, q, f, g


def rest_of(name, per_item):
    """The rest shape of a case: the mesh [V, 3], or per item [B, V, 3] the mesh scaled by 1 + 0.1 b -- still
    un-jittered, and a wrong item stride shows."""
    p, q = inputs(name)[:2]
    if not per_item:
        return p
    return p[None] * (1. + 0.1 * torch.arange(q.shape[0], dtype=p.dtype))[:, None, None]


def weights_of(name, kind):
    """'cotangent', 'uniform', or for 'tensor' a seeded symmetric [nnz] float64 tensor."""
    if kind != "tensor":
        return kind
    p, _, f, _ = inputs(name)
    return symmetric_weights(nr.mesh_topology(f, p.shape[0]), sum(map(ord, name)) + 2)


@functools.lru_cache(maxsize=None)
def case(name, kind="cotangent", per_item=False):
    """(rest, deformed, faces, upstream gradient, weights, reference(...)) of a case, computed once."""
    _, q, f, g = inputs(name)
    p, w = rest_of(name, per_item), weights_of(name, kind)
    return p, q, f, g, w, reference(q, p, f, w, g)

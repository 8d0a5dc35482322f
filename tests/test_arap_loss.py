"""The ARAP energy's torch composition, its definition and its gradient, and the argument checks of the Python
layer and the C entry points: no GPU needed."""
import math
import os
import re

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import _lib, mesh_loss, synthetic
from arap_cases import axis_rotation, deform, inputs, symmetric_weights
from conftest import ROOT

TRIANGLE = torch.as_tensor(np.eye(3)), np.array([[0, 1, 2]], np.int32)


def entry_sum(topo, p, w):
    """sum over the neighbour entries of w |e|^2."""
    rows, cols = topo.composition_index()[:2]
    e = p[rows] - p[cols]
    return float((w * (e * e).sum(-1)).sum())


@pytest.mark.parametrize("weights", ["cotangent", "uniform"])
def test_one_triangle_under_a_known_rotation(weights):
    """q = p R^T + t: every neighbourhood finds R, and the loss is 0."""
    p, f = TRIANGLE
    R = torch.as_tensor(axis_rotation([0.3, -1., 0.5], 0.7))
    q = p @ R.T + torch.tensor([0.2, -0.1, 0.4], dtype=torch.float64)
    got = nr.arap_rotations_torch(q, p, f, weights)
    assert got.shape == (3, 3, 3) and float((got - R).abs().max()) <= 1e-12
    assert float(nr.arap_loss_torch(q, p, f, weights)) <= 1e-24
    assert float((torch.linalg.det(got) - 1).abs().max()) <= 1e-12


@pytest.mark.parametrize("weights", ["cotangent", "uniform"])
def test_pure_scale(weights):
    """q = s p: the best rotation is I, and every entry is left with (s - 1) e: loss = (s - 1)^2 sum w |e|^2."""
    v, f = synthetic.icosphere(1)
    p = torch.as_tensor(np.asarray(v, np.float64))
    topo = nr.mesh_topology(f, p.shape[0])
    w = mesh_loss.cot_weights_torch(p[None], topo)[0] if weights == "cotangent" else torch.ones(topo.nbr_index.numel(), dtype=p.dtype)
    for s in (0.5, 1.3):
        want = (s - 1) ** 2 * entry_sum(topo, p, w)
        assert float(nr.arap_loss_torch(s * p, p, f, weights)) == pytest.approx(want, rel=1e-12)
        assert float((nr.arap_rotations_torch(s * p, p, f, weights) - torch.eye(3, dtype=p.dtype)).abs().max()) <= 1e-12
    # the same through an explicit weights tensor, [nnz] and [B, nnz]
    assert float(nr.arap_loss_torch(1.3 * p, p, f, w)) == pytest.approx(0.09 * entry_sum(topo, p, w), rel=1e-12)
    both = nr.arap_loss_torch(torch.stack([1.3 * p, 0.5 * p]), p, f, torch.stack([w, 2 * w]))
    assert both.tolist() == pytest.approx([0.09 * entry_sum(topo, p, w), 0.5 * entry_sum(topo, p, w)], rel=1e-12)


def test_zero_and_mirrored_neighbourhoods():
    """S = 0 (every vertex on one point) gives R = I; a mirrored rest shape still gives proper rotations."""
    p, f = TRIANGLE
    q = torch.zeros_like(p) + 0.25
    assert torch.equal(nr.arap_rotations_torch(q, p, f, "uniform"), torch.eye(3, dtype=p.dtype).expand(3, 3, 3))
    v, faces = synthetic.icosphere(1)
    rest = torch.as_tensor(np.asarray(v, np.float64))
    R = nr.arap_rotations_torch(rest, rest * torch.tensor([-1., 1., 1.], dtype=rest.dtype), faces, "uniform")
    assert float((torch.linalg.det(R) - 1).abs().max()) <= 1e-12
    assert float((R @ R.transpose(-1, -2) - torch.eye(3, dtype=rest.dtype)).abs().max()) <= 1e-12


def svd_through(q, p, f, w):
    """The energy with autograd running through the SVD: the rotations as functions of q."""
    topo = nr.mesh_topology(f, q.shape[1])
    rows, cols = topo.composition_index()[:2]
    e, d = p[:, rows] - p[:, cols], q[:, rows] - q[:, cols]
    S = torch.zeros(q.shape[:2] + (3, 3), dtype=q.dtype).index_add_(1, rows, (w[:, :, None] * e)[:, :, :, None] * d[:, :, None, :])
    U, _, Vh = torch.linalg.svd(S)
    Vm, Ut = Vh.transpose(-1, -2), U.transpose(-1, -2)
    flip = torch.stack([torch.ones_like(S[..., 0, 0]), torch.ones_like(S[..., 0, 0]), torch.linalg.det(Vm @ Ut).detach()], -1)
    R = (Vm * flip[..., None, :]) @ Ut
    r = d - (R[:, rows] @ e[..., None])[..., 0]
    return (w * (r * r).sum(-1)).sum(1)


@pytest.mark.parametrize("name", ["hinge", "ico2", "grid_fin", "fan70"])
@pytest.mark.parametrize("weights", ["cotangent", "uniform", "tensor"])
def test_envelope_identity(name, weights):
    """The rotations maximise, so holding them constant gives the exact gradient: the composition's gradient
    against autograd through the SVD in float64, within 1e-6 of the largest gradient magnitude; and against
    the closed form 2 g sum_j w_ij (2 d_ij - (R_i + R_j) e_ij)."""
    p, q, f, g = inputs(name)
    topo = nr.mesh_topology(f, p.shape[0])
    if weights == "tensor":
        w = symmetric_weights(topo, 5)
        arg = w
    else:
        w = mesh_loss._arap_weights_torch(p[None], topo, weights, 1e-12)[0]
        arg = weights
    y = q.clone().requires_grad_(True)
    nr.arap_loss_torch(y, p, f, arg).backward(g)
    z = q.clone().requires_grad_(True)
    svd_through(z, p[None], f, w[None]).backward(g)
    scale = float(y.grad.abs().max())
    assert scale > 0 and float((y.grad - z.grad).abs().max()) <= 1e-6 * scale
    rows, cols = topo.composition_index()[:2]
    R = nr.arap_rotations_torch(q, p, f, arg)
    e, d = (p[rows] - p[cols])[None], q[:, rows] - q[:, cols]
    both = ((R[:, rows] + R[:, cols]) @ e[..., None])[..., 0]
    formula = torch.zeros_like(q).index_add_(1, rows, w[None, :, None] * (2 * d - both)) * (2 * g)[:, None, None]
    assert float((y.grad - formula).abs().max()) <= 1e-12 * scale


def test_rest_shape_and_weights_take_no_gradient():
    p, q, f, g = inputs("ico2")
    topo = nr.mesh_topology(f, p.shape[0])
    rest = p.clone().requires_grad_(True)
    w = symmetric_weights(topo, 3).requires_grad_(True)
    y = q.clone().requires_grad_(True)
    nr.arap_loss_torch(y, rest, f, w).sum().backward()
    assert rest.grad is None and w.grad is None and float(y.grad.abs().max()) > 0


def test_shapes_average_and_module():
    p, q, f, g = inputs("ico2")
    per_item = nr.arap_loss_torch(q, p, f)
    assert per_item.shape == (q.shape[0],)
    one = nr.arap_loss_torch(q[1], p, f)
    assert one.ndim == 0 and float(one) == pytest.approx(float(per_item[1]), rel=1e-12)
    assert float(nr.arap_loss_torch(q, p, f, average=True)) == pytest.approx(float(per_item.mean()), rel=1e-12)
    assert nr.arap_rotations_torch(q[1], p, f).shape == (p.shape[0], 3, 3)
    stacked = torch.stack([p, 1.1 * p, 1.2 * p])
    assert nr.arap_loss_torch(q, stacked, f).tolist() == pytest.approx(
        [float(nr.arap_loss_torch(q[b], stacked[b], f)) for b in range(3)], rel=1e-12)
    for weights in ("cotangent", "uniform", symmetric_weights(nr.mesh_topology(f, p.shape[0]), 1)):
        for average in (False, True):
            module = nr.ArapLoss(p, f, weights=weights, average=average)
            assert torch.equal(module(q), nr.arap_loss(q, p, f, weights, average=average))
            assert torch.equal(module(q), nr.arap_loss_torch(q, p, f, weights, average=average))  # the CPU runs the composition
    assert "rest_vertices" in dict(nr.ArapLoss(p, f).named_buffers())
    w = nr.cot_weights(p, f)
    assert w.shape == (nr.mesh_topology(f, p.shape[0]).nbr_index.numel(),)
    assert torch.equal(w, mesh_loss.cot_weights_torch(p[None], nr.mesh_topology(f, p.shape[0]))[0])


def test_bad_arguments():
    p, q, f, g = inputs("ico0")
    topo = nr.mesh_topology(f, p.shape[0])
    nnz = topo.nbr_index.numel()
    for fn in (nr.arap_loss, nr.arap_loss_torch, nr.arap_rotations, nr.arap_rotations_torch):
        with pytest.raises(ValueError):
            fn(q[..., :2], p, f)                        # vertices not [.., 3]
        with pytest.raises(ValueError):
            fn(q, p[:-1], f)                            # a rest shape of another V
        with pytest.raises(ValueError):
            fn(q, torch.stack([p, p]), f)               # a rest batch that is neither 1 nor B
        with pytest.raises(ValueError):
            fn(q, p.reshape(-1), f)
        with pytest.raises(ValueError):
            fn(q, p, f, torch.ones(nnz + 1, dtype=p.dtype))  # weights of the wrong length
        with pytest.raises(ValueError):
            fn(q, p, f, torch.ones((2, nnz), dtype=p.dtype))  # a weights batch that is neither 1 nor B
        with pytest.raises(ValueError):
            fn(q, p, f, torch.ones(nnz, dtype=torch.int64))
        with pytest.raises(ValueError):
            fn(q, p, f, "cot")
        with pytest.raises(ValueError):
            fn(q, p, nr.mesh_topology(f, p.shape[0] + 1))  # a topology built for another V
    with pytest.raises(ValueError):
        nr.cot_weights(q, nr.mesh_topology(f, p.shape[0] + 1))
    with pytest.raises(ValueError):
        nr.ArapLoss(p.reshape(-1), f)


def test_cpu_runs_the_composition(monkeypatch):
    def no_library():
        raise AssertionError("the HIP library was loaded")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(mesh_loss.ArapFunction, "apply", lambda *a: no_library())
    p, q, f, g = inputs("ico2")
    x = q.float().requires_grad_(True)
    nr.arap_loss(x, p.float(), f).sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0.
    assert nr.arap_rotations(q.float(), p.float(), f).shape == q.shape + (3,)
    assert nr.cot_weights(q.float(), f).shape[0] == q.shape[0]


def test_deform_is_what_its_docstring_says():
    v = np.array([[0., 0., 0.5], [1., 0., 0.5], [0., 2., -0.25]])
    x = deform(v, 2, 11)
    assert x.shape == (2, 3, 3) and not np.array_equal(x[0], x[1])
    # noise of 0.01 std(v) on a rotation and a twist, both of which keep the distance from the origin
    assert np.abs(np.linalg.norm(x, axis=-1) - np.linalg.norm(v, axis=-1)).max() < 6 * 0.01 * v.std() * math.sqrt(3)


def test_abi_names_and_argument_checks():
    """The new entry points are in the header and in the binding's table, and validate before any launch (no
    GPU touched)."""
    header = open(os.path.join(ROOT, "include", "nr_raster.h")).read()
    names = ["nr_cot_weights_workspace_bytes", "nr_cot_weights", "nr_arap_workspace_bytes", "nr_arap_forward", "nr_arap_backward"]
    for name in names:
        assert re.search(r"^NR_API \w+ %s\(" % name, header, re.M), name
        assert name in _lib.SIGNATURES and name in _lib.EXPORTS
    L = _lib.lib()
    p, err, big = 4096, L.nr_last_error, 1 << 40  # p: a non-null pointer value, never dereferenced on these paths
    assert L.nr_cot_weights_workspace_bytes(0, 5) == 0 and L.nr_cot_weights_workspace_bytes(2, 10) == 256
    assert L.nr_cot_weights_workspace_bytes(64, 50000) == 64 * 50000 * 12
    assert L.nr_arap_workspace_bytes(2, 257) == L.nr_mesh_loss_workspace_bytes(2, 257) == 256

    def weights(vertices=p, faces=p, coff=p, corners=p, B=1, V=4, F=2, nnz=10, eps=1e-12, w=p, ws=p, nbytes=big):
        return L.nr_cot_weights(vertices, faces, coff, corners, B, V, F, nnz, eps, w, ws, nbytes, None)
    assert weights(B=-1) == 1 and b"bad sizes" in err()
    assert weights(nnz=-1) == 1 and b"bad sizes" in err()
    assert weights(F=2 ** 30) == 1 and b"2^31" in err()
    assert weights(B=2 ** 24, nnz=2 ** 31 - 1) == 1 and b"too many neighbours" in err()
    assert weights(eps=-1.) == 1 and b"bad eps" in err()
    assert weights(V=0) == 1 and weights(F=0) == 1
    assert weights(w=None) == 1 and weights(vertices=None) == 1 and weights(corners=None) == 1 and b"null pointer" in err()
    assert weights(ws=None, nbytes=0) == 3 and weights(nbytes=255) == 3
    assert weights(B=0) == 0 and weights(nnz=0, w=None) == 0

    def fwd(q=p, rest=p, rest_bs=0, w=p, w_bs=0, off=p, idx=p, B=1, V=4, nnz=10, rot=None, loss=p, ws=p, nbytes=big):
        return L.nr_arap_forward(q, rest, rest_bs, w, w_bs, off, idx, B, V, nnz, rot, loss, ws, nbytes, None)
    assert fwd(B=-1) == 1 and b"bad sizes" in err()
    assert fwd(nnz=-1) == 1 and b"bad size" in err()
    assert fwd(rest_bs=11) == 1 and b"rest_batch_stride" in err()
    assert fwd(w_bs=9) == 1 and b"w_batch_stride" in err()
    assert fwd(B=2 ** 30, V=2 ** 30) == 1 and b"too many" in err()
    assert fwd(loss=None) == 1 and b"null loss" in err()
    assert fwd(V=0) == 1 and b"without vertices" in err()
    assert fwd(q=None) == 1 and fwd(rest=None) == 1 and fwd(off=None) == 1 and fwd(idx=None) == 1
    assert fwd(rot=4100) == 1 and b"16-byte" in err()
    assert fwd(ws=None, nbytes=0) == 3 and fwd(V=300, nbytes=4) == 3
    assert fwd(B=0, loss=None) == 0

    def bwd(q=p, rest=p, rest_bs=12, w=p, w_bs=10, rot=p, off=p, idx=p, g=p, B=1, V=4, nnz=10, gv=p):
        return L.nr_arap_backward(q, rest, rest_bs, w, w_bs, rot, off, idx, g, B, V, nnz, gv, None)
    assert bwd(B=-1) == 1 and b"bad sizes" in err()
    assert bwd(rest_bs=13) == 1 and bwd(w_bs=11) == 1
    assert bwd(rot=None) == 1 and b"null pointer" in err()
    assert bwd(g=None) == 1 and bwd(gv=None) == 1 and bwd(q=None) == 1 and bwd(idx=None) == 1
    assert bwd(rot=4104) == 1 and b"16-byte" in err()
    assert bwd(B=0) == 0 and bwd(V=0, nnz=0, rest_bs=0, w_bs=0) == 0

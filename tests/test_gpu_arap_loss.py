"""The fused ARAP energy, its rotations and the fused cotangent weights on the GPU (float32) against the
torch composition in float64 on the CPU.

Inputs are arap_cases': test_gpu_mesh_loss.CASES' meshes un-jittered as the rest shape, deformed per item
by a rotation, a twist and noise.  Loss and gradient tolerances are test_gpu_mesh_loss's close_out and
close_grads unchanged.  Every comparison first asserts, on its float64 reference, that the inputs keep
(s2 + det s3) / s1 >= 1e-3 at every vertex; the smallest values are 0.0020 (grid257, teapot uniform) and
0.0033 (fan70 with the weights tensor).

What the composition itself loses in float32 on the CPU (torch.linalg.svd) against float64 on exactly these
inputs, as the worst fraction of each tolerance over the three kinds of weights and both forms of the rest
shape:

  case          loss    gradient        case          loss    gradient
  one_triangle  1.9 %   0.7 %           ico3          0.7 %   3.5 %
  hinge         2.0 %   1.3 %           fan70         6.2 %   2.2 %
  ico0          4.3 %   1.0 %           teapot        1.0 %   2.8 %
  ico2          1.2 %   2.5 %           grid257       0.8 %   11.8 %
  grid_fin      1.7 %   1.7 %           no_faces      0       0

so another rotation algorithm has 8x of margin at the least.

The rotations themselves (ROTATION_ERROR): the largest |R32 - R64| element of float32 torch.linalg.svd on
the CPU against float64, over the vertices whose ratio above is >= 0.1, the three kinds of weights and both
forms of the rest shape.  It grows with the mesh because S itself is summed in float32 from edges that are
differences of coordinates: grid257's edges are 4e-3 long at coordinates up to 0.5.  The fused rotations
are allowed 4x that figure per case.

cot_weights against float64: float32 cot_weights_torch on the CPU is within 5.5 % of close_out on every
case's rest shape (fan70) and within 9.1 % on the deformed shapes of the cases up to fan70; the deformed
teapot and grid257 hold slivers whose weights reach 300, where float32 itself is off by 1.9x and 15x the
tolerance, so those two are compared on their rest shape only."""
import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import mesh_loss
from arap_cases import WEIGHTS, assert_conditioned, axis_rotation, case, inputs, reference, symmetric_weights
from test_gpu_mesh_loss import CASES, close_grads, close_out

pytestmark = pytest.mark.gpu

ROTATION_ERROR = {  # measured: float32 torch.linalg.svd on the CPU against float64 (the module docstring)
    "no_faces": 0., "one_triangle": 4.27e-7, "hinge": 7.81e-7, "ico0": 7.86e-7, "ico2": 1.21e-6, "grid_fin": 8.77e-7,
    "ico3": 1.48e-6, "fan70": 7.86e-7, "teapot": 6.04e-6, "grid257": 7.48e-5,
}


def rotation_tol(name):
    return 4 * ROTATION_ERROR[name]


def on(dev, t):
    return t.to(device=dev, dtype=torch.float32) if torch.is_tensor(t) else t


def fused(q, p, f, w, g, dev, **kw):
    y = on(dev, q).requires_grad_(True)
    out = nr.arap_loss(y, on(dev, p), torch.as_tensor(f, device=dev), on(dev, w), **kw)
    out.backward(on(dev, g))
    return out.detach(), y.grad


@pytest.mark.parametrize("per_item", [False, True], ids=["shared", "per_item"])
@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("name", list(CASES))
def test_fused_matches_float64(dev, name, kind, per_item):
    p, q, f, g, w, ref = case(name, kind, per_item)
    assert_conditioned(ref, name)
    out, grad = fused(q, p, f, w, g, dev)
    assert out.shape == (q.shape[0],) and out.dtype == torch.float32 and grad.shape == q.shape
    print("%s %s: loss %s ref %s, grad max |d| %.3g of scale %.3g" % (
        name, kind, out.tolist(), ref["loss"].tolist(), float((grad.cpu().double() - ref["grad"]).abs().max()),
        float(ref["grad"].abs().max())))
    close_out(out, ref["loss"], "%s %s" % (name, kind))
    close_grads(grad, ref["grad"], "%s %s grad" % (name, kind))
    if name == "no_faces":
        assert float(out.abs().max()) == 0. and float(grad.abs().max()) == 0.
    if name == "grid_fin":
        assert float(grad[:, 26].abs().max()) == 0.  # the isolated vertex


@pytest.mark.parametrize("name", list(CASES))
def test_rotations(dev, name):
    """Orthonormal and proper everywhere; the float64 rotation where it is well determined."""
    for kind in WEIGHTS:
        for per_item in (False, True):
            p, q, f, g, w, ref = case(name, kind, per_item)
            assert_conditioned(ref, name)
            R = nr.arap_rotations(on(dev, q), on(dev, p), torch.as_tensor(f, device=dev), on(dev, w))
            assert R.shape == q.shape + (3,) and R.dtype == torch.float32 and not R.requires_grad
            R = R.cpu().double()
            assert float((R @ R.transpose(-1, -2) - torch.eye(3, dtype=R.dtype)).abs().max()) <= 1e-5
            assert bool((torch.linalg.det(R) > 0).all())
            sure = ref["condition"] >= 0.1
            assert int(sure.sum()) > 0
            err = float((R - ref["R"])[sure].abs().max())
            print("%s %s per_item=%d: rotations max |d| %.3g over %d of %d vertices (allowed %.3g)" % (
                name, kind, per_item, err, int(sure.sum()), sure.numel(), rotation_tol(name)))
            assert err <= rotation_tol(name)
            if name == "grid_fin":  # the isolated vertex: S = 0
                assert torch.equal(R[:, 26], torch.eye(3, dtype=R.dtype).expand(R.shape[0], 3, 3))


@pytest.mark.parametrize("angle", [0.7, 3.1])
@pytest.mark.parametrize("name", ["ico2", "ico3"])
def test_rigid_motion(dev, name, angle):
    """q = p R^T + t per item (3.1 rad: a quaternion whose scalar part is near 0): no energy, no gradient, and
    every neighbourhood finds R."""
    p, _, f, _ = inputs(name)
    rng = np.random.RandomState(int(angle * 10))
    Rs = torch.as_tensor(np.stack([axis_rotation(rng.normal(size=3), angle) for _ in range(2)]))
    q = p[None] @ Rs.transpose(-1, -2) + torch.as_tensor(rng.normal(size=(2, 1, 3)))
    faces = torch.as_tensor(f, device=dev)
    topo = nr.mesh_topology(f, p.shape[0])
    rows, cols = topo.composition_index()[:2]
    length = (p[rows] - p[cols]).norm(dim=-1)
    for kind in ("cotangent", "uniform"):
        w = nr.cot_weights_torch(p[None], topo)[0] if kind == "cotangent" else torch.ones_like(length)
        y = on(dev, q).requires_grad_(True)
        out = nr.arap_loss(y, on(dev, p), faces, kind)
        out.sum().backward()
        out = out.detach()
        bound = 1e-9 * float((w * length * length).sum())
        grad_bound = 1e-4 * float(4 * torch.zeros(p.shape[0], dtype=p.dtype).index_add_(0, rows, w * length).max())
        print("%s %s %.1f rad: loss %s (allowed %.3g), grad max %.3g (allowed %.3g)" % (
            name, kind, angle, out.tolist(), bound, float(y.grad.abs().max()), grad_bound))
        assert bool((out >= 0).all()) and float(out.max()) <= bound
        assert float(y.grad.norm(dim=-1).max()) <= grad_bound
        R = nr.arap_rotations(on(dev, q), on(dev, p), faces, kind).cpu().double()
        assert float((R - Rs[:, None]).abs().max()) <= rotation_tol(name)


def test_mirrored_rest_shape(dev):
    """The rest shape of ico2 mirrored (x -> -x): no rotation matches a neighbourhood, the best ones stay
    proper, and loss and gradient are the composition's."""
    p, q, f, g = inputs("ico2")
    m = p * torch.tensor([-1., 1., 1.], dtype=p.dtype)
    ref = reference(q, m, f, "cotangent", g)
    assert_conditioned(ref, "mirrored ico2")
    out, grad = fused(q, m, f, "cotangent", g, dev)
    close_out(out, ref["loss"], "mirrored")
    close_grads(grad, ref["grad"], "mirrored grad")
    R = nr.arap_rotations(on(dev, q), on(dev, m), torch.as_tensor(f, device=dev)).cpu().double()
    assert bool((torch.linalg.det(R) > 0).all())
    assert float((R @ R.transpose(-1, -2) - torch.eye(3, dtype=R.dtype)).abs().max()) <= 1e-5
    sure = ref["condition"] >= 0.1
    assert int(sure.sum()) > 0 and float((R - ref["R"])[sure].abs().max()) <= rotation_tol("ico2")


def test_coincident_vertices_and_identity(dev):
    p, q, f, g = inputs("ico2")
    faces = torch.as_tensor(f, device=dev)
    eye = torch.eye(3, device=dev).expand(1, p.shape[0], 3, 3)
    for kind in ("cotangent", "uniform"):
        # every deformed vertex on one point: S = 0 everywhere, R = I, the energy is sum w |e|^2
        y = torch.full((1, p.shape[0], 3), 0.25, device=dev).requires_grad_(True)
        out = nr.arap_loss(y, on(dev, p), faces, kind)
        out.sum().backward()
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(y.grad).all())
        assert torch.equal(nr.arap_rotations(y.detach(), on(dev, p), faces, kind), eye)
        close_out(out, nr.arap_loss_torch(torch.full((1, p.shape[0], 3), 0.25, dtype=p.dtype), p, f, kind), "coincident")
        # every rest vertex on one point as well: nothing at all
        z = y.detach().clone().requires_grad_(True)
        flat = nr.arap_loss(z, y.detach()[0], faces, "uniform")
        flat.sum().backward()
        assert float(flat.detach().abs().max()) == 0. and float(z.grad.abs().max()) == 0.
        # q = p exactly: S is symmetric, the quaternion stays (1, 0, 0, 0): loss 0, R = I, gradient 0
        x = on(dev, p)[None].clone().requires_grad_(True)
        same = nr.arap_loss(x, on(dev, p), faces, kind)
        same.sum().backward()
        assert float(same.detach().abs().max()) == 0. and float(x.grad.abs().max()) == 0.
        assert torch.equal(nr.arap_rotations(x.detach(), on(dev, p), faces, kind), eye)


@pytest.mark.parametrize("name", list(CASES))
def test_cot_weights(dev, name):
    """Bit-symmetric, cot_laplacian_loss's own weights bit for bit, and the float64 composition's within
    close_out (on the shapes the module docstring names)."""
    p, q, f, g = inputs(name)
    topo = nr.mesh_topology(torch.as_tensor(f, device=dev), p.shape[0])
    rows, cols = topo.composition_index()[:2]
    V = max(p.shape[0], 1)
    back = torch.searchsorted(rows * V + cols, cols * V + rows)  # the entry (j, i) of every entry (i, j)
    shapes = [p[None]] + ([q] if name not in ("teapot", "grid257") else [])
    for x in shapes:
        w = nr.cot_weights(on(dev, x), topo)
        assert w.shape == (x.shape[0], topo.nbr_index.numel()) and w.dtype == torch.float32 and not w.requires_grad
        assert torch.equal(w[:, back], w) and bool((w >= 0).all())
        close_out(w, nr.cot_weights_torch(x, nr.mesh_topology(f, p.shape[0])), "%s weights" % name)
        y = on(dev, x).requires_grad_(True)
        out = mesh_loss.CotLaplacianFunction.apply(y, topo, 1e-12)  # held: its node owns the saved tensors
        assert torch.equal(out.grad_fn.saved_tensors[1], w)
    one = nr.cot_weights(on(dev, p), topo, 1e-10)
    assert one.shape == (topo.nbr_index.numel(),)
    assert torch.equal(one, nr.cot_weights(on(dev, p)[None], torch.as_tensor(f, device=dev), eps=1e-10)[0])


def test_single_mesh_average_and_expanded_batch(dev):
    p, q, f, g, w, ref = case("ico2")
    faces = torch.as_tensor(f, device=dev)
    pd = on(dev, p)
    # [V, 3]: a 0-dim loss
    y = on(dev, q[1]).requires_grad_(True)
    one = nr.arap_loss(y, pd, faces)
    assert one.ndim == 0
    one.backward()
    single = reference(q[1], p, f, "cotangent")
    close_out(one, ref["loss"][1], "single")
    close_grads(y.grad, single["grad"], "single grad")
    assert nr.arap_rotations(on(dev, q[1]), pd, faces).shape == (p.shape[0], 3, 3)
    # average=True: the mean over the items
    avg = nr.arap_loss(on(dev, q), pd, faces, average=True)
    assert avg.ndim == 0
    close_out(avg, ref["loss"].mean(), "average")
    # a batch-expanded mesh: the gradient lands on the base and is the item sum
    base = on(dev, q[0]).requires_grad_(True)
    out = nr.arap_loss(base[None].expand(3, -1, -1), pd, faces)
    out.backward(on(dev, g))
    b64 = q[0].clone().requires_grad_(True)
    nr.arap_loss_torch(b64[None].expand(3, -1, -1), p, f).backward(g)
    assert base.grad.shape == base.shape
    close_grads(base.grad, b64.grad, "expanded grad")
    per_item = torch.autograd.grad(nr.arap_loss(base[None].expand(3, -1, -1).contiguous(), pd, faces), base, on(dev, g))[0]
    close_grads(base.grad, per_item, "expanded against contiguous")
    # a rest shape given as [1, V, 3] is the shared one; weights as [1, nnz] too
    wd = nr.cot_weights(pd, faces)
    assert torch.equal(nr.arap_loss(on(dev, q), pd[None], faces, wd[None]), nr.arap_loss(on(dev, q), pd, faces))


def test_runs_are_bitwise_reproducible(dev):
    p, q, f, g, w, _ = case("teapot")
    first = fused(q, p, f, w, g, dev)
    rot = nr.arap_rotations(on(dev, q), on(dev, p), torch.as_tensor(f, device=dev))
    for _ in range(2):
        again = fused(q, p, f, w, g, dev)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
        assert torch.equal(rot, nr.arap_rotations(on(dev, q), on(dev, p), torch.as_tensor(f, device=dev)))


@pytest.mark.parametrize("kind", WEIGHTS)
def test_no_gradient_needed(dev, kind, monkeypatch):
    """Vertices that take no gradient: the same loss, nothing saved, and no backward launch.  The forward is one
    library call, after one more that forms the cotangent weights where they are asked for."""
    p, q, f, g, w, _ = case("ico2", kind)
    faces = torch.as_tensor(f, device=dev)
    pd, wd = on(dev, p), on(dev, w)
    with_grad, _ = fused(q, p, f, w, g, dev)
    forward_calls = 2 if kind == "cotangent" else 1
    L = mesh_loss._lib.lib()
    calls = []
    monkeypatch.setattr(mesh_loss._lib, "lib", lambda: calls.append(1) or L)
    plain = nr.arap_loss(on(dev, q), pd, faces, wd)
    assert not plain.requires_grad and plain.grad_fn is None
    assert torch.equal(plain, with_grad)
    assert len(calls) == forward_calls
    # beside another leaf that does take a gradient, the backward runs without touching the library
    scale = torch.ones(q.shape[0], device=dev, requires_grad=True)
    out = nr.arap_loss(on(dev, q), pd, faces, wd) * scale
    assert out.grad_fn.next_functions[0][0] is None  # no node of the loss: nothing saved
    out.sum().backward()
    assert len(calls) == 2 * forward_calls and torch.equal(scale.grad, plain)
    # the module forms the weights once: one call per forward from then on
    module = nr.ArapLoss(pd, faces, weights=wd)
    module(on(dev, q))
    del calls[:]
    assert torch.equal(module(on(dev, q)), plain) and len(calls) == 1


def test_graph_capture_matches_eager(dev):
    """The loss (function and module) plus the backward captured once in a HIP graph and replayed after the
    vertices changed in place: bit for bit the eager results."""
    p, q, f, g, w, _ = case("ico2")
    faces = torch.as_tensor(f, device=dev)
    pd, gd = on(dev, p), on(dev, g)
    module = nr.ArapLoss(pd, faces, weights="uniform")
    v = on(dev, q).requires_grad_(True)
    moved = on(dev, q + 0.01 * torch.as_tensor(np.random.RandomState(77).normal(size=tuple(q.shape))))

    def step(y):
        cot, uni = nr.arap_loss(y, pd, faces), module(y)
        (cot + 0.1 * uni).backward(gd)
        return cot, uni

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            v.grad = None
            before = step(v)[0].clone()
    torch.cuda.current_stream().wait_stream(side)
    v.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cot, uni = step(v)
    with torch.no_grad():
        v.copy_(moved)
    graph.replay()
    torch.cuda.synchronize()
    got = cot.clone(), uni.clone(), v.grad.clone()
    e = moved.clone().requires_grad_(True)
    ecot, euni = step(e)
    torch.cuda.synchronize()
    assert torch.equal(got[0], ecot) and torch.equal(got[1], euni) and torch.equal(got[2], e.grad)
    assert not torch.equal(got[0], before)  # the replay saw the new vertices


def test_descent_trajectory(dev):
    """8 steps of plain gradient descent from the deformed ico2: the float64 composition's loss falls every
    step at this rate, and the fused float32 trajectory stays on it.  The rate: the energy's curvature is at
    most 8 max_i sum_j w_ij (about 8 x 3.6 with the cotangent weights of ico2), so 0.02 is well inside 2 / that."""
    p, q, f, g = inputs("ico2")
    faces = torch.as_tensor(f, device=dev)
    lr, steps = 0.02, 8

    def descend(x, rest, fn, fc):
        history = []
        for _ in range(steps + 1):
            y = x.clone().requires_grad_(True)
            loss = fn(y, rest, fc)
            history.append(loss.detach().cpu().double())
            if len(history) <= steps:
                loss.sum().backward()
                x = x - lr * y.grad
        return x, history

    ref, ref_hist = descend(q, p, nr.arap_loss_torch, f)
    for a, b in zip(ref_hist, ref_hist[1:]):
        assert bool((b < a).all()), ref_hist  # the learning rate suits the reference
    got, hist = descend(on(dev, q), on(dev, p), nr.arap_loss, faces)
    close_grads(got, ref, "vertices after %d steps" % steps)
    assert bool((hist[-1] < hist[0]).all())
    close_out(hist[-1], ref_hist[-1], "final loss")


def test_module_gives_what_the_function_gives(dev):
    p, q, f, g = inputs("ico2")
    qd, pd = on(dev, q), on(dev, p)
    faces = torch.as_tensor(f, device=dev)
    tensor = on(dev, symmetric_weights(nr.mesh_topology(f, p.shape[0]), 9))
    stacked = on(dev, torch.stack([p, 1.1 * p, 1.2 * p]))
    for rest in (pd, stacked):
        for weights in ("cotangent", "uniform", tensor):
            for average in (False, True):
                for src in (f, faces):  # host faces (the topology moves to the vertices' device) and device faces
                    y = qd.clone().requires_grad_(True)
                    module = nr.ArapLoss(rest.cpu(), src, weights=weights, average=average)  # a buffer: moved by .to()
                    out = module.to(dev)(y)
                    out.sum().backward()
                    z = qd.clone().requires_grad_(True)
                    want = nr.arap_loss(z, rest, faces, weights, average=average)
                    want.sum().backward()
                    assert torch.equal(out, want) and torch.equal(y.grad, z.grad)
                    assert module.rest_vertices.device == qd.device

"""The fused edge-length and cotangent Laplacian losses on the GPU (float32) against the torch
compositions in float64 on the CPU.

Cases, batch sizes and jitter are test_gpu_mesh_loss.CASES' (plus the kite of test_mesh_regularizers at
sigma 0.002), every case seeded with sum(map(ord, name)), and the tolerances are that file's: losses
rtol = atol = 1e-5, gradients 1e-4 of the reference gradient's largest magnitude plus 1e-4 relative.
What the compositions themselves lose in float32 on the CPU against float64 on exactly these inputs
(eps 1e-12), as the worst fraction of each tolerance over a case's elements:

  loss           worst of loss tol   worst of grad tol   teapot grad   grid257 grad
  cotangent      1.1 % (ico0)        38 % (grid257)      25 %          38 %
  edge, L = 0.1  1.2 % (grid257)     7.7 % (grid257)     3.8 %         7.7 %
  edge, L = 0    0.9 % (ico2)        8.5 % (grid257)     1.0 %         8.5 %

Every other case stays below 2 % of the gradient tolerance.  No figure is above a half, so no seed is
picked.  No vertex of any case has 0 < W_i < 1e-3: the smallest positive W_i is 0.45 (grid_fin), and the
only W_i <= NR_COT_MIN_WEIGHT are grid_fin's isolated vertex and the three vertices of no_faces, so the
one discontinuity of the definition is never near."""
import functools

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import mesh_loss
from mesh_loss_cases import jitter
from test_gpu_mesh_loss import CASES as MESH_CASES, close_grads, close_out, ico
from test_mesh_regularizers import KITE_F, KITE_V

pytestmark = pytest.mark.gpu

CASES = dict(MESH_CASES, kite=(lambda: (KITE_V, KITE_F), 2, 0.002))
LOSSES = {  # name: (fused, composition, keywords)
    "cot": (nr.cot_laplacian_loss, nr.cot_laplacian_loss_torch, {}),
    "edge0": (nr.edge_length_loss, nr.edge_length_loss_torch, {"target_length": 0.}),
    "edge": (nr.edge_length_loss, nr.edge_length_loss_torch, {"target_length": 0.1}),
}


def inputs(name):
    """Float64 CPU vertices [B, V, 3], faces and the upstream gradient [B] of a case."""
    mesh, B, sigma = CASES[name]
    v, f = mesh()
    seed = sum(map(ord, name))
    x = torch.as_tensor(jitter(v, B, sigma, seed))
    g = torch.as_tensor(np.random.RandomState(seed + 1).normal(size=B))
    return x, f, g


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs(name) and per loss the float64 composition's value and vertex gradient."""
    x, f, g = inputs(name)
    ref = {}
    for loss, (_, composition, kw) in LOSSES.items():
        y = x.clone().requires_grad_(True)
        out = composition(y, f, **kw)
        out.backward(g)
        ref[loss] = (out.detach(), y.grad)
    return x, f, g, ref


def fused(loss, x, faces, g, dev):
    fn, _, kw = LOSSES[loss]
    y = x.to(device=dev, dtype=torch.float32).requires_grad_(True)
    out = fn(y, faces, **kw)
    out.backward(g.to(device=dev, dtype=torch.float32))
    return out.detach(), y.grad


@pytest.mark.parametrize("loss", sorted(LOSSES))
@pytest.mark.parametrize("name", list(CASES))
def test_fused_matches_float64(dev, name, loss):
    x, f, g, ref = case(name)
    faces = torch.as_tensor(f, device=dev)
    out, grad = fused(loss, x, faces, g, dev)
    assert out.shape == (x.shape[0],) and out.dtype == torch.float32 and grad.shape == x.shape
    print("%s %s: loss %s ref %s, grad max |d| %.3g of scale %.3g" % (
        name, loss, out.tolist(), ref[loss][0].tolist(), float((grad.cpu().double() - ref[loss][1]).abs().max()),
        float(ref[loss][1].abs().max())))
    close_out(out, ref[loss][0], "%s %s" % (name, loss))
    close_grads(grad, ref[loss][1], "%s %s grad" % (name, loss))
    if name == "no_faces":
        assert float(out.abs().max()) == 0. and float(grad.abs().max()) == 0.
    if name == "grid_fin":
        assert float(grad[:, 26].abs().max()) == 0.  # the isolated vertex


def test_saved_weights_are_symmetric(dev):
    """w of entry (i, j) and of (j, i) sum the same corners in the same order: equal bit for bit, which
    the backward relies on."""
    x, f, g, _ = case("teapot")
    topo = nr.mesh_topology(torch.as_tensor(f, device=dev), x.shape[1])
    y = x.to(device=dev, dtype=torch.float32).requires_grad_(True)
    out = mesh_loss.CotLaplacianFunction.apply(y, topo, 1e-12)
    delta, w, winv = out.grad_fn.saved_tensors
    assert w.shape == (x.shape[0], topo.nbr_index.numel()) and winv.shape == x.shape[:2] and delta.shape == x.shape
    rows, cols = topo.composition_index()[:2]
    V = x.shape[1]
    back = torch.searchsorted(rows * V + cols, cols * V + rows)  # the entry (j, i) of every entry (i, j)
    assert torch.equal((rows * V + cols)[back], cols * V + rows)
    assert torch.equal(w[:, back], w) and bool((w >= 0).all()) and float(w.max()) > 0.
    # winv is 1 / W of these weights: a row has 24 entries at most, so W summed in another order differs by
    # 24 * 2^-24 = 1.4e-6 relative at most
    W = torch.zeros(x.shape[:2], dtype=torch.float32, device=dev).index_add_(1, rows, w)
    assert bool((winv > 0).all()) and float((winv * W - 1).abs().max()) <= 1e-5


@pytest.mark.parametrize("loss", sorted(LOSSES))
def test_single_mesh_average_and_expanded_batch(dev, loss):
    x, f, g, ref = case("ico2")
    fn, composition, kw = LOSSES[loss]
    faces = torch.as_tensor(f, device=dev)
    # [V, 3]: a 0-dim loss
    y = x[1].to(device=dev, dtype=torch.float32).requires_grad_(True)
    one = fn(y, faces, **kw)
    assert one.ndim == 0
    one.backward()
    y64 = x[1].clone().requires_grad_(True)
    composition(y64, f, **kw).backward()
    close_out(one, ref[loss][0][1], "single")
    close_grads(y.grad, y64.grad, "single grad")
    # average=True: the mean over the items
    avg = fn(x.to(device=dev, dtype=torch.float32), faces, average=True, **kw)
    assert avg.ndim == 0
    close_out(avg, ref[loss][0].mean(), "average")
    # a batch-expanded mesh: the gradient lands on the base and is the item sum
    base = x[0].to(device=dev, dtype=torch.float32).requires_grad_(True)
    out = fn(base[None].expand(3, -1, -1), faces, **kw)
    out.backward(g.to(device=dev, dtype=torch.float32))
    b64 = x[0].clone().requires_grad_(True)
    composition(b64[None].expand(3, -1, -1), f, **kw).backward(g)
    assert base.grad.shape == base.shape
    close_grads(base.grad, b64.grad, "expanded grad")
    per_item = torch.autograd.grad(fn(base[None].expand(3, -1, -1).contiguous(), faces, **kw), base, g.to(dev).float())[0]
    close_grads(base.grad, per_item, "expanded against contiguous")


@pytest.mark.parametrize("loss", sorted(LOSSES))
def test_runs_are_bitwise_reproducible(dev, loss):
    x, f, g, _ = case("teapot")
    faces = torch.as_tensor(f, device=dev)
    first = fused(loss, x, faces, g, dev)
    for _ in range(2):
        again = fused(loss, x, faces, g, dev)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


@pytest.mark.parametrize("loss", sorted(LOSSES))
def test_no_gradient_needed(dev, loss, monkeypatch):
    """Vertices that take no gradient: the same loss, nothing saved, and no backward launch."""
    x, f, g, _ = case("ico2")
    fn, _, kw = LOSSES[loss]
    faces = torch.as_tensor(f, device=dev)
    with_grad, _ = fused(loss, x, faces, g, dev)
    L = mesh_loss._lib.lib()
    calls = []
    monkeypatch.setattr(mesh_loss._lib, "lib", lambda: calls.append(1) or L)
    plain = fn(x.to(device=dev, dtype=torch.float32), faces, **kw)
    assert not plain.requires_grad and plain.grad_fn is None
    assert torch.equal(plain, with_grad)
    assert len(calls) == 1  # the forward alone
    # beside another leaf that does take a gradient, the backward runs without touching the library
    w = torch.ones(x.shape[0], device=dev, requires_grad=True)
    out = fn(x.to(device=dev, dtype=torch.float32), faces, **kw) * w
    assert out.grad_fn.next_functions[0][0] is None  # no node of the loss: nothing saved
    out.sum().backward()
    assert len(calls) == 2 and torch.equal(w.grad, plain)


def test_graph_capture_matches_eager(dev):
    """Both losses plus the backward captured once in a HIP graph and replayed after the vertices changed
    in place: bit for bit the eager results."""
    x, f, g, _ = case("ico2")
    faces = torch.as_tensor(f, device=dev)
    gd = g.to(device=dev, dtype=torch.float32)
    v = x.to(device=dev, dtype=torch.float32).requires_grad_(True)
    moved = (x + torch.as_tensor(jitter(np.zeros(x.shape[1:]), x.shape[0], 0.01, 77))).to(device=dev, dtype=torch.float32)

    def step(y):
        cot, edge = nr.cot_laplacian_loss(y, faces), nr.edge_length_loss(y, faces, 0.1)
        (cot + 0.1 * edge).backward(gd)
        return cot, edge

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
        cot, edge = step(v)
    with torch.no_grad():
        v.copy_(moved)
    graph.replay()
    torch.cuda.synchronize()
    got = cot.clone(), edge.clone(), v.grad.clone()
    e = moved.clone().requires_grad_(True)
    ecot, eedge = step(e)
    torch.cuda.synchronize()
    assert torch.equal(got[0], ecot) and torch.equal(got[1], eedge) and torch.equal(got[2], e.grad)
    assert not torch.equal(got[0], before)  # the replay saw the new vertices


def test_descent_trajectory(dev):
    """8 steps of plain gradient descent on cot_laplacian + 0.1 edge_length(L = the mean initial edge) on
    jittered ico2: the float64 composition's total falls every step at this rate, the fused float32
    trajectory stays on it, and both terms end lower than they began."""
    v, f = ico(2)
    x0 = torch.as_tensor(jitter(v, 2, 0.02, 21))
    faces = torch.as_tensor(f, device=dev)
    rows, cols = nr.mesh_topology(f, v.shape[0]).composition_index()[:2]
    target = float((x0[:, rows] - x0[:, cols]).norm(dim=-1).mean())
    lr, steps = 0.05, 8

    def descend(x, cot_fn, edge_fn, fc):
        history = []
        for _ in range(steps + 1):
            y = x.clone().requires_grad_(True)
            cot, edge = cot_fn(y, fc), edge_fn(y, fc, target)
            history.append((cot.detach().cpu().double(), edge.detach().cpu().double()))
            if len(history) <= steps:
                (cot + 0.1 * edge).sum().backward()
                x = x - lr * y.grad
        return x, history

    ref, ref_hist = descend(x0, nr.cot_laplacian_loss_torch, nr.edge_length_loss_torch, f)
    total = [cot + 0.1 * edge for cot, edge in ref_hist]
    for a, b in zip(total, total[1:]):
        assert bool((b < a).all()), total  # the learning rate suits the reference
    got, hist = descend(x0.to(device=dev, dtype=torch.float32), nr.cot_laplacian_loss, nr.edge_length_loss, faces)
    close_grads(got, ref, "vertices after %d steps" % steps)
    for k in (0, 1):
        assert bool((hist[-1][k] < hist[0][k]).all()) and bool((ref_hist[-1][k] < ref_hist[0][k]).all())
        close_out(hist[-1][k], ref_hist[-1][k], "final loss %d" % k)


def test_modules_give_what_the_functions_give(dev):
    x, f, g, _ = case("ico2")
    xd = x.to(device=dev, dtype=torch.float32)
    faces = torch.as_tensor(f, device=dev)
    V = x.shape[1]
    for fn, mod, kw in ((nr.edge_length_loss, nr.EdgeLengthLoss, {"target_length": 0.1}),
                        (nr.cot_laplacian_loss, nr.CotLaplacianLoss, {"eps": 1e-10})):
        for average in (False, True):
            for src in (f, faces):  # host faces (the topology moves to the vertices' device) and device faces
                y = xd.clone().requires_grad_(True)
                out = mod(src, V, average=average, **kw)(y)
                out.sum().backward()
                z = xd.clone().requires_grad_(True)
                want = fn(z, faces, average=average, **kw)
                want.sum().backward()
                assert torch.equal(out, want) and torch.equal(y.grad, z.grad)

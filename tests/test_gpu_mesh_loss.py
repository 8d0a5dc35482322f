"""The fused Laplacian and flatten losses on the GPU (float32) against the torch composition in float64
on the CPU.

Tolerances are test_gpu_projection's: losses rtol = atol = 1e-5, gradients 1e-4 of the reference
gradient's largest magnitude plus 1e-4 relative.  Float32 torch on the CPU stays below 1.5e-6 of the
float64 losses and 2.5e-6 of the gradients' scale on these inputs (the teapot's flatten gradient: 6e-6,
its shortest edges are 1.3e-3 long, where eps matters; see SEEDS): a quarter of any tolerance at most.
grid257 (66049 vertices, 196096 two-face edges: more than 256 partials per item for both losses) sums
many more terms: float32 torch uses 0.08 % (Laplacian) and 2.7 % (flatten) of the loss tolerance there,
and 22 % and 18 % of the gradient tolerance."""
import functools

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import mesh_loss, synthetic
from mesh_loss_cases import fan, grid, grid_fin, hinge, jitter, teapot

pytestmark = pytest.mark.gpu

OUT_TOL = 1e-5
GRAD_TOL = 1e-4
LOSSES = {"laplacian": (nr.laplacian_loss, nr.laplacian_loss_torch), "flatten": (nr.flatten_loss, nr.flatten_loss_torch)}


def close_grads(a, b, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = float(b.abs().max()) if b.numel() else 0.
    err = (a - b).abs()
    bad = err > GRAD_TOL * scale + GRAD_TOL * b.abs()
    assert not bad.any(), "%s: %d of %d elements off, max |d| %g (scale %g)" % (
        what, int(bad.sum()), bad.numel(), float(err.max()), scale)


def close_out(a, b, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    assert bool((err <= OUT_TOL + OUT_TOL * b.abs()).all()), "%s: max |d| %g of %s" % (what, float(err.max()), b.tolist())


def ico(level):
    v, f = synthetic.icosphere(level)
    return v.astype(np.float64), f


CASES = {  # name: (mesh, B, jitter sigma)
    "no_faces": (lambda: (np.eye(3), np.zeros((0, 3), np.int32)), 2, 0.02),
    "one_triangle": (lambda: (np.eye(3), np.array([[0, 1, 2]], np.int32)), 2, 0.02),
    "hinge": (lambda: hinge(2.2), 2, 0.02),
    "ico0": (lambda: ico(0), 3, 0.02),        # V 12: less than a wave
    "ico2": (lambda: ico(2), 3, 0.02),        # V 162, E2 480: a partial vertex block, two edge blocks
    "grid_fin": (grid_fin, 2, 0.02),          # boundary edges, a non-manifold edge, an isolated vertex
    "ico3": (lambda: ico(3), 3, 0.02),        # V 642, E2 1920: several blocks per item
    "fan70": (fan, 2, 0.02),                  # a degree above the wave width
    "teapot": (teapot, 2, 0.002),
    # V 66049: 259 vertex blocks, E2 196096: 766 edge blocks -- k_mesh_loss_sum's strided loop takes a second
    # and a third trip for both losses.  The spacing is 3.9e-3, so sigma 5e-4 bends the patch without folding it.
    "grid257": (lambda: grid(257), 2, 5e-4),
}
# The teapot's jitter (sigma 0.002) is longer than its shortest edges (1.3e-3), so a draw can nearly
# collapse an edge, where float32 itself loses the flatten gradient: float32 torch on the CPU against
# float64 is off by 6e-6 to 3e-5 of the gradient's scale at most seeds, but 9e-5 and 1.5e-4 at two of
# the thirteen tried.  This seed is picked by that figure alone (6e-6): the reference's own float32 error
# uses a sixteenth of the tolerance.
SEEDS = {"teapot": 3}


@functools.lru_cache(maxsize=None)
def case(name):
    """Float64 CPU vertices [B, V, 3], faces, the upstream gradient [B], and per loss the float64
    composition's value and vertex gradient."""
    mesh, B, sigma = CASES[name]
    v, f = mesh()
    seed = SEEDS.get(name, sum(map(ord, name)))
    x = torch.as_tensor(jitter(v, B, sigma, seed))
    g = torch.as_tensor(np.random.RandomState(seed + 1).normal(size=B))
    ref = {}
    for loss, (_, composition) in LOSSES.items():
        y = x.clone().requires_grad_(True)
        out = composition(y, f)
        out.backward(g)
        ref[loss] = (out.detach(), y.grad)
    return x, f, g, ref


def fused(fn, x, faces, g, dev, **kw):
    y = x.to(device=dev, dtype=torch.float32).requires_grad_(True)
    out = fn(y, faces, **kw)
    out.backward(g.to(device=dev, dtype=torch.float32))
    return out.detach(), y.grad


@pytest.mark.parametrize("loss", sorted(LOSSES))
@pytest.mark.parametrize("name", list(CASES))
def test_fused_matches_float64(dev, name, loss):
    x, f, g, ref = case(name)
    faces = torch.as_tensor(f, device=dev)
    out, grad = fused(LOSSES[loss][0], x, faces, g, dev)
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


@pytest.mark.parametrize("loss", sorted(LOSSES))
def test_single_mesh_average_and_expanded_batch(dev, loss):
    x, f, g, ref = case("ico2")
    fn, composition = LOSSES[loss]
    faces = torch.as_tensor(f, device=dev)
    # [V, 3]: a 0-dim loss
    y = x[1].to(device=dev, dtype=torch.float32).requires_grad_(True)
    one = fn(y, faces)
    assert one.ndim == 0
    one.backward()
    y64 = x[1].clone().requires_grad_(True)
    composition(y64, f).backward()
    close_out(one, ref[loss][0][1], "single")
    close_grads(y.grad, y64.grad, "single grad")
    # average=True: the mean over the items
    avg = fn(x.to(device=dev, dtype=torch.float32), faces, average=True)
    assert avg.ndim == 0
    close_out(avg, ref[loss][0].mean(), "average")
    # a batch-expanded mesh: the gradient lands on the base and is the item sum
    base = x[0].to(device=dev, dtype=torch.float32).requires_grad_(True)
    out = fn(base[None].expand(3, -1, -1), faces)
    out.backward(g.to(device=dev, dtype=torch.float32))
    b64 = x[0].clone().requires_grad_(True)
    composition(b64[None].expand(3, -1, -1), f).backward(g)
    assert base.grad.shape == base.shape
    close_grads(base.grad, b64.grad, "expanded grad")
    per_item = torch.autograd.grad(fn(base[None].expand(3, -1, -1).contiguous(), faces), base, g.to(dev).float())[0]
    close_grads(base.grad, per_item, "expanded against contiguous")


@pytest.mark.parametrize("loss", sorted(LOSSES))
def test_runs_are_bitwise_reproducible(dev, loss):
    x, f, g, _ = case("teapot")
    faces = torch.as_tensor(f, device=dev)
    first = fused(LOSSES[loss][0], x, faces, g, dev)
    for _ in range(2):
        again = fused(LOSSES[loss][0], x, faces, g, dev)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


@pytest.mark.parametrize("loss", sorted(LOSSES))
def test_no_gradient_needed(dev, loss, monkeypatch):
    """Vertices that take no gradient: the same loss, nothing saved, and no backward launch."""
    x, f, g, _ = case("ico2")
    fn = LOSSES[loss][0]
    faces = torch.as_tensor(f, device=dev)
    with_grad, _ = fused(fn, x, faces, g, dev)
    L = mesh_loss._lib.lib()
    calls = []
    monkeypatch.setattr(mesh_loss._lib, "lib", lambda: calls.append(1) or L)
    plain = fn(x.to(device=dev, dtype=torch.float32), faces)
    assert not plain.requires_grad and plain.grad_fn is None
    assert torch.equal(plain, with_grad)
    assert len(calls) == 1  # the forward alone
    # beside another leaf that does take a gradient, the backward runs without touching the library
    w = torch.ones(x.shape[0], device=dev, requires_grad=True)
    (fn(x.to(device=dev, dtype=torch.float32), faces) * w).sum().backward()
    assert len(calls) == 2 and torch.equal(w.grad, plain)


def test_graph_capture_matches_eager(dev):
    """Loss plus backward of both losses captured once in a HIP graph and replayed after the vertices
    changed in place: bit for bit the eager results (no atomics anywhere)."""
    x, f, g, _ = case("ico2")
    faces = torch.as_tensor(f, device=dev)
    gd = g.to(device=dev, dtype=torch.float32)
    v = x.to(device=dev, dtype=torch.float32).requires_grad_(True)
    moved = (x + torch.as_tensor(jitter(np.zeros(x.shape[1:]), x.shape[0], 0.01, 77))).to(device=dev, dtype=torch.float32)

    def step():
        lap, flat = nr.laplacian_loss(v, faces), nr.flatten_loss(v, faces)
        (lap + 0.1 * flat).backward(gd)
        return lap, flat

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            v.grad = None
            before = step()[0].clone()
    torch.cuda.current_stream().wait_stream(side)
    v.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lap, flat = step()
    with torch.no_grad():
        v.copy_(moved)
    graph.replay()
    torch.cuda.synchronize()
    got = lap.clone(), flat.clone(), v.grad.clone()
    e = moved.clone().requires_grad_(True)
    elap, eflat = nr.laplacian_loss(e, faces), nr.flatten_loss(e, faces)
    (elap + 0.1 * eflat).backward(gd)
    torch.cuda.synchronize()
    assert torch.equal(got[0], elap) and torch.equal(got[1], eflat) and torch.equal(got[2], e.grad)
    assert not torch.equal(got[0], before)  # the replay saw the new vertices


def test_descent_trajectory(dev):
    """8 steps of plain gradient descent on laplacian + 0.1 flatten: the fused float32 trajectory stays
    on the float64 composition's, and both losses end lower than they began."""
    v, f = ico(2)
    x0 = torch.as_tensor(jitter(v, 2, 0.02, 21))
    faces = torch.as_tensor(f, device=dev)
    lr, steps = 0.05, 8

    def descend(x, lap_fn, flat_fn, fc):
        history = []
        for _ in range(steps + 1):
            y = x.clone().requires_grad_(True)
            lap, flat = lap_fn(y, fc), flat_fn(y, fc)
            history.append((lap.detach().cpu().double(), flat.detach().cpu().double()))
            if len(history) <= steps:
                (lap + 0.1 * flat).sum().backward()
                x = x - lr * y.grad
        return x, history

    ref, ref_hist = descend(x0, nr.laplacian_loss_torch, nr.flatten_loss_torch, f)
    total = [lap + 0.1 * flat for lap, flat in ref_hist]
    for a, b in zip(total, total[1:]):
        assert bool((b < a).all()), total  # the learning rate suits the reference
    got, hist = descend(x0.to(device=dev, dtype=torch.float32), nr.laplacian_loss, nr.flatten_loss, faces)
    close_grads(got, ref, "vertices after %d steps" % steps)
    for k in (0, 1):
        assert bool((hist[-1][k] < hist[0][k]).all()) and bool((ref_hist[-1][k] < ref_hist[0][k]).all())
        close_out(hist[-1][k], ref_hist[-1][k], "final loss %d" % k)


def test_modules_give_what_the_functions_give(dev):
    x, f, g, _ = case("ico2")
    xd = x.to(device=dev, dtype=torch.float32)
    faces = torch.as_tensor(f, device=dev)
    V = x.shape[1]
    for fn, mod in ((nr.laplacian_loss, nr.LaplacianLoss), (nr.flatten_loss, nr.FlattenLoss)):
        for average in (False, True):
            for src in (f, faces):  # host faces (the topology moves to the vertices' device) and device faces
                y = xd.clone().requires_grad_(True)
                out = mod(src, V, average=average)(y)
                out.sum().backward()
                z = xd.clone().requires_grad_(True)
                want = fn(z, faces, average=average)
                want.sum().backward()
                assert torch.equal(out, want) and torch.equal(y.grad, z.grad)

"""The fused calibrated camera (camera.projection_transform) and the fused 'look' on the GPU, against
the float64 CPU compositions (projection.projection, perspective(look(...))).

Tolerances are test_gpu_parity's: outputs rtol = atol = 1e-5, gradients 1e-4 of the reference's scale.
At the inputs drawn here (z >= 1.13, mostly above 1.4) float32 torch itself stays under 2 % of the output tolerance and
under 0.3 % of every gradient tolerance against float64.  The two ten_blocks cases (2500 vertices per item, seeds
as drawn: nothing was picked) use 2.2 % and 1.7 % of the output tolerance and at most 0.4 % of a gradient
tolerance (R's), far below the quarter a reference may use."""
import functools
import os

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import camera
from conftest import DATA
from test_projection import look_at_as_krt

pytestmark = pytest.mark.gpu

OUT_TOL = 1e-5
GRAD_TOL = 1e-4
S = 64
NAMES = ("vertices", "K", "R", "t", "dist")


def close_grads(a, b, what):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = float(b.abs().max())
    err = (a - b).abs()
    bad = err > GRAD_TOL * scale + GRAD_TOL * b.abs()
    assert not bad.any(), "%s: %d of %d elements off, max |d| %g (scale %g)" % (
        what, int(bad.sum()), bad.numel(), float(err.max()), scale)


def close_out(a, b, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    assert bool((err <= OUT_TOL + OUT_TOL * b.abs()).all()), "%s: max |d| %g" % (what, float(err.max()))


def rotations(r, n):
    q = np.linalg.qr(r.normal(size=(n, 3, 3)))[0]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]  # proper: det = +1
    return q


CASES = {  # name: (B, V, shared mesh, shared parameters)
    "one": (1, 1, False, False),
    "partial_wave": (3, 67, False, False),
    "two_blocks": (2, 300, False, False),
    "shared_mesh": (4, 300, True, False),
    "shared_params": (3, 129, False, True),
    "ten_blocks": (3, 2500, False, False),               # 10 slab records per item: k_proj_params' slices loop twice
    "ten_blocks_shared_params": (3, 2500, False, True),  # 30 records summed in block 0: up to four trips
}


@functools.lru_cache(maxsize=None)
def case(name):
    """Float64 CPU leaves, the upstream gradient, and the float64 reference output and gradients."""
    B, V, shared_mesh, shared_params = CASES[name]
    r = np.random.RandomState(sum(map(ord, name)))
    n = 1 if shared_params else B
    K = np.zeros((n, 3, 3))
    K[:, 0, 0], K[:, 1, 1] = r.uniform(1.5, 2.5, n) * S, r.uniform(1.5, 2.5, n) * S
    K[:, 0, 1], K[:, 1, 0] = r.uniform(-0.05, 0.05, n) * S, r.uniform(-0.05, 0.05, n) * S
    K[:, 0, 2], K[:, 1, 2] = r.uniform(0.45, 0.55, n) * S, r.uniform(0.45, 0.55, n) * S
    K[:, 2, 2] = 1.
    t = np.concatenate((r.uniform(-0.2, 0.2, (n, 2)), r.uniform(2., 3., (n, 1))), 1)
    d = r.uniform(-0.1, 0.1, (n, 5))
    d[:, 2:4] = r.uniform(-0.01, 0.01, (n, 2))  # (k1, k2, p1, p2, k3)
    leaves = {"vertices": r.uniform(-0.5, 0.5, (1 if shared_mesh else B, V, 3)), "K": K, "R": rotations(r, n), "t": t, "dist": d}
    leaves = {k: torch.as_tensor(x, dtype=torch.float64) for k, x in leaves.items()}
    g = torch.as_tensor(r.normal(size=(B, V, 3)))
    out, grads = run(leaves, g, torch.device("cpu"), torch.float64, nr.projection)
    return leaves, g, out, grads


def run(leaves, g, device, dtype, fn, requires=NAMES):
    """fn on fresh leaves of the given device and dtype; returns the output and {name: gradient}."""
    B = g.shape[0]
    x = {k: v.detach().clone().to(device=device, dtype=dtype).requires_grad_(k in requires) for k, v in leaves.items()}
    verts = x["vertices"]
    if verts.shape[0] != B:
        verts = verts.expand(B, -1, -1)  # a batch-expanded mesh
    out = fn(verts, x["K"], x["R"], x["t"], x["dist"], S)
    out.backward(g.to(device=device, dtype=dtype))
    return out.detach(), {k: x[k].grad for k in NAMES}


@pytest.mark.parametrize("name", sorted(CASES))
def test_projection_matches_float64(dev, name):
    leaves, g, ref_out, ref = case(name)
    out, grads = run(leaves, g, dev, torch.float32, camera.projection_transform)
    torch.cuda.synchronize()
    close_out(out, ref_out, name)
    assert float(ref_out[..., 2].min()) >= 2. - 0.5 * 3 ** 0.5  # t_z >= 2, |v| <= sqrt(3) / 2: well in front
    for k in NAMES:
        assert grads[k] is not None and grads[k].shape == leaves[k].shape, (k, grads[k])
        close_grads(grads[k], ref[k], "%s grad %s" % (name, k))
    assert float(grads["K"][:, 2].abs().max()) == 0.


@pytest.mark.parametrize("only", ["t", "vertices", "dist"])
def test_projection_gradient_subsets(dev, only):
    """Only the leaves that require a gradient get one, and it is the all-on run's."""
    leaves, g, _, _ = case("partial_wave")
    out_all, all_on = run(leaves, g, dev, torch.float32, camera.projection_transform)
    out, grads = run(leaves, g, dev, torch.float32, camera.projection_transform, requires=(only,))
    torch.cuda.synchronize()
    assert torch.equal(out, out_all)
    for k in NAMES:
        if k == only:
            assert torch.equal(grads[k], all_on[k]), k
        else:
            assert grads[k] is None, k


def test_projection_parameter_gradients_are_deterministic(dev):
    leaves, g, _, _ = case("shared_mesh")
    x = {k: v.to(device=dev, dtype=torch.float32).requires_grad_(True) for k, v in leaves.items()}
    out = camera.projection_transform(x["vertices"].expand(g.shape[0], -1, -1), x["K"], x["R"], x["t"], x["dist"], S)
    gd = g.to(device=dev, dtype=torch.float32)
    params = [x[k] for k in ("K", "R", "t", "dist")]
    first = torch.autograd.grad(out, params, gd, retain_graph=True)
    second = torch.autograd.grad(out, params, gd)
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    _, fresh = run(leaves, g, dev, torch.float32, camera.projection_transform)
    for k, a in zip(("K", "R", "t", "dist"), first):
        assert torch.equal(a, fresh[k]), k


@pytest.mark.parametrize("B,V", [(0, 5), (2, 0)])
def test_projection_empty(dev, B, V):
    x = {"vertices": torch.zeros(B, V, 3), "K": torch.eye(3).repeat(1, 1, 1), "R": torch.eye(3).repeat(max(B, 1), 1, 1),
         "t": torch.tensor([[0., 0., 2.]]), "dist": torch.zeros(max(B, 1), 5)}
    x = {k: v.to(dev).requires_grad_(True) for k, v in x.items()}
    out = camera.projection_transform(x["vertices"], x["K"], x["R"], x["t"], x["dist"], S)
    assert out.shape == (B, V, 3)
    out.sum().backward()
    torch.cuda.synchronize()
    for k in NAMES:
        assert x[k].grad is not None and x[k].grad.shape == x[k].shape, k
        assert float(x[k].grad.abs().sum()) == 0., k


# ---- fused look ----
@pytest.mark.parametrize("perspective", [True, False])
@pytest.mark.parametrize("direction", [[0., 0., 1.], [0.3, -0.2, 1.]])
@pytest.mark.parametrize("shared_eye", [False, True])
@pytest.mark.parametrize("B", [2, 3])
def test_fused_look_matches_float64(dev, B, shared_eye, direction, perspective):
    r = np.random.RandomState(10 * B + shared_eye)
    V = 67
    v64 = torch.as_tensor(r.uniform(-0.5, 0.5, (B, V, 3))).requires_grad_(True)
    n = 1 if shared_eye else B
    eye = np.concatenate((r.uniform(-0.3, 0.3, (n, 2)), r.uniform(-3., -2.5, (n, 1))), 1)
    e64 = torch.as_tensor(eye[0] if shared_eye else eye).requires_grad_(True)
    g = torch.as_tensor(r.normal(size=(B, V, 3)))
    f64 = lambda x: torch.tensor(x, dtype=torch.float64)
    ref = nr.look(v64, e64, f64(direction), f64([0., 1., 0.]))
    if perspective:
        ref = nr.perspective(ref, angle=f64(30.))
    ref.backward(g)

    v32 = v64.detach().float().to(dev).requires_grad_(True)
    e32 = e64.detach().float().to(dev).requires_grad_(True)
    out = camera.camera_transform(v32, e32, perspective=perspective, angle=30., direction=direction)
    out.backward(g.float().to(dev))
    torch.cuda.synchronize()
    close_out(out, ref, "look")
    assert e32.grad.shape == e64.shape
    close_grads(v32.grad, v64.grad, "look grad vertices")
    close_grads(e32.grad, e64.grad, "look grad eye")


def test_renderer_look_routes_to_the_fused_path(dev):
    r = np.random.RandomState(5)
    v = torch.as_tensor(r.uniform(-0.5, 0.5, (2, 40, 3)).astype(np.float32), device=dev)
    ren = nr.Renderer()
    ren.camera_mode = 'look'
    ren.viewpoints = torch.tensor([[0.1, 0.2, -2.7], [-0.2, 0.1, -2.6]], device=dev)
    ren.camera_direction = [0.3, -0.2, 1.]
    fused = ren.transform_vertices(v)
    assert torch.equal(fused, camera.camera_transform(v, ren.viewpoints, direction=ren.camera_direction))
    # per-item directions keep the torch composition; the first item is the fused result
    ren.camera_direction = torch.tensor([[0.3, -0.2, 1.], [0., 0., 1.]], device=dev)
    composed = ren.transform_vertices(v)
    close_out(fused[:1], composed[:1], "look composition")
    assert not torch.allclose(fused[1], composed[1], atol=1e-3)


# ---- end to end ----
def test_renderer_projection_end_to_end(dev):
    v_np, f_np = nr.load_obj(os.path.join(DATA, "teapot.obj"))
    B = 2
    v = torch.as_tensor(v_np, device=dev)[None].expand(B, -1, -1)
    faces = torch.as_tensor(f_np, device=dev)
    eyes = torch.as_tensor(np.stack([nr.get_points_from_angles(2.732, 0, 0), nr.get_points_from_angles(2.732, 30, 40)]),
                           dtype=torch.float32)
    K, R, t = look_at_as_krt(eyes, 30., S)

    ren = nr.Renderer()
    ren.image_size = 64
    ren.camera_mode = 'projection'
    ren.orig_size = S
    ren.K, ren.R, ren.t = [x.float().to(dev).requires_grad_(True) for x in (K, R, t)]
    sil = ren.render_silhouettes(v, faces)
    proj = camera.projection_transform(v, ren.K, ren.R, ren.t, None, S)
    proj.retain_grad()
    param = nr.RasterizeParam(background_color=ren.background_color, backgrounds=None)
    direct = nr.rasterize_silhouettes(proj, faces, param, ren._hyper())
    assert torch.equal(sil, direct)

    look = nr.Renderer()
    look.image_size = 64
    look.viewpoints = eyes.to(dev)
    sil_look = look.render_silhouettes(v, faces)
    assert sil_look.shape == sil.shape and float(sil_look.sum()) > 100.
    flips = int((sil_look != sil).sum())
    assert flips <= 0.001 * sil.numel(), flips

    # the gradients that reach the Renderer's K, R, t; then the same loss through `direct`, whose
    # projected-vertex gradient is at hand (the raster backward adds with float atomics: the two agree
    # within the gradient tolerance, not bit for bit)
    w = torch.as_tensor(np.random.RandomState(8).normal(size=tuple(sil.shape)).astype(np.float32), device=dev)
    (sil * w).sum().backward()
    through_renderer = {"K": ren.K.grad, "R": ren.R.grad, "t": ren.t.grad}
    ren.K.grad = ren.R.grad = ren.t.grad = None
    (direct * w).sum().backward()
    torch.cuda.synchronize()
    got = {"K": ren.K.grad, "R": ren.R.grad, "t": ren.t.grad}
    k2, r2, t2 = [x.detach().clone().requires_grad_(True) for x in (ren.K, ren.R, ren.t)]
    again = torch.autograd.grad(camera.projection_transform(v, k2, r2, t2, None, S), [k2, r2, t2], proj.grad)
    k64, r64, t64 = [x.detach().cpu().double().requires_grad_(True) for x in (ren.K, ren.R, ren.t)]
    ref = torch.autograd.grad(nr.projection(v.cpu().double(), k64, r64, t64, None, S), [k64, r64, t64],
                              proj.grad.cpu().double())
    for name, a, b in zip(("K", "R", "t"), again, ref):
        gq = got[name]
        assert gq is not None and torch.isfinite(gq).all() and float(gq.abs().max()) > 0., name
        assert torch.equal(gq, a), name
        close_grads(gq, b, "end to end grad " + name)
        gr = through_renderer[name]
        assert gr is not None and gr.shape == gq.shape and torch.isfinite(gr).all() and float(gr.abs().max()) > 0., name
        close_grads(gr, b, "Renderer grad " + name)


def test_projection_graph_capture_matches_eager(dev):
    """Forward + backward issue no host synchronisation and no allocation of their own: one linear
    capture, whose replay equals the eager run bit for bit (the sums have a fixed order)."""
    leaves, g, _, _ = case("two_blocks")
    x = {k: v.to(device=dev, dtype=torch.float32).requires_grad_(True) for k, v in leaves.items()}
    gd = g.to(device=dev, dtype=torch.float32)

    def step():
        out = camera.projection_transform(x["vertices"], x["K"], x["R"], x["t"], x["dist"], S)
        out.backward(gd)
        return out.detach()

    def clear():
        for k in NAMES:
            x[k].grad = None

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            clear()
            eager = step().clone()
    torch.cuda.current_stream().wait_stream(side)
    eager_grads = {k: x[k].grad.clone() for k in NAMES}
    clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    for k in NAMES:
        assert torch.equal(x[k].grad, eager_grads[k]), k

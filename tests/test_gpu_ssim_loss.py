"""The fused SSIM loss on the GPU (float32) against the torch composition in float64 on the CPU.

Inputs are drawn in float64 and rounded to float32 once, so both sides see the same numbers.  Two kinds:
`uniform` (x, t i.i.d. in [0, 1)) and `render` (a zero background with a shaded disc, x noisy and shifted
against t: flat dark regions, where float32 cancels against C2).  The upstream gradient is N(0, 1) per item.

Tolerances: the loss at the project's rtol = atol = 1e-5.  The gradient in the project's form,
tol max|ref| + tol |ref|, with tol = max(1e-4, 4 e32) per case, where e32 is the largest gradient error of
the float32 CPU composition against the float64 one on the same inputs over max|ref|, computed by the test:
another summation order and the saved-map form of the backward cannot be expected to round better than a
few times the reference's own float32 rounding.  Every case prints e32 and the fused path's error in the
same unit.

Measured (MI355X; T = 32; the loss error stayed under 5.2e-7 in every case):

  uniform, every case:   e32 2.0e-7 .. 1.1e-6   fused 1.2e-7 .. 9.7e-7   tol 1e-4

  render          e32      fused    tol       | render          e32      fused    tol
  all_halo        3.1e-08  3.1e-08  1.00e-04  | window3_same    5.2e-05  4.9e-05  2.07e-04
  one_pixel       1.0e-06  8.3e-07  1.00e-04  | window3_valid   3.9e-05  3.9e-05  1.55e-04
  partial_same    3.4e-06  3.3e-06  1.00e-04  | window5_same    4.0e-05  4.1e-05  1.58e-04
  partial_valid   4.1e-06  3.8e-06  1.00e-04  | window5_valid   3.4e-05  3.3e-05  1.34e-04
  odd_same        2.8e-05  2.4e-05  1.14e-04  | window7_same    1.4e-05  1.6e-05  1.00e-04
  odd_valid       1.9e-05  1.6e-05  1.00e-04  | window7_valid   8.7e-06  8.3e-06  1.00e-04
  many_tiles      3.1e-05  2.9e-05  1.24e-04  | window9_same    4.1e-06  3.6e-06  1.00e-04
  range255        4.6e-06  4.2e-06  1.00e-04  | window9_valid   5.1e-06  5.9e-06  1.00e-04

The fused path sits at the float32 composition's own error, at most 0.26 of the bound. Through the
renderer (test_with_the_renderer): vertex gradient 6e-8 of scale 0.122, texture gradient 7e-9 of scale 3.6e-3.
"""
import functools

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import _lib, image_loss, synthetic

pytestmark = pytest.mark.gpu

OUT_TOL = 1e-5
GRAD_TOL = 1e-4
T = _lib.NR_SSIM_TILE
MANY = 7 * T + 8  # 8 x 8 tiles a channel: with 5 channels 320 tiles per item, the finish loop's second trip

# name -> (shape, padding, window_size, sigma, data_range)
CASES = {
    "all_halo": ((2, 1, 3, 5), "same", 11, 1.5, 1.0),      # the image is smaller than the window
    "one_pixel": ((1, 1, 11, 11), "valid", 11, 1.5, 1.0),  # a one-pixel map
    "partial_same": ((2, 3, T + 1, T + 15), "same", 11, 1.5, 1.0),   # partial tiles in both axes, W no multiple of 4
    "partial_valid": ((2, 3, T + 1, T + 15), "valid", 11, 1.5, 1.0),
    "odd_same": ((3, 1, 2 * T + 3, 2 * T + 3), "same", 11, 1.5, 1.0),  # odd N: items 1 and 2 sit off 16 bytes
    "odd_valid": ((3, 1, 2 * T + 3, 2 * T + 3), "valid", 11, 1.5, 1.0),
    "many_tiles": ((2, 5, MANY, MANY), "same", 11, 1.5, 1.0),
    "range255": ((2, 3, T + 1, T + 15), "same", 11, 1.5, 255.0),
}
for _w, _s in ((3, 0.8), (5, 1.0), (7, 1.5), (9, 2.0)):
    for _p in ("same", "valid"):
        CASES["window%d_%s" % (_w, _p)] = ((3, 1, 2 * T + 3, 2 * T + 3), _p, _w, _s, 1.0)
KINDS = ("uniform", "render")


def draw(kind, shape, seed, data_range=1.0):
    """(x, t, g) float64 CPU tensors whose values are float32 numbers."""
    rs = np.random.RandomState(seed)
    B, C, H, W = shape
    if kind == "uniform":
        x, t = rs.uniform(0, 1, shape), rs.uniform(0, 1, shape)
    else:
        row, col = np.mgrid[0:H, 0:W].astype(np.float64)
        shade = np.stack([0.5 + 0.4 * np.sin(col / 5 + c) * np.cos(row / 7) for c in range(C)])
        r = 0.3 * min(H, W)

        def disc(cx):
            return ((col - cx * W) ** 2 + (row - 0.5 * H) ** 2 <= r * r).astype(np.float64)
        x = np.clip(shade[None] + rs.uniform(-0.05, 0.05, shape), 0, 1) * disc(0.45)
        t = np.broadcast_to(shade * disc(0.55), shape)
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a * data_range, dtype=np.float32)).double()
    return f32(x), f32(t), torch.as_tensor(rs.normal(size=B).astype(np.float32)).double()


def composition(x, t, g, **kw):
    """Loss and gradient to x of the CPU composition in the dtype of x."""
    y = x.clone().requires_grad_(True)
    out = nr.ssim_loss_torch(y, t.to(x.dtype), **kw)
    out.backward(g.to(x.dtype))
    return out.detach(), y.grad


def kwargs_of(name):
    _, padding, window_size, sigma, data_range = CASES[name]
    return dict(window_size=window_size, sigma=sigma, data_range=data_range, padding=padding)


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """Inputs, the float64 reference (loss, gradient) and e32 of one case."""
    x, t, g = draw(kind, CASES[name][0], sum(map(ord, name + kind)), CASES[name][4])
    kw = kwargs_of(name)
    want, want_grad = composition(x, t, g, **kw)
    _, grad32 = composition(x.float(), t, g, **kw)
    scale = float(want_grad.abs().max())
    e32 = float((grad32.double() - want_grad).abs().max()) / scale if scale else 0.
    return x, t, g, want, want_grad, e32


def to_dev(t, dev):
    return t.to(device=dev, dtype=torch.float32)


def fused(x, t, g, **kw):
    """Loss and gradient of the fused path for float32 GPU tensors."""
    y = x.detach().requires_grad_(True)
    out = nr.ssim_loss(y, t, **kw)
    out.backward(g if out.ndim else None)
    return out.detach(), y.grad


def close_out(a, b, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    assert bool((err <= OUT_TOL + OUT_TOL * b.abs()).all()), "%s: max |d| %g of %s" % (what, float(err.max()), b.tolist())


def close_grads(a, b, what, tol=GRAD_TOL):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = float(b.abs().max()) if b.numel() else 0.
    err = (a - b).abs()
    bad = err > tol * scale + tol * b.abs()
    assert not bad.any(), "%s: %d of %d elements off, max |d| %g (scale %g, tol %g)" % (
        what, int(bad.sum()), bad.numel(), float(err.max()), scale, tol)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(CASES))
def test_fused_matches_float64(dev, name, kind):
    x, t, g, want, want_grad, e32 = case(name, kind)
    out, grad = fused(to_dev(x, dev), to_dev(t, dev), to_dev(g, dev), **kwargs_of(name))
    assert out.dtype == torch.float32 and out.shape == (x.shape[0],) and grad.shape == x.shape
    scale = float(want_grad.abs().max())
    err = float((grad.cpu().double() - want_grad).abs().max()) / scale
    tol = max(GRAD_TOL, 4 * e32)
    print("%s %s: loss err %.2e, e32 %.2e, fused grad err %.2e, tol %.2e" % (
        name, kind, float((out.cpu().double() - want).abs().max()), e32, err, tol))
    close_out(out, want, name)
    close_grads(grad, want_grad, name + " grad", tol)


def test_cases_reach_their_paths():
    assert CASES["many_tiles"][0][1] * ((MANY + T - 1) // T) ** 2 >= 257
    H, W = CASES["partial_same"][0][2:]
    assert H % T and W % T and W % 4 and H > T and W > T
    N = int(np.prod(CASES["odd_same"][0][1:]))
    assert N % 4 and (2 * N) % 4
    x, t, *_ = case("partial_same", "render")
    assert float((x == 0).double().mean()) > 0.3 and float((t == 0).double().mean()) > 0.3  # a real zero background


@pytest.mark.parametrize("view", ["alpha", "colour"])
def test_strided_items_are_read_in_place(dev, view, monkeypatch):
    """rgba[:, 3] and rgba[:, :3]: each item is one contiguous run at the batch stride of rgba, so the kernels
    read the view's own memory (no copy) and give what they give for a contiguous copy, bit for bit."""
    rgba64, _, g64 = draw("uniform", (2, 4, T + 3, T + 2), 5)
    sel = (lambda a: a[:, 3]) if view == "alpha" else (lambda a: a[:, :3])
    t64 = draw("uniform", sel(rgba64).shape if view == "colour" else (2, 1, T + 3, T + 2), 6)[1].reshape(sel(rgba64).shape)
    want, want_grad = composition(sel(rgba64), t64, g64)
    rgba, t, g = to_dev(rgba64, dev), to_dev(t64, dev), to_dev(g64, dev)
    leaf = rgba.clone().requires_grad_(True)
    images = sel(leaf)
    assert not images.is_contiguous()
    seen = []
    real_ptr = image_loss._lib.ptr
    monkeypatch.setattr(image_loss._lib, "ptr", lambda a: seen.append(None if a is None else a.data_ptr()) or real_ptr(a))
    out = nr.ssim_loss(images, t)
    assert images.data_ptr() in seen  # the kernel was given the view's own memory
    assert images.data_ptr() == leaf.data_ptr() + 4 * images.storage_offset()
    out.backward(g)
    monkeypatch.undo()
    close_out(out, want, "strided")
    close_grads(sel(leaf.grad), want_grad, "strided grad")
    rest = leaf.grad[:, :3] if view == "alpha" else leaf.grad[:, 3]
    assert float(rest.abs().max()) == 0.  # the other channels take no gradient
    copy_out, copy_grad = fused(sel(rgba).contiguous(), t, g)
    assert torch.equal(out.detach(), copy_out) and torch.equal(sel(leaf.grad), copy_grad)


def test_other_layouts_are_copied(dev):
    """x[..., ::2] is not item-contiguous: the copy fallback gives the values of a contiguous tensor."""
    wide64, _, g64 = draw("uniform", (2, 1, 16, 2 * T + 6), 7)
    t64 = draw("uniform", (2, 1, 16, T + 3), 8)[1]
    want, want_grad = composition(wide64[..., ::2], t64, g64)
    t, g = to_dev(t64, dev), to_dev(g64, dev)
    leaf = to_dev(wide64, dev).requires_grad_(True)
    out = nr.ssim_loss(leaf[..., ::2], t)
    out.backward(g)
    close_out(out, want, "every other column")
    close_grads(leaf.grad[..., ::2], want_grad, "every other column grad")
    assert float(leaf.grad[..., 1::2].abs().max()) == 0.
    copy_out, copy_grad = fused(leaf.detach()[..., ::2].contiguous(), t, g)
    assert torch.equal(out.detach(), copy_out) and torch.equal(leaf.grad[..., ::2], copy_grad)


@pytest.mark.parametrize("padding", ["same", "valid"])
def test_target_forms_are_bit_identical(dev, padding):
    x64, t64, g64 = draw("uniform", (3, 2, T + 5, T + 1), 9)
    x, t, g = to_dev(x64, dev), to_dev(t64, dev), to_dev(g64, dev)
    want, want_grad = composition(x64, t64[:1], g64, padding=padding)
    results = [fused(x, form, g, padding=padding) for form in (
        t[:1].expand(3, -1, -1, -1).contiguous(), t[:1].contiguous(), t[0].contiguous(), t[0][None].expand(3, -1, -1, -1))]
    close_out(results[0][0], want, "shared target")
    close_grads(results[0][1], want_grad, "shared target grad")
    for out, grad in results[1:]:
        assert torch.equal(out, results[0][0]) and torch.equal(grad, results[0][1])
    # [B, H, W] is [B, 1, H, W]
    a, b = fused(x[:, 0], t[0, 0], g, padding=padding), fused(x[:, :1].contiguous(), t[:1, :1].contiguous(), g, padding=padding)
    assert a[1].shape == (3, T + 5, T + 1) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1][:, 0])


@pytest.mark.parametrize("name", ["odd_valid", "partial_same"])
def test_runs_are_bitwise_reproducible(dev, name):
    x, t, g, *_ = case(name, "render")
    x, t, g = to_dev(x, dev), to_dev(t, dev), to_dev(g, dev)
    first = fused(x, t, g, **kwargs_of(name))
    for _ in range(2):
        again = fused(x, t, g, **kwargs_of(name))
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


class Spy:
    """The library with a record of (entry point, arguments) of every call made through it."""

    def __init__(self, L):
        self.L, self.calls = L, []

    def __getattr__(self, name):
        fn = getattr(self.L, name)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


def test_no_gradient_needed(dev, monkeypatch):
    """Images that take no gradient: the same loss, no saved maps, and no backward launch."""
    x, t, g, *_ = case("partial_valid", "uniform")
    x, t, g = to_dev(x, dev), to_dev(t, dev), to_dev(g, dev)
    with_grad, _ = fused(x, t, g, padding="valid")
    spy = Spy(image_loss._lib.lib())
    monkeypatch.setattr(image_loss._lib, "lib", lambda: spy)
    plain = nr.ssim_loss(x, t, padding="valid")
    assert not plain.requires_grad and plain.grad_fn is None
    assert torch.equal(plain, with_grad)
    w = torch.ones(x.shape[0], device=dev, requires_grad=True)
    (nr.ssim_loss(x, t, padding="valid") * w).sum().backward()
    assert torch.equal(w.grad, plain)
    forwards = [args for name, args in spy.calls if name == "nr_ssim_loss_forward"]
    assert len(forwards) == 2 and all(args[14].value is None for args in forwards)  # saved: a null pointer
    assert not [name for name, _ in spy.calls if name == "nr_ssim_loss_backward"]
    # and with a gradient the maps are there
    nr.ssim_loss(x.clone().requires_grad_(True), t, padding="valid").backward(g)
    assert [args[14].value for name, args in spy.calls if name == "nr_ssim_loss_forward"][-1] is not None
    assert [name for name, _ in spy.calls].count("nr_ssim_loss_backward") == 1


def test_other_operands_reach_the_composition(dev, monkeypatch):
    """On the GPU too: targets that require grad, float64 images and a window of 13 never reach the library."""
    x64, t64, g64 = draw("uniform", (2, 2, 20, 21), 10)

    def boom():
        raise AssertionError("the fused path was taken")
    monkeypatch.setattr(image_loss._lib, "lib", boom)
    x = to_dev(x64, dev).requires_grad_(True)
    t = to_dev(t64, dev).requires_grad_(True)
    out = nr.ssim_loss(x, t)
    out.sum().backward()
    assert t.grad is not None and x.grad is not None and torch.equal(out, nr.ssim_loss_torch(x, t))
    assert nr.ssim_loss(x64.to(dev), t64.to(dev)).dtype == torch.float64
    assert nr.ssim_loss(x.detach(), t64.to(dev)).dtype == torch.float64  # mixed dtypes
    out13 = nr.ssim_loss(x, t.detach(), window_size=13, sigma=2.0)
    assert torch.equal(out13, nr.ssim_loss_torch(x, t.detach(), window_size=13, sigma=2.0))
    close_out(out13, composition(x64, t64, g64, window_size=13, sigma=2.0)[0], "window 13")
    for kw in (dict(window_size=4), dict(padding="reflect"), dict(sigma=0.)):
        with pytest.raises(ValueError):
            nr.ssim_loss(x, t.detach(), **kw)
    with pytest.raises(ValueError):
        nr.ssim_loss(x, t.detach()[:, :, :-1])
    with pytest.raises(ValueError):
        nr.ssim_loss(x[:, :, :10], t.detach()[:, :, :10], padding="valid")


@pytest.mark.parametrize("shape", [(0, 3, 8, 8), (2, 3, 0, 8)])
def test_empty_batch_and_empty_items(dev, shape):
    x = torch.zeros(shape, device=dev, requires_grad=True)
    out = nr.ssim_loss(x, torch.zeros(shape, device=dev))
    assert out.shape == (shape[0],) and out.dtype == torch.float32
    assert torch.equal(out.detach().cpu(), torch.zeros(shape[0]))
    out.sum().backward()
    assert x.grad is not None and x.grad.shape == shape


def test_average_and_module(dev):
    x, t, g, want, want_grad, _ = case("partial_same", "uniform")
    x, t = to_dev(x, dev), to_dev(t, dev)
    per_item, _ = fused(x, t, to_dev(g, dev))
    avg, avg_grad = fused(x, t, None, average=True)
    assert avg.ndim == 0
    torch.testing.assert_close(avg, per_item.mean(), rtol=1e-6, atol=0)
    ones_grad = composition(x.cpu().double(), t.cpu().double(), torch.full((2,), 0.5))[1]
    close_grads(avg_grad, ones_grad, "average grad")
    mod = nr.SSIMLoss(t[0], window_size=7, sigma=1.2, data_range=2.0, padding="valid", average=True).to(dev)
    assert mod.targets.device.type == "cuda" and "targets" in dict(mod.named_buffers())
    y = x.clone().requires_grad_(True)
    out = mod(y)
    out.backward()
    f_out, f_grad = fused(x, t[0], None, window_size=7, sigma=1.2, data_range=2.0, padding="valid", average=True)
    assert torch.equal(out.detach(), f_out) and torch.equal(y.grad, f_grad)


def test_graph_capture_matches_eager(dev):
    """The loss with both paddings and its backward captured in a HIP graph and replayed after the images
    changed in place: bit for bit the eager results on the new values."""
    x64, t64, g64, *_ = case("odd_same", "render")
    t, g = to_dev(t64, dev), to_dev(g64, dev)
    x = to_dev(x64, dev).requires_grad_(True)
    moved = to_dev(draw("render", CASES["odd_same"][0], 99)[0], dev)

    def step(y):
        same = nr.ssim_loss(y, t)
        valid = nr.ssim_loss(y, t[0], window_size=7, padding="valid")
        (same + 0.5 * valid).backward(g)
        return same, valid

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            x.grad = None
            before = [o.detach().clone() for o in step(x)]  # detached: no autograd graph outlives the warm-up
    torch.cuda.current_stream().wait_stream(side)
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(x)
    with torch.no_grad():
        x.copy_(moved)
    graph.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in outs] + [x.grad.clone()]
    e = moved.clone().requires_grad_(True)
    want = list(step(e)) + [e.grad]
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    for a, b in zip(got, before):
        assert not torch.equal(a, b)  # the replay saw the new images


def test_with_the_renderer(dev):
    """An rgb render of a textured icosphere at 32 x 32 against a render from a shifted viewpoint: loss,
    vertex and texture gradients through the fused loss agree with those through the composition on the
    same render at the rasterizer's own gradient tolerance (its float atomics keep two backward passes from
    being bitwise equal)."""
    v, f = synthetic.icosphere(1)
    faces = torch.as_tensor(f, device=dev)
    vt, ft, tex = nr.create_textures(f.shape[0], texture_size=4)
    tex = np.random.RandomState(3).uniform(0, 1, tex.shape).astype(np.float32)
    vt, ft = torch.as_tensor(vt, device=dev)[None].expand(2, -1, -1), torch.as_tensor(ft, device=dev)
    textures = torch.as_tensor(tex, device=dev).requires_grad_(True)
    ren = nr.Renderer()
    ren.image_size = 32
    ren.viewpoints = nr.get_points_from_angles(3.4, 10, 40)
    with torch.no_grad():
        target = ren.render_rgb(torch.as_tensor(synthetic.jittered(v, 2), device=dev), faces, vt, ft,
                                textures.detach()[None].expand(2, -1, -1, -1)).contiguous()
    ren.viewpoints = nr.get_points_from_angles(2.732, 30, -15)
    verts = torch.as_tensor(synthetic.jittered(v, 2), device=dev).requires_grad_(True)
    rgb = ren.render_rgb(verts, faces, vt, ft, textures[None].expand(2, -1, -1, -1))
    assert rgb.shape == (2, 3, 32, 32) and float((rgb.detach() - target).abs().max()) > 0.2
    g = torch.as_tensor([1., -0.5], device=dev)
    out, want = nr.ssim_loss(rgb, target), nr.ssim_loss_torch(rgb, target)
    assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith("SSIMLossFunction")
    close_out(out, want, "ssim_loss")
    got = torch.autograd.grad(out, (verts, textures), g, retain_graph=True)
    ref = torch.autograd.grad(want, (verts, textures), g, retain_graph=True)
    for what, a, b in zip(("vertex", "texture"), got, ref):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        scale, err = float(b.abs().max()), float((a - b).abs().max())
        print("ssim_loss: %s grad max |d| %.3g of scale %.3g" % (what, err, scale))
        assert err <= 1e-4 * scale, (what, err, scale)

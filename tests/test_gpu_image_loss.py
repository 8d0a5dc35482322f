"""The fused squared-error, Huber and IoU image losses on the GPU (float32) against the torch composition in
float64 on the CPU.

Tolerances are test_gpu_mesh_loss's: losses rtol = atol = 1e-5, gradients 1e-4 of the reference gradient's
largest magnitude plus 1e-4 relative.  On these inputs (images uniform in [0, 1), targets 0 / 1 or uniform,
weights uniform in [0, 2), upstream gradient N(0, 1) per item) float32 torch on the CPU stays under 1 % of
both tolerances against float64, so the reference alone is well inside them; that holds for the shapes of
more than 256 chunks per item too (many_chunks: 0.4 % of the loss and 0.2 % of the gradient tolerance,
many_chunks_odd: 0.7 % and 0.2 %) and for wrap_small and wrap_straddle (0.8 % and 0.2 %); wrap_small_chunks
uses 1.1 % of the loss tolerance (Huber, full weights) and 0.2 % of the gradient's."""
import functools

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import image_loss, synthetic

pytestmark = pytest.mark.gpu

OUT_TOL = 1e-5
GRAD_TOL = 1e-4
DELTA = 0.25

SHAPES = {
    "tiny": (2, 1, 1, 3),       # fewer elements than a wave, N no multiple of 4
    "tail": (2, 3, 5, 7),       # N = 105: a scalar tail; mask period 35: scalar weight loads
    "odd": (3, 1, 67, 67),      # N = 4489, odd: items 1 and 2 are not 16-byte aligned; two chunks, the last partial
    "aligned": (2, 5, 64, 64),  # N = 20480: five full chunks per item, five channels sharing a mask
    # vector weight loads that wrap: a mask period of 240 is below the 1024 elements between a lane's loads, so
    # every lane's offset advances by 1024 % 240 = 64 per load and wraps.  N = 720 is less than those 1024
    # elements: only a lane's first load counts, at an offset of i0 % period in the second and third period
    "wrap_small": (2, 3, 12, 20),
    # the same period with N = 4800: one full chunk, where all four loads of a lane count and their offsets
    # wrap at different loads from lane to lane, and a partial one that starts inside a period (4096 % 240 = 16)
    "wrap_small_chunks": (2, 20, 12, 20),
    # N = 11520, mask period 2304: chunks 1 and 2 start inside a period, and a lane's later loads cross its end
    "wrap_straddle": (2, 5, 48, 48),
    # more than 256 partials per item, so the second stage's strided loop takes a second trip:
    # N = 1310720 is 320 chunks on the vector path (mask period 262144)
    "many_chunks": (2, 5, 512, 512),
    # N = 1050625 is 257 chunks, the last partial; N is odd, so item 1 is off 16 bytes: the scalar path
    "many_chunks_odd": (2, 1, 1025, 1025),
}
# the weight forms a shape runs with, where not all of them (the large shapes: the float64 reference costs)
FORMS = {"many_chunks": ("none", "shared_mask"), "many_chunks_odd": ("none", "shared_mask")}
# (fused, composition, extra arguments) -- the targets are binary for IoU, uniform otherwise
LOSSES = {
    "squared": (nr.squared_error_loss, nr.squared_error_loss_torch, ()),
    "huber": (nr.huber_loss, nr.huber_loss_torch, (DELTA,)),
    "iou": (nr.iou_loss, nr.iou_loss_torch, ()),
}
WEIGHTS = ("none", "full", "mask", "shared_mask")


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


def call(fn, extra, x, t, w, **kw):
    if w is None:
        return fn(x, t, *extra, **kw)
    return fn(x, t, *extra, weights=w, **kw)


def reference(loss, x, t, w, g):
    """The float64 CPU composition's loss and gradient to x (float64 CPU tensors in)."""
    y = x.clone().requires_grad_(True)
    out = call(LOSSES[loss][1], LOSSES[loss][2], y, t, w)
    out.backward(g)
    return out.detach(), y.grad


def draw(shape, seed):
    """Float64 CPU inputs of one image shape [B, C, H, W]."""
    rs = np.random.RandomState(seed)
    B, C, H, W = shape
    return {"x": torch.as_tensor(rs.uniform(0, 1, shape)), "t": torch.as_tensor(rs.uniform(0, 1, shape)),
            "tb": torch.as_tensor((rs.uniform(0, 1, shape) < 0.4).astype(np.float64)),
            "full": torch.as_tensor(rs.uniform(0, 2, shape)), "mask": torch.as_tensor(rs.uniform(0, 2, (B, 1, H, W))),
            "g": torch.as_tensor(rs.normal(size=B))}


def weights_of(d, form):
    return {"none": None, "full": d["full"], "mask": d["mask"], "shared_mask": d["mask"][:1]}[form]


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of SHAPES[name] and, per (loss, weight form), the float64 reference (loss, gradient)."""
    d = draw(SHAPES[name], sum(map(ord, name)))
    ref = {}
    for loss in LOSSES:
        for form in FORMS.get(name, WEIGHTS) if loss != "iou" else ("none",):
            ref[loss, form] = reference(loss, d["x"], d["tb" if loss == "iou" else "t"], weights_of(d, form), d["g"])
    return d, ref


def to_dev(t, dev):
    return None if t is None else t.to(device=dev, dtype=torch.float32)


def fused(loss, x, t, w, g, **kw):
    """Loss and gradient of the fused path for float32 GPU tensors."""
    y = x.detach().requires_grad_(True)
    out = call(LOSSES[loss][0], LOSSES[loss][2], y, t, w, **kw)
    out.backward(g if out.ndim else None)
    return out.detach(), y.grad


COMBOS = [(loss, form) for loss in LOSSES for form in (WEIGHTS if loss != "iou" else ("none",))]
NAMED_COMBOS = [(name, loss, form) for loss, form in COMBOS for name in SHAPES if form in FORMS.get(name, WEIGHTS)]


@pytest.mark.parametrize("name,loss,form", NAMED_COMBOS)
def test_fused_matches_float64(dev, name, loss, form):
    d, ref = case(name)
    x, t, w, g = (to_dev(a, dev) for a in (d["x"], d["tb" if loss == "iou" else "t"], weights_of(d, form), d["g"]))
    out, grad = fused(loss, x, t, w, g)
    want, want_grad = ref[loss, form]
    assert out.shape == (x.shape[0],) and out.dtype == torch.float32 and grad.shape == x.shape and grad.is_contiguous()
    print("%s %s %s: loss %s ref %s, grad max |d| %.3g of scale %.3g" % (
        name, loss, form, out.tolist(), want.tolist(), float((grad.cpu().double() - want_grad).abs().max()),
        float(want_grad.abs().max())))
    close_out(out, want, "%s %s %s" % (name, loss, form))
    close_grads(grad, want_grad, "%s %s %s grad" % (name, loss, form))


def test_huber_takes_both_branches():
    d, _ = case("aligned")
    a = (d["x"] - d["t"]).abs()
    assert bool((a < DELTA).any()) and bool((a > DELTA).any())
    assert 0.2 < float((a < DELTA).double().mean()) < 0.8


@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("view", ["alpha", "colour"])
def test_strided_items_are_read_in_place(dev, loss, view, monkeypatch):
    """rgba[:, 3] and rgba[:, :3]: each item is one contiguous run at the batch stride of rgba, so the kernels
    read the view's own memory (no copy) and give what they give for a contiguous copy, bit for bit."""
    rs = np.random.RandomState(5)
    rgba64 = torch.as_tensor(rs.uniform(0, 1, (2, 4, 32, 32)))
    sel = (lambda a: a[:, 3]) if view == "alpha" else (lambda a: a[:, :3])
    t64 = torch.as_tensor((rs.uniform(0, 1, sel(rgba64).shape) < 0.5).astype(np.float64))
    g64 = torch.as_tensor(rs.normal(size=2))
    want, want_grad = reference(loss, sel(rgba64), t64, None, g64)
    rgba, t, g = to_dev(rgba64, dev), to_dev(t64, dev), to_dev(g64, dev)
    leaf = rgba.clone().requires_grad_(True)
    images = sel(leaf)
    assert not images.is_contiguous()
    seen = []
    real_ptr = image_loss._lib.ptr
    monkeypatch.setattr(image_loss._lib, "ptr", lambda a: seen.append(None if a is None else a.data_ptr()) or real_ptr(a))
    out = call(LOSSES[loss][0], LOSSES[loss][2], images, t, None)
    assert images.data_ptr() in seen  # the kernel was given the view's own memory
    assert images.data_ptr() == leaf.data_ptr() + 4 * images.storage_offset()
    out.backward(g)
    monkeypatch.undo()
    close_out(out, want, "strided " + loss)
    close_grads(sel(leaf.grad), want_grad, "strided grad " + loss)
    rest = leaf.grad[:, :3] if view == "alpha" else leaf.grad[:, 3]
    assert float(rest.abs().max()) == 0.  # the other channels take no gradient
    copy_out, copy_grad = fused(loss, sel(rgba).contiguous(), t, None, g)
    assert torch.equal(out.detach(), copy_out) and torch.equal(sel(leaf.grad), copy_grad)


@pytest.mark.parametrize("loss", list(LOSSES))
def test_other_layouts_are_copied(dev, loss):
    """x[..., ::2] is not item-contiguous: the copy fallback gives the values of a contiguous tensor."""
    rs = np.random.RandomState(6)
    wide64 = torch.as_tensor(rs.uniform(0, 1, (2, 1, 16, 32)))
    t64 = torch.as_tensor((rs.uniform(0, 1, (2, 1, 16, 16)) < 0.5).astype(np.float64))
    g64 = torch.as_tensor(rs.normal(size=2))
    want, want_grad = reference(loss, wide64[..., ::2], t64, None, g64)
    t, g = to_dev(t64, dev), to_dev(g64, dev)
    leaf = to_dev(wide64, dev).requires_grad_(True)
    out = call(LOSSES[loss][0], LOSSES[loss][2], leaf[..., ::2], t, None)
    out.backward(g)
    close_out(out, want, "every other column " + loss)
    close_grads(leaf.grad[..., ::2], want_grad, "every other column grad " + loss)
    assert float(leaf.grad[..., 1::2].abs().max()) == 0.
    copy_out, copy_grad = fused(loss, leaf.detach()[..., ::2].contiguous(), t, None, g)
    assert torch.equal(out.detach(), copy_out) and torch.equal(leaf.grad[..., ::2], copy_grad)


@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("shape", [(0, 3, 8, 8), (2, 0)])
def test_empty_batch_and_empty_items(dev, loss, shape):
    x = torch.zeros(shape, device=dev, requires_grad=True)
    t = torch.zeros(shape, device=dev)
    out = call(LOSSES[loss][0], LOSSES[loss][2], x, t, None)
    assert out.shape == (shape[0],) and out.dtype == torch.float32
    assert torch.equal(out.detach().cpu(), torch.full((shape[0],), 1. if loss == "iou" else 0.))
    out.sum().backward()
    assert x.grad is not None and x.grad.shape == shape
    if loss != "iou" and len(shape) == 4:
        w = torch.ones((1, 1, 8, 8), device=dev)
        assert call(LOSSES[loss][0], LOSSES[loss][2], x, t, w).shape == (0,)


@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("name", ["odd", "aligned"])
def test_target_forms_are_bit_identical(dev, name, loss):
    d, _ = case(name)
    x, g = to_dev(d["x"], dev), to_dev(d["g"], dev)
    one = to_dev(d["tb" if loss == "iou" else "t"][0], dev)
    B = x.shape[0]
    per_item = one[None].expand(B, -1, -1, -1).contiguous()
    first = fused(loss, x, per_item, None, g)
    # the per-item result is right, so the others are
    want = reference(loss, d["x"], d["tb" if loss == "iou" else "t"][:1], None, d["g"])
    close_out(first[0], want[0], "shared target")
    close_grads(first[1], want[1], "shared target grad")
    for form, t in (("leading one", one[None]), ("no batch", one), ("expanded", one[None].expand(B, -1, -1, -1))):
        again = fused(loss, x, t, None, g)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), form


@pytest.mark.parametrize("loss", ["squared", "huber"])
@pytest.mark.parametrize("name", ["tail", "aligned"])
def test_weight_forms_are_bit_identical(dev, name, loss):
    d, _ = case(name)
    x, t, g = to_dev(d["x"], dev), to_dev(d["t"], dev), to_dev(d["g"], dev)
    B, C = x.shape[:2]
    for kind in ("full", "mask"):
        one = to_dev(d[kind][0], dev)
        per_item = one[None].expand(B, -1, -1, -1).contiguous()
        first = fused(loss, x, t, per_item, g)
        forms = [("leading one", one[None]), ("no batch", one), ("expanded", one[None].expand(B, -1, -1, -1))]
        if kind == "mask":  # the mask written out over the channels as full weights
            forms.append(("mask as full", per_item.expand(-1, C, -1, -1).contiguous()))
        for form, w in forms:
            again = fused(loss, x, t, w, g)
            assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), (kind, form)


def off_sixteen(w):
    """The values of the contiguous float32 tensor w as a view that starts one float into a buffer one float
    longer: w's own base is on 16 bytes (asserted), the view's is 4 past them."""
    buf = torch.empty(w.numel() + 1, dtype=w.dtype, device=w.device)
    view = buf[1:1 + w.numel()].view(w.shape)
    view.copy_(w)
    assert w.is_contiguous() and view.is_contiguous() and torch.equal(view, w)
    assert w.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4, (w.data_ptr() % 16, view.data_ptr() % 16)
    return view


@pytest.mark.parametrize("loss", ["squared", "huber"])
def test_vector_weights_equal_scalar_weights_bitwise(dev, loss):
    """Weights whose base is on 16 bytes take 16-byte loads at an offset that advances and wraps per load;
    the same values one float off 16 bytes take scalar loads at i % period in the same lanes and order.  The
    mask's H * W is a multiple of 4 at all these shapes, so the base alone decides: loss and gradient must
    be bit for bit the same, through wrapping periods (the wrap shapes) as without (aligned)."""
    for name in ("wrap_small", "wrap_small_chunks", "wrap_straddle", "aligned"):
        d, _ = case(name)
        x, t, g = to_dev(d["x"], dev), to_dev(d["t"], dev), to_dev(d["g"], dev)
        assert x.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0 and (x.shape[2] * x.shape[3]) % 4 == 0
        for form in ("mask", "shared_mask"):
            w = to_dev(weights_of(d, form), dev).contiguous()
            vector = fused(loss, x, t, w, g)
            scalar = fused(loss, x, t, off_sixteen(w), g)
            assert vector[1].data_ptr() % 16 == 0 and scalar[1].data_ptr() % 16 == 0
            assert torch.equal(vector[0], scalar[0]) and torch.equal(vector[1], scalar[1]), (name, form)
            close_out(vector[0], case(name)[1][loss, form][0], "%s %s %s" % (name, loss, form))


@pytest.mark.parametrize("loss", list(LOSSES))
def test_average_is_the_mean_over_the_items(dev, loss):
    d, ref = case("odd")
    x, t, g = to_dev(d["x"], dev), to_dev(d["tb" if loss == "iou" else "t"], dev), to_dev(d["g"], dev)
    per_item, _ = fused(loss, x, t, None, g)
    avg, grad = fused(loss, x, t, None, None, average=True)
    assert avg.ndim == 0 and torch.equal(avg, per_item.mean())
    close_out(avg, ref[loss, "none"][0].mean(), "average")
    want = reference(loss, d["x"], d["tb" if loss == "iou" else "t"], None, torch.full((x.shape[0],), 1. / x.shape[0],
                                                                                     dtype=torch.float64))[1]
    close_grads(grad, want, "average grad")


def test_modules_give_what_the_functions_give(dev):
    d, _ = case("aligned")
    x, t, tb, g = (to_dev(d[k], dev) for k in ("x", "t", "tb", "g"))
    mask = to_dev(d["mask"][:1], dev)
    for average in (False, True):
        pairs = [
            (nr.SquaredErrorLoss(t.cpu(), mask.cpu(), average=average).to(dev), lambda y: nr.squared_error_loss(y, t, mask, average)),
            (nr.SquaredErrorLoss(t, average=average), lambda y: nr.squared_error_loss(y, t, None, average)),
            (nr.HuberLoss(t, DELTA, mask, average=average), lambda y: nr.huber_loss(y, t, DELTA, mask, average)),
            (nr.IoULoss(tb[0], 1e-6, average=average), lambda y: nr.iou_loss(y, tb[0], 1e-6, average)),
        ]
        for mod, fn in pairs:
            y = x.clone().requires_grad_(True)
            out = mod(y)
            out.sum().backward()
            z = x.clone().requires_grad_(True)
            want = fn(z)
            want.sum().backward()
            assert torch.equal(out, want) and torch.equal(y.grad, z.grad), type(mod).__name__
    assert "targets" in dict(nr.HuberLoss(t, DELTA, mask).named_buffers())


@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("name", ["odd", "aligned"])
def test_runs_are_bitwise_reproducible(dev, name, loss):
    d, _ = case(name)
    x, t, g = to_dev(d["x"], dev), to_dev(d["tb" if loss == "iou" else "t"], dev), to_dev(d["g"], dev)
    w = None if loss == "iou" else to_dev(d["mask"], dev)
    first = fused(loss, x, t, w, g)
    for _ in range(2):
        again = fused(loss, x, t, w, g)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


@pytest.mark.parametrize("loss", list(LOSSES))
def test_no_gradient_needed(dev, loss, monkeypatch):
    """Images that take no gradient: the same loss, nothing saved, and no backward launch."""
    d, _ = case("tail")
    x, t, g = to_dev(d["x"], dev), to_dev(d["tb" if loss == "iou" else "t"], dev), to_dev(d["g"], dev)
    fn, _, extra = LOSSES[loss]
    with_grad, _ = fused(loss, x, t, None, g)
    L = image_loss._lib.lib()
    calls = []
    monkeypatch.setattr(image_loss._lib, "lib", lambda: calls.append(1) or L)
    plain = fn(x, t, *extra)
    assert not plain.requires_grad and plain.grad_fn is None
    assert torch.equal(plain, with_grad)
    assert len(calls) == 1  # the forward alone
    # beside another leaf that does take a gradient, the backward runs without touching the library
    w = torch.ones(x.shape[0], device=dev, requires_grad=True)
    (fn(x, t, *extra) * w).sum().backward()
    assert len(calls) == 2 and torch.equal(w.grad, plain)


@pytest.mark.parametrize("loss", list(LOSSES))
def test_operands_that_take_a_gradient_reach_the_composition(dev, loss, monkeypatch):
    """On the GPU too: a target or a weight that requires grad, and float64 images, never reach the library."""
    d, _ = case("tail")
    fn, composition, extra = LOSSES[loss]

    def boom():
        raise AssertionError("the fused path was taken")
    monkeypatch.setattr(image_loss._lib, "lib", boom)
    x = to_dev(d["x"], dev).requires_grad_(True)
    t = to_dev(d["tb" if loss == "iou" else "t"], dev).requires_grad_(True)
    out = fn(x, t, *extra)
    out.sum().backward()
    assert t.grad is not None and x.grad is not None and torch.equal(out, composition(x, t, *extra))
    if loss != "iou":
        w = to_dev(d["mask"], dev).requires_grad_(True)
        fn(x, t.detach(), *extra, weights=w).sum().backward()
        assert w.grad is not None and float(w.grad.abs().max()) > 0
    x64 = d["x"].to(dev)
    assert fn(x64, d["tb" if loss == "iou" else "t"].to(dev), *extra).dtype == torch.float64
    assert fn(x.detach(), d["tb" if loss == "iou" else "t"].to(dev), *extra).dtype == torch.float64  # mixed dtypes
    with pytest.raises(ValueError):
        fn(x, t.detach()[:, :, :-1], *extra)


def test_graph_capture_matches_eager(dev):
    """One loss of each kind and its backward captured in a HIP graph and replayed after the images changed
    in place: bit for bit the eager results on the new values."""
    d, _ = case("odd")
    later = draw(SHAPES["odd"], 99)
    t, tb, g, mask = (to_dev(d[k], dev) for k in ("t", "tb", "g", "mask"))
    x = to_dev(d["x"], dev).requires_grad_(True)
    moved = to_dev(later["x"], dev)

    def step(y):
        sq = nr.squared_error_loss(y, t, mask)
        hub = nr.huber_loss(y, t, DELTA)
        iou = nr.iou_loss(y, tb)
        (sq + 0.5 * hub + 10. * iou).backward(g)
        return sq, hub, iou

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
    """Silhouettes of an icosphere through Renderer.render_silhouettes (the [:, 0] view of the rasterizer's
    output) against a target from a shifted viewpoint: the vertex gradients through the fused losses agree
    with those through the composition on the same render at the rasterizer's own gradient tolerance (its
    float atomics keep two backward passes from being bitwise equal)."""
    v, f = synthetic.icosphere(1)
    faces = torch.as_tensor(f, device=dev)
    ren = nr.Renderer()
    ren.image_size = 32
    ren.viewpoints = nr.get_points_from_angles(3.4, 10, 40)  # further away too: a sphere looks alike from all sides
    with torch.no_grad():
        target = ren.render_silhouettes(torch.as_tensor(synthetic.jittered(v, 2), device=dev), faces).contiguous()
    ren.viewpoints = nr.get_points_from_angles(2.732, 30, -15)
    verts = torch.as_tensor(synthetic.jittered(v, 2), device=dev).requires_grad_(True)
    sil = ren.render_silhouettes(verts, faces)
    assert sil.shape == (2, 32, 32) and float((sil.detach() - target).abs().max()) > 0.5
    g = torch.as_tensor([1., -0.5], device=dev)
    for fn, composition in ((nr.squared_error_loss, nr.squared_error_loss_torch), (nr.iou_loss, nr.iou_loss_torch)):
        out, want = fn(sil, target), composition(sil, target)
        close_out(out, want, fn.__name__)
        got_grad, = torch.autograd.grad(out, verts, g, retain_graph=True)
        want_grad, = torch.autograd.grad(want, verts, g, retain_graph=True)
        assert bool(torch.isfinite(got_grad).all()) and float(got_grad.abs().max()) > 0
        scale = float(want_grad.abs().max())
        err = float((got_grad - want_grad).abs().max())
        print("%s: vertex grad max |d| %.3g of scale %.3g" % (fn.__name__, err, scale))
        assert err <= 1e-4 * scale, (fn.__name__, err, scale)

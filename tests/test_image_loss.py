"""The image losses without a GPU: the torch compositions against a plain numpy restatement over every
target and weight form, their gradients (gradcheck), the dispatch rule, the shape errors and the result
shapes."""
import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import image_loss

B, C, H, W = 3, 2, 4, 5


def np_pointwise(x, t, w, kind, delta):
    """Per-item loop over flat items: nothing shared with the composition but the formulas."""
    out = np.zeros(x.shape[0])
    for b in range(x.shape[0]):
        for i, (xi, ti, wi) in enumerate(zip(x[b].reshape(-1), t[b].reshape(-1), w[b].reshape(-1))):
            d = xi - ti
            if kind == "squared":
                h = d * d
            else:
                h = 0.5 * d * d if abs(d) < delta else delta * (abs(d) - 0.5 * delta)
            out[b] += wi * h
    return out


def np_iou(p, t, eps):
    out = np.zeros(p.shape[0])
    for b in range(p.shape[0]):
        pb, tb = p[b].reshape(-1), t[b].reshape(-1)
        out[b] = 1 - (pb * tb).sum() / ((pb + tb - pb * tb).sum() + eps)
    return out


def data(seed=0):
    rs = np.random.RandomState(seed)
    x = rs.uniform(0, 1, (B, C, H, W))
    t = rs.uniform(0, 1, (B, C, H, W))
    w = rs.uniform(0, 2, (B, C, H, W))
    m = rs.uniform(0, 2, (B, 1, H, W))
    return x, t, w, m


def forms(full, per_item=True):
    """(name, tensor given to the loss, its full [B, ...] numpy expansion) for every batch form of `full`
    ([B, ...] numpy): per item, leading 1, no batch dimension, batch-expanded view."""
    out = []
    if per_item:
        out.append(("per_item", torch.as_tensor(full), full))
    one = np.broadcast_to(full[:1], full.shape)
    out.append(("leading_one", torch.as_tensor(full[:1].copy()), one))
    out.append(("no_batch", torch.as_tensor(full[0].copy()), one))
    out.append(("expanded", torch.as_tensor(full[0].copy())[None].expand(full.shape[0], *[-1] * (full.ndim - 1)), one))
    return out


def test_compositions_match_numpy_over_every_target_and_weight_form():
    x, t, w, m = data()
    xt = torch.as_tensor(x)
    ones = np.ones_like(x)
    weight_forms = [("none", None, ones)] + [("full_" + n, a, e) for n, a, e in forms(w)] + [
        ("mask_" + n, a, np.broadcast_to(e, x.shape)) for n, a, e in forms(m)]
    seen = 0
    for tn, tt, te in forms(t):
        for wn, wt, we in weight_forms:
            got = nr.squared_error_loss_torch(xt, tt, wt)
            assert got.shape == (B,) and got.dtype == torch.float64
            np.testing.assert_allclose(got.numpy(), np_pointwise(x, te, we, "squared", 0.), rtol=1e-12, err_msg=tn + " " + wn)
            got = nr.huber_loss_torch(xt, tt, 0.25, wt)
            np.testing.assert_allclose(got.numpy(), np_pointwise(x, te, we, "huber", 0.25), rtol=1e-12, err_msg=tn + " " + wn)
            seen += 1
        got = nr.iou_loss_torch(xt[:, 0], tt[..., 0, :, :], 1e-6)
        np.testing.assert_allclose(got.numpy(), np_iou(x[:, 0], te[:, 0], 1e-6), rtol=1e-12, err_msg=tn)
    assert seen == 4 * 9
    assert (np.abs(x - t) < 0.25).any() and (np.abs(x - t) > 0.25).any()  # both Huber branches
    # huber agrees with torch's own on the plain form
    ref = torch.nn.functional.huber_loss(xt, torch.as_tensor(t), reduction="none", delta=0.25).sum((1, 2, 3))
    np.testing.assert_allclose(nr.huber_loss_torch(xt, torch.as_tensor(t), 0.25).numpy(), ref.numpy(), rtol=1e-12)


def test_public_functions_take_the_composition_on_the_cpu():
    x, t, w, m = data(1)
    xt, tt = torch.as_tensor(x), torch.as_tensor(t)
    for wt in (None, torch.as_tensor(w), torch.as_tensor(m[:1])):
        assert torch.equal(nr.squared_error_loss(xt, tt, wt), nr.squared_error_loss_torch(xt, tt, wt))
        assert torch.equal(nr.huber_loss(xt, tt, 0.25, wt), nr.huber_loss_torch(xt, tt, 0.25, wt))
    assert torch.equal(nr.iou_loss(xt, tt), nr.iou_loss_torch(xt, tt))


def test_gradcheck():
    rs = np.random.RandomState(2)
    x = torch.as_tensor(rs.uniform(0, 1, (2, 2, 3, 3))).requires_grad_(True)
    t = torch.as_tensor(rs.uniform(0, 1, (2, 2, 3, 3))).requires_grad_(True)
    w = torch.as_tensor(rs.uniform(0.5, 2, (1, 1, 3, 3))).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b, c: nr.squared_error_loss(a, b, c), (x, t, w))
    assert torch.autograd.gradcheck(lambda a, b: nr.iou_loss(a, b), (x, t))
    # Huber: keep |x - t| at least 0.05 away from delta = 0.25 (gradcheck steps by 1e-6)
    d = rs.uniform(-0.6, 0.6, (2, 2, 3, 3))
    d = np.where(np.abs(np.abs(d) - 0.25) < 0.05, d * 0.5, d)
    assert (np.abs(np.abs(d) - 0.25) >= 0.02).all() and (np.abs(d) < 0.25).any() and (np.abs(d) > 0.25).any()
    xh = (t.detach() + torch.as_tensor(d)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b, c: nr.huber_loss(a, b, 0.25, c), (xh, t, w))


@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the fused path was taken")
    monkeypatch.setattr(image_loss._lib, "lib", boom)


def test_dispatch_reaches_the_composition(no_library):
    x, t, w, m = data(3)
    for dtype in (torch.float32, torch.float64):  # CPU tensors of the fused dtype, and float64
        xt = torch.as_tensor(x, dtype=dtype).requires_grad_(True)
        tt, wt = torch.as_tensor(t, dtype=dtype), torch.as_tensor(m, dtype=dtype)
        total = nr.squared_error_loss(xt, tt, wt).sum() + nr.huber_loss(xt, tt, 0.25, wt).sum() + nr.iou_loss(xt, tt).sum()
        total.backward()
        assert xt.grad is not None and xt.grad.dtype == dtype
    # a target and a weight that require grad get their gradients
    xt = torch.as_tensor(x, dtype=torch.float32)
    tt = torch.as_tensor(t, dtype=torch.float32).requires_grad_(True)
    wt = torch.as_tensor(w, dtype=torch.float32).requires_grad_(True)
    (nr.squared_error_loss(xt, tt, wt).sum() + nr.huber_loss(xt, tt, 0.25, wt).sum() + nr.iou_loss(xt, tt).sum()).backward()
    assert tt.grad is not None and float(tt.grad.abs().max()) > 0
    assert wt.grad is not None and float(wt.grad.abs().max()) > 0
    assert image_loss._fusable(xt, tt.detach(), wt.detach()) is False  # a CPU tensor
    for mod in (nr.SquaredErrorLoss(tt.detach(), wt.detach()), nr.HuberLoss(tt.detach(), 0.25, wt.detach()), nr.IoULoss(tt.detach())):
        assert mod(xt).shape == (B,)


def test_shape_errors():
    x = torch.zeros(2, 3, 4, 5)
    bad_targets = [torch.zeros(2, 3, 4, 4), torch.zeros(3, 4), torch.zeros(2, 1, 4, 5), torch.zeros(4, 5), torch.zeros(())]
    for fn in (nr.squared_error_loss, nr.huber_loss, nr.iou_loss, nr.squared_error_loss_torch, nr.huber_loss_torch,
               nr.iou_loss_torch):
        for t in bad_targets:
            with pytest.raises(ValueError):
                fn(x, t)
        with pytest.raises(ValueError):
            fn(torch.zeros(5), torch.zeros(5))  # no item dimensions
    bad_weights = [torch.zeros(2, 1, 4, 4), torch.zeros(2, 2, 4, 5), torch.zeros(1, 1, 5, 4), torch.zeros(5), torch.zeros(3, 1, 4, 5)]
    for fn in (nr.squared_error_loss, nr.huber_loss, nr.squared_error_loss_torch, nr.huber_loss_torch):
        for w in bad_weights:
            with pytest.raises(ValueError):
                fn(x, torch.zeros_like(x), weights=w)
    with pytest.raises(ValueError):
        nr.squared_error_loss(torch.zeros(2, 20), torch.zeros(2, 20), torch.zeros(2, 1, 4, 5))  # a mask needs 4-D images
    with pytest.raises(ValueError):
        nr.huber_loss(x, x, delta=0.)


def test_result_shapes():
    x, t, w, m = data(4)
    xt, tt = torch.as_tensor(x), torch.as_tensor(t)
    for fn in (nr.squared_error_loss, nr.huber_loss, nr.iou_loss):
        per_item = fn(xt, tt)
        assert per_item.shape == (B,)
        avg = fn(xt, tt, average=True)
        assert avg.ndim == 0 and torch.allclose(avg, per_item.mean(), rtol=1e-12, atol=0)
        flat = fn(xt.reshape(B, -1), tt.reshape(B, -1))  # [B, N]
        assert flat.shape == (B,) and torch.allclose(flat, per_item, rtol=1e-12, atol=0)
        shared = fn(xt.reshape(B, -1), tt.reshape(B, -1)[0])  # [B, N] against [N]
        assert shared.shape == (B,)
    assert nr.squared_error_loss(torch.zeros(0, 3, 4, 4), torch.zeros(3, 4, 4)).shape == (0,)
    assert torch.equal(nr.squared_error_loss(torch.zeros(2, 0), torch.zeros(2, 0)), torch.zeros(2))
    assert torch.equal(nr.iou_loss(torch.zeros(2, 0), torch.zeros(2, 0)), torch.ones(2))


def test_iou_of_empty_silhouettes_is_one():
    p = torch.zeros(2, 8, 8, dtype=torch.float64, requires_grad=True)
    loss = nr.iou_loss(p, torch.zeros(2, 8, 8, dtype=torch.float64))
    assert torch.equal(loss, torch.ones(2, dtype=torch.float64))
    loss.sum().backward()
    assert bool(torch.isfinite(p.grad).all())
    p32 = torch.zeros(2, 8, 8, requires_grad=True)
    loss = nr.iou_loss(p32, torch.zeros(8, 8))
    assert torch.equal(loss, torch.ones(2))
    loss.sum().backward()
    assert bool(torch.isfinite(p32.grad).all())


def test_abi_rejects_bad_arguments():
    """The entry points check sizes, pointers, kind, delta, the weight period and the workspace before any
    launch (no GPU needed: every call here returns from the argument checks)."""
    from neural_renderer_v2_pytorch_amd import _lib
    L = _lib.lib()
    ARGS, WORKSPACE = 1, 3  # NR_ERR_ARGS, NR_ERR_WORKSPACE
    assert L.nr_image_loss_workspace_bytes(0, 5) == 0 and L.nr_image_loss_workspace_bytes(5, 0) == 0
    assert L.nr_image_loss_workspace_bytes(2, 4097) >= 2 * 2 * 2 * 4
    p = 4096  # a non-null address that is never dereferenced

    def forward(images=p, targets=p, weights=None, period=1, kind=0, delta=1.0, B=2, N=8, loss=p, ws=p, ws_bytes=1 << 20):
        return L.nr_pointwise_loss_forward(images, 8, targets, 8, weights, 0, period, kind, delta, B, N, loss, ws, ws_bytes, None)

    assert forward(B=-1) == ARGS and forward(N=-1) == ARGS
    assert forward(N=2 ** 31 - 1) == ARGS  # past INT_MAX - 4096
    assert forward(B=2 ** 20, N=2 ** 24) == ARGS  # too many blocks
    assert forward(images=None) == ARGS and forward(targets=None) == ARGS and forward(loss=None) == ARGS
    assert forward(kind=2) == ARGS
    assert forward(kind=1, delta=0.) == ARGS and forward(kind=1, delta=float("inf")) == ARGS
    assert forward(weights=p, period=3) == ARGS and forward(weights=p, period=0) == ARGS  # 3 does not divide 8
    assert forward(ws=None) == WORKSPACE and forward(ws_bytes=4) == WORKSPACE
    assert b"workspace" in L.nr_last_error()
    assert L.nr_pointwise_loss_backward(p, 8, p, 8, None, 0, 1, 0, 1.0, 2, 8, None, p, None) == ARGS
    assert L.nr_pointwise_loss_backward(p, -8, p, 8, None, 0, 1, 0, 1.0, 2, 8, p, p, None) == ARGS
    assert L.nr_iou_loss_forward(p, 8, p, 8, 1e-6, 2, 8, p, None, p, 1 << 20, None) == ARGS
    assert L.nr_iou_loss_forward(p, 8, p, 8, 1e-6, 2, 8, p, p, p, 4, None) == WORKSPACE
    assert L.nr_iou_loss_backward(p, 8, None, 1e-6, 2, 8, p, p, None) == ARGS
    # nothing to do: no pointer is needed
    assert forward(B=0, images=None, targets=None, loss=None, ws=None) == 0
    assert L.nr_pointwise_loss_backward(None, 0, None, 0, None, 0, 1, 0, 1.0, 2, 0, None, None, None) == 0
    assert L.nr_iou_loss_backward(None, 0, None, 1e-6, 0, 8, None, None, None) == 0

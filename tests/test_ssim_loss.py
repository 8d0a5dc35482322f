"""The SSIM loss without a GPU: the torch composition against a direct numpy evaluation (plain loops over
the 2-D window: no separable filter, no convolution), its gradients (gradcheck), the identities of the
definition, the target forms, the argument errors, the dispatch rule and the argument checks of the ABI."""
import ctypes

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import _lib, image_loss


def np_ssim_loss(x, t, window_size, sigma, data_range, padding):
    """x, t [B, C, H, W] float64 -> loss [B]: every map pixel sums its own (2R + 1)^2 window."""
    R = window_size // 2
    g = np.array([np.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(-R, R + 1)])
    g = g / g.sum()
    G = np.outer(g, g)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    B, C, H, W = x.shape
    if padding == "same":
        x = np.pad(x, ((0, 0), (0, 0), (R, R), (R, R)))
        t = np.pad(t, ((0, 0), (0, 0), (R, R), (R, R)))
    mh, mw = x.shape[2] - 2 * R, x.shape[3] - 2 * R
    out = np.zeros(B)
    for b in range(B):
        total = 0.0
        for c in range(C):
            for i in range(mh):
                for j in range(mw):
                    px, pt = x[b, c, i:i + 2 * R + 1, j:j + 2 * R + 1], t[b, c, i:i + 2 * R + 1, j:j + 2 * R + 1]
                    mu1, mu2 = (G * px).sum(), (G * pt).sum()
                    s11 = (G * px * px).sum() - mu1 * mu1
                    s22 = (G * pt * pt).sum() - mu2 * mu2
                    s12 = (G * px * pt).sum() - mu1 * mu2
                    total += (2 * mu1 * mu2 + c1) * (2 * s12 + c2) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))
        out[b] = 1 - total / (C * mh * mw)
    return out


def pair(shape, seed=0):
    rs = np.random.RandomState(seed)
    return rs.uniform(0, 1, shape), rs.uniform(0, 1, shape)


@pytest.mark.parametrize("window_size,sigma,padding", [(11, 1.5, "same"), (11, 1.5, "valid"), (3, 0.8, "same"), (3, 0.8, "valid")])
def test_composition_matches_direct_evaluation(window_size, sigma, padding):
    x, t = pair((2, 2, 13, 14))
    got = nr.ssim_loss_torch(torch.as_tensor(x), torch.as_tensor(t), window_size, sigma, 1.0, padding)
    assert got.shape == (2,) and got.dtype == torch.float64
    np.testing.assert_allclose(got.numpy(), np_ssim_loss(x, t, window_size, sigma, 1.0, padding), rtol=0, atol=1e-12)


def test_gradcheck():
    x, t = pair((1, 1, 7, 8), 1)
    xt, tt = torch.as_tensor(x).requires_grad_(True), torch.as_tensor(t).requires_grad_(True)
    for padding in ("same", "valid"):
        assert torch.autograd.gradcheck(lambda a, b: nr.ssim_loss(a, b, 5, 1.0, 1.0, padding), (xt, tt))


def test_identities():
    x, t = pair((2, 3, 12, 15), 2)
    for dtype in (torch.float32, torch.float64):
        xt, tt = torch.as_tensor(x, dtype=dtype), torch.as_tensor(t, dtype=dtype)
        for padding in ("same", "valid"):
            assert torch.equal(nr.ssim_loss(xt, xt.clone(), padding=padding), torch.zeros(2, dtype=dtype)), (dtype, padding)
            a, b = nr.ssim_loss(xt, tt, padding=padding), nr.ssim_loss(tt, xt, padding=padding)
            assert float(a.min()) > 0.1  # unrelated noise is dissimilar
            torch.testing.assert_close(a, b, rtol=1e-6 if dtype == torch.float32 else 1e-13, atol=0)
    xt, tt = torch.as_tensor(x), torch.as_tensor(t)
    for padding in ("same", "valid"):
        torch.testing.assert_close(nr.ssim_loss(255 * xt, 255 * tt, data_range=255.0, padding=padding),
                                   nr.ssim_loss(xt, tt, padding=padding), rtol=1e-12, atol=0)
    # the 'valid' map of an 11 x 11 image is its centre pixel: one full window
    x, t = pair((1, 1, 11, 11), 3)
    g = image_loss._ssim_window(11, 1.5).numpy()
    G = np.outer(g, g)
    mu1, mu2 = (G * x[0, 0]).sum(), (G * t[0, 0]).sum()
    s11, s22, s12 = (G * x[0, 0] ** 2).sum() - mu1 ** 2, (G * t[0, 0] ** 2).sum() - mu2 ** 2, (G * x[0, 0] * t[0, 0]).sum() - mu1 * mu2
    S = (2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4) / ((mu1 ** 2 + mu2 ** 2 + 1e-4) * (s11 + s22 + 9e-4))
    np.testing.assert_allclose(nr.ssim_loss(torch.as_tensor(x), torch.as_tensor(t), padding="valid").numpy(), [1 - S], rtol=0, atol=1e-12)


def test_window():
    g = image_loss._ssim_window(11, 1.5)
    assert g.dtype == torch.float64 and g.shape == (11,)
    assert abs(float(g.sum()) - 1) < 1e-15 and torch.equal(g, g.flip(0)) and int(g.argmax()) == 5
    np.testing.assert_allclose(float(g[4] / g[5]), np.exp(-1 / 4.5), rtol=1e-14)


def test_target_forms_shapes_and_average():
    x, t = pair((3, 2, 9, 10), 4)
    xt, tt = torch.as_tensor(x), torch.as_tensor(t)
    for padding in ("same", "valid"):
        kw = dict(window_size=5, sigma=1.0, padding=padding)
        want = nr.ssim_loss(xt, tt[:1].expand(3, -1, -1, -1).contiguous(), **kw)
        for form in (tt[:1], tt[0], tt[0][None].expand(3, -1, -1, -1)):
            assert torch.equal(nr.ssim_loss(xt, form, **kw), want)
        per_item = nr.ssim_loss(xt, tt, **kw)
        assert per_item.shape == (3,)
        avg = nr.ssim_loss(xt, tt, average=True, **kw)
        assert avg.ndim == 0 and torch.allclose(avg, per_item.mean(), rtol=1e-14, atol=0)
        # [B, H, W] is [B, 1, H, W], with every target form of its own
        want = nr.ssim_loss(xt[:, :1], tt[:, :1], **kw)
        assert torch.equal(nr.ssim_loss(xt[:, 0], tt[:, 0], **kw), want)
        assert torch.equal(nr.ssim_loss(xt[:, 0], tt[0, 0], **kw), nr.ssim_loss(xt[:, :1], tt[:1, :1], **kw))
        assert torch.equal(nr.ssim_loss(xt[:, 0], tt[:1, 0], **kw), nr.ssim_loss(xt[:, :1], tt[:1, :1], **kw))


def test_module():
    x, t = pair((2, 3, 12, 12), 5)
    xt, tt = torch.as_tensor(x), torch.as_tensor(t)
    mod = nr.SSIMLoss(tt[0], window_size=7, sigma=1.2, data_range=2.0, padding="valid", average=True)
    assert "targets" in dict(mod.named_buffers()) and not list(mod.parameters())
    assert torch.equal(mod(xt), nr.ssim_loss(xt, tt[0], 7, 1.2, 2.0, "valid", True))
    assert torch.equal(nr.SSIMLoss(tt)(xt), nr.ssim_loss(xt, tt))
    assert mod.double().targets.dtype == torch.float64


def test_argument_errors():
    x = torch.rand(2, 3, 12, 13)
    for fn in (nr.ssim_loss, nr.ssim_loss_torch):
        for bad in (4, 0, 12, -3, 5.0):
            with pytest.raises(ValueError):
                fn(x, x, window_size=bad)
        for bad in ("reflect", "SAME", None, 0):
            with pytest.raises(ValueError):
                fn(x, x, padding=bad)
        for t in (torch.zeros(2, 3, 12, 12), torch.zeros(3, 3, 12, 13), torch.zeros(12, 13), torch.zeros(2, 1, 12, 13), torch.zeros(())):
            with pytest.raises(ValueError):
                fn(x, t)
        with pytest.raises(ValueError):
            fn(torch.rand(2, 3, 10, 13), torch.rand(2, 3, 10, 13), padding="valid")  # H below the window
        with pytest.raises(ValueError):
            fn(torch.rand(2, 3, 13, 10), torch.rand(2, 3, 13, 10), padding="valid")  # W below the window
        assert fn(torch.rand(2, 3, 10, 13), torch.rand(2, 3, 10, 13), padding="same").shape == (2,)
        for kw in (dict(sigma=0.), dict(sigma=-1.), dict(sigma=float("inf")), dict(sigma=float("nan")), dict(data_range=0.),
                   dict(data_range=float("inf"))):
            with pytest.raises(ValueError):
                fn(x, x, **kw)
        with pytest.raises(ValueError):
            fn(torch.rand(2, 12), torch.rand(2, 12))  # no image dimensions
        with pytest.raises(ValueError):
            fn(torch.rand(2, 1, 3, 12, 12), torch.rand(2, 1, 3, 12, 12))


@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the fused path was taken")
    monkeypatch.setattr(image_loss._lib, "lib", boom)


def test_cpu_images_take_the_composition(no_library):
    x, t = pair((2, 3, 12, 12), 6)
    for dtype in (torch.float32, torch.float64):
        xt = torch.as_tensor(x, dtype=dtype).requires_grad_(True)
        tt = torch.as_tensor(t, dtype=dtype).requires_grad_(True)
        loss = nr.ssim_loss(xt, tt)
        assert torch.equal(loss, nr.ssim_loss_torch(xt, tt))
        loss.sum().backward()
        assert xt.grad.dtype == dtype and float(xt.grad.abs().max()) > 0 and float(tt.grad.abs().max()) > 0
    assert image_loss._fusable(torch.as_tensor(x, dtype=torch.float32), torch.as_tensor(t, dtype=torch.float32)) is False
    assert nr.SSIMLoss(torch.as_tensor(t, dtype=torch.float32))(torch.as_tensor(x, dtype=torch.float32)).shape == (2,)


def test_exports_and_tile():
    for name in ("nr_ssim_loss_workspace_bytes", "nr_ssim_loss_forward", "nr_ssim_loss_backward"):
        assert name in _lib.EXPORTS
    assert _lib.NR_SSIM_TILE in (16, 32) and _lib.NR_SSIM_MAX_WINDOW == 11
    for name in ("ssim_loss", "ssim_loss_torch", "SSIMLoss"):
        assert hasattr(nr, name)


def test_abi_rejects_bad_arguments():
    """The entry points check sizes, window, padding, pointers and the workspace before any launch (no GPU
    needed: every call here returns from the argument checks)."""
    L = _lib.lib()
    ARGS, WORKSPACE = 1, 3  # NR_ERR_ARGS, NR_ERR_WORKSPACE
    T = _lib.NR_SSIM_TILE
    size = L.nr_ssim_loss_workspace_bytes
    assert size(0, 3, 64, 64, 11, 0) == 0 and size(2, 3, 0, 64, 11, 0) == 0 and size(2, 3, 64, 64, 4, 0) == 0
    assert size(2, 3, 2 * T + 1, T, 11, 0) >= 2 * 3 * 3 * 4  # 3 x 1 tiles per channel
    assert 2 * 3 * 2 * 4 <= size(2, 3, 2 * T + 1, T + 10, 11, 1) <= size(2, 3, 2 * T + 1, T + 10, 11, 0)  # 'valid': 2 x 1 tiles
    p = 4096  # a non-null address that is never dereferenced
    win = (ctypes.c_float * 11)(*([1 / 11.] * 11))

    def forward(images=p, targets=p, B=2, C=3, H=40, W=40, K=11, window=win, c1=1e-4, c2=9e-4, padding=0, loss=p, saved=None, ws=p,
                ws_bytes=1 << 20, istride=4800):
        return L.nr_ssim_loss_forward(images, istride, targets, 4800, B, C, H, W, K, window, c1, c2, padding, loss, saved, ws, ws_bytes, None)

    def backward(images=p, targets=p, saved=p, B=2, C=3, H=40, W=40, K=11, window=win, padding=0, g=p, grad=p):
        return L.nr_ssim_loss_backward(images, 4800, targets, 4800, saved, B, C, H, W, K, window, padding, g, grad, None)

    assert forward(B=-1) == ARGS and forward(C=-1) == ARGS and forward(H=-1) == ARGS and forward(W=-1) == ARGS
    for K in (4, 13, 1, 0, -3):
        assert forward(K=K) == ARGS and backward(K=K) == ARGS
        assert b"window" in L.nr_last_error()
    assert forward(padding=2) == ARGS and forward(padding=-1) == ARGS and backward(padding=2) == ARGS
    assert b"padding" in L.nr_last_error()
    assert forward(H=10, padding=1) == ARGS and forward(W=10, padding=1) == ARGS and backward(H=10, padding=1) == ARGS
    assert forward(H=10, padding=0, ws_bytes=0) == WORKSPACE  # 'same' takes the small image
    assert forward(C=3, H=2 ** 15, W=2 ** 15) == ARGS  # C H W past INT_MAX
    assert forward(B=2 ** 20, C=2 ** 10, H=64, W=64) == ARGS  # too many tiles
    assert forward(images=None) == ARGS and forward(targets=None) == ARGS and forward(loss=None) == ARGS and forward(window=None) == ARGS
    assert forward(istride=-1) == ARGS
    assert forward(c1=float("nan")) == ARGS and forward(c2=-1.) == ARGS
    assert forward(ws=None) == WORKSPACE and forward(ws_bytes=4) == WORKSPACE
    assert b"workspace" in L.nr_last_error()
    assert backward(saved=None) == ARGS and backward(g=None) == ARGS and backward(grad=None) == ARGS and backward(images=None) == ARGS
    # nothing to do: no pointer is needed
    assert forward(B=0, images=None, targets=None, loss=None, ws=None, window=None) == 0
    assert backward(B=0, images=None, targets=None, saved=None, g=None, grad=None, window=None) == 0
    assert backward(H=0, images=None, targets=None, saved=None, g=None, grad=None, window=None) == 0

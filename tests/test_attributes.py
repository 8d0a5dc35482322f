"""Vertex-attribute rendering without a GPU: the torch interpolation (attributes_from_maps_torch, the reference
of tests/test_gpu_attributes.py) against a per-pixel numpy loop and its own closed-form gradients, the
argument handling of rasterize_attributes, and the C ABI's argument checks (no launch)."""
import ctypes

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr


def hand_scene():
    """A 4 x 4 face-index map with two faces and some background, hand-set weights, corner depths that
    differ, C = 2; float64."""
    fim = np.array([[[-1, 0, 0, -1],
                     [0, 0, 1, 1],
                     [-1, 1, 1, -1],
                     [-1, -1, 1, 0]]], np.int32)
    rs = np.random.RandomState(11)
    w = rs.uniform(0.05, 1.0, (1, 4, 4, 3))
    w /= w.sum(-1, keepdims=True)
    w[fim < 0] = 0.0
    faces_v = rs.uniform(-1, 1, (1, 2, 3, 3))
    faces_v[..., 2] = np.array([[1.5, 2.0, 3.25], [2.5, 1.75, 4.0]])
    faces_a = rs.normal(size=(1, 2, 3, 2))
    return fim, w, faces_v, faces_a


def numpy_loop(fim, w, faces_v, faces_a, perspective_correct):
    B, S = fim.shape[:2]
    C = faces_a.shape[-1]
    out = np.zeros((B, S, S, C))
    for b in range(B):
        for y in range(S):
            for x in range(S):
                f = fim[b, y, x]
                if f < 0:
                    continue
                for c in range(C):
                    if perspective_correct:
                        q = [w[b, y, x, k] / (faces_v[b, f, k, 2] + 1e-10) for k in range(3)]
                        dn = sum(qk + 1e-10 for qk in q)
                        out[b, y, x, c] = sum(q[k] * faces_a[b, f, k, c] for k in range(3)) / dn
                    else:
                        out[b, y, x, c] = sum(w[b, y, x, k] * faces_a[b, f, k, c] for k in range(3))
    return out


@pytest.mark.parametrize("pc", [True, False])
def test_interpolation_matches_numpy_loop(pc):
    fim, w, fv, fa = hand_scene()
    got = nr.attributes_from_maps_torch(torch.as_tensor(fim), torch.as_tensor(w), torch.as_tensor(fv), torch.as_tensor(fa),
                                        perspective_correct=pc)
    assert got.dtype == torch.float64 and got.shape == (1, 4, 4, 2)
    ref = numpy_loop(fim, w, fv, fa, pc)
    assert np.abs(got.numpy() - ref).max() <= 1e-12
    assert np.all(got.numpy()[fim < 0] == 0.0)  # background exactly 0
    # a table shared by the batch, [1, F, 3, C] against B = 2 maps
    fim2, w2, fv2 = np.concatenate([fim, fim[:, ::-1]]), np.concatenate([w, w[:, ::-1]]), np.concatenate([fv, fv])
    got2 = nr.attributes_from_maps_torch(torch.as_tensor(fim2.copy()), torch.as_tensor(w2.copy()), torch.as_tensor(fv2),
                                         torch.as_tensor(fa), perspective_correct=pc)
    ref2 = numpy_loop(fim2, w2, fv2, np.concatenate([fa, fa]), pc)
    assert np.abs(got2.numpy() - ref2).max() <= 1e-12


@pytest.mark.parametrize("pc", [True, False])
def test_interpolation_gradients(pc):
    """gradcheck pins autograd's gradient to faces_a and faces_v; the closed forms of the issue follow:
    d/da_kc = coef_k g_c, d/dz_k = -(q_k / (z_k + 1e-10)) / Dn sum_c g_c (a_kc - out_c), zero in the linear
    mode, and zero for x, y (the weights are constants)."""
    fim, w, fv, fa = hand_scene()
    fim_t, w_t = torch.as_tensor(fim), torch.as_tensor(w)
    fv_t = torch.as_tensor(fv).requires_grad_(True)
    fa_t = torch.as_tensor(fa).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, v: nr.attributes_from_maps_torch(fim_t, w_t, v, a, pc), (fa_t, fv_t),
                                    eps=1e-6, atol=1e-8, rtol=1e-6)
    g = torch.as_tensor(np.random.RandomState(5).normal(size=(1, 4, 4, 2)))
    out = nr.attributes_from_maps_torch(fim_t, w_t, fv_t, fa_t, pc)
    out.backward(g)
    # (the linear mode does not read faces_v at all: autograd then leaves its gradient unset, i.e. zero)
    gfv = fv_t.grad if fv_t.grad is not None else torch.zeros_like(fv_t)
    assert pc or fv_t.grad is None or torch.all(fv_t.grad == 0)
    assert torch.all(gfv[..., :2] == 0)  # x, y: the weights are constants here
    if not pc:
        assert torch.all(gfv[..., 2] == 0)
    # the closed forms, scattered per pixel
    ga, gz = np.zeros_like(fa), np.zeros((1, 2, 3))
    o = out.detach().numpy()
    for y in range(4):
        for x in range(4):
            f = fim[0, y, x]
            if f < 0:
                continue
            for k in range(3):
                if pc:
                    q = [w[0, y, x, j] / (fv[0, f, j, 2] + 1e-10) for j in range(3)]
                    dn = sum(qj + 1e-10 for qj in q)
                    coef = q[k] / dn
                    gz[0, f, k] += -(q[k] / (fv[0, f, k, 2] + 1e-10)) / dn * sum(
                        g[0, y, x, c].item() * (fa[0, f, k, c] - o[0, y, x, c]) for c in range(2))
                else:
                    coef = w[0, y, x, k]
                ga[0, f, k] += coef * g[0, y, x].numpy()
    assert np.abs(fa_t.grad.numpy() - ga).max() <= 1e-12
    assert np.abs(gfv[..., 2].numpy() - gz).max() <= 1e-12


def test_argument_handling():
    v = torch.zeros(2, 5, 3)
    f = torch.tensor([[0, 1, 2], [2, 3, 4]])
    with pytest.raises(ValueError):
        nr.rasterize_attributes(v, f, torch.zeros(2, 5, 0))
    with pytest.raises(ValueError):
        nr.rasterize_attributes(v, f, torch.zeros(2, 5, 65))
    assert nr.NR_ATTR_MAX_CHANNELS == 64
    with pytest.raises(ValueError):
        nr.rasterize_attributes(torch.zeros(5, 3), f, torch.zeros(5, 3))  # vertices without a batch
    with pytest.raises(ValueError):
        nr.rasterize_attributes(v, f, torch.zeros(2, 5, 3, 1))
    with pytest.raises(ValueError):
        nr.rasterize_attributes(v, f, torch.zeros(3, 5, 3))  # batch neither 1 nor B
    with pytest.raises(AssertionError):
        nr.rasterize_attributes(v, torch.tensor([0, 1, 2]), torch.zeros(2, 5, 3))  # faces [3]
    with pytest.raises(ValueError):
        nr.rasterize_attributes(v, f, torch.zeros(6, 3), faces_attributes=torch.tensor([[0, 1, 2]]))  # one row, F = 2
    with pytest.raises(IndexError):
        nr.rasterize_attributes(v, torch.tensor([[0, 1, 5]]), torch.zeros(2, 5, 3))
    with pytest.raises(IndexError):
        nr.rasterize_attributes(v, f, torch.zeros(6, 3), faces_attributes=torch.tensor([[0, 1, 2], [3, 4, 6]]))
    with pytest.raises(IndexError):
        nr.rasterize_attributes(v, f, torch.zeros(4, 3))  # faces as faces_attributes past a shorter table
    # CPU tensors: the package's GPU-only error
    for fn in (nr.rasterize_attributes, nr.rasterize_attributes_torch):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(v, f, torch.zeros(2, 5, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        nr.Renderer().render_attributes(torch.zeros(2, 5, 3), f, torch.zeros(5, 3))


def test_abi_rejects_bad_arguments():
    """The entry points check sizes, pointers, the channel count and the workspace before any launch (no GPU
    needed: every call here returns from the argument checks)."""
    from neural_renderer_v2_pytorch_amd import _lib
    L = _lib.lib()
    ARGS, WORKSPACE = 1, 3  # NR_ERR_ARGS, NR_ERR_WORKSPACE
    assert L.nr_attribute_args_size() == ctypes.sizeof(_lib.NrAttributeArgs)
    assert L.nr_attributes_backward_workspace_bytes(0, 5, 3) == 0 and L.nr_attributes_backward_workspace_bytes(2, 0, 3) == 0
    assert L.nr_attributes_backward_workspace_bytes(2, 5, 3) >= 2 * 5 * 3 * 6 * 4
    p = 4096  # a non-null address that is never dereferenced

    def args(**kw):
        a = _lib.NrAttributeArgs()
        a.batch_size, a.num_faces, a.num_vertices, a.num_attributes, a.num_channels = 2, 4, 6, 6, 3
        a.image_size, a.anti_aliasing, a.perspective_correct = 8, 1, 1
        a.face_index = a.face_records = a.faces = a.faces_attributes = a.attributes = a.internal = p
        a.attr_batch_stride = 18
        for k, val in kw.items():
            setattr(a, k, val)
        return a

    def fwd(images=p, **kw):
        return L.nr_attributes_forward(args(**kw), images, None)

    def bwd(g=p, gv=p, ga=p, csr=p, ws=p, ws_bytes=1 << 20, **kw):
        return L.nr_attributes_backward(args(**kw), g, gv, ga, csr, csr, csr, csr, ws, ws_bytes, None)

    for call in (fwd, bwd):
        assert call(batch_size=-1) == ARGS and call(num_faces=-1) == ARGS and call(num_vertices=-1) == ARGS
        assert call(num_attributes=-1) == ARGS and call(image_size=0) == ARGS and call(image_size=8193) == ARGS
        assert call(num_channels=0) == ARGS and call(num_channels=65) == ARGS
        assert b"channel" in L.nr_last_error()
        assert call(batch_size=65536) == ARGS and call(attr_batch_stride=-1) == ARGS
        assert call(face_index=None) == ARGS and call(face_records=None) == ARGS
        assert call(faces_attributes=None) == ARGS and call(attributes=None) == ARGS
    assert L.nr_attributes_forward(None, p, None) == ARGS and fwd(images=None) == ARGS
    assert L.nr_attributes_backward(None, p, p, p, p, p, p, p, p, 1 << 20, None) == ARGS
    assert bwd(g=None) == ARGS and bwd(csr=None) == ARGS
    assert bwd(internal=None) == ARGS  # grad_vertices reads the forward's internal image
    assert bwd(ws=None) == WORKSPACE and bwd(ws_bytes=2 * 4 * 3 * 6 * 4 - 1) == WORKSPACE
    assert b"workspace" in L.nr_last_error()
    # nothing to do: no pointer is needed
    assert L.nr_attributes_forward(args(batch_size=0, face_index=None, attributes=None), None, None) == 0
    assert bwd(g=None, gv=None, ga=None, csr=None, ws=None, batch_size=0) == 0
    assert bwd(gv=None, ga=None, ws=None) == 0  # no gradient asked for

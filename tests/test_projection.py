"""Calibrated camera (projection.py) on the CPU: the stated math, its equivalence with look_at +
perspective, argument shapes, and the host side of the nr_projection_* C ABI (no GPU needed)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import _lib, synthetic


def look_at_as_krt(eyes, angle, S):
    """K, R, t of the camera that look_at(., eyes) + perspective(., angle) describe, in float64:
    R = diag(1, -1, 1) R_look_at, t = -R eye, fx = fy = S / (2 w), cx = cy = S / 2."""
    eyes = eyes.double()
    B = eyes.shape[0]
    # the rows of R_look_at are the camera axes (at = 0, up = y)
    z =torch.nn.functional.normalize(-eyes)
    up = torch.tensor([0., 1., 0.], dtype=torch.float64).expand(B, 3)
    x = torch.nn.functional.normalize(torch.cross(up, z, dim=-1))
    y = torch.nn.functional.normalize(torch.cross(z, x, dim=-1))
    R = torch.stack((x, -y, z), 1)
    t = -torch.matmul(R, eyes[:, :, None])[:, :, 0]
    w = math.tan(angle / 180. * 3.1416)
    K = torch.tensor([[S / (2 * w), 0., S / 2.], [0., S / (2 * w), S / 2.], [0., 0., 1.]], dtype=torch.float64)[None]
    return K, R, t


def test_worked_example():
    v = torch.tensor([[[0.2, -0.1, 0.]]], dtype=torch.float64)
    K = torch.tensor([[[100., 0., 32.], [0., 100., 32.], [0., 0., 1.]]], dtype=torch.float64)
    R = torch.eye(3, dtype=torch.float64)[None]
    t = torch.tensor([[0., 0., 2.]], dtype=torch.float64)
    d = torch.tensor([[0.1, 0., 0., 0., 0.]], dtype=torch.float64)
    out = nr.projection(v, K, R, t, d, orig_size=64, eps=0.)
    assert out.dtype == torch.float64 and out.shape == (1, 1, 3)
    np.testing.assert_allclose(out.flatten().numpy(), [0.312890625, 0.1564453125, 2.], rtol=0, atol=1e-12)


def test_equals_look_at_plus_perspective():
    B, V, S, angle = 3, 50, 64, 30.
    v = torch.as_tensor(np.random.RandomState(0).uniform(-0.5, 0.5, (B, V, 3)))
    eyes = torch.as_tensor(synthetic.viewpoints(B)).double()
    K, R, t = look_at_as_krt(eyes, angle, S)
    out = nr.projection(v, K, R, t, None, orig_size=S, eps=0.)
    f64 = lambda x: torch.tensor(x, dtype=torch.float64)
    ref = nr.perspective(nr.look_at(v, eyes, at=f64([0., 0., 0.]), up=f64([0., 1., 0.])), angle=f64(angle))
    assert ref.dtype == torch.float64
    assert float((out - ref).abs().max()) <= 1e-12


def test_shapes():
    r = np.random.RandomState(1)
    B, V = 4, 9
    v = torch.as_tensor(r.uniform(-0.5, 0.5, (B, V, 3)))
    K = torch.tensor([[[120., 1., 30.], [0., 110., 34.], [0., 0., 1.]]], dtype=torch.float64)
    R = torch.as_tensor(np.linalg.qr(r.normal(size=(3, 3)))[0])[None]
    t = torch.tensor([[0.1, -0.1, 2.5]], dtype=torch.float64)
    d = torch.as_tensor(r.uniform(-0.1, 0.1, (1, 5)))
    shared = nr.projection(v, K, R, t, d, orig_size=64)
    full = nr.projection(v, K.expand(B, 3, 3), R.expand(B, 3, 3), t.expand(B, 3), d.expand(B, 5), orig_size=64)
    assert torch.equal(shared, full)
    assert torch.equal(nr.projection(v, K[0], R[0], t[0], d[0], orig_size=64), shared)
    assert torch.equal(nr.projection(v, K, R, t.expand(B, 3)[:, None, :], d, orig_size=64), shared)
    assert torch.equal(nr.projection(v, K, R, t[:, None, :], d, orig_size=64), shared)
    assert torch.equal(nr.projection(v, K, R, t, None, orig_size=64),
                       nr.projection(v, K, R, t, torch.zeros(B, 5, dtype=torch.float64), orig_size=64))
    # float32 in, float32 out; parameters given as lists
    out32 = nr.projection(v.float(), K[0].tolist(), R[0].tolist(), t[0].tolist(), orig_size=64)
    assert out32.dtype == torch.float32
    assert torch.allclose(out32.double(), nr.projection(v, K, R, t, orig_size=64), rtol=1e-5, atol=1e-5)


def test_gradient_at_the_axis_is_finite():
    v = torch.tensor([[[0., 0., 0.]]], dtype=torch.float64, requires_grad=True)
    d = torch.full((1, 5), 0.1, dtype=torch.float64, requires_grad=True)
    out = nr.projection(v, torch.eye(3, dtype=torch.float64), torch.eye(3, dtype=torch.float64),
                        torch.tensor([0., 0., 2.], dtype=torch.float64), d, orig_size=2)
    out.sum().backward()
    assert torch.isfinite(v.grad).all() and torch.isfinite(d.grad).all()


def test_renderer_projection_mode_validates():
    ren = nr.Renderer()
    assert ren.K is None and ren.R is None and ren.t is None and ren.dist_coeffs is None and ren.orig_size == 1024
    ren.camera_mode = 'projection'
    v = torch.rand(2, 5, 3)
    for missing in ('K', 'R', 't'):
        ren.K, ren.R, ren.t = torch.eye(3), torch.eye(3), torch.tensor([0., 0., 2.])
        setattr(ren, missing, None)
        with pytest.raises(ValueError, match=r"\b%s\b" % missing):
            ren.transform_vertices(v)
    # CPU tensors take the torch composition; perspective and viewing_angle are ignored
    ren.K, ren.R, ren.t, ren.orig_size = torch.eye(3), torch.eye(3), torch.tensor([0., 0., 2.]), 2
    ren.perspective, ren.viewing_angle = False, 77
    assert torch.equal(ren.transform_vertices(v), nr.projection(v, ren.K, ren.R, ren.t, None, 2))


def test_renderer_defaults_unchanged(golden):
    d = golden("teapot_sil")
    ren = nr.Renderer()
    assert ren.camera_mode == 'look_at'
    ren.viewpoints = nr.get_points_from_angles(2.732, 0, 0)
    proj = ren.transform_vertices(torch.as_tensor(d["vertices"]))
    np.testing.assert_allclose(proj.numpy(), d["proj"], rtol=1e-6, atol=1e-6)


def test_look_is_per_item():
    """look: the rotation of one direction applies to every item; rows are the camera axes."""
    v = torch.as_tensor(np.random.RandomState(2).uniform(-1, 1, (2, 7, 3)))
    eye = torch.tensor([[0.1, 0.2, -2.], [0.3, -0.1, -3.]], dtype=torch.float64)
    out = nr.look(v, eye, torch.tensor([0., 0., 1.], dtype=torch.float64), torch.tensor([0., 1., 0.], dtype=torch.float64))
    assert torch.allclose(out, v - eye[:, None, :], atol=1e-15)
    out = nr.look(v, eye[0], torch.tensor([1., 0., 0.], dtype=torch.float64), torch.tensor([0., 1., 0.], dtype=torch.float64))
    d = v - eye[0]
    assert torch.allclose(out, torch.stack((-d[..., 2], d[..., 1], d[..., 0]), -1), atol=1e-15)


def test_abi_projection_rejects_bad_arguments():
    """Argument validation runs before any launch (no GPU touched)."""
    L = _lib.lib()
    assert L.nr_projection_args_size() == ctypes.sizeof(_lib.NrProjectionArgs)
    assert L.nr_projection_forward(None, None, None) == 1 and b"null projection args" in L.nr_last_error()
    assert L.nr_projection_backward(None, None, None, None, None, None, None, None, 0, None) == 1
    p = _lib.NrProjectionArgs()
    p.batch_size, p.num_vertices = -1, 4
    assert L.nr_projection_forward(ctypes.byref(p), None, None) == 1 and b"bad sizes" in L.nr_last_error()
    p.batch_size, p.num_vertices = 2, -4
    assert L.nr_projection_backward(ctypes.byref(p), None, None, None, None, None, None, None, 0, None) == 1
    assert b"bad sizes" in L.nr_last_error()
    p.batch_size, p.num_vertices = 2, 4
    assert L.nr_projection_forward(ctypes.byref(p), None, None) == 1 and b"null vertices" in L.nr_last_error()
    # empty problems succeed without a launch and need no workspace
    p.batch_size, p.num_vertices = 0, 4
    assert L.nr_projection_forward(ctypes.byref(p), None, None) == 0
    p.batch_size, p.num_vertices = 2, 0
    assert L.nr_projection_forward(ctypes.byref(p), None, None) == 0
    assert L.nr_projection_workspace_bytes(0, 5) == 0 and L.nr_projection_workspace_bytes(5, 0) == 0
    assert L.nr_projection_workspace_bytes(3, 257) >= 3 * 2 * 24 * 4
    # the look mode is a valid camera mode; an unknown one is not
    c = _lib.NrCameraArgs()
    c.mode = 3
    assert L.nr_camera_forward(ctypes.byref(c), None, None) == 1 and b"bad camera mode" in L.nr_last_error()
    c.mode = _lib.NR_CAMERA_LOOK
    assert L.nr_camera_forward(ctypes.byref(c), None, None) == 0


def test_stale_library_asks_for_a_rebuild(tmp_path, monkeypatch):
    """A library of the same ABI version without the nr_projection_* symbols: the usual rebuild error."""
    import subprocess
    src = tmp_path / "stale.c"
    src.write_text("int nr_version(void) { return %d; }\n" % _lib.ABI_VERSION)
    so = str(tmp_path / "libstale.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", so])
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", so)
    with pytest.raises(RuntimeError, match="rebuild"):
        _lib.lib()

"""rigid_align_torch and icp_torch on the CPU: exact recovery, the closed-form backward against autograd through the
SVD composition, the corner cases, validation, dispatch and the ABI's names.  No GPU is touched."""
import os
import re

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import _lib, rigid
from conftest import ROOT
from rigid_cases import closed_form_backward, rotation, teapot_scan

EYE = torch.eye(3, dtype=torch.float64)


def cloud(B, N, seed=1):
    return torch.as_tensor(np.random.RandomState(seed).normal(size=(B, N, 3)))


def proper(R, tol=1e-12):
    assert bool(torch.isfinite(R).all())
    assert float((R @ R.transpose(-1, -2) - torch.eye(3, dtype=R.dtype)).abs().max()) <= tol
    assert bool((torch.linalg.det(R) > 0).all())


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("scale", [False, True])
def test_recovers_a_known_similarity(scale, weighted):
    x = cloud(3, 40)
    R0 = torch.stack([rotation((1., 2., 3.), 0.5), rotation((-1., 0.5, 0.2), 2.9), rotation((0., 0., 1.), 1e-3)])
    t0 = torch.as_tensor(np.random.RandomState(2).normal(size=(3, 3)))
    s0 = torch.tensor([1.3, 0.6, 2.], dtype=torch.float64) if scale else torch.ones(3, dtype=torch.float64)
    y = s0[:, None, None] * (x @ R0.transpose(1, 2)) + t0[:, None]
    w = torch.as_tensor(np.random.RandomState(3).uniform(0., 1., (3, 40))) if weighted else None
    R, t, s, c = nr.rigid_align_torch(x, y, w, scale, return_condition=True)
    assert float((R - R0).abs().max()) <= 1e-12 and float((t - t0).abs().max()) <= 1e-12 and float((s - s0).abs().max()) <= 1e-12
    proper(R)
    assert bool((c > 0.1).all())
    # unbatched, and a shared y
    R1, t1, s1 = nr.rigid_align_torch(x[0], y[0], None if w is None else w[0], scale)
    assert R1.shape == (3, 3) and t1.shape == (3,) and s1.shape == ()
    assert float((R1 - R0[0]).abs().max()) <= 1e-12
    Rs, ts, ss = nr.rigid_align_torch(x, y[0], w, scale)
    assert Rs.shape == (3, 3, 3) and float((Rs[0] - R0[0]).abs().max()) <= 1e-12


def test_mirrored_cloud_stays_proper():
    x = cloud(2, 30)
    y = x * torch.tensor([-1., 1., 1.], dtype=torch.float64) + 0.3
    R, t, s, c = nr.rigid_align_torch(x, y, scale=True, return_condition=True)
    proper(R)
    # condition follows the definition: (s2 + d s3) / s1 with d = -1 here
    xc, yc = x - x.mean(1, keepdim=True), y - y.mean(1, keepdim=True)
    S = torch.linalg.svdvals(torch.einsum("bni,bnj->bij", yc, xc))
    assert float((c - (S[:, 1] - S[:, 2]) / S[:, 0]).abs().max()) <= 1e-12
    assert float((s - (S[:, 0] + S[:, 1] - S[:, 2]) / (xc * xc).sum((1, 2))).abs().max()) <= 1e-12


@pytest.mark.parametrize("shared", [False, True], ids=["per_item", "shared_y"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("scale", [False, True])
def test_closed_form_backward_matches_autograd(scale, weighted, shared):
    B, N = 3, 25
    x = cloud(B, N, 4)
    y = 1.2 * (x @ torch.stack([rotation((1., -1., 0.5), 0.4 + b) for b in range(B)]).transpose(1, 2)) + 0.1 * cloud(B, N, 5)
    if shared:
        y = y[0]
    y[..., 0] *= -1. if weighted else 1.  # reflected inputs as well
    w = torch.as_tensor(np.random.RandomState(6).uniform(0.1, 1., (B, N))) if weighted else torch.ones((B, N), dtype=torch.float64)
    rng = np.random.RandomState(7)
    gR, gt, gs = (torch.as_tensor(rng.normal(size=shape)) for shape in ((B, 3, 3), (B, 3), (B,)))
    a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    R, t, s = nr.rigid_align_torch(a, b, w if weighted else None, scale)
    ((R * gR).sum() + (t * gt).sum() + (s * gs).sum()).backward()
    gx, gy = closed_form_backward(x, y if y.ndim == 3 else y[None].expand(B, -1, -1), w, scale, gR, gt, gs)
    if shared:
        gy = gy.sum(0)
    for got, want in ((gx, a.grad), (gy, b.grad)):
        assert float((got - want).abs().max()) <= 1e-10 * float(want.abs().max())


def test_corner_cases():
    x, y = cloud(2, 5, 8), cloud(2, 5, 9)
    # W == 0
    R, t, s, c = nr.rigid_align_torch(x, y, torch.zeros((2, 5), dtype=torch.float64), True, return_condition=True)
    assert torch.equal(R, EYE.expand(2, 3, 3)) and torch.equal(t, torch.zeros_like(t)) and torch.equal(s, torch.ones_like(s))
    assert torch.equal(c, torch.zeros_like(c))
    # N == 1: A == 0
    R, t, s, c = nr.rigid_align_torch(x[:, :1], y[:, :1], None, True, return_condition=True)
    assert torch.equal(R, EYE.expand(2, 3, 3)) and torch.equal(s, torch.ones_like(s)) and torch.equal(c, torch.zeros_like(c))
    assert float((t - (y[:, 0] - x[:, 0])).abs().max()) <= 1e-15
    # coincident points
    R, t, s = nr.rigid_align_torch(x[:, :1].expand(-1, 5, -1), y, None, True)
    assert torch.equal(R, EYE.expand(2, 3, 3)) and torch.equal(s, torch.ones_like(s))
    assert float((t - (y.mean(1) - x[:, 0])).abs().max()) <= 1e-15
    # N == 2 and collinear points: any maximiser, proper; the pairs are still matched where the lengths agree
    for xs, ys in ((x[:, :2], y[:, :2]), (x[:, :1] + torch.arange(5.)[None, :, None] * x[:, 1:2], y)):
        R, t, s, c = nr.rigid_align_torch(xs, ys, None, True, return_condition=True)
        proper(R)
        assert bool(torch.isfinite(t).all() and torch.isfinite(s).all() and (c.abs() <= 1e-12).all())
    R, t, s = nr.rigid_align_torch(x[:, :2], y[:, :2], None, True)
    assert float((s[:, None, None] * (x[:, :2] @ R.transpose(1, 2)) + t[:, None] - y[:, :2]).abs().max()) <= 1e-12


def test_icp_torch_recovers_the_teapot_motion():
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 2e-6)):
        x, y, R, t, want = teapot_scan(dtype)
        res = nr.icp_torch(x, y, iterations=30)
        assert isinstance(res, nr.ICPResult) and res.rmse.shape == (3, 31) and res.index.dtype == torch.int32
        assert float((res.R.double() - R).abs().max()) <= tol and float((res.t.double() - t).abs().max()) <= tol
        assert torch.equal(res.index.long(), want[None].expand(3, -1)) and float(res.rmse[:, -1].max()) <= 1e-6
        assert torch.equal(res.s, torch.ones(3, dtype=dtype)) and not res.R.requires_grad
    one = nr.icp_torch(x[0], y, iterations=2, init=(R[0], t[0], 1.))
    assert one.R.shape == (3, 3) and one.rmse.shape == (3,) and one.index.shape == (x.shape[1],)
    assert float(one.rmse[0]) <= 1e-6


def test_icp_torch_rejection_and_zero_iterations():
    x, y, R, t, want = teapot_scan(torch.float64)
    init = (R, t, torch.ones(3, dtype=torch.float64))
    res = nr.icp_torch(x, y, iterations=0, init=init)
    assert torch.equal(res.R, R) and torch.equal(res.t, t) and res.rmse.shape == (3, 1)
    # every weight 0: the transform stays at init and rmse is 0
    far = nr.icp_torch(x + 5., y, iterations=3, max_distance=1e-3, init=init)
    assert torch.equal(far.R, R) and torch.equal(far.t, t) and torch.equal(far.rmse, torch.zeros(3, 4, dtype=torch.float64))
    # outliers beyond max_distance change nothing
    out = torch.cat([x, x[:, :50] + 10.], 1)
    a, b = nr.icp_torch(x, y, iterations=20, max_distance=0.5), nr.icp_torch(out, y, iterations=20, max_distance=0.5)
    assert float((a.R - b.R).abs().max()) <= 1e-12 and float((a.t - b.t).abs().max()) <= 1e-12
    assert bool((b.dist2[:, -50:] > 0.25).all())


def test_validation():
    x, y = torch.zeros(2, 4, 3), torch.zeros(2, 4, 3)
    for call in (lambda: nr.rigid_align(x[:, :0], y[:, :0]), lambda: nr.rigid_align(x, y[:, :3]), lambda: nr.rigid_align(x, y[:1]),
                 lambda: nr.rigid_align(x, y, torch.zeros(2, 3)), lambda: nr.rigid_align(x[0], y),
                 lambda: nr.icp(x[:, :0], y), lambda: nr.icp(x, y[:, :0]), lambda: nr.icp(x, y, iterations=-1),
                 lambda: nr.icp(x, torch.zeros(3, 4, 3)), lambda: nr.icp(x, y, max_distance=-1.),
                 lambda: nr.icp(x, y, init=(torch.zeros(2, 3), torch.zeros(2, 3), torch.ones(2))),
                 lambda: nr.icp_torch(x, y, iterations=-1), lambda: nr.icp_torch(x, y, max_distance=-0.5)):
        with pytest.raises(ValueError):
            call()


def test_cpu_and_float64_run_the_composition(monkeypatch):
    def no_library(*a):
        raise AssertionError("the HIP library was loaded")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(rigid.RigidAlignFunction, "apply", no_library)
    x = cloud(2, 9).float().requires_grad_(True)
    y = cloud(2, 9, 3).float()
    R, t, s, c = nr.rigid_align(x, y, scale=True, return_condition=True)
    assert R.dtype == torch.float32 and c.shape == (2,)
    (R.sum() + t.sum() + s.sum()).backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0.
    assert nr.rigid_align(x.double(), y.double())[0].dtype == torch.float64
    res = nr.icp(x.detach().double(), y.double(), iterations=2)
    assert res.R.dtype == torch.float64 and res.index.dtype == torch.int32 and res.dist2.dtype == torch.float64


def test_abi_names_and_argument_checks():
    """The new entry points are in the header and in the binding's table, and validate before any launch (no GPU
    touched)."""
    header = open(os.path.join(ROOT, "include", "nr_raster.h")).read()
    for name in ("nr_rigid_workspace_bytes", "nr_rigid_align_forward", "nr_rigid_align_backward", "nr_icp_workspace_bytes", "nr_icp"):
        assert re.search(r"^NR_API \w+ %s\(" % name, header, re.M), name
        assert name in _lib.SIGNATURES and name in _lib.EXPORTS
    assert re.search(r"^#define NR_RIGID_MIN_CONDITION 1e-6f$", header, re.M)
    assert nr.NR_RIGID_MIN_CONDITION == _lib.NR_RIGID_MIN_CONDITION == 1e-6
    for name in ("rigid_align", "rigid_align_torch", "icp", "icp_torch", "ICPResult"):
        assert hasattr(nr, name)
    L = _lib.lib()
    p, err, big = 4096, L.nr_last_error, 1 << 40  # p: a non-null pointer value, never dereferenced on these paths
    assert L.nr_rigid_workspace_bytes(0, 5) == 0 and L.nr_rigid_workspace_bytes(2, 0) == 0
    assert L.nr_rigid_workspace_bytes(1, 1024) == 512 and L.nr_rigid_workspace_bytes(8, 1025) == 2 * 8 * (8 + 12) * 4
    assert L.nr_icp_workspace_bytes(1, 5, 0) == 0 and L.nr_icp_workspace_bytes(1, 1024, 100) == 512
    # few queries against many targets: the split path's partial (d2, j) pairs on top
    assert L.nr_icp_workspace_bytes(1, 5, 3074) == 512 + 2 * 256

    def fwd(x=p, y=p, y_bs=0, w=None, w_bs=0, B=1, N=4, scale=0, R=p, t=p, s=p, cond=None, rec=None, ws=p, nbytes=big):
        return L.nr_rigid_align_forward(x, y, y_bs, w, w_bs, B, N, scale, R, t, s, cond, rec, ws, nbytes, None)
    assert fwd(B=-1) == 1 and b"bad batch size" in err()
    assert fwd(N=0) == 1 and b"empty point set" in err()
    assert fwd(B=65536) == 1 and b"too many items" in err()
    assert fwd(B=4096, N=2 ** 20) == 1 and b"too many points" in err()
    assert fwd(y_bs=7) == 1 and b"y_batch_stride" in err()
    assert fwd(w=p, w_bs=3) == 1 and b"w_batch_stride" in err()
    assert fwd(x=None) == 1 and fwd(R=None) == 1 and fwd(s=None) == 1 and b"null" in err()
    assert fwd(ws=None, nbytes=0) == 3 and fwd(nbytes=511) == 3
    assert fwd(B=0, x=None) == 0

    def bwd(x=p, y=p, y_bs=12, w=None, w_bs=0, rec=p, B=1, N=4, gx=p, gy=p, ws=p, nbytes=big):
        return L.nr_rigid_align_backward(x, y, y_bs, w, w_bs, rec, p, p, p, B, N, 1, gx, gy, ws, nbytes, None)
    assert bwd(N=0) == 1 and bwd(y_bs=11) == 1 and bwd(rec=None) == 1 and bwd(x=None) == 1
    assert bwd(nbytes=8) == 3 and bwd(gx=None, gy=None, x=None) == 0 and bwd(B=0) == 0

    def run(x=p, y=p, y_bs=0, B=1, N=4, M=5, it=3, maxd=-1., T=p, rmse=p, idx=p, d2=p, ws=p, nbytes=big):
        return L.nr_icp(x, y, y_bs, B, N, M, it, 0, maxd, T, rmse, idx, d2, ws, nbytes, None)
    assert run(M=0) == 1 and b"empty point set" in err()
    assert run(it=-1) == 1 and b"negative iterations" in err()
    assert run(y_bs=9) == 1 and b"y_batch_stride" in err()
    assert run(maxd=float("nan")) == 1 and b"NaN" in err()
    assert run(T=None) == 1 and run(rmse=None) == 1 and run(idx=None) == 1 and run(d2=None) == 1 and b"null pointer" in err()
    assert run(ws=None, nbytes=0) == 3 and run(nbytes=100) == 3
    assert run(B=0) == 0
    t, f = _lib.c_int(), _lib.c_int()
    assert L.nr_last_launch(b"k_icp_nn", t, f) == 1 and b"no k_icp_nn launch recorded" in err()

"""The fused rigid_align on the GPU (float32) against rigid_align_torch in float64 on the CPU, which receives the
same float32 values widened.

Inputs are rigid_cases.CASES: per item a uniform cloud of extent 1 and a rotated, scaled, shifted and noised copy,
for N = 1, 2, 3, 63, 65, 257, 1025 (just past one chunk of the sums) and 263,173 (257 chunks: every loop over
partial sums takes a second trip), B = 1 and 3, and `far`, whose centroids lie 100 extents from the origin.  Each
case runs with y per item and shared, scale off and on, and no weights, random weights and random weights with
a block of zeros (rigid_cases.VARIANTS).

Tolerances follow test_gpu_arap_loss's protocol.  FLOAT32_ERROR is what rigid_align_torch itself loses in float32
on the CPU (torch.linalg.svd) against float64 on exactly these inputs: the largest |d| over the twelve variants
and over the items whose float64 condition is at least 0.1 (rigid_cases.float32_error):

  case        R          t          s          condition
  n3          3.00e-7    4.69e-8    1.21e-7    5.63e-8
  n63         3.40e-7    9.98e-8    2.98e-7    5.09e-7
  n65         2.73e-7    4.05e-8    1.06e-7    5.69e-7
  n257        4.11e-7    5.55e-8    3.49e-7    7.08e-7
  n1025       5.06e-7    9.05e-8    2.71e-7    6.82e-7
  two_trips   3.54e-7    3.40e-8    1.29e-7    2.53e-7
  far         3.50e-7    5.26e-5    2.90e-7    8.25e-7

(n1 and n2 have no such item; n3 has some in the eight variants without a zero weight.)  The fused path is allowed 4x these
figures.  The float64 conditions are 0.92 to 1.99 from n63 on.  Items below 0.1 (N <= 3, or fewer effective points
through zero weights) are checked for orthonormality, det > 0 and finiteness only.  Gradients: close_grads of
test_gpu_point_loss, on the items that qualify."""
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import rigid
from rigid_cases import CASES, SURE, VARIANTS, pairs, reference, upstream, weights, wide
from test_gpu_point_loss import close_grads

pytestmark = pytest.mark.gpu

FLOAT32_ERROR = {  # measured: float32 rigid_align_torch on the CPU against float64 (the module docstring)
    "n1": dict(R=0., t=0., s=0., condition=0.), "n2": dict(R=0., t=0., s=0., condition=0.),
    "n3": dict(R=3.00e-7, t=4.69e-8, s=1.21e-7, condition=5.63e-8),
    "n63": dict(R=3.40e-7, t=9.98e-8, s=2.98e-7, condition=5.09e-7),
    "n65": dict(R=2.73e-7, t=4.05e-8, s=1.06e-7, condition=5.69e-7),
    "n257": dict(R=4.11e-7, t=5.55e-8, s=3.49e-7, condition=7.08e-7),
    "n1025": dict(R=5.06e-7, t=9.05e-8, s=2.71e-7, condition=6.82e-7),
    "two_trips": dict(R=3.54e-7, t=3.40e-8, s=1.29e-7, condition=2.53e-7),
    "far": dict(R=3.50e-7, t=5.26e-5, s=2.90e-7, condition=8.25e-7),
}
EYE = torch.eye(3, dtype=torch.float64)


def tolerance(name, key):
    return 4 * FLOAT32_ERROR[name][key]


def on(dev, t):
    return None if t is None else t.to(dev)


def fused(name, shared, scale, kind, dev, grads=True):
    x, y = pairs(name, shared)
    a, b = x.to(dev).requires_grad_(grads), y.to(dev).requires_grad_(grads)
    out = nr.rigid_align(a, b, on(dev, weights(name, kind)), scale, return_condition=True)
    if grads:
        gR, gt, gs = (g.to(device=dev, dtype=torch.float32) for g in upstream(name))
        torch.autograd.backward(out[:3], (gR, gt, gs))
    return tuple(o.detach() for o in out) + (a.grad, b.grad)


def check_proper(R, t, s, c, what):
    assert all(bool(torch.isfinite(v).all()) for v in (R, t, s, c)), what
    assert float((R @ R.transpose(-1, -2) - EYE).abs().max()) <= 1e-5, what
    assert bool((torch.linalg.det(R) > 0).all()), what
    assert bool(((c >= 0) & (c <= 2.00001)).all()), what


@pytest.mark.parametrize("name", list(CASES))
def test_fused_matches_float64(dev, name):
    B, N, _ = CASES[name]
    compared = 0
    for shared, scale, kind in VARIANTS:
        what = "%s shared=%d scale=%d %s" % (name, shared, scale, kind)
        ref = reference(name, shared, scale, kind)
        R, t, s, c, gx, gy = fused(name, shared, scale, kind, dev)
        assert R.shape == (B, 3, 3) and t.shape == (B, 3) and s.shape == (B,) and c.shape == (B,) and R.dtype == torch.float32
        assert not c.requires_grad and gx.shape == (B, N, 3) and gy.shape == pairs(name, shared)[1].shape
        R, t, s, c = (v.cpu().double() for v in (R, t, s, c))
        check_proper(R, t, s, c, what)
        assert bool(torch.isfinite(gx).all() and torch.isfinite(gy).all()), what
        if not scale:
            assert torch.equal(s, torch.ones_like(s)), what
        sure = ref["condition"] >= SURE  # asserted on the float64 reference, before any rotation is compared
        if N >= 63:
            assert bool(sure.all()), (what, ref["condition"].tolist())
        if not bool(sure.any()):
            continue
        compared += 1
        err = {k: float((v - ref[k])[sure].abs().max()) for k, v in (("R", R), ("t", t), ("s", s), ("condition", c))}
        print("%s: %s allowed %s" % (what, {k: "%.3g" % v for k, v in err.items()},
                                     {k: "%.3g" % tolerance(name, k) for k in err}))
        for k in err:
            assert err[k] <= tolerance(name, k), (what, k, err[k], tolerance(name, k))
        if bool(sure.all()):
            close_grads(gx, ref["gx"], what + " grad x")
            close_grads(gy, ref["gy"], what + " grad y")
    assert compared == (0 if N < 3 else 8 if N == 3 else len(VARIANTS)), compared


def test_stated_values_of_the_corner_cases(dev):
    x, y = (v.to(dev) for v in pairs("n63", False))
    B = x.shape[0]
    eye = torch.eye(3, device=dev).expand(B, 3, 3)
    # W == 0
    R, t, s, c = nr.rigid_align(x, y, torch.zeros(x.shape[:2], device=dev), True, return_condition=True)
    assert torch.equal(R, eye) and torch.equal(t, torch.zeros_like(t)) and torch.equal(s, torch.ones_like(s))
    assert torch.equal(c, torch.zeros_like(c))
    # N == 1, and coincident points: A == 0 and var == 0 exactly
    R, t, s, c = nr.rigid_align(x[:, :1], y[:, :1], None, True, return_condition=True)
    assert torch.equal(R, eye) and torch.equal(s, torch.ones_like(s)) and torch.equal(c, torch.zeros_like(c))
    assert float((t - (y[:, 0] - x[:, 0])).abs().max()) <= 1e-7
    R, t, s = nr.rigid_align(x[:, :1].expand(-1, 63, -1), y, None, True)
    assert torch.equal(R, eye) and torch.equal(s, torch.ones_like(s))
    assert float((t.cpu().double() - (y.cpu().double().mean(1) - x[:, 0].cpu().double())).abs().max()) <= 1e-6
    # collinear points: some maximiser, proper
    line = x[:, :1] + torch.arange(63., device=dev)[None, :, None] * (x[:, 1:2] - x[:, :1])
    out = nr.rigid_align(line, y, None, True, return_condition=True)
    check_proper(*(v.cpu().double() for v in out), "collinear")
    # unbatched inputs give unbatched results
    R, t, s, c = nr.rigid_align(x[0], y[0], return_condition=True)
    assert R.shape == (3, 3) and t.shape == (3,) and s.shape == () and c.shape == ()


def test_ill_conditioned_gradients_are_finite(dev):
    """N = 2: condition is below NR_RIGID_MIN_CONDITION, the rotation passes no gradient, t and s still do."""
    x, y = pairs("n2", False)
    a, b = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    R, t, s, c = nr.rigid_align(a, b, None, True, return_condition=True)
    assert float(c.max()) <= 1e-5
    (R.sum() + t.sum() + s.sum()).backward()
    assert bool(torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all())
    assert float(b.grad.abs().max()) > 0.
    # the rotation alone: nothing where condition <= NR_RIGID_MIN_CONDITION
    a.grad = None
    R, t, s, c = nr.rigid_align(a, b, None, False, return_condition=True)
    R.sum().backward()
    assert bool(torch.isfinite(a.grad).all())
    dead = c <= nr.NR_RIGID_MIN_CONDITION
    assert float(a.grad[dead].abs().max() if bool(dead.any()) else 0.) == 0.


@pytest.mark.parametrize("name", ["n257", "n1025", "far"])
def test_reproducible_and_independent_of_the_batch(dev, name):
    for shared, scale, kind in ((False, True, "random"), (True, False, "zeros")):
        first = fused(name, shared, scale, kind, dev)
        again = fused(name, shared, scale, kind, dev)
        for u, v in zip(first, again):
            assert torch.equal(u, v)
        # item 0 alone
        x, y = pairs(name, shared)
        w = weights(name, kind)
        a = x[:1].to(dev).requires_grad_(True)
        b = (y if shared else y[:1]).to(dev).requires_grad_(True)
        out = nr.rigid_align(a, b, w[:1].to(dev), scale, return_condition=True)
        gR, gt, gs = (g[:1].to(device=dev, dtype=torch.float32) for g in upstream(name))
        torch.autograd.backward(out[:3], (gR, gt, gs))
        for u, v in zip(first[:4], out):
            assert torch.equal(u[:1], v.detach())
        assert torch.equal(first[4][:1], a.grad)
        if not shared:
            assert torch.equal(first[5][:1], b.grad)


def test_weights_that_require_grad_take_the_composition(dev, monkeypatch):
    x, y = (v.to(dev) for v in pairs("n65", False))
    w = weights("n65", "random").to(dev)
    want = nr.rigid_align(x, y, w, True, return_condition=True)

    def no_fused(*a):
        raise AssertionError("the fused path ran")
    monkeypatch.setattr(rigid.RigidAlignFunction, "apply", no_fused)
    wg = w.clone().requires_grad_(True)
    got = nr.rigid_align(x, y, wg, True, return_condition=True)
    for u, v, tol in zip(got, want, (2e-6, 2e-6, 2e-6, 4e-6)):
        assert float((u.detach() - v).abs().max()) <= tol
    (got[0].sum() + got[1].sum() + got[2].sum()).backward()
    assert bool(torch.isfinite(wg.grad).all()) and float(wg.grad.abs().max()) > 0.
    # float64 on the GPU as well
    assert nr.rigid_align(x.double(), y.double())[0].dtype == torch.float64

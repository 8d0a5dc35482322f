"""mesh_point_distance / closest_points_to_faces on the CPU: the torch composition against a brute-force loop
over the faces built from closest_points_on_mesh_torch, the tie and degenerate-face rules, the point= override,
gradcheck, the host logic (shapes, flags, errors) and the example's flag.  The fused path is covered by
test_gpu_mesh_point.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import point_loss, synthetic
from conftest import ROOT


def jittered_icosphere(level, B=None, seed=5, F=None):
    v, f = synthetic.icosphere(level, radius=0.5)
    rs = np.random.RandomState(seed)
    shape = v.shape if B is None else (B,) + v.shape
    return torch.as_tensor(v + rs.uniform(-0.02, 0.02, shape)), torch.as_tensor(f[:F].astype(np.int64))


def box_points(n, seed=6, B=None):
    return torch.as_tensor(np.random.RandomState(seed).uniform(-1, 1, (n, 3) if B is None else (B, n, 3)))


def per_face(p, v, f):
    """[B, F, N] float64: the squared distance of every (face, point) pair, one face at a time through
    closest_points_on_mesh_torch."""
    return torch.stack([nr.closest_points_on_mesh_torch(p, v, f[k:k + 1])[0] for k in range(f.shape[0])], 1)


def test_composition_matches_brute_force():
    B, N, F = 2, 50, 30
    v, f = jittered_icosphere(1, B=B, F=F)
    p = box_points(N, B=B, seed=9)
    dist2, point, w = nr.closest_points_to_faces_torch(v, f, p)
    assert dist2.shape == (B, F) and dist2.dtype == torch.float64 and point.shape == (B, F) and point.dtype == torch.int32
    assert w.shape == (B, F, 3)
    pairs = per_face(p, v, f)
    want_d2, want_i = pairs.min(2)
    assert torch.equal(point.long(), want_i)
    assert float((dist2 - want_d2).abs().max()) <= 1e-15
    # the global minimum over all pairs is the same number from both directions.  The point set (seed 9) is one
    # whose globally nearest pair lies inside its face in both items: on an edge two faces share the closest
    # point, and each direction may report it through the other face's weights, one rounding apart
    assert all(bool((w[b, int(dist2[b].argmin())] > 0).all()) for b in range(B))
    other = nr.closest_points_on_mesh_torch(p, v, f)[0]
    assert torch.equal(dist2.min(1)[0], other.min(1)[0])
    # dist2 is the squared distance to the point the weights describe
    assert bool((w >= 0).all()) and bool((w <= 1).all()) and float((w.sum(-1) - 1).abs().max()) <= 1e-12
    c = (w[..., None] * v[:, f]).sum(2)
    q = p.gather(1, point.long()[..., None].expand(-1, -1, 3))
    assert float((((q - c) ** 2).sum(-1) - dist2).abs().max()) <= 1e-15
    loss = nr.mesh_point_distance_torch(v, f, p)
    assert torch.allclose(loss, want_d2.mean(1), rtol=1e-13, atol=0)


def test_first_of_equal_minima():
    v, f = jittered_icosphere(1, B=2, F=30)
    p = box_points(20, B=2)
    _, point, _ = nr.closest_points_to_faces_torch(v, f, p)
    twice = torch.cat([p, p, p], 1)
    d2, again, _ = nr.closest_points_to_faces_torch(v, f, twice)
    assert int(again.max()) < 20 and torch.equal(again, point)
    # the copies first: the winner is the copy's index
    moved = torch.cat([p.flip(1), p], 1)
    assert torch.equal(nr.closest_points_to_faces_torch(v, f, moved)[1], 19 - point)


# the sibling test's small-integer segments: corners 0 and 3 coincide, corner 2 is the midpoint of 0 and 1
DEGENERATE_V = [[0., 0, 0], [4, 0, 0], [2, 0, 0], [0, 0, 0], [7, 7, 7]]
DEGENERATE = {  # name: (face, the segment's end corners as positions in the face, or one position for a point)
    "repeated_index": ([0, 1, 1], (0, 1)),
    "coincident_corners": ([0, 3, 1], (0, 2)),
    "collinear": ([0, 2, 1], (0, 2)),
    "collinear_rotated": ([2, 1, 0], (1, 2)),
    "point": ([0, 3, 3], (0,)),
}
DEGENERATE_P = [[1., 2, 0], [3, 1, 0], [-1, 1, 0], [6, 0, 1], [2, 0, 0.5], [0.5, -3, 2]]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_faces_are_segments_or_points(name, dtype):
    face, ends = DEGENERATE[name]
    v = torch.tensor(DEGENERATE_V, dtype=dtype)
    p = torch.tensor(DEGENERATE_P, dtype=dtype)
    dist2, idx, w = nr.closest_points_to_faces_torch(v, torch.tensor([face, [0, 1, 4]]), p)
    corners = v[torch.tensor(face)]
    if len(ends) == 1:
        all_d2 = ((p - corners[ends[0]]) ** 2).sum(-1)
        t = None
    else:
        a, b = corners[ends[0]], corners[ends[1]]
        t = (((p - a) * (b - a)).sum(-1) / ((b - a) ** 2).sum()).clamp(0, 1)
        all_d2 = ((p - (a + t[:, None] * (b - a))) ** 2).sum(-1)
    best = int(all_d2.argmin())
    want_w = torch.zeros(3, dtype=dtype)
    if t is None:
        want_w[ends[0]] = 1
    else:
        want_w[ends[0]], want_w[ends[1]] = 1 - t[best], t[best]
    assert int(idx[0]) == best and torch.equal(dist2[0], all_d2[best])  # small integers and quarters: exact
    assert torch.equal(w[0], want_w), (w[0], want_w)
    assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(dist2).all())
    # the regular face beside it is not disturbed
    alone = nr.closest_points_to_faces_torch(v, torch.tensor([[0, 1, 4]]), p)
    assert torch.equal(dist2[1], alone[0][0]) and int(idx[1]) == int(alone[1][0])


def test_point_override_uses_the_given_points():
    v, f = jittered_icosphere(1, B=2, F=30)
    p = box_points(40, B=2)
    own = nr.closest_points_to_faces_torch(v, f, p)[1]
    assert torch.equal(nr.mesh_point_distance_torch(v, f, p, point=own), nr.mesh_point_distance_torch(v, f, p))
    pairs = per_face(p, v, f)
    for k in (0, 17):
        forced = nr.mesh_point_distance_torch(v, f, p, point=torch.full((2, 30), k))
        assert torch.allclose(forced, pairs[:, :, k].mean(1), rtol=1e-13, atol=0)
        assert bool((forced > nr.mesh_point_distance_torch(v, f, p)).all())
    mixed = (own.long() + torch.arange(30) % 2) % 40
    want = pairs.gather(2, mixed[..., None])[..., 0].mean(1)
    assert torch.allclose(nr.mesh_point_distance_torch(v, f, p, point=mixed), want, rtol=1e-13, atol=0)
    with pytest.raises(IndexError):
        nr.mesh_point_distance_torch(v, f, p, point=torch.full((2, 30), 40))


def test_gradcheck_with_the_points_fixed():
    v, f = jittered_icosphere(0, B=2)
    p = box_points(12, B=2)
    point = nr.closest_points_to_faces_torch(v, f, p)[1]
    a, b = v.clone().requires_grad_(True), p.clone().requires_grad_(True)
    # the weights are constants of the composition: by the envelope theorem the analytic gradient is still the
    # derivative of the squared distance, which the numeric side sees with the weights following
    assert torch.autograd.gradcheck(lambda x, y: nr.mesh_point_distance_torch(x, f, y, point=point), (a, b), eps=1e-6, atol=1e-6,
                                    rtol=1e-4)
    # and the issue's closed forms
    g = torch.as_tensor(np.random.RandomState(7).normal(size=2))
    nr.mesh_point_distance_torch(a, f, b, point=point).backward(g)
    _, _, w = nr.closest_points_to_faces_torch(v, f, p)
    F = f.shape[0]
    q = p.gather(1, point.long()[..., None].expand(-1, -1, 3))
    d = g[:, None, None] * (2. / F) * (q - (w[..., None] * v[:, f]).sum(2))
    gv, gp = torch.zeros_like(v), torch.zeros_like(p)
    for item in range(2):
        gp[item].index_add_(0, point[item].long(), d[item])
        for k in range(3):
            gv[item].index_add_(0, f[:, k], -w[item, :, k, None] * d[item])
    assert float((a.grad - gv).abs().max()) <= 1e-14 and float((b.grad - gp).abs().max()) <= 1e-14
    assert float(gv.abs().max()) > 0 and float(gp.abs().max()) > 0


def test_shapes_and_flags():
    v, f = jittered_icosphere(1, B=3)
    p = box_points(50, B=3)
    loss = nr.mesh_point_distance(v, f, p)
    assert loss.shape == (3,) and loss.dtype == torch.float64
    assert torch.equal(loss, nr.mesh_point_distance_torch(v, f, p))  # CPU float64: the composition
    assert torch.equal(nr.mesh_point_distance(v, f, p, average=True), loss.mean())
    one = nr.mesh_point_distance(v[1], f, p[1])
    assert one.ndim == 0 and torch.allclose(one, loss[1], rtol=1e-14, atol=0)
    # shared points against a batch of meshes
    shared = nr.mesh_point_distance(v, f, p[0])
    assert shared.shape == (3,) and torch.equal(shared, nr.mesh_point_distance(v, f, p[:1].expand(3, -1, -1)))
    s = p[0].clone().requires_grad_(True)
    nr.mesh_point_distance(v, f, s).sum().backward()
    e = p[:1].expand(3, -1, -1).clone().requires_grad_(True)
    nr.mesh_point_distance(v, f, e).sum().backward()
    assert s.grad.shape == (50, 3) and torch.allclose(s.grad, e.grad.sum(0), rtol=1e-13, atol=1e-16)
    # closest_points_to_faces: shapes, dtypes, detached; single inputs drop the item axis
    F = f.shape[0]
    d2, point, w = nr.closest_points_to_faces(v.clone().requires_grad_(True), f, p.clone().requires_grad_(True))
    assert d2.shape == (3, F) and point.shape == (3, F) and point.dtype == torch.int32 and w.shape == (3, F, 3)
    assert not (d2.requires_grad or w.requires_grad)
    assert torch.allclose(d2.mean(1), loss, rtol=1e-14, atol=0)
    d1, p1, w1 = nr.closest_points_to_faces(v[2], f, p[2])
    assert d1.shape == (F,) and torch.equal(p1, point[2]) and w1.shape == (F, 3)
    # float32 on the CPU takes the composition too, in float32
    l32 = nr.mesh_point_distance(v.float(), f, p.float())
    assert l32.dtype == torch.float32 and torch.allclose(l32.double(), loss, rtol=1e-5, atol=0)
    # numpy faces, int32 faces
    assert torch.equal(nr.mesh_point_distance(v, f.numpy().astype(np.int32), p), loss)


def test_errors():
    v, f = jittered_icosphere(0, B=2)
    p = box_points(10, B=2)
    with pytest.raises(ValueError):
        nr.mesh_point_distance(v, f, p[:, :0])  # N = 0
    with pytest.raises(ValueError):
        nr.mesh_point_distance(v, f[:0], p)  # F = 0
    with pytest.raises(ValueError):
        nr.mesh_point_distance(v, f, box_points(10, B=3))  # batch mismatch
    with pytest.raises(ValueError):
        nr.mesh_point_distance(v[0], f, p)  # batched points against a single mesh
    with pytest.raises(ValueError):
        nr.closest_points_to_faces(v, f, p[..., :2])
    bad = f.clone()
    bad[3, 1] = v.shape[1]
    with pytest.raises(IndexError):
        nr.mesh_point_distance(v, bad, p)
    bad[3, 1] = -1
    with pytest.raises(IndexError):
        nr.closest_points_to_faces(v, bad, p)


def test_module():
    v, f = jittered_icosphere(1, B=2)
    p = box_points(30)
    mod = nr.MeshPointLoss(p)
    assert "points" in dict(mod.named_buffers()) and not list(mod.parameters())
    assert torch.equal(mod(v, f), nr.mesh_point_distance(v, f, p))
    other = box_points(30, seed=9, B=2)
    assert torch.equal(mod(v, f, other), nr.mesh_point_distance(v, f, other))
    assert torch.equal(nr.MeshPointLoss(p, average=True)(v, f), nr.mesh_point_distance(v, f, p, average=True))
    assert torch.equal(nr.MeshPointLoss()(v, f, points=p), nr.mesh_point_distance(v, f, p))
    with pytest.raises(ValueError):
        nr.MeshPointLoss()(v, f)
    assert mod.double().points.dtype == torch.float64


def test_composition_is_chunked(monkeypatch):
    """The nearest-point search in chunks of a few faces gives what one chunk gives."""
    v, f = jittered_icosphere(1, B=2)
    p = box_points(37, B=2)
    whole = nr.closest_points_to_faces_torch(v, f, p)
    monkeypatch.setattr(point_loss, "_CHUNK_PAIRS", 7 * 2 * 37)
    parts = nr.closest_points_to_faces_torch(v, f, p)
    assert all(torch.equal(a, b) for a, b in zip(whole, parts))


def test_example_flag():
    spec = importlib.util.spec_from_file_location("example_scan_fit", os.path.join(ROOT, "examples", "example_scan_fit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parser().parse_args([]).mesh_to_scan == "sampled"
    assert mod.parser().parse_args(["--mesh-to-scan", "exact"]).mesh_to_scan == "exact"
    with pytest.raises(SystemExit):
        mod.parser().parse_args(["--mesh-to-scan", "both"])

"""point_mesh_distance / closest_points_on_mesh on the CPU: the torch composition against an independent
brute force, the degenerate-face rule, the face= override, the closed-form gradients, and the host logic
(shapes, flags, errors).  The fused path is covered by test_gpu_point_mesh.py."""
import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import point_loss, synthetic

GRID = 40  # barycentric steps per edge of the brute force


def jittered_icosphere(level, B=None, seed=5):
    v, f = synthetic.icosphere(level, radius=0.5)
    rs = np.random.RandomState(seed)
    shape = v.shape if B is None else (B,) + v.shape
    return torch.as_tensor(v + rs.uniform(-0.02, 0.02, shape)), torch.as_tensor(f.astype(np.int64))


def box_points(n, seed=6, B=None):
    return torch.as_tensor(np.random.RandomState(seed).uniform(-1, 1, (n, 3) if B is None else (B, n, 3)))


def segment_dist2(p, a, b):
    e = b - a
    t = (((p - a) * e).sum(-1) / (e * e).sum(-1)).clamp(0, 1)
    d = p - (a + t[..., None] * e)
    return (d * d).sum(-1)


def brute_force(p, v, f):
    """[N, F] float64: per face the least squared distance from p to a dense barycentric grid of the
    triangle and to its three segments (exact).  Never below the true distance, and above it by at most
    (longest edge / GRID)^2: where the closest point is interior the offset to the nearest grid point lies
    in the plane, at right angles to p - c; elsewhere it is on a segment."""
    i, j = np.meshgrid(np.arange(GRID + 1), np.arange(GRID + 1), indexing="ij")
    keep = i + j <= GRID
    bary = torch.as_tensor(np.stack([GRID - i[keep] - j[keep], i[keep], j[keep]], -1) / GRID)  # [G, 3]
    out = []
    for tri in v[f]:  # [3, 3]
        grid = bary @ tri  # [G, 3]
        d = p[:, None] - grid[None]
        best = (d * d).sum(-1).min(1)[0]
        for k in range(3):
            best = torch.minimum(best, segment_dist2(p, tri[k], tri[(k + 1) % 3]))
        out.append(best)
    return torch.stack(out, 1)


def test_composition_matches_brute_force():
    v, f = jittered_icosphere(1)
    p = box_points(500)
    dist2, face, w = nr.closest_points_on_mesh_torch(p, v, f)
    assert dist2.dtype == torch.float64 and face.dtype == torch.int32 and w.shape == (500, 3)
    per_face = brute_force(p, v, f)
    brute = per_face.min(1)[0]
    tri = v[f]
    longest = max(float((tri[:, k] - tri[:, (k + 1) % 3]).norm(dim=-1).max()) for k in range(3))
    gap = brute - dist2
    print("brute force - composition: min %.3g max %.3g (allowed %.3g)" % (float(gap.min()), float(gap.max()), (longest / GRID) ** 2))
    assert float(gap.min()) >= -1e-12 and float(gap.max()) <= (longest / GRID) ** 2
    # the chosen face is a nearest one by the brute force too, and the weights describe the closest point
    assert bool((per_face.gather(1, face.long()[:, None])[:, 0] - brute <= (longest / GRID) ** 2).all())
    assert bool((w >= 0).all()) and bool((w <= 1).all()) and float((w.sum(-1) - 1).abs().max()) <= 1e-12
    c = (w[..., None] * v[f[face.long()]]).sum(1)
    assert float((((p - c) ** 2).sum(-1) - dist2).abs().max()) <= 1e-15
    # every region occurs: interior, edge and corner closest points
    ones, zeros = (w == 1).any(-1), (w == 0).sum(-1)
    assert bool(ones.any()) and bool((zeros == 1).any()) and bool((zeros == 0).any())


# small-integer coordinates: corners 0 and 3 coincide, corner 2 is the midpoint of 0 and 1
DEGENERATE_V = [[0., 0, 0], [4, 0, 0], [2, 0, 0], [0, 0, 0], [7, 7, 7]]
DEGENERATE = {  # name: (face, the segment's end corners as positions in the face, or one position for a point)
    "repeated_index": ([0, 1, 1], (0, 1)),       # ab and ac equally long: ab
    "coincident_corners": ([0, 3, 1], (0, 2)),   # ab has no length; ac and bc equally long: ac
    "collinear": ([0, 2, 1], (0, 2)),            # the middle corner is unused
    "collinear_rotated": ([2, 1, 0], (1, 2)),    # bc is the longest
    "point": ([0, 3, 3], (0,)),
}
DEGENERATE_P = [[1., 2, 0], [3, 1, 0], [-1, 1, 0], [6, 0, 1], [2, 0, 0], [0.5, -3, 2]]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_faces_are_segments_or_points(name, dtype):
    face, ends = DEGENERATE[name]
    v = torch.tensor(DEGENERATE_V, dtype=dtype)
    p = torch.tensor(DEGENERATE_P, dtype=dtype)
    dist2, idx, w = nr.closest_points_on_mesh_torch(p, v, torch.tensor([face]))
    assert bool((idx == 0).all()) and bool(torch.isfinite(w).all()) and bool(torch.isfinite(dist2).all())
    corners = v[torch.tensor(face)]
    if len(ends) == 1:
        want = ((p - corners[ends[0]]) ** 2).sum(-1)
        want_w = torch.zeros(len(p), 3, dtype=dtype)
        want_w[:, ends[0]] = 1
    else:
        a, b = corners[ends[0]], corners[ends[1]]
        want = segment_dist2(p, a, b)
        t = (((p - a) * (b - a)).sum(-1) / ((b - a) ** 2).sum()).clamp(0, 1)
        want_w = torch.zeros(len(p), 3, dtype=dtype)
        want_w[:, ends[0]], want_w[:, ends[1]] = 1 - t, t
    assert torch.equal(dist2, want), (dist2, want)  # small integers and quarters: exact
    assert torch.equal(w, want_w), (w, want_w)
    # and beside regular faces: the degenerate face wins where it is nearer
    both = torch.tensor([[0, 1, 4], face])
    d_both, idx_both, _ = nr.closest_points_on_mesh_torch(p, v, both)
    d_reg = nr.closest_points_on_mesh_torch(p, v, both[:1])[0]
    assert torch.equal(d_both, torch.minimum(d_reg, want)) and bool((idx_both[want < d_reg] == 1).all())


def test_face_override_uses_the_given_faces():
    v, f = jittered_icosphere(1, B=2)
    p = box_points(60, B=2)
    own = nr.closest_points_on_mesh_torch(p, v, f)[1]
    assert torch.equal(nr.point_mesh_distance_torch(p, v, f, face=own), nr.point_mesh_distance_torch(p, v, f))
    for k in (0, 17):
        forced = nr.point_mesh_distance_torch(p, v, f, face=torch.full((2, 60), k))
        assert torch.equal(forced, nr.point_mesh_distance_torch(p, v, f[k:k + 1]))
        assert bool((forced > nr.point_mesh_distance_torch(p, v, f)).all())
    mixed = (own.long() + torch.arange(60) % 2) % f.shape[0]
    per_face = torch.stack([nr.closest_points_on_mesh_torch(p, v, f[k:k + 1])[0] for k in range(f.shape[0])], -1)
    want = per_face.gather(2, mixed[..., None])[..., 0].mean(1)
    assert torch.allclose(nr.point_mesh_distance_torch(p, v, f, face=mixed), want, rtol=1e-13, atol=0)
    with pytest.raises(IndexError):
        nr.point_mesh_distance_torch(p, v, f, face=torch.full((2, 60), f.shape[0]))


def closed_form_gradients(p, v, f, g):
    """The issue's closed forms from closest_points_on_mesh_torch's face and weights."""
    B, N = p.shape[0], p.shape[1]
    _, face, w = nr.closest_points_on_mesh_torch(p, v, f)
    ids = f[face.long()]  # [B, N, 3]
    c = sum(w[..., k, None] * v.gather(1, ids[..., k, None].expand(-1, -1, 3)) for k in range(3))
    gp = g[:, None, None] * (2. / N) * (p - c)
    gv = torch.zeros_like(v)
    for b in range(B):
        for k in range(3):
            gv[b].index_add_(0, ids[b, :, k], -w[b, :, k, None] * gp[b])
    return gp, gv


def test_autograd_gradients_equal_the_closed_forms():
    v, f = jittered_icosphere(1, B=3)
    p = box_points(200, B=3)
    g = torch.as_tensor(np.random.RandomState(7).normal(size=3))
    a, b = p.clone().requires_grad_(True), v.clone().requires_grad_(True)
    nr.point_mesh_distance_torch(a, b, f).backward(g)
    gp, gv = closed_form_gradients(p, v, f, g)
    assert float((a.grad - gp).abs().max()) <= 1e-14 and float((b.grad - gv).abs().max()) <= 1e-14
    assert float(gp.abs().max()) > 0 and float(gv.abs().max()) > 0
    # the envelope theorem: a finite difference of the loss itself along a random direction
    dp, dv = torch.as_tensor(np.random.RandomState(8).normal(size=p.shape)), torch.as_tensor(np.random.RandomState(9).normal(size=v.shape))
    h = 1e-6
    fd = ((nr.point_mesh_distance_torch(p + h * dp, v + h * dv, f) - nr.point_mesh_distance_torch(p - h * dp, v - h * dv, f)) * g).sum() / (2 * h)
    an = (gp * dp).sum() + (gv * dv).sum()
    assert abs(float(fd - an)) <= 1e-5 * abs(float(an)) + 1e-8, (float(fd), float(an))


def test_shapes_and_flags():
    v, f = jittered_icosphere(1, B=3)
    p = box_points(50, B=3)
    loss = nr.point_mesh_distance(p, v, f)
    assert loss.shape == (3,) and loss.dtype == torch.float64
    assert torch.equal(loss, nr.point_mesh_distance_torch(p, v, f))  # CPU float64: the composition
    assert torch.equal(nr.point_mesh_distance(p, v, f, average=True), loss.mean())
    one = nr.point_mesh_distance(p[1], v[1], f)
    assert one.ndim == 0 and torch.allclose(one, loss[1], rtol=1e-14, atol=0)
    # shared points against a batch of meshes
    shared = nr.point_mesh_distance(p[0], v, f)
    assert shared.shape == (3,) and torch.equal(shared, nr.point_mesh_distance(p[:1].expand(3, -1, -1), v, f))
    s = p[0].clone().requires_grad_(True)
    nr.point_mesh_distance(s, v, f).sum().backward()
    e = p[:1].expand(3, -1, -1).clone().requires_grad_(True)
    nr.point_mesh_distance(e, v, f).sum().backward()
    assert s.grad.shape == (50, 3) and torch.allclose(s.grad, e.grad.sum(0), rtol=1e-13, atol=1e-16)
    # closest_points_on_mesh: shapes, dtypes, detached; single inputs drop the item axis
    d2, face, w = nr.closest_points_on_mesh(p.clone().requires_grad_(True), v.clone().requires_grad_(True), f)
    assert d2.shape == (3, 50) and face.shape == (3, 50) and face.dtype == torch.int32 and w.shape == (3, 50, 3)
    assert not (d2.requires_grad or w.requires_grad)
    assert torch.allclose(d2.mean(1), loss, rtol=1e-14, atol=0)
    d1, f1, w1 = nr.closest_points_on_mesh(p[2], v[2], f)
    assert d1.shape == (50,) and torch.equal(f1, face[2]) and w1.shape == (50, 3)
    # float32 on the CPU takes the composition too, in float32
    l32 = nr.point_mesh_distance(p.float(), v.float(), f)
    assert l32.dtype == torch.float32 and torch.allclose(l32.double(), loss, rtol=1e-5, atol=0)
    # numpy faces, int32 faces
    assert torch.equal(nr.point_mesh_distance(p, v, f.numpy().astype(np.int32)), loss)


def test_errors():
    v, f = jittered_icosphere(0, B=2)
    p = box_points(10, B=2)
    with pytest.raises(ValueError):
        nr.point_mesh_distance(p[:, :0], v, f)  # N = 0
    with pytest.raises(ValueError):
        nr.point_mesh_distance(p, v, f[:0])  # F = 0
    with pytest.raises(ValueError):
        nr.point_mesh_distance(box_points(10, B=3), v, f)  # batch mismatch
    with pytest.raises(ValueError):
        nr.point_mesh_distance(p, v[0], f)  # batched points against a single mesh
    with pytest.raises(ValueError):
        nr.closest_points_on_mesh(p[..., :2], v, f)
    bad = f.clone()
    bad[3, 1] = v.shape[1]
    with pytest.raises(IndexError):
        nr.point_mesh_distance(p, v, bad)
    bad[3, 1] = -1
    with pytest.raises(IndexError):
        nr.closest_points_on_mesh(p, v, bad)


def test_module():
    v, f = jittered_icosphere(1, B=2)
    p = box_points(30)
    mod = nr.PointMeshLoss(p)
    assert "points" in dict(mod.named_buffers()) and not list(mod.parameters())
    assert torch.equal(mod(v, f), nr.point_mesh_distance(p, v, f))
    other = box_points(30, seed=9, B=2)
    assert torch.equal(mod(v, f, other), nr.point_mesh_distance(other, v, f))
    assert torch.equal(nr.PointMeshLoss(p, average=True)(v, f), nr.point_mesh_distance(p, v, f, average=True))
    assert torch.equal(nr.PointMeshLoss()(v, f, points=p), nr.point_mesh_distance(p, v, f))
    with pytest.raises(ValueError):
        nr.PointMeshLoss()(v, f)
    assert mod.double().points.dtype == torch.float64


def test_composition_is_chunked(monkeypatch):
    """The nearest-face search in chunks of a few points gives what one chunk gives."""
    v, f = jittered_icosphere(1, B=2)
    p = box_points(37, B=2)
    whole = nr.closest_points_on_mesh_torch(p, v, f)
    monkeypatch.setattr(point_loss, "_CHUNK_PAIRS", 5 * 2 * f.shape[0])
    parts = nr.closest_points_on_mesh_torch(p, v, f)
    assert all(torch.equal(a, b) for a, b in zip(whole, parts))


def test_abi_rejects_bad_arguments():
    """The entry points check sizes, the 32-bit index products, pointers and the workspace before any launch (no
    GPU needed: every call here returns from the argument checks)."""
    from neural_renderer_v2_pytorch_amd import _lib
    L = _lib.lib()
    ARGS = 1  # NR_ERR_ARGS
    T, Q = _lib.NR_POINT_MESH_TILE, _lib.NR_POINT_MESH_QBLOCK
    size = L.nr_point_mesh_workspace_bytes
    assert size(0, 5, 5) == 0 and size(5, 0, 5) == 0 and size(5, 5, 0) == 0
    assert size(2, 10, 7) >= 2 * 7 * 96 + 3 * 2 * 10 * 4
    assert size(1, 5, 3 * T + 2) >= size(1, 5, T) + (2 * T + 2) * 96 + 2 * 3 * 5 * 4  # three ranges of partials
    full = _lib.NR_POINT_MESH_SPLIT_BLOCKS * Q  # enough query blocks: no partials
    assert size(1, full, 3 * T + 2) < (3 * T + 2) * 96 + 3 * full * 4 + 4 * 4096 <= size(1, full - Q, 3 * T + 2)
    p = 4096  # a non-null address that is never dereferenced

    def forward(points=p, stride=30, vertices=p, faces=p, B=2, N=10, V=9, F=7, dist2=p, face=p, weights=p, loss=p, ws=p,
                ws_bytes=1 << 20):
        return L.nr_point_mesh_forward(points, stride, vertices, faces, B, N, V, F, dist2, face, weights, loss, ws, ws_bytes, None)

    def backward(points=p, stride=30, vertices=p, faces=p, face=p, weights=p, grad_loss=p, B=2, N=10, V=9, F=7, gp=p, gv=p):
        return L.nr_point_mesh_backward(points, stride, vertices, faces, face, weights, grad_loss, B, N, V, F, gp, gv, None)

    for call in (forward, backward):
        assert call(B=-1) == ARGS and call(N=0) == ARGS and call(F=0) == ARGS and call(V=0) == ARGS
        assert call(B=65536) == ARGS and b"65535" in L.nr_last_error()
        assert call(B=4, N=2 ** 29) == ARGS and call(B=4, F=2 ** 29) == ARGS and call(B=4, V=2 ** 28) == ARGS
        assert call(stride=-30) == ARGS
        assert call(points=None) == ARGS and call(vertices=None) == ARGS and call(faces=None) == ARGS
    assert forward(dist2=None, face=None, weights=None, loss=None) == ARGS
    assert forward(ws=None) == ARGS and forward(ws_bytes=size(2, 10, 7) - 1) == ARGS
    assert b"workspace" in L.nr_last_error()
    assert backward(face=None) == ARGS and backward(weights=None) == ARGS and backward(grad_loss=None) == ARGS
    # nothing to do: no pointer is needed
    assert forward(B=0, points=None, vertices=None, faces=None, ws=None) == 0
    assert backward(B=0, points=None, vertices=None, faces=None) == 0
    assert backward(gp=None, gv=None, points=None) == 0

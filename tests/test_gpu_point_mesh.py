"""The fused point_mesh_distance / closest_points_on_mesh on the GPU (float32) against the torch composition
in float64 on the CPU, which receives the same float32 values widened.

Test meshes are triangle soups: synthetic.icosphere(level, radius=0.5) with the vertices jittered by
+-0.02 (fixed seed), the faces sliced or repeated to the wanted F.  Queries are uniform in [-1, 1]^3.

On such inputs about two thirds of the queries have their closest point on an edge or a vertex that
several faces share (only 30-34 % have a relative gap above 1e-5 between the best and the second-best
face), so the returned index is NOT compared with the reference's in general.  Asserted at every point:
  dist2    |dist2 - ref| <= 1e-6 ref + 1e-6 sqrt(ref): the closest point carries a few float32 roundings of
           coordinates of size <= 1 and d^2 inherits 2 d times that (the float32 composition measured
           1.4e-7 sqrt(ref) against float64 on the CPU);
  face     the float64 distance from p to the returned face is <= ref + that tolerance;
  weights  finite, in [0, 1], summing to 1 within 1e-6; within 1e-5 of the float64 weights of the closest
           point on that same face; dist2 equals |p - sum_k w_k v_k|^2 within the dist2 tolerance;
  loss     test_gpu_mesh_loss's output tolerance (rtol = atol = 1e-5);
  grads    against the float64 autograd of point_mesh_distance_torch(..., face=the kernel's own faces) under a
           random upstream [B]: 1e-4 of the reference's largest magnitude plus 1e-4 relative.
The index must EQUAL the reference's only where a test first asserts a relative gap above 1e-5."""
import functools

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import _lib, point_loss, synthetic

pytestmark = pytest.mark.gpu

OUT_TOL = 1e-5
GRAD_TOL = 1e-4
WEIGHT_TOL = 1e-5
GAP = 1e-5
T, Q = _lib.NR_POINT_MESH_TILE, _lib.NR_POINT_MESH_QBLOCK
KERNEL = "k_point_face_nn"

CASES = {  # name: (B, N, F)
    "wave": (3, 65, 63),                      # either side of a wave; not split
    "partial": (3, 257, 300),                 # partial block; a second, partial tile without a split
    # several query blocks; four blocks do not fill the chip, so the faces split into ranges of T + 1 and T: the
    # first range ends with a tile of one face ("partial" is the unsplit walk over a second tile)
    "blocks_tiles": (2, Q + 1, 2 * T + 1),
    "one_point": (2, 1, 40),
    "one_face": (2, 40, 1),
    "three_ranges": (1, 5, 3 * T + 2),        # 3 face ranges, the first 2 one face longer
    "five_ranges": (2, 3, 5 * T + 3),         # 5 ranges, the first 3 one face longer
}
RANGES = {"three_ranges": 3, "five_ranges": 5}
SPLIT = set(RANGES) | {"blocks_tiles"}


def soup(B, F, seed=31):
    """float32 CPU vertices [B, V, 3] and int64 faces [F, 3]: the smallest icosphere level (from 2) with at
    least F faces, sliced; F beyond level 4's 5120 repeats the faces."""
    level = 2 if F <= 320 else 3 if F <= 1280 else 4
    v, f = synthetic.icosphere(level, radius=0.5)
    vb = v[None] + np.random.RandomState(seed).uniform(-0.02, 0.02, (B,) + v.shape)
    return torch.as_tensor(vb.astype(np.float32)), torch.as_tensor(np.resize(f, (F, 3)).astype(np.int64))


def queries(B, N, seed=103):
    return torch.as_tensor(np.random.RandomState(seed).uniform(-1, 1, (B, N, 3)).astype(np.float32))


def tolerance(ref):
    return 1e-6 * ref + 1e-6 * ref.sqrt()


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


def reference(p, v, f):
    """float64: (dist2 [B, N], face [B, N]) of the composition."""
    d2, face, _ = point_loss._closest_torch(p.double(), v.double(), f, None)
    return d2, face


def check_forward(p, v, f, got, ref_d2, what):
    """Everything the module docstring asserts about (dist2, face, weights) on the CPU; returns the int64 faces."""
    d2, face, w = (t.cpu() for t in got)
    B, N, F = p.shape[0], p.shape[1], f.shape[0]
    assert d2.shape == (B, N) and d2.dtype == torch.float32 and face.shape == (B, N) and face.dtype == torch.int32
    assert w.shape == (B, N, 3) and w.dtype == torch.float32
    assert int(face.min()) >= 0 and int(face.max()) < F
    face = face.long()
    tol = tolerance(ref_d2)
    err = (d2.double() - ref_d2).abs()
    print("%s: dist2 error at most %.3g of the tolerance" % (what, float((err / tol).max())))
    assert bool((err <= tol).all()), "%s: %d dist2 off" % (what, int((err > tol).sum()))
    own_d2, _, own_w = point_loss._closest_torch(p.double(), v.double(), f, face)
    over = own_d2 - ref_d2
    print("%s: returned face beyond the nearest by at most %.3g of the tolerance" % (what, float((over / tol).max())))
    assert bool((over <= tol).all()), "%s: %d faces are not nearest" % (what, int((over > tol).sum()))
    wd = w.double()
    assert bool(torch.isfinite(w).all()) and float(w.min()) >= 0. and float(w.max()) <= 1.
    assert float((wd.sum(-1) - 1).abs().max()) <= 1e-6
    werr = float((wd - own_w).abs().max())
    print("%s: weights within %.3g of float64" % (what, werr))
    assert werr <= WEIGHT_TOL
    corners = v.double().gather(1, f[face].reshape(B, N * 3, 1).expand(-1, -1, 3)).reshape(B, N, 3, 3)
    c = (wd[..., None] * corners).sum(2)
    assert bool(((((p.double() - c) ** 2).sum(-1) - d2.double()).abs() <= tol).all())
    return face


@functools.lru_cache(maxsize=None)
def case(name):
    """float32 CPU points, vertices, int64 faces, the upstream gradient [B], the float64 reference dist2."""
    B, N, F = CASES[name]
    v, f = soup(B, F)
    p = queries(B, N)
    g = torch.as_tensor(np.random.RandomState(7).normal(size=B))
    return p, v, f, g, reference(p, v, f)[0]


def fused(p, v, f, g, dev, p_grad=True, v_grad=True):
    a, b = p.to(dev).requires_grad_(p_grad), v.to(dev).requires_grad_(v_grad)
    loss = nr.point_mesh_distance(a, b, f.to(dev).int())
    loss.backward(g.to(device=dev, dtype=torch.float32))
    return loss.detach(), a.grad, b.grad


def reference_grads(p, v, f, g, face):
    a, b = p.double().requires_grad_(True), v.double().requires_grad_(True)
    nr.point_mesh_distance_torch(a, b, f, face=face).backward(g)
    return a.grad, b.grad


@pytest.mark.parametrize("name", list(CASES))
def test_matches_float64(dev, name):
    p, v, f, g, ref_d2 = case(name)
    fd = f.to(dev).int()
    got = nr.closest_points_on_mesh(p.to(dev), v.to(dev), fd)
    threads, flags = _lib.last_launch(KERNEL)
    assert threads == 256 and flags == (_lib.NR_LAUNCH_SPLIT_FACES if name in SPLIT else 0), (threads, flags)
    face = check_forward(p, v, f, got, ref_d2, name)
    loss, gp, gv = fused(p, v, f, g, dev)
    assert loss.shape == (p.shape[0],) and loss.dtype == torch.float32
    close_out(loss, ref_d2.mean(1), name + " loss")
    assert torch.equal(loss, nr.point_mesh_distance(p.to(dev), v.to(dev), fd))  # the same faces again
    want_gp, want_gv = reference_grads(p, v, f, g, face)
    close_grads(gp, want_gp, name + " grad points")
    close_grads(gv, want_gv, name + " grad vertices")
    if name == "blocks_tiles":
        assert 0 < T < f.shape[0] - 1 and p.shape[1] > Q


def relative_gaps(p, v, f):
    """float64 [B, N]: (second - best) / second over the faces' squared distances, and the best face."""
    tri, deg = point_loss._mesh_corners(v.double(), f)
    d = point_loss._point_triangle(p.double()[:, :, None], tri[:, None, :, 0], tri[:, None, :, 1], tri[:, None, :, 2], deg[:, None], False)
    two, idx = d.topk(2, dim=2, largest=False)
    return (two[..., 1] - two[..., 0]) / two[..., 1], idx[..., 0]


@pytest.mark.parametrize("name", list(RANGES))
def test_every_face_range_holds_a_winner(dev, name):
    """Queries 0.01 above the centroids of two faces of every range (n equal shares of F, the remainder one each
    to the first ranges): each partial wins for two queries.  The picks are a range's first and last face, or,
    where the jitter has folded a neighbour over one of them so that the float64 reference itself finds another
    face nearer, the nearest face to that end of the range for which it does not (at most 8 faces in; the first
    and the last face of the whole mesh must hold as they are).  The reference's choice and its gap are asserted
    first; the index must equal."""
    _, v, f, _, _ = case(name)
    B, F, n = v.shape[0], f.shape[0], RANGES[name]
    share, rem = divmod(F, n)
    los = [s * share + min(s, rem) for s in range(n + 1)]
    assert los[-1] == F and 0 < rem < n

    def above(faces):
        tri = v.double()[:, f[faces]]  # [B, P, 3, 3]
        normal = torch.linalg.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], dim=-1)
        return (tri.mean(2) + 0.01 * normal / normal.norm(dim=-1, keepdim=True)).float()

    ends = torch.as_tensor([[los[s] + k for k in range(8)] + [los[s + 1] - 1 - k for k in range(8)] for s in range(n)]).reshape(-1)
    gaps, best = relative_gaps(above(ends), v, f)
    holds = ((best == ends[None]) & (gaps > GAP)).all(0).reshape(n, 2, 8)
    assert bool(holds.any(2).all()) and bool(holds[0, 0, 0]) and bool(holds[n - 1, 1, 0])
    picks = ends.reshape(n, 2, 8).gather(2, holds.int().argmax(2, keepdim=True)).reshape(-1)
    print("%s: picks %s of the ranges starting at %s" % (name, picks.tolist(), los))
    q = above(picks)
    gaps, best = relative_gaps(q, v, f)
    print("%s: smallest relative gap %.3g" % (name, float(gaps.min())))
    assert torch.equal(best, picks[None].expand(B, -1)) and float(gaps.min()) > GAP
    got = nr.closest_points_on_mesh(q.to(dev), v.to(dev), f.to(dev).int())
    assert _lib.last_launch(KERNEL) == (256, _lib.NR_LAUNCH_SPLIT_FACES)
    assert torch.equal(got[1].cpu().long(), best), (got[1].cpu().tolist(), picks.tolist())
    check_forward(q, v, f, got, reference(q, v, f)[0], name + " picks")


def test_ties_pick_the_lowest_index_bitwise(dev):
    """The faces given twice (one range; two ranges) and three times (three ranges of one copy each, so every
    tie spans all partials of the combine): every index stays in the first copy, dist2 and weights are bit for
    bit those of the single copy."""
    for F, copies, split in ((100, 2, False), (T + 1, 2, True), (T + 1, 3, True)):
        v, f = soup(2, F)
        p = queries(2, 70).to(dev)
        vd = v.to(dev)
        d2, face, w = nr.closest_points_on_mesh(p, vd, f.to(dev).int())
        assert _lib.last_launch(KERNEL)[1] == 0
        d2c, facec, wc = nr.closest_points_on_mesh(p, vd, torch.cat([f] * copies).to(dev).int())
        assert bool(_lib.last_launch(KERNEL)[1] & _lib.NR_LAUNCH_SPLIT_FACES) == split
        assert int(facec.max()) < F and torch.equal(facec, face)
        assert torch.equal(d2c, d2) and torch.equal(wc, w)


def test_split_independence_bitwise(dev):
    """Three points alone (three face ranges), inside a 2,000-point set (other blocks, still split: two query
    blocks do not fill the chip) and inside a set of as many query blocks as the split aims for (4.2 M points,
    not split): bit for bit the same."""
    F = 3 * T + 2
    v, f = soup(1, F)
    vd, fd = v.to(dev), f.to(dev).int()
    big = queries(1, (_lib.NR_POINT_MESH_SPLIT_BLOCKS - 1) * Q + 1).to(dev)
    alone = nr.closest_points_on_mesh(big[:, :3].contiguous(), vd, fd)
    assert _lib.last_launch(KERNEL) == (256, _lib.NR_LAUNCH_SPLIT_FACES)
    some = nr.closest_points_on_mesh(big[:, :2000].contiguous(), vd, fd)
    assert _lib.last_launch(KERNEL) == (256, _lib.NR_LAUNCH_SPLIT_FACES)
    whole = nr.closest_points_on_mesh(big, vd, fd)
    assert _lib.last_launch(KERNEL) == (256, 0)
    for other in (some, whole):
        assert all(torch.equal(a, b[:, :3]) for a, b in zip(alone, other))
    assert all(torch.equal(a[:, :2000], b) for a, b in zip(whole, some))


# small-integer corners far from the soup: one segment per degenerate face, four units apart, and a point
DEGENERATE_V = [[4., 0, 0], [8, 0, 0],                # repeated index: [0, 1, 1]
                [4, 4, 0], [4, 4, 0], [8, 4, 0],      # coincident corners: [2, 3, 4]
                [4, 8, 0], [6, 8, 0], [8, 8, 0],      # collinear, the middle corner first: [6, 5, 7]
                [4, 16, 0], [4, 16, 0]]               # a point, eight units on: [8, 9, 9]
DEGENERATE_F = [[0, 1, 1], [2, 3, 4], [6, 5, 7], [8, 9, 9]]
# per face: the segment's ends as positions in the face (ab, ac, bc in this order, the first among equally long)
DEGENERATE_ENDS = [(0, 1), (0, 2), (1, 2), (0,)]
DEGENERATE_OFFSETS = [[1., 1, 0], [3, -1, 1], [-1, 1, 0], [5, 0, 1], [2, 0, 0]]


def test_degenerate_faces(dev):
    B = 2
    v, f = soup(B, 320)
    V0, F0 = v.shape[1], f.shape[0]
    dv = torch.tensor(DEGENERATE_V)
    v = torch.cat([v, dv[None].expand(B, -1, -1)], 1)
    f = torch.cat([f[:100], torch.tensor(DEGENERATE_F) + V0, f[100:]])
    starts = torch.tensor([[4., 0, 0], [4, 4, 0], [4, 8, 0], [4, 16, 0]])
    near = (starts[:, None] + torch.tensor(DEGENERATE_OFFSETS)[None]).reshape(-1, 3)  # 20 queries, five per face
    p = torch.cat([queries(B, 40), near[None].expand(B, -1, -1)], 1).contiguous()
    got = nr.closest_points_on_mesh(p.to(dev), v.to(dev), f.to(dev).int())
    ref_d2 = reference(p, v, f)[0]
    face = check_forward(p, v, f, got, ref_d2, "degenerate")
    d2, _, w = (t.cpu() for t in got)
    assert bool((face[:, :40] < 100).logical_or(face[:, :40] >= 104).all())
    for k, ends in enumerate(DEGENERATE_ENDS):
        rows = slice(40 + 5 * k, 45 + 5 * k)
        assert bool((face[:, rows] == 100 + k).all()), (k, face[:, rows])
        corners = dv[torch.tensor(DEGENERATE_F[k])]
        q = p[0, rows]
        want_w = torch.zeros(5, 3)
        if len(ends) == 1:
            want_w[:, 0] = 1
            c = corners[0].expand(5, -1)
        else:
            a, b = corners[ends[0]], corners[ends[1]]
            t = (((q - a) * (b - a)).sum(-1) / ((b - a) ** 2).sum()).clamp(0, 1)
            want_w[:, ends[0]], want_w[:, ends[1]] = 1 - t, t
            c = a + t[:, None] * (b - a)
        want_d2 = ((q - c) ** 2).sum(-1)
        for b in range(B):  # small integers and quarters: exact
            assert torch.equal(w[b, rows], want_w), (k, w[b, rows], want_w)
            assert torch.equal(d2[b, rows], want_d2), (k, d2[b, rows], want_d2)
    g = torch.as_tensor(np.random.RandomState(7).normal(size=B))
    loss, gp, gv = fused(p, v, f, g, dev)
    want_gp, want_gv = reference_grads(p, v, f, g, face)
    close_out(loss, ref_d2.mean(1), "degenerate loss")
    close_grads(gp, want_gp, "degenerate grad points")
    close_grads(gv, want_gv, "degenerate grad vertices")
    assert bool(torch.isfinite(gp).all()) and bool(torch.isfinite(gv).all())


def test_interface(dev):
    p, v, f, g, ref_d2 = case("partial")
    B, N = p.shape[0], p.shape[1]
    fd = f.to(dev).int()
    gd = g.to(device=dev, dtype=torch.float32)
    batched = nr.point_mesh_distance(p.to(dev), v.to(dev), fd)
    # shared [N, 3] points against B meshes: read in place, bit for bit the expanded copy
    shared = p[0].to(dev)
    expanded = shared[None].expand(B, -1, -1).contiguous()
    a = v.to(dev).requires_grad_(True)
    loss = nr.point_mesh_distance(shared, a, fd)
    loss.backward(gd)
    b = v.to(dev).requires_grad_(True)
    loss_e = nr.point_mesh_distance(expanded, b, fd)
    loss_e.backward(gd)
    assert loss.shape == (B,) and torch.equal(loss, loss_e)
    close_grads(a.grad, b.grad, "shared points: grad vertices")
    assert all(torch.equal(x, y) for x, y in zip(nr.closest_points_on_mesh(shared, v.to(dev), fd),
                                                  nr.closest_points_on_mesh(expanded, v.to(dev), fd)))
    # shared points that take a gradient receive the item sum
    s = shared.clone().requires_grad_(True)
    nr.point_mesh_distance(s, v.to(dev), fd).backward(gd)
    e = expanded.clone().requires_grad_(True)
    nr.point_mesh_distance(e, v.to(dev), fd).backward(gd)
    assert s.grad.shape == (N, 3)
    close_grads(s.grad, e.grad.sum(0), "shared points: summed gradient")
    face = nr.closest_points_on_mesh(shared, v.to(dev), fd)[1].cpu().long()
    s64 = p[0].double().requires_grad_(True)
    nr.point_mesh_distance_torch(s64, v.double(), f, face=face).backward(g)
    close_grads(s.grad, s64.grad, "shared points: gradient against float64")
    # single [N, 3] / [V, 3]; average; the module
    one = nr.point_mesh_distance(p[1].to(dev), v[1].to(dev), fd)
    assert one.ndim == 0 and torch.equal(one, batched[1])
    d1 = nr.closest_points_on_mesh(p[1].to(dev), v[1].to(dev), fd)
    assert d1[0].shape == (N,) and d1[1].shape == (N,) and d1[2].shape == (N, 3)
    avg = nr.point_mesh_distance(p.to(dev), v.to(dev), fd, average=True)
    assert avg.ndim == 0
    close_out(avg, ref_d2.mean(), "average")
    mod = nr.PointMeshLoss(p[0]).to(dev)
    assert torch.equal(mod(v.to(dev), fd), loss.detach())
    assert torch.equal(mod(v.to(dev), fd, p.to(dev)), batched)
    # CPU int64 faces are converted
    assert torch.equal(nr.point_mesh_distance(p.to(dev), v.to(dev), f), batched)
    # non-contiguous views of points and vertices
    wide_p, wide_v = torch.zeros((B, N, 5)), torch.zeros((B, v.shape[1], 4))
    wide_p[..., 1:4], wide_v[..., :3] = p, v
    wp, wv = wide_p.to(dev).requires_grad_(True), wide_v.to(dev).requires_grad_(True)
    sp, sv = wp[..., 1:4], wv[..., :3]
    assert not sp.is_contiguous() and not sv.is_contiguous()
    sliced = nr.point_mesh_distance(sp, sv, fd)
    sliced.backward(gd)
    whole = fused(p, v, f, g, dev)
    assert torch.equal(sliced, whole[0]) and torch.equal(wp.grad[..., 1:4], whole[1])
    close_grads(wv.grad[..., :3], whole[2], "slice grad vertices")
    assert float(wp.grad[..., 0].abs().max()) == 0. and float(wv.grad[..., 3].abs().max()) == 0.
    # requires_grad on one input only: the other gradient is None, the one taken is unchanged
    only_p = fused(p, v, f, g, dev, v_grad=False)
    assert only_p[2] is None and torch.equal(only_p[1], whole[1])
    only_v = fused(p, v, f, g, dev, p_grad=False)
    assert only_v[1] is None
    close_grads(only_v[2], whole[2], "vertices only")
    plain = nr.point_mesh_distance(p.to(dev), v.to(dev), fd)
    assert not plain.requires_grad and plain.grad_fn is None and torch.equal(plain, whole[0])
    # closest_points_on_mesh is detached
    out = nr.closest_points_on_mesh(p.to(dev).requires_grad_(True), v.to(dev).requires_grad_(True), fd)
    assert not any(t.requires_grad for t in out)
    # error cases reach the fused path's checks too
    with pytest.raises(ValueError):
        nr.point_mesh_distance(p[:, :0].to(dev), v.to(dev), fd)
    with pytest.raises(ValueError):
        nr.point_mesh_distance(p.to(dev), v.to(dev), fd[:0])
    with pytest.raises(ValueError):
        nr.point_mesh_distance(p[:2].to(dev), v.to(dev), fd)
    bad = fd.clone()
    bad[5, 2] = v.shape[1]
    with pytest.raises(IndexError):
        nr.point_mesh_distance(p.to(dev), v.to(dev), bad)


@pytest.mark.parametrize("name", ["partial", "three_ranges"])
def test_runs_are_reproducible(dev, name):
    p, v, f, g, _ = case(name)
    fd = f.to(dev).int()
    first = fused(p, v, f, g, dev)
    first_q = nr.closest_points_on_mesh(p.to(dev), v.to(dev), fd)
    for _ in range(2):
        again = fused(p, v, f, g, dev)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
        close_grads(again[2], first[2], "grad vertices again")
        assert all(torch.equal(a, b) for a, b in zip(first_q, nr.closest_points_on_mesh(p.to(dev), v.to(dev), fd)))


@pytest.mark.parametrize("name", ["partial", "three_ranges"])
def test_non_finite_queries(dev, name):
    """A few all-NaN points and one with a single NaN coordinate among clean ones, unsplit and split: every
    face stays inside [0, F) (a NaN distance compares false and keeps the first face of its range: 0 after the
    combine too), the clean points' results do not move by a bit, and the backward runs."""
    p, v, f, g, _ = case(name)
    B, N, F = p.shape[0], p.shape[1], f.shape[0]
    fd = f.to(dev).int()
    clean = [t.cpu() for t in nr.closest_points_on_mesh(p.to(dev), v.to(dev), fd)]
    assert bool(_lib.last_launch(KERNEL)[1] & _lib.NR_LAUNCH_SPLIT_FACES) == (name in RANGES)
    q = p.clone()
    q[:, 0] = float("nan")
    q[:, N - 1] = float("nan")
    q[:, 2, 1] = float("nan")
    hit = torch.isnan(q).any(-1)
    assert int(hit.sum()) == 3 * B
    d2, face, w = (t.cpu() for t in nr.closest_points_on_mesh(q.to(dev), v.to(dev), fd))
    assert int(face.min()) >= 0 and int(face.max()) < F and bool((face[hit] == 0).all())
    assert torch.equal(face[~hit], clean[1][~hit]) and torch.equal(d2[~hit], clean[0][~hit]) and torch.equal(w[~hit], clean[2][~hit])
    loss, gp, gv = fused(q, v, f, g, dev)
    torch.cuda.synchronize()
    assert gp.shape == q.shape and gv.shape == v.shape
    assert torch.equal(gp[~hit], fused(p, v, f, g, dev)[1][~hit])


def test_null_outputs_leave_the_others_unchanged(dev):
    """nr_point_mesh_forward itself (the wrappers always ask for dist2, face and weights), unsplit with a partial last
    block and split: the loss alone, then each of dist2, face and weights alone, is bit for bit what the call with
    every output writes.  Each array starts at -1, which no result holds."""
    L = _lib.lib()
    for name in ("partial", "three_ranges"):
        p, v, f, _, _ = case(name)
        B, N, V, F = p.shape[0], p.shape[1], v.shape[1], f.shape[0]
        pd, vd, fd = p.to(dev), v.to(dev), f.to(dev).int()
        ws = torch.empty(L.nr_point_mesh_workspace_bytes(B, N, F), dtype=torch.uint8, device=dev)

        def run(*want):
            out = {"dist2": torch.full((B, N), -1., device=dev), "face": torch.full((B, N), -1, dtype=torch.int32, device=dev),
                   "weights": torch.full((B, N, 3), -1., device=dev), "loss": torch.full((B,), -1., device=dev)}
            ptrs = [_lib.ptr(out[k] if k in want else None) for k in ("dist2", "face", "weights", "loss")]
            _lib.check(L.nr_point_mesh_forward(_lib.ptr(pd), N * 3, _lib.ptr(vd), _lib.ptr(fd), B, N, V, F, *ptrs, _lib.ptr(ws),
                                               ws.numel(), _lib.stream_of(vd)), "nr_point_mesh_forward")
            assert _lib.last_launch(KERNEL) == (256, _lib.NR_LAUNCH_SPLIT_FACES if name in SPLIT else 0)
            return out

        full = run("dist2", "face", "weights", "loss")
        assert float(full["dist2"].min()) >= 0 and int(full["face"].min()) >= 0 and float(full["weights"].min()) >= 0
        assert float(full["loss"].min()) > 0
        for only in ("loss", "dist2", "face", "weights"):
            assert torch.equal(run(only)[only], full[only]), (name, only)

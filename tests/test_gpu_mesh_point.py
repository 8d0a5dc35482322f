"""The fused mesh_point_distance / closest_points_to_faces on the GPU (float32) against the torch composition in
float64 on the CPU, which receives the same float32 values widened.

Inputs are test_gpu_point_mesh.py's: soup(B, F) triangle soups (a jittered icosphere of radius 0.5, the faces
sliced or repeated) and queries(B, N) uniform in [-1, 1]^3.  Its tolerances hold here for its reasons:
  dist2    |dist2 - ref| <= 1e-6 ref + 1e-6 sqrt(ref): the closest point carries a few float32 roundings of
           coordinates of size <= 1 and d^2 inherits 2 d times that;
  point    the float64 distance from the returned point to the face is <= ref + that tolerance;
  weights  finite, in [0, 1], summing to 1 within 1e-6; within 1e-5 of the float64 weights of that same pair;
  loss     rtol = atol = 1e-5;
  grads    against the float64 autograd of mesh_point_distance_torch(..., point=the kernel's own) under a random
           upstream [B]: 1e-4 of the reference's largest magnitude plus 1e-4 relative.
Unlike the sibling's direction, random points are almost never equidistant from a face: every test first asserts
in float64 that at least 99 % of its faces have a relative gap above 1e-5 between the best and the second-best
point, and the returned index must EQUAL the reference's at every such face; the others fall under the "nearest
within tolerance" check alone."""
import functools

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import _lib, point_loss
import test_gpu_point_mesh as sibling
from test_gpu_point_mesh import GAP, WEIGHT_TOL, close_grads, close_out, queries, soup, tolerance

pytestmark = pytest.mark.gpu

TP, FQ = _lib.NR_FACE_POINT_TILE, _lib.NR_FACE_POINT_FBLOCK
KERNEL = "k_face_point_nn"
SPLIT_FLAG = _lib.NR_LAUNCH_SPLIT_POINTS

CASES = {  # name: (B, N, F)
    "wave": (3, 63, 65),                      # either side of a wave; not split
    "partial": (3, TP + 44, 257),             # a partial face block; a second, partial tile without a split
    # two face blocks; the points split into ranges of TP + 1 and TP: the first ends in a tile of one point
    "blocks_tiles": (2, 2 * TP + 1, FQ + 1),
    "one_point": (2, 1, 40),
    "one_face": (2, 40, 1),
    "three_ranges": (1, 3 * TP + 2, 5),       # 3 point ranges, the first 2 one point longer
    "five_ranges": (2, 5 * TP + 3, 3),        # 5 ranges, the first 3 one point longer
}
RANGES = {"three_ranges": 3, "five_ranges": 5}
SPLIT = set(RANGES) | {"blocks_tiles"}


def reference(p, v, f):
    """float64: (dist2 [B, F], point [B, F]) of the composition."""
    d2, point, _ = point_loss._closest_to_faces_torch(p.double(), v.double(), f, None)
    return d2, point


def relative_gaps(p, v, f):
    """float64 [B, F]: (second - best) / second over the points' squared distances to each face (1 with a single
    point), and the best point."""
    tri, deg = point_loss._mesh_corners(v.double(), f)
    d = point_loss._point_triangle(p.double()[:, None], tri[:, :, None, 0], tri[:, :, None, 1], tri[:, :, None, 2], deg[:, :, None], False)
    if d.shape[2] == 1:
        return torch.ones_like(d[..., 0]), torch.zeros_like(d[..., 0], dtype=torch.long)
    two, idx = d.topk(2, dim=2, largest=False)
    return (two[..., 1] - two[..., 0]) / two[..., 1], idx[..., 0]


def check_forward(p, v, f, got, what):
    """Everything the module docstring asserts about (dist2, point, weights) on the CPU; returns the int64 points
    and the float64 reference dist2."""
    d2, point, w = (t.cpu() for t in got)
    B, N, F = p.shape[0], p.shape[1], f.shape[0]
    assert d2.shape == (B, F) and d2.dtype == torch.float32 and point.shape == (B, F) and point.dtype == torch.int32
    assert w.shape == (B, F, 3) and w.dtype == torch.float32
    assert int(point.min()) >= 0 and int(point.max()) < N
    point = point.long()
    ref_d2, ref_point = reference(p, v, f)
    tol = tolerance(ref_d2)
    err = (d2.double() - ref_d2).abs()
    print("%s: dist2 error at most %.3g of the tolerance" % (what, float((err / tol).max())))
    assert bool((err <= tol).all()), "%s: %d dist2 off" % (what, int((err > tol).sum()))
    own_d2, _, own_w = point_loss._closest_to_faces_torch(p.double(), v.double(), f, point)
    over = own_d2 - ref_d2
    print("%s: returned point beyond the nearest by at most %.3g of the tolerance" % (what, float((over / tol).max())))
    assert bool((over <= tol).all()), "%s: %d points are not nearest" % (what, int((over > tol).sum()))
    wd = w.double()
    assert bool(torch.isfinite(w).all()) and float(w.min()) >= 0. and float(w.max()) <= 1.
    assert float((wd.sum(-1) - 1).abs().max()) <= 1e-6
    werr = float((wd - own_w).abs().max())
    print("%s: weights within %.3g of float64" % (what, werr))
    assert werr <= WEIGHT_TOL
    c = (wd[..., None] * v.double()[:, f]).sum(2)
    q = p.double().gather(1, point[..., None].expand(-1, -1, 3))
    assert bool(((((q - c) ** 2).sum(-1) - d2.double()).abs() <= tol).all())
    # the index itself, wherever the reference's choice is clear
    gaps, best = relative_gaps(p, v, f)
    clear = gaps > GAP
    print("%s: %d of %d faces have a clear nearest point, smallest gap %.3g" % (what, int(clear.sum()), clear.numel(), float(gaps.min())))
    assert torch.equal(best[clear], ref_point[clear])
    assert int(clear.sum()) >= 0.99 * clear.numel()
    assert torch.equal(point[clear], ref_point[clear]), "%s: %d indices differ" % (what, int((point != ref_point)[clear].sum()))
    return point, ref_d2


@functools.lru_cache(maxsize=None)
def case(name):
    """float32 CPU points, vertices, int64 faces, the upstream gradient [B]."""
    B, N, F = CASES[name]
    v, f = soup(B, F)
    return queries(B, N), v, f, torch.as_tensor(np.random.RandomState(7).normal(size=B))


def fused(p, v, f, g, dev, p_grad=True, v_grad=True):
    a, b = p.to(dev).requires_grad_(p_grad), v.to(dev).requires_grad_(v_grad)
    loss = nr.mesh_point_distance(b, f.to(dev).int(), a)
    loss.backward(g.to(device=dev, dtype=torch.float32))
    return loss.detach(), a.grad, b.grad


def reference_grads(p, v, f, g, point):
    a, b = p.double().requires_grad_(True), v.double().requires_grad_(True)
    nr.mesh_point_distance_torch(b, f, a, point=point).backward(g)
    return a.grad, b.grad


@pytest.mark.parametrize("name", list(CASES))
def test_matches_float64(dev, name):
    p, v, f, g = case(name)
    fd = f.to(dev).int()
    got = nr.closest_points_to_faces(v.to(dev), fd, p.to(dev))
    threads, flags = _lib.last_launch(KERNEL)
    assert threads == 256 and flags == (SPLIT_FLAG if name in SPLIT else 0), (threads, flags)
    point, ref_d2 = check_forward(p, v, f, got, name)
    loss, gp, gv = fused(p, v, f, g, dev)
    assert loss.shape == (p.shape[0],) and loss.dtype == torch.float32
    close_out(loss, ref_d2.mean(1), name + " loss")
    assert torch.equal(loss, nr.mesh_point_distance(v.to(dev), fd, p.to(dev)))  # the same points again
    want_gp, want_gv = reference_grads(p, v, f, g, point)
    close_grads(gp, want_gp, name + " grad points")
    close_grads(gv, want_gv, name + " grad vertices")
    if name == "blocks_tiles":
        assert f.shape[0] > FQ and p.shape[1] == 2 * TP + 1


@pytest.mark.parametrize("name", list(RANGES))
def test_every_point_range_holds_a_winner(dev, name):
    """For every range of the split (n equal shares of N, the remainder one each to the first ranges) its first
    and its last point are placed 0.01 above the centroids of faces 0 and 1: that range's partial wins both
    faces.  The reference's choice and its gap are asserted first; the index must equal."""
    p, v, f, _ = case(name)
    B, N, n = p.shape[0], p.shape[1], RANGES[name]
    share, rem = divmod(N, n)
    los = [s * share + min(s, rem) for s in range(n + 1)]
    assert los[-1] == N and 0 < rem < n and f.shape[0] >= 2
    tri = v.double()[:, f[:2]]  # [B, 2, 3, 3]
    normal = torch.linalg.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], dim=-1)
    above = (tri.mean(2) + 0.01 * normal / normal.norm(dim=-1, keepdim=True)).float()
    fd = f.to(dev).int()
    for s in range(n):
        q = p.clone()
        first, last = los[s], los[s + 1] - 1
        q[:, first], q[:, last] = above[:, 0], above[:, 1]
        gaps, best = relative_gaps(q, v, f)
        want = torch.tensor([first, last])[None].expand(B, -1)
        assert torch.equal(best[:, :2], want) and float(gaps[:, :2].min()) > GAP, (s, best[:, :2], gaps[:, :2])
        got = nr.closest_points_to_faces(v.to(dev), fd, q.to(dev))
        assert _lib.last_launch(KERNEL) == (256, SPLIT_FLAG)
        assert torch.equal(got[1].cpu().long()[:, :2], want), (s, got[1].cpu()[:, :2], want)
        check_forward(q, v, f, got, "%s range %d" % (name, s))


def test_ties_pick_the_lowest_index_bitwise(dev):
    """The points given twice (one range; two ranges) and three times (three ranges of one copy each, so every tie
    spans all partials of the combine): every index stays in the first copy, dist2 and weights are bit for bit
    those of the single copy."""
    for N, copies, split in ((40, 2, False), (TP + 1, 2, True), (TP + 1, 3, True)):
        v, f = soup(2, 70)
        vd, fd = v.to(dev), f.to(dev).int()
        p = queries(2, N).to(dev)
        d2, point, w = nr.closest_points_to_faces(vd, fd, p)
        assert _lib.last_launch(KERNEL)[1] == 0
        d2c, pointc, wc = nr.closest_points_to_faces(vd, fd, torch.cat([p] * copies, 1))
        assert bool(_lib.last_launch(KERNEL)[1] & SPLIT_FLAG) == split
        assert int(pointc.max()) < N and torch.equal(pointc, point)
        assert torch.equal(d2c, d2) and torch.equal(wc, w)


def test_split_independence_bitwise(dev):
    """Five faces against 3 TP + 2 points alone (three point ranges), inside a 2,000-face mesh (other blocks, still
    split: eight face blocks do not fill the chip) and inside a mesh of as many face blocks as the split aims for
    (about a million repeated faces, not split): bit for bit the same."""
    N = 3 * TP + 2
    v, f = soup(1, (_lib.NR_FACE_POINT_SPLIT_BLOCKS - 1) * FQ + 1)
    vd, pd = v.to(dev), queries(1, N).to(dev)
    alone = nr.closest_points_to_faces(vd, f[:5].to(dev).int(), pd)
    assert _lib.last_launch(KERNEL) == (256, SPLIT_FLAG)
    some = nr.closest_points_to_faces(vd, f[:2000].to(dev).int(), pd)
    assert _lib.last_launch(KERNEL) == (256, SPLIT_FLAG)
    whole = nr.closest_points_to_faces(vd, f.to(dev).int(), pd)
    assert _lib.last_launch(KERNEL) == (256, 0)
    for other in (some, whole):
        assert all(torch.equal(a, b[:, :5]) for a, b in zip(alone, other))
    assert all(torch.equal(a[:, :2000], b) for a, b in zip(whole, some))


def test_degenerate_faces(dev):
    """The sibling's segments and point, four units apart and far from the soup, with its five points about each:
    a segment's nearest point lies on it (offset (2, 0, 0): the middle, weights a half each at the segment's ends
    and 0 at the unused corner); the point face is equally far from two of its five and takes the first, with the
    weights (1, 0, 0)."""
    B = 2
    v, f = soup(B, 320)
    V0 = v.shape[1]
    dv = torch.tensor(sibling.DEGENERATE_V)
    v = torch.cat([v, dv[None].expand(B, -1, -1)], 1)
    f = torch.cat([f[:100], torch.tensor(sibling.DEGENERATE_F) + V0, f[100:]])
    starts = torch.tensor([[4., 0, 0], [4, 4, 0], [4, 8, 0], [4, 16, 0]])
    near = (starts[:, None] + torch.tensor(sibling.DEGENERATE_OFFSETS)[None]).reshape(-1, 3)  # 20 points, five per face
    p = torch.cat([queries(B, 40), near[None].expand(B, -1, -1)], 1).contiguous()
    got = nr.closest_points_to_faces(v.to(dev), f.to(dev).int(), p.to(dev))
    point, ref_d2 = check_forward(p, v, f, got, "degenerate")
    d2, _, w = (t.cpu() for t in got)
    for k, ends in enumerate(sibling.DEGENERATE_ENDS):
        corners = dv[torch.tensor(sibling.DEGENERATE_F[k])]
        want_w = torch.zeros(3)
        if len(ends) == 1:
            want_i, want_d2 = 40 + 5 * k, 2.  # offsets (1, 1, 0) and (-1, 1, 0) are equally far: the first
            want_w[0] = 1
        else:
            want_i, want_d2 = 40 + 5 * k + 4, 0.
            a, b = corners[ends[0]], corners[ends[1]]
            t = float(((p[0, want_i] - a) * (b - a)).sum() / ((b - a) ** 2).sum())
            assert t == 0.5
            want_w[ends[0]], want_w[ends[1]] = 1 - t, t
        for b in range(B):  # small integers and halves: exact
            assert int(point[b, 100 + k]) == want_i, (k, int(point[b, 100 + k]))
            assert float(d2[b, 100 + k]) == want_d2 and torch.equal(w[b, 100 + k], want_w), (k, d2[b, 100 + k], w[b, 100 + k])
    g = torch.as_tensor(np.random.RandomState(7).normal(size=B))
    loss, gp, gv = fused(p, v, f, g, dev)
    want_gp, want_gv = reference_grads(p, v, f, g, point)
    close_out(loss, ref_d2.mean(1), "degenerate loss")
    close_grads(gp, want_gp, "degenerate grad points")
    close_grads(gv, want_gv, "degenerate grad vertices")
    assert bool(torch.isfinite(gp).all()) and bool(torch.isfinite(gv).all())


@pytest.mark.parametrize("name", ["partial", "three_ranges"])
def test_runs_are_reproducible(dev, name):
    """loss, dist2, point, weights and the vertex gradient bit for bit; the point gradient (float atomics, many
    faces per point) within the gradient tolerance."""
    p, v, f, g = case(name)
    fd = f.to(dev).int()
    first = fused(p, v, f, g, dev)
    first_q = nr.closest_points_to_faces(v.to(dev), fd, p.to(dev))
    distinct = len(torch.unique(first_q[1][0])) / f.shape[0]
    print("%s: %.0f %% of the faces of item 0 hold distinct points" % (name, 100 * distinct))
    for _ in range(2):
        again = fused(p, v, f, g, dev)
        assert torch.equal(first[0], again[0]) and torch.equal(first[2], again[2])
        close_grads(again[1], first[1], "grad points again")
        assert all(torch.equal(a, b) for a, b in zip(first_q, nr.closest_points_to_faces(v.to(dev), fd, p.to(dev))))


@pytest.mark.parametrize("name", ["partial", "three_ranges"])
def test_non_finite_points(dev, name):
    """A few all-NaN points, one with a single NaN coordinate and one with an infinite one among clean ones,
    unsplit and split: every index stays inside [0, N), the faces whose nearest point is still finite do not move
    by a bit, and the backward runs."""
    p, v, f, g = case(name)
    B, N, F = p.shape[0], p.shape[1], f.shape[0]
    vd, fd = v.to(dev), f.to(dev).int()
    clean = [t.cpu() for t in nr.closest_points_to_faces(vd, fd, p.to(dev))]
    assert bool(_lib.last_launch(KERNEL)[1] & SPLIT_FLAG) == (name in RANGES)
    q = p.clone()
    q[:, 0] = float("nan")
    q[:, N - 1] = float("nan")
    q[:, 2, 1] = float("nan")
    q[:, TP, 0] = float("inf")
    hit = ~torch.isfinite(q).all(-1)
    assert int(hit.sum()) == 4 * B
    d2, point, w = (t.cpu() for t in nr.closest_points_to_faces(vd, fd, q.to(dev)))
    assert int(point.min()) >= 0 and int(point.max()) < N
    kept = ~hit.gather(1, clean[1].long())  # faces whose nearest point was not replaced
    assert bool(kept.any())
    assert torch.equal(point[kept], clean[1][kept]) and torch.equal(d2[kept], clean[0][kept]) and torch.equal(w[kept], clean[2][kept])
    loss, gp, gv = fused(q, v, f, g, dev)
    torch.cuda.synchronize()
    assert gp.shape == q.shape and gv.shape == v.shape


def test_interface(dev):
    p, v, f, g = case("partial")
    B, N = p.shape[0], p.shape[1]
    vd, fd = v.to(dev), f.to(dev).int()
    gd = g.to(device=dev, dtype=torch.float32)
    batched = nr.mesh_point_distance(vd, fd, p.to(dev))
    # shared [N, 3] points against B meshes: read in place, bit for bit the expanded copy
    shared = p[0].to(dev)
    expanded = shared[None].expand(B, -1, -1).contiguous()
    a = v.to(dev).requires_grad_(True)
    loss = nr.mesh_point_distance(a, fd, shared)
    loss.backward(gd)
    b = v.to(dev).requires_grad_(True)
    loss_e = nr.mesh_point_distance(b, fd, expanded)
    loss_e.backward(gd)
    assert loss.shape == (B,) and torch.equal(loss, loss_e) and torch.equal(a.grad, b.grad)
    assert all(torch.equal(x, y) for x, y in zip(nr.closest_points_to_faces(vd, fd, shared), nr.closest_points_to_faces(vd, fd, expanded)))
    # shared points that take a gradient receive the item sum
    s = shared.clone().requires_grad_(True)
    nr.mesh_point_distance(vd, fd, s).backward(gd)
    e = expanded.clone().requires_grad_(True)
    nr.mesh_point_distance(vd, fd, e).backward(gd)
    assert s.grad.shape == (N, 3)
    close_grads(s.grad, e.grad.sum(0), "shared points: summed gradient")
    point = nr.closest_points_to_faces(vd, fd, shared)[1].cpu().long()
    s64 = p[0].double().requires_grad_(True)
    nr.mesh_point_distance_torch(v.double(), f, s64, point=point).backward(g)
    close_grads(s.grad, s64.grad, "shared points: gradient against float64")
    # single [V, 3] / [N, 3]; average; the module
    one = nr.mesh_point_distance(v[1].to(dev), fd, p[1].to(dev))
    assert one.ndim == 0 and torch.equal(one, batched[1])
    d1 = nr.closest_points_to_faces(v[1].to(dev), fd, p[1].to(dev))
    F = f.shape[0]
    assert d1[0].shape == (F,) and d1[1].shape == (F,) and d1[2].shape == (F, 3)
    avg = nr.mesh_point_distance(vd, fd, p.to(dev), average=True)
    assert avg.ndim == 0
    close_out(avg, reference(p, v, f)[0].mean(), "average")
    mod = nr.MeshPointLoss(p[0]).to(dev)
    assert torch.equal(mod(vd, fd), loss.detach())
    assert torch.equal(mod(vd, fd, p.to(dev)), batched)
    # CPU int64 faces are converted
    assert torch.equal(nr.mesh_point_distance(vd, f, p.to(dev)), batched)
    # either gradient alone: the other is None, the one taken is unchanged
    whole = fused(p, v, f, g, dev)
    only_p = fused(p, v, f, g, dev, v_grad=False)
    assert only_p[2] is None
    close_grads(only_p[1], whole[1], "points only")
    only_v = fused(p, v, f, g, dev, p_grad=False)
    assert only_v[1] is None and torch.equal(only_v[2], whole[2])
    plain = nr.mesh_point_distance(vd, fd, p.to(dev))
    assert not plain.requires_grad and plain.grad_fn is None and torch.equal(plain, whole[0])
    out = nr.closest_points_to_faces(v.to(dev).requires_grad_(True), fd, p.to(dev).requires_grad_(True))
    assert not any(t.requires_grad for t in out)
    # error cases reach the fused path's checks too
    with pytest.raises(ValueError):
        nr.mesh_point_distance(vd, fd, p[:, :0].to(dev))
    with pytest.raises(ValueError):
        nr.mesh_point_distance(vd, fd[:0], p.to(dev))
    with pytest.raises(ValueError):
        nr.mesh_point_distance(vd, fd, p[:2].to(dev))
    bad = fd.clone()
    bad[5, 2] = v.shape[1]
    with pytest.raises(IndexError):
        nr.mesh_point_distance(vd, bad, p.to(dev))


@pytest.mark.parametrize("name", ["partial", "three_ranges"])
def test_graph_replay_equals_eager(dev, name):
    """Forward + backward (gradient to the vertices: every bit of it is reproducible) captured in a HIP graph."""
    p, v, f, g = case(name)
    pd, fd = p.to(dev), f.to(dev).int()
    gd = g.to(device=dev, dtype=torch.float32)
    x = v.to(dev).requires_grad_(True)

    def step():
        x.grad = None
        loss = nr.mesh_point_distance(x, fd, pd)
        loss.backward(gd)
        return loss.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            eager = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager, eager_grad = eager.clone(), x.grad.clone()
    graph = torch.cuda.CUDAGraph()
    x.grad = None
    with torch.cuda.graph(graph):
        out = step()
    grad = x.grad
    for _ in range(2):
        out.zero_()
        grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(grad, eager_grad)
    assert float(eager_grad.abs().max()) > 0


def test_abi_rejects_bad_arguments(dev):
    """The entry points check sizes, the 32-bit index products, pointers and the workspace before any launch."""
    L = _lib.lib()
    ARGS = 1  # NR_ERR_ARGS
    size = L.nr_face_point_workspace_bytes
    assert size(0, 5, 5) == 0 and size(5, 0, 5) == 0 and size(5, 5, 0) == 0
    assert size(2, 10, 7) >= 2 * 7 * 96 + 3 * 2 * 7 * 4
    assert size(1, 3 * TP + 2, 5) >= size(1, TP, 5) + 2 * 3 * 5 * 4  # three ranges of partials
    p = 4096  # a non-null address that is never dereferenced

    def forward(points=p, stride=30, vertices=p, faces=p, B=2, N=10, V=9, F=7, dist2=p, point=p, weights=p, loss=p, ws=p,
                ws_bytes=1 << 20):
        return L.nr_face_point_forward(points, stride, vertices, faces, B, N, V, F, dist2, point, weights, loss, ws, ws_bytes, None)

    def backward(points=p, stride=30, vertices=p, faces=p, offsets=p, index=p, point=p, weights=p, grad_loss=p, B=2, N=10, V=9, F=7,
                 gp=p, gv=p):
        return L.nr_face_point_backward(points, stride, vertices, faces, offsets, index, point, weights, grad_loss, B, N, V, F, gp, gv,
                                        None)

    for call in (forward, backward):
        assert call(B=-1) == ARGS and call(N=0) == ARGS and call(F=0) == ARGS and call(V=0) == ARGS
        assert call(B=65536) == ARGS and b"65535" in L.nr_last_error()
        assert call(B=4, N=2 ** 29) == ARGS and call(B=4, F=2 ** 29) == ARGS and call(B=4, V=2 ** 28) == ARGS
        assert call(B=1, F=2 ** 31 - 4096) == ARGS  # B F above INT_MAX - 4096
        assert call(stride=-30) == ARGS
        assert call(points=None) == ARGS and call(vertices=None) == ARGS and call(faces=None) == ARGS
    assert forward(dist2=None, point=None, weights=None, loss=None) == ARGS
    assert forward(ws=None) == ARGS and forward(ws_bytes=size(2, 10, 7) - 1) == ARGS
    assert b"workspace" in L.nr_last_error()
    assert backward(point=None) == ARGS and backward(weights=None) == ARGS and backward(grad_loss=None) == ARGS
    assert backward(offsets=None) == ARGS and backward(index=None) == ARGS
    # nothing to do: no pointer is needed
    assert forward(B=0, points=None, vertices=None, faces=None, ws=None) == 0
    assert backward(B=0, points=None, vertices=None, faces=None) == 0
    assert backward(gp=None, gv=None, points=None) == 0


def test_null_outputs_leave_the_others_unchanged(dev):
    """nr_face_point_forward itself (the wrappers always ask for dist2, point and weights), unsplit with a partial last
    block and split: the loss alone, then each of dist2, point and weights alone, is bit for bit what the call with
    every output writes.  Each array starts at -1, which no result holds."""
    L = _lib.lib()
    for name in ("partial", "three_ranges"):
        p, v, f, _ = case(name)
        B, N, V, F = p.shape[0], p.shape[1], v.shape[1], f.shape[0]
        pd, vd, fd = p.to(dev), v.to(dev), f.to(dev).int()
        ws = torch.empty(L.nr_face_point_workspace_bytes(B, N, F), dtype=torch.uint8, device=dev)

        def run(*want):
            out = {"dist2": torch.full((B, F), -1., device=dev), "point": torch.full((B, F), -1, dtype=torch.int32, device=dev),
                   "weights": torch.full((B, F, 3), -1., device=dev), "loss": torch.full((B,), -1., device=dev)}
            ptrs = [_lib.ptr(out[k] if k in want else None) for k in ("dist2", "point", "weights", "loss")]
            _lib.check(L.nr_face_point_forward(_lib.ptr(pd), N * 3, _lib.ptr(vd), _lib.ptr(fd), B, N, V, F, *ptrs, _lib.ptr(ws),
                                               ws.numel(), _lib.stream_of(vd)), "nr_face_point_forward")
            assert _lib.last_launch(KERNEL) == (256, SPLIT_FLAG if name in SPLIT else 0)
            return out

        full = run("dist2", "point", "weights", "loss")
        assert float(full["dist2"].min()) >= 0 and int(full["point"].min()) >= 0 and float(full["weights"].min()) >= 0
        assert float(full["loss"].min()) > 0
        for only in ("loss", "dist2", "point", "weights"):
            assert torch.equal(run(only)[only], full[only]), (name, only)

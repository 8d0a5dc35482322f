"""The fused chamfer distance, nearest_points and sample_points on the GPU (float32) against the torch
compositions in float64 on the CPU, which receive the same float32 values widened.

Tolerances are test_gpu_mesh_loss's: losses rtol = atol = 1e-5, gradients 1e-4 of the reference
gradient's largest magnitude plus 1e-4 relative.  Per-point squared distances: rtol 1e-6 (the difference
form carries at most five float32 roundings over non-negative terms, about 3e-7).  Nearest indices must
EQUAL the reference's at every point: each case first asserts that the reference's nearest and
second-nearest squared distances differ by more than 1e-5 relative everywhere, which the float32 error
cannot bridge."""
import functools

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import _lib, point_loss, synthetic
from mesh_loss_cases import grid_fin, jitter

pytestmark = pytest.mark.gpu

OUT_TOL = 1e-5
GRAD_TOL = 1e-4
DIST_RTOL = 1e-6
GAP = 1e-5
DIRECTIONS = ("both", "x_to_y", "y_to_x")

CASES = {  # name: (B, N, M)
    "wave": (3, 65, 63),            # either side of a wave
    "partial_block": (3, 257, 300),
    "few_x": (2, 3, 2500),          # few queries: the split-target path in x_to_y
    "few_y": (2, 2500, 3),          # the same in y_to_x
    "blocks_tiles": (2, 1025, 2049),  # several query blocks; CHAMFER_TILE lies strictly inside M and N + 1
    "one_x": (2, 1, 40),
    "one_y": (2, 40, 1),
    # more than two target ranges per query block (the cases above split in two at most): the remainder goes
    # to the first ranges, and the combine walks past its first step
    # (none of these five queries chooses the middle range: test_every_target_range_holds_a_nearest_point does)
    "three_ranges": (1, 5, 3074),   # 3 ranges of 1025, 1025, 1024 targets; smallest relative gap 1.4e-4
    "five_ranges": (2, 3, 5123),    # 5 ranges, the first 3 one target longer; smallest relative gap 2.6e-4
}
SPLIT = {"few_x": _lib.NR_LAUNCH_SPLIT_X_TO_Y, "few_y": _lib.NR_LAUNCH_SPLIT_Y_TO_X,
         "three_ranges": _lib.NR_LAUNCH_SPLIT_X_TO_Y, "five_ranges": _lib.NR_LAUNCH_SPLIT_X_TO_Y}


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


def points(B, N, M):
    x = np.random.RandomState(103).uniform(-1, 1, (B, N, 3)).astype(np.float32)
    y = np.random.RandomState(203).uniform(-1, 1, (B, M, 3)).astype(np.float32)
    return torch.as_tensor(x), torch.as_tensor(y)


def relative_gap(q, t):
    """The smallest (second - nearest) / second squared distance over the queries q against the targets t
    (float64); inf with a single target."""
    if t.shape[1] < 2:
        return float("inf")
    worst = float("inf")
    for i in range(0, q.shape[1], 256):
        diff = q[:, i:i + 256, None] - t[:, None]
        two = (diff * diff).sum(-1).topk(2, dim=2, largest=False)[0]
        worst = min(worst, float(((two[..., 1] - two[..., 0]) / two[..., 1]).min()))
    return worst


@functools.lru_cache(maxsize=None)
def case(name):
    """float32 CPU x, y; the upstream gradient [B]; the float64 reference: nearest (dist2, index) both ways,
    and per directions value the loss and both gradients.  Asserts the gap precondition."""
    x, y = points(*CASES[name])
    x64, y64 = x.double(), y.double()
    gaps = relative_gap(x64, y64), relative_gap(y64, x64)
    print("%s: smallest relative gaps %.3g (x to y) %.3g (y to x)" % (name, gaps[0], gaps[1]))
    assert min(gaps) > GAP, gaps
    g = torch.as_tensor(np.random.RandomState(7).normal(size=x.shape[0]))
    ref = {"xy": nr.nearest_points_torch(x64, y64), "yx": nr.nearest_points_torch(y64, x64)}
    for directions in DIRECTIONS:
        a, b = x64.clone().requires_grad_(True), y64.clone().requires_grad_(True)
        loss = nr.chamfer_distance_torch(a, b, directions)
        loss.backward(g)
        ref[directions] = (loss.detach(), a.grad, b.grad)
    return x, y, g, ref


def fused(x, y, g, dev, directions="both", y_grad=True):
    a = x.to(dev).requires_grad_(True)
    b = y.to(dev).requires_grad_(y_grad)
    loss = nr.chamfer_distance(a, b, directions)
    loss.backward(g.to(device=dev, dtype=torch.float32))
    return loss.detach(), a.grad, b.grad


@pytest.mark.parametrize("name", list(CASES))
def test_nearest_points_match_float64(dev, name):
    x, y, _, ref = case(name)
    for key, (q, t) in (("xy", (x, y)), ("yx", (y, x))):
        d2, idx = nr.nearest_points(q.to(dev), t.to(dev))
        assert d2.dtype == torch.float32 and idx.dtype == torch.int32 and d2.shape == q.shape[:2] and idx.shape == q.shape[:2]
        assert torch.equal(idx.cpu(), ref[key][1]), "%s %s: %d indices differ" % (
            name, key, int((idx.cpu() != ref[key][1]).sum()))
        err = ((d2.cpu().double() - ref[key][0]).abs() / ref[key][0]).max()
        print("%s %s: dist2 max relative error %.3g" % (name, key, float(err)))
        assert float(err) <= DIST_RTOL
    if name in SPLIT:
        q, t = (x, y) if SPLIT[name] == _lib.NR_LAUNCH_SPLIT_X_TO_Y else (y, x)
        nr.nearest_points(q.to(dev), t.to(dev))
        assert _lib.last_launch("k_chamfer_nn") == (256, _lib.NR_LAUNCH_SPLIT_X_TO_Y)


@pytest.mark.parametrize("directions", DIRECTIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_chamfer_matches_float64(dev, name, directions):
    x, y, g, ref = case(name)
    loss, gx, gy = fused(x, y, g, dev, directions)
    threads, flags = _lib.last_launch("k_chamfer_nn")
    want, want_gx, want_gy = ref[directions]
    assert loss.shape == (x.shape[0],) and loss.dtype == torch.float32 and gx.shape == x.shape and gy.shape == y.shape
    print("%s %s: loss %s ref %s" % (name, directions, loss.tolist(), want.tolist()))
    close_out(loss, want, "%s %s" % (name, directions))
    close_grads(gx, want_gx, "%s %s grad x" % (name, directions))
    close_grads(gy, want_gy, "%s %s grad y" % (name, directions))
    if name in SPLIT and directions != ("y_to_x" if SPLIT[name] == _lib.NR_LAUNCH_SPLIT_X_TO_Y else "x_to_y"):
        assert threads == 256 and flags & SPLIT[name], (threads, flags)  # the few-against-many direction ran split
    if name == "wave":
        assert flags == 0  # small sets: no split
    if name == "blocks_tiles":
        assert 0 < point_loss.CHAMFER_TILE < y.shape[1] - 1 and point_loss.CHAMFER_TILE < x.shape[1]


def test_single_set_and_average(dev):
    x, y, g, ref = case("partial_block")
    one = nr.chamfer_distance(x[1].to(dev), y[1].to(dev))
    assert one.ndim == 0
    close_out(one, ref["both"][0][1], "single")
    avg = nr.chamfer_distance(x.to(dev), y.to(dev), average=True)
    assert avg.ndim == 0
    close_out(avg, ref["both"][0].mean(), "average")
    mod = nr.ChamferLoss(y[0]).to(dev)
    assert torch.equal(mod(x.to(dev)), nr.chamfer_distance(x.to(dev), y[0].to(dev)))


def test_shared_target_equals_expanded_bitwise(dev):
    x, y, g, _ = case("partial_block")
    B = x.shape[0]
    shared = y[0].to(dev)
    a = x.to(dev).requires_grad_(True)
    loss = nr.chamfer_distance(a, shared)
    loss.backward(g.to(device=dev, dtype=torch.float32))
    b = x.to(dev).requires_grad_(True)
    loss_e = nr.chamfer_distance(b, shared[None].expand(B, -1, -1).contiguous())
    loss_e.backward(g.to(device=dev, dtype=torch.float32))
    assert torch.equal(loss, loss_e) and torch.equal(a.grad, b.grad)
    # a shared target that takes a gradient receives the item sum
    s = shared.clone().requires_grad_(True)
    nr.chamfer_distance(x.to(dev), s).backward(g.to(device=dev, dtype=torch.float32))
    e = shared[None].expand(B, -1, -1).contiguous().requires_grad_(True)
    nr.chamfer_distance(x.to(dev), e).backward(g.to(device=dev, dtype=torch.float32))
    assert s.grad.shape == shared.shape
    close_grads(s.grad, e.grad.sum(0), "shared grad y")
    s64 = y[0].double().requires_grad_(True)
    nr.chamfer_distance_torch(x.double(), s64).backward(g)
    close_grads(s.grad, s64.grad, "shared grad y against float64")


def test_identical_sets(dev):
    x, _, g, _ = case("partial_block")
    assert len(np.unique(x.numpy().reshape(-1, 3), axis=0)) == x.shape[0] * x.shape[1]  # distinct points
    loss, gx, gy = fused(x, x.clone(), g, dev)
    assert float(loss.abs().max()) == 0. and float(gx.abs().max()) == 0. and float(gy.abs().max()) == 0.
    d2, idx = nr.nearest_points(x.to(dev), x.clone().to(dev))
    assert float(d2.abs().max()) == 0.
    assert torch.equal(idx.cpu(), torch.arange(x.shape[1], dtype=torch.int32)[None].expand(x.shape[0], -1))


def test_duplicated_targets_pick_the_lowest_index(dev):
    # 2500 targets: the second half repeats the first, so every tie crosses the split's ranges and tiles
    x, y = points(2, 70, 1250)
    y2 = torch.cat([y, y], 1)
    d2, idx = nr.nearest_points(x.to(dev), y2.to(dev))
    assert _lib.last_launch("k_chamfer_nn")[1] & _lib.NR_LAUNCH_SPLIT_X_TO_Y
    want = nr.nearest_points_torch(x.double(), y2.double())[1]
    assert int(idx.max()) < 1250 and torch.equal(idx.cpu(), want)
    # 3075 targets, 1025 repeated three times against 5 queries: three ranges of 1025, so every tie spans all
    # three partials of the combine
    x, y = points(2, 5, 1025)
    assert relative_gap(x.double(), y.double()) > GAP
    y3 = torch.cat([y, y, y], 1)
    d2, idx = nr.nearest_points(x.to(dev), y3.to(dev))
    assert _lib.last_launch("k_chamfer_nn")[1] & _lib.NR_LAUNCH_SPLIT_X_TO_Y
    want = nr.nearest_points_torch(x.double(), y3.double())[1]
    assert int(idx.max()) < 1025 and torch.equal(idx.cpu(), want)
    assert torch.equal(idx.cpu(), nr.nearest_points_torch(x.double(), y.double())[1])
    x, y = points(2, 70, 1250)
    # within one block: targets 3 and 9 equal
    y3 = y[:, :40].clone()
    y3[:, 9] = y3[:, 3]
    q = torch.cat([x[:, :5], y3[:, 9:10] + 1e-3], 1)
    idx = nr.nearest_points(q.to(dev), y3.to(dev))[1]
    assert idx[:, 5].tolist() == [3, 3] and not bool((idx == 9).any())


@pytest.mark.parametrize("name", ["three_ranges", "five_ranges"])
def test_every_target_range_holds_a_nearest_point(dev, name):
    """With the file's draw no query of three_ranges has its nearest target in the middle range, so a combine
    that skipped a partial would pass there.  Here the queries sit 1e-3 beside the first and the last target of
    every range (n equal shares of M, the remainder one each to the first ranges): each partial wins for two
    queries, and a range boundary off by one would lose or double one of these targets."""
    _, y, _, _ = case(name)
    B, M = y.shape[0], y.shape[1]
    n = {"three_ranges": 3, "five_ranges": 5}[name]
    share, rem = divmod(M, n)
    los = [s * share + min(s, rem) for s in range(n + 1)]
    assert los[-1] == M and 0 < rem < n
    picks = torch.as_tensor([j for s in range(n) for j in (los[s], los[s + 1] - 1)])
    q = (y[:, picks] + torch.as_tensor([1e-3, -1e-3, 1e-3])).contiguous()
    want_d2, want = nr.nearest_points_torch(q.double(), y.double())
    assert torch.equal(want.long(), picks[None].expand(B, -1)) and relative_gap(q.double(), y.double()) > GAP
    d2, idx = nr.nearest_points(q.to(dev), y.to(dev))
    assert _lib.last_launch("k_chamfer_nn")[1] & _lib.NR_LAUNCH_SPLIT_X_TO_Y
    assert torch.equal(idx.cpu(), want), (idx.cpu().tolist(), picks.tolist())
    assert float(((d2.cpu().double() - want_d2).abs() / want_d2).max()) <= DIST_RTOL


@pytest.mark.parametrize("name", ["partial_block", "three_ranges"])
def test_nearest_points_with_nan_coordinates(dev, name):
    """The saved indices stay inside the other set whatever the coordinates hold: a distance to or from a
    NaN compares false, so a NaN query keeps the first target of its range (index 0 after the combine too),
    a NaN target is never chosen, and no other point's result moves.  Forward only, unsplit and split."""
    x, y, _, _ = case(name)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    nan = float("nan")
    clean_d2, clean_idx = (a.cpu() for a in nr.nearest_points(x.to(dev), y.to(dev)))
    assert bool(_lib.last_launch("k_chamfer_nn")[1] & _lib.NR_LAUNCH_SPLIT_X_TO_Y) == (name in SPLIT)
    # queries: row 0 all NaN, the last row all NaN, row 2 with one NaN coordinate
    xq = x.clone()
    xq[:, 0] = nan
    xq[:, N - 1] = nan
    xq[:, 2, 1] = nan
    hit = torch.isnan(xq).any(-1)
    d2, idx = (a.cpu() for a in nr.nearest_points(xq.to(dev), y.to(dev)))
    assert int(idx.min()) >= 0 and int(idx.max()) < M
    assert int(hit.sum()) == 3 * B and bool((idx[hit] == 0).all())
    assert torch.equal(idx[~hit], clean_idx[~hit]) and torch.equal(d2[~hit], clean_d2[~hit])
    # targets: the first and last target, the first of the second and third ranges where there are such, and
    # per item the target that query 1 chose
    yt = y.clone()
    dead = torch.zeros((B, M), dtype=torch.bool)
    dead[:, [0, 7, min(1025, M - 2), min(2050, M - 3), M - 1]] = True
    dead[torch.arange(B), clean_idx[:, 1].long()] = True
    yt[dead] = nan
    d2, idx = (a.cpu() for a in nr.nearest_points(x.to(dev), yt.to(dev)))
    assert int(idx.min()) >= 0 and int(idx.max()) < M
    assert not bool(dead.gather(1, idx.long()).any())  # a NaN target is never the nearest
    kept = ~dead.gather(1, clean_idx.long())
    assert not bool(kept[:, 1].any()) and bool(kept.any(1).all())
    assert torch.equal(idx[kept], clean_idx[kept]) and torch.equal(d2[kept], clean_d2[kept])
    assert bool(torch.isfinite(d2).all()) and bool((d2[~kept] > clean_d2[~kept]).all())


def test_non_contiguous_x(dev):
    x, y, g, ref = case("partial_block")
    wide = torch.zeros((x.shape[0], x.shape[1], 5))
    wide[..., 1:4] = x
    wd = wide.to(dev).requires_grad_(True)
    sl = wd[..., 1:4]
    assert not sl.is_contiguous()
    loss = nr.chamfer_distance(sl, y.to(dev))
    loss.backward(g.to(device=dev, dtype=torch.float32))
    close_out(loss, ref["both"][0], "slice")
    close_grads(wd.grad[..., 1:4], ref["both"][1], "slice grad")
    assert float(wd.grad[..., 0].abs().max()) == 0. and float(wd.grad[..., 4].abs().max()) == 0.
    d2, idx = nr.nearest_points(sl.detach(), y.to(dev))
    assert torch.equal(idx.cpu(), ref["xy"][1])


def test_runs_are_bitwise_reproducible(dev):
    x, y, g, _ = case("partial_block")
    first = fused(x, y, g, dev)
    for _ in range(2):
        again = fused(x, y, g, dev)
        assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_no_gradient_needed(dev):
    x, y, g, _ = case("wave")
    with_grad = fused(x, y, g, dev)[0]
    plain = nr.chamfer_distance(x.to(dev), y.to(dev))
    assert not plain.requires_grad and plain.grad_fn is None and torch.equal(plain, with_grad)
    # only y takes a gradient
    b = y.to(dev).requires_grad_(True)
    nr.chamfer_distance(x.to(dev), b).backward(g.to(device=dev, dtype=torch.float32))
    assert torch.equal(b.grad, fused(x, y, g, dev)[2])


def test_graph_capture_matches_eager(dev):
    """Forward + backward of the partial-block case captured in a HIP graph on one stream after a warm-up
    call and replayed twice: bit for bit the eager loss and gradients."""
    x, y, g, _ = case("partial_block")
    gd = g.to(device=dev, dtype=torch.float32)
    a, b = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)

    def step():
        a.grad = b.grad = None
        loss = nr.chamfer_distance(a, b)
        loss.backward(gd)
        return loss.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    a.grad = b.grad = None
    with torch.cuda.graph(graph):
        loss = step()
    ga, gb = a.grad, b.grad
    eager = fused(x, y, g, dev)
    for _ in range(2):
        loss.zero_(), ga.zero_(), gb.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, eager[0]) and torch.equal(ga, eager[1]) and torch.equal(gb, eager[2])


# ---- sample_points ----
def fin_with_dead_face():
    v, f = grid_fin()
    return v, np.concatenate([f, [[3, 3, 8]]]).astype(np.int32)


MESHES = {"ico0": lambda: synthetic.icosphere(0), "ico2": lambda: synthetic.icosphere(2), "grid_fin_dead": fin_with_dead_face}


@pytest.mark.parametrize("S", [1, 64, 1000])
@pytest.mark.parametrize("mesh", list(MESHES))
def test_sample_points(dev, mesh, S):
    v, f = MESHES[mesh]()
    vb = torch.as_tensor(jitter(v, 3, 0.02, 31).astype(np.float32))
    u = torch.as_tensor(np.random.RandomState(7).uniform(0, 1, (3, S, 3)).astype(np.float32))
    check_sample_points(dev, vb, f, u, 1e-5, "%s S=%d" % (mesh, S))


def check_sample_points(dev, vb, f, u, margin, what):
    """sample_points of the float32 CPU vertices vb [B, V, 3], faces f and u [B, S, 3] against the float64
    composition: weights, points, the chosen face's cdf bracket, no face of zero area in an item that has
    area, the vertex gradient, and the composition's own faces wherever u0 * total is further than
    margin * total from the chosen face's cdf boundaries.  Returns (faces, the float64 composition's faces,
    whether each sample is outside the margin)."""
    B, S, F = u.shape[0], u.shape[1], f.shape[0]
    vd = vb.to(dev).requires_grad_(True)
    pts, face, w = nr.sample_points(vd, torch.as_tensor(f, device=dev), S, u=u.to(dev), return_faces=True)
    assert pts.shape == (B, S, 3) and face.shape == (B, S) and face.dtype == torch.int32 and w.shape == (B, S, 3)
    up = torch.as_tensor(np.random.RandomState(8).normal(size=(B, S, 3)).astype(np.float32))
    pts.backward(up.to(dev))
    face_c, w_c, pts_c = face.cpu().long(), w.cpu().double(), pts.detach().cpu().double()
    assert int(face_c.min()) >= 0 and int(face_c.max()) < F
    v64, u64 = vb.double(), u.double()
    tri = v64[:, torch.as_tensor(f).long()]
    area = 0.5 * torch.linalg.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], dim=-1).norm(dim=-1)
    C = torch.cumsum(area, 1)
    total = C[:, -1:]
    t = u64[..., 0] * total
    upper = C.gather(1, face_c)
    lower = torch.where(face_c > 0, C.gather(1, (face_c - 1).clamp(min=0)), torch.zeros_like(upper))
    assert bool((lower - 1e-5 * total <= t).all()) and bool((t <= upper + 1e-5 * total).all())
    assert bool(((area.gather(1, face_c) > 0) | (total == 0)).all())
    r = torch.sqrt(u64[..., 1])
    want_w = torch.stack([1 - r, r * (1 - u64[..., 2]), r * u64[..., 2]], -1)
    assert float((w_c - want_w).abs().max()) <= 1e-6
    corners = tri.gather(1, face_c[..., None, None].expand(-1, -1, 3, 3))  # [B, S, 3 corners, 3]
    assert float((pts_c - (w_c[..., None] * corners).sum(2)).abs().max()) <= 1e-6
    # the composition's gradient with the returned faces and weights
    want_g = torch.zeros_like(v64)
    ids = torch.as_tensor(f).long()[face_c]
    for b in range(B):
        for k in range(3):
            want_g[b].index_add_(0, ids[b, :, k], w_c[b, :, k, None] * up[b].double())
    close_grads(vd.grad, want_g, "%s vertex grad" % what)
    # and the composition itself chooses the same faces wherever u0 is not at a face's boundary
    face_t = nr.sample_points_torch(v64, f, S, u=u64, return_faces=True)[1].long()
    inside = torch.minimum((t - lower).abs(), (upper - t).abs()) > margin * total
    assert torch.equal(face_c[inside], face_t[inside])
    return face_c, face_t, inside


MARGIN_CHUNKS = 1e-6  # of the total area; see ico5_dead


@functools.lru_cache(maxsize=None)
def ico5_dead(S):
    """The icosphere L5 (F 20480: five 4096-face chunks of the scan, all of its 16 waves at work) with faces
    of zero area (a repeated vertex) at the very start (0, 1: the cdf is 0 before the first live face), on a
    wave border (255, 256), on a chunk border (4094..4097), every 512th face from 100 on, and at the end
    (the last three).  B 3, jitter 0.002; the last item has all-zero vertices (no area at all).  u is the
    file's draw, with the first samples' u0 replaced by 0, 1, the largest float32 below 1, and 0.5.

    A face is 4.9e-5 of the total area wide, so the agreement with the float64 composition's faces is asked
    outside a margin of 1e-6 of the total, not 1e-5: float32 torch's cdf is within 4.7e-8 of the total of the
    float64 one (asserted here at 1e-7), u0 * total rounds by 6e-8 relative, and the margin is about ten
    times their sum.  It excludes 4.5 % of 2000 samples (asserted here at 5 %).
    Returns float32 CPU vertices [3, V, 3], faces, u [3, S, 3], the dead faces."""
    v, f = synthetic.icosphere(5)
    F = f.shape[0]
    dead = sorted(set([0, 1, 255, 256, 4094, 4095, 4096, 4097] + list(range(100, F, 512)) + [F - 3, F - 2, F - 1]))
    f = f.copy()
    f[dead] = f[dead][:, [0, 0, 1]]
    vb = torch.as_tensor(jitter(v, 3, 0.002, 31).astype(np.float32))
    vb[2] = 0.
    u = torch.as_tensor(np.random.RandomState(7).uniform(0, 1, (3, S, 3)).astype(np.float32))
    special = torch.tensor([0., 1., float(np.nextafter(np.float32(1), np.float32(0))), 0.5])
    u[:, :min(S, 4), 0] = special[:S]
    fl = torch.as_tensor(f).long()
    c32, c64 = point_loss._face_cdf(vb, fl), point_loss._face_cdf(vb.double(), fl)
    total = c64[:2, -1:]
    assert float(total.min()) > 0 and float(c64[2].max()) == 0.
    cdf_err = float(((c32[:2].double() - c64[:2]).abs() / total).max())
    assert cdf_err <= 1e-7, cdf_err
    # the dead faces repeat their predecessor's value, the live ones rise
    rise = torch.diff(c64[:2], dim=1, prepend=torch.zeros(2, 1, dtype=torch.float64)) > 0
    live = torch.ones(F, dtype=torch.bool)
    live[dead] = False
    assert torch.equal(rise, live[None].expand(2, -1))
    t = (u[:2, :, 0].double() * total).contiguous()
    edges = torch.cat([torch.zeros(2, 1, dtype=torch.float64), c64[:2]], 1)  # ascending: the nearest edge is a neighbour
    j = torch.searchsorted(edges, t).clamp(1, F)
    near = torch.minimum((t - edges.gather(1, j - 1)).abs(), (edges.gather(1, j) - t).abs())
    excluded = float((near <= MARGIN_CHUNKS * total).double().mean())
    print("ico5_dead S=%d: cdf error %.3g of the total, %.3g of the samples inside the margin" % (S, cdf_err, excluded))
    if S >= 1000:
        assert excluded <= 0.05, excluded
    return vb, f, u, dead


@pytest.mark.parametrize("S", [1, 64, 2000])
def test_sample_points_across_chunks(dev, S):
    """A mesh of five scan chunks with zero-area faces on every kind of border, and an item without area
    beside two that have some: everything test_sample_points asserts, the start of the cdf, and the fallback
    for u0 * total == total (the last face of positive area, which is not the last face)."""
    vb, f, u, dead = ico5_dead(S)
    F = f.shape[0]
    face, face64, inside = check_sample_points(dev, vb, f, u, MARGIN_CHUNKS, "ico5_dead S=%d" % S)
    assert not bool(np.isin(face[:2].numpy(), dead).any())
    assert bool((face[2] == F - 1).all()) and bool((face64[2] == F - 1).all())  # the item without area
    if S >= 1000:
        assert float(inside[:2].double().mean()) >= 0.95
    face32 = nr.sample_points_torch(vb, f, S, u=u, return_faces=True)[1].long()
    assert F - 4 not in dead and F - 3 in dead
    for name, got in (("fused", face), ("float64", face64), ("float32", face32)):
        assert got[:2, 0].tolist() == [2, 2], (name, got[:2, 0])  # u0 = 0: the first face of positive area
        if S >= 2:
            assert got[:2, 1].tolist() == [F - 4, F - 4], (name, got[:2, 1])  # u0 = 1: the last one, by the second search


def test_sample_points_item_without_area(dev):
    v, f = synthetic.icosphere(0)
    vb = torch.as_tensor(np.stack([v, np.zeros_like(v)]).astype(np.float32), device=dev)
    pts, face, w = nr.sample_points(vb, f, 50, return_faces=True, generator=torch.Generator(device=dev).manual_seed(3))
    torch.cuda.synchronize()
    assert face[1].tolist() == [f.shape[0] - 1] * 50 and float(pts[1].abs().max()) == 0.
    assert len(set(face[0].tolist())) > 5
    single = nr.sample_points(vb[0], f, 9)
    assert single.shape == (9, 3)


def descend(vertices, faces, target, u, chamfer, sample):
    """Twenty nr.Adam steps of chamfer(sample(vertices), target); the summed loss before every step and after the last."""
    param = vertices.clone().requires_grad_(True)
    opt = nr.Adam([param], lr=0.002)
    history = []
    for _ in range(21):
        opt.zero_grad()
        loss = chamfer(sample(param, faces, u.shape[1], u=u), target).sum()
        history.append(float(loss.detach()))
        if len(history) <= 20:
            loss.backward()
            opt.step()
    return history


def test_fit_to_sampled_target(dev):
    """Twenty nr.Adam steps (lr 0.002) pulling the icosphere L2 (B 2) towards 400 points sampled from a
    jittered copy (sigma 0.05), 400 samples per step from one fixed u.  The float64 composition on the CPU
    takes the summed loss from 0.035748 to 0.028758 (a decrease of 0.006990); the fused path must achieve
    half of the reference's decrease, measured in the same run."""
    v, f = synthetic.icosphere(2)
    B, S = 2, 400
    start = torch.as_tensor(np.repeat(v[None], B, 0).astype(np.float32))
    copy = torch.as_tensor(jitter(v, B, 0.05, 41).astype(np.float32))
    u_t = torch.as_tensor(np.random.RandomState(42).uniform(0, 1, (B, S, 3)).astype(np.float32))
    u = torch.as_tensor(np.random.RandomState(43).uniform(0, 1, (B, S, 3)).astype(np.float32))
    target64 = nr.sample_points_torch(copy.double(), f, S, u=u_t.double())
    ref = descend(start.double(), f, target64, u.double(), nr.chamfer_distance_torch, nr.sample_points_torch)
    faces = torch.as_tensor(f, device=dev)
    target = nr.sample_points(copy.to(dev), faces, S, u=u_t.to(dev))
    got = descend(start.to(dev), faces, target, u.to(dev), nr.chamfer_distance, nr.sample_points)
    print("reference %.6f -> %.6f, fused %.6f -> %.6f" % (ref[0], ref[-1], got[0], got[-1]))
    assert ref[-1] < ref[0]
    assert got[-1] < got[0]
    assert got[0] - got[-1] >= 0.5 * (ref[0] - ref[-1])

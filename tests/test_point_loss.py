"""point_loss on the host: the torch compositions against plain double loops and torch's gradcheck, the
properties of sample_points_torch, the argument checks of the C entry points, and the Python-level errors."""
import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import _lib, point_loss, synthetic
from mesh_loss_cases import grid_fin


def brute_nearest(x, y):
    """dist2 [N] and index [N] of the nearest y of every x by a double loop; strict <: the lowest index."""
    d2, idx = np.zeros(len(x)), np.zeros(len(x), np.int64)
    for i, p in enumerate(x):
        best, arg = np.inf, -1
        for j, q in enumerate(y):
            d = float(((p - q) ** 2).sum())
            if d < best:
                best, arg = d, j
        d2[i], idx[i] = best, arg
    return d2, idx


def brute_chamfer(x, y, directions):
    out = np.zeros(len(x))
    for b in range(len(x)):
        yb = y[b] if y.ndim == 3 else y
        if directions in ("both", "x_to_y"):
            out[b] += brute_nearest(x[b], yb)[0].mean()
        if directions in ("both", "y_to_x"):
            out[b] += brute_nearest(yb, x[b])[0].mean()
    return out


def sets(B=2, N=5, M=7, seed=0):
    r = np.random.RandomState(seed)
    return r.uniform(-1, 1, (B, N, 3)), r.uniform(-1, 1, (B, M, 3))


@pytest.mark.parametrize("directions", ["both", "x_to_y", "y_to_x"])
@pytest.mark.parametrize("shared", [False, True])
def test_compositions_match_brute_force(directions, shared):
    x, y = sets()
    if shared:
        y = y[0]
    got = nr.chamfer_distance_torch(torch.as_tensor(x), torch.as_tensor(y), directions)
    assert got.shape == (2,) and got.dtype == torch.float64
    assert np.allclose(got.numpy(), brute_chamfer(x, y, directions), rtol=1e-13, atol=0)
    d2, idx = nr.nearest_points_torch(torch.as_tensor(x), torch.as_tensor(y))
    assert d2.shape == (2, 5) and idx.shape == (2, 5) and idx.dtype == torch.int32
    for b in range(2):
        want_d2, want_idx = brute_nearest(x[b], y if shared else y[b])
        assert np.array_equal(idx[b].numpy(), want_idx) and np.allclose(d2[b].numpy(), want_d2, rtol=1e-13, atol=0)
    # chunking over N changes nothing
    old = point_loss._CHUNK_ELEMS
    try:
        point_loss._CHUNK_ELEMS = 1
        again = nr.chamfer_distance_torch(torch.as_tensor(x), torch.as_tensor(y), directions)
    finally:
        point_loss._CHUNK_ELEMS = old
    assert torch.equal(again, got)


def test_duplicated_target_picks_the_lower_index():
    x, y = sets()
    y[:, 5] = y[:, 2]  # the same point twice
    x[:, 0] = y[:, 2] + 1e-3
    for fn in (nr.nearest_points_torch, nr.nearest_points):
        d2, idx = fn(torch.as_tensor(x), torch.as_tensor(y))
        assert idx[:, 0].tolist() == [2, 2]
        assert not bool((idx == 5).any())
    # and in the other direction: two equal queries choose alike
    _, back = nr.nearest_points_torch(torch.as_tensor(y), torch.as_tensor(x))
    assert torch.equal(back[:, 5], back[:, 2])


def test_shapes_average_and_module():
    x, y = (torch.as_tensor(t) for t in sets(3, 4, 6, 1))
    per_item = nr.chamfer_distance(x, y)
    assert per_item.shape == (3,)
    one = nr.chamfer_distance(x[1], y[1])
    assert one.ndim == 0 and float(one) == float(per_item[1])
    avg = nr.chamfer_distance(x, y, average=True)
    assert avg.ndim == 0 and abs(float(avg) - float(per_item.mean())) <= 1e-15
    # a shared target is the expanded one
    assert torch.equal(nr.chamfer_distance(x, y[0]), nr.chamfer_distance(x, y[0][None].expand(3, -1, -1)))
    both = nr.chamfer_distance(x, y, "x_to_y") + nr.chamfer_distance(x, y, "y_to_x")
    assert float((both - per_item).abs().max()) <= 1e-15
    mod = nr.ChamferLoss(y[0], directions="x_to_y", average=True)
    assert torch.equal(mod(x), nr.chamfer_distance(x, y[0], "x_to_y", average=True))
    assert torch.equal(nr.ChamferLoss()(x, y), per_item)
    assert "target" in dict(mod.named_buffers())
    with pytest.raises(ValueError):
        nr.ChamferLoss()(x)
    d2, idx = nr.nearest_points(x[0], y[0])
    assert d2.shape == (4,) and idx.shape == (4,) and not d2.requires_grad


def gap(x, y):
    """The smallest relative gap between the nearest and the second-nearest squared distance, both ways."""
    worst = np.inf
    for a, b in ((x, y), (y, x)):
        d = np.sort(((a[:, :, None] - b[:, None]) ** 2).sum(-1), axis=2)
        worst = min(worst, float(((d[..., 1] - d[..., 0]) / d[..., 1]).min()))
    return worst


@pytest.mark.parametrize("directions", ["both", "x_to_y", "y_to_x"])
def test_gradcheck_of_the_composition(directions):
    x, y = sets(2, 5, 7, 126)  # a seed with wide gaps (0.147 and, against y[0] shared, 0.118)
    assert gap(x, y) > 0.05  # gradcheck's 1e-6 probe cannot flip a nearest index
    xt, yt = torch.as_tensor(x).requires_grad_(True), torch.as_tensor(y).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: nr.chamfer_distance_torch(a, b, directions), (xt, yt))
    shared = torch.as_tensor(y[0]).requires_grad_(True)
    assert gap(x, np.broadcast_to(y[0], y.shape)) > 0.05
    assert torch.autograd.gradcheck(lambda a, b: nr.chamfer_distance_torch(a, b, directions), (xt, shared))


def test_gradient_formula():
    """The stated gradient: direct term g (2/N)(x_i - y_nn(i)), gathered term g (2/M) sum_{nn(j) = i} (x_i - y_j)."""
    x, y = sets(1, 5, 7, 126)
    xt, yt = torch.as_tensor(x).requires_grad_(True), torch.as_tensor(y).requires_grad_(True)
    g = 1.7
    (nr.chamfer_distance_torch(xt, yt) * g).sum().backward()
    nn_xy, nn_yx = brute_nearest(x[0], y[0])[1], brute_nearest(y[0], x[0])[1]
    gx, gy = np.zeros((5, 3)), np.zeros((7, 3))
    for i in range(5):
        gx[i] += g * 2 / 5 * (x[0, i] - y[0, nn_xy[i]])
        gy[nn_xy[i]] += g * 2 / 5 * (y[0, nn_xy[i]] - x[0, i])
    for j in range(7):
        gy[j] += g * 2 / 7 * (y[0, j] - x[0, nn_yx[j]])
        gx[nn_yx[j]] += g * 2 / 7 * (x[0, nn_yx[j]] - y[0, j])
    assert np.allclose(xt.grad[0].numpy(), gx, rtol=1e-12, atol=1e-15)
    assert np.allclose(yt.grad[0].numpy(), gy, rtol=1e-12, atol=1e-15)


# ---- sample_points_torch ----
def degenerate_mesh():
    """Icosphere L1 with a zero-area face (three collinear vertices) and a repeated-index face inserted
    in the middle, and a repeated-index face at the end."""
    v, f = synthetic.icosphere(1)
    v = np.concatenate([v, [[2., 0., 0.], [3., 0., 0.], [4., 0., 0.]]]).astype(np.float64)
    n = len(v) - 3
    f = np.concatenate([f[:9], [[n, n + 1, n + 2]], [[4, 4, 7]], f[9:], [[1, 2, 1]]]).astype(np.int32)
    return v, f, (9, 10, len(f) - 1)


def areas64(v, f):
    tri = v[f]
    return 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=-1)


def test_face_selection_against_a_python_loop():
    v, f, dead = degenerate_mesh()
    B, S = 2, 400
    vb = np.stack([v, 1.5 * v + 0.1])
    u = np.random.RandomState(5).uniform(0, 1, (B, S, 3))
    pts, face, w = nr.sample_points_torch(torch.as_tensor(vb), f, S, u=torch.as_tensor(u), return_faces=True)
    assert pts.shape == (B, S, 3) and face.shape == (B, S) and face.dtype == torch.int32 and w.shape == (B, S, 3)
    for b in range(B):
        a = areas64(vb[b], f)
        assert all(a[k] == 0 for k in dead)
        c = np.cumsum(a)
        for s in range(S):
            want = next(k for k in range(len(f)) if c[k] > u[b, s, 0] * c[-1])
            assert int(face[b, s]) == want
    assert not np.isin(face.numpy(), dead).any()
    # weights: non-negative, sum to 1, the stated formula; points: the weighted corner sum
    r = np.sqrt(u[..., 1])
    want_w = np.stack([1 - r, r * (1 - u[..., 2]), r * u[..., 2]], -1)
    assert np.allclose(w.numpy(), want_w, rtol=0, atol=1e-15) and float(w.min()) >= 0.
    assert float((w.sum(-1) - 1).abs().max()) <= 1e-15
    for b in range(B):
        corners = vb[b][f[face[b].numpy()]]
        assert np.allclose(pts[b].numpy(), (want_w[b][..., None] * corners).sum(1), rtol=0, atol=1e-14)


def test_edge_draws_and_zero_area_items():
    v, f, dead = degenerate_mesh()
    # u0 = 0 takes the first face of positive area even behind a zero-area face 0
    f0 = np.concatenate([[[1, 1, 2]], f]).astype(np.int32)
    u = torch.zeros((1, 3, 3), dtype=torch.float64)
    u[0, 1, 0] = 1 - 2 ** -53
    u[0, 2, 0] = 0.5
    face = nr.sample_points_torch(torch.as_tensor(v)[None], f0, 3, u=u, return_faces=True)[1]
    assert int(face[0, 0]) == 1
    assert int(face[0, 1]) == len(f0) - 2  # the last face of positive area, not the dead tail
    # an item without area: no error, face F - 1
    flat = np.zeros((1,) + v.shape)
    pts, face, _ = nr.sample_points_torch(torch.as_tensor(flat), f, 5, return_faces=True,
                                          generator=torch.Generator().manual_seed(1))
    assert face.tolist() == [[len(f) - 1] * 5] and float(pts.abs().max()) == 0.


def test_points_lie_inside_the_triangle():
    tri = np.array([[0.2, 0.1, 0.], [1.3, 0.4, 0.5], [0.1, 1.1, -0.3]])
    g = (np.arange(40) + 0.5) / 40
    u = np.stack(np.meshgrid([0.5], g, g, indexing="ij"), -1).reshape(1, -1, 3)
    pts = nr.sample_points_torch(torch.as_tensor(tri), np.array([[0, 1, 2]], np.int32), u.shape[1], u=torch.as_tensor(u[0]))
    assert pts.shape == (1600, 3)
    # barycentric coordinates of every point by least squares: inside, and on the triangle's plane
    A = np.concatenate([tri.T, np.ones((1, 3))])
    bary = np.linalg.lstsq(A, np.concatenate([pts.numpy().T, np.ones((1, len(pts)))]), rcond=None)[0]
    assert float(np.abs(A @ bary - np.concatenate([pts.numpy().T, np.ones((1, len(pts)))])).max()) <= 1e-12
    assert float(bary.min()) >= -1e-12 and float(bary.max()) <= 1 + 1e-12
    # area-uniform: the centroid of the grid's points is the triangle's to the grid's resolution
    assert float(np.abs(pts.numpy().mean(0) - tri.mean(0)).max()) <= 2e-3


def test_vertex_gradient_is_the_index_add_of_the_weights():
    v, f = synthetic.icosphere(1)
    B, S = 2, 300
    vb = torch.as_tensor(np.stack([v, 0.7 * v]).astype(np.float64)).requires_grad_(True)
    u = torch.as_tensor(np.random.RandomState(2).uniform(0, 1, (B, S, 3)))
    pts, face, w = nr.sample_points(vb, f, S, u=u, return_faces=True)
    assert not face.requires_grad and not w.requires_grad
    up = torch.as_tensor(np.random.RandomState(3).normal(size=(B, S, 3)))
    pts.backward(up)
    want = torch.zeros_like(vb)
    corners = torch.as_tensor(f).long()[face.long()]
    for b in range(B):
        for k in range(3):
            want[b].index_add_(0, corners[b, :, k], w[b, :, k, None] * up[b])
    assert float((vb.grad - want).abs().max()) <= 1e-14
    # the same draws from the same generator seed
    a = nr.sample_points(vb.detach(), f, 7, generator=torch.Generator().manual_seed(11))
    b = nr.sample_points(vb.detach(), f, 7, generator=torch.Generator().manual_seed(11))
    assert torch.equal(a, b) and a.shape == (B, 7, 3)
    assert nr.sample_points(vb.detach()[0], f, 7).shape == (7, 3)


# ---- the C entry points and the Python-level errors ----
def test_abi_rejects_bad_point_loss_arguments():
    """Argument validation of the C entry points runs before any launch (no GPU touched)."""
    L = _lib.lib()
    p = 4096  # a non-null pointer value; never dereferenced on these paths
    big = 1 << 40
    assert L.nr_chamfer_workspace_bytes(0, 5, 5, 3) == 0 and L.nr_chamfer_workspace_bytes(2, 0, 5, 3) == 0
    need = L.nr_chamfer_workspace_bytes(2, 5, 7, 3)
    assert need >= 2 * (5 + 7) * 4 and L.nr_chamfer_workspace_bytes(2, 5, 7, 1) < need
    assert L.nr_chamfer_workspace_bytes(2, 3, 2500, 1) > L.nr_chamfer_workspace_bytes(2, 3, 1000, 1)  # the split's partials

    def fwd(x=p, y=p, B=2, N=5, M=7, dirs=3, ixy=p, iyx=p, loss=p, ws=p, ws_bytes=big):
        return L.nr_chamfer_forward(x, y, 21, B, N, M, dirs, ixy, iyx, None, None, loss, ws, ws_bytes, None)

    def err():
        return L.nr_last_error()

    assert fwd(N=0) == 1 and b"empty point set" in err() and b"N=0" in err()
    assert fwd(M=0) == 1 and b"empty point set" in err() and b"M=0" in err()
    assert fwd(N=-3) == 1 and fwd(B=-1) == 1 and b"batch size" in err()
    assert fwd(dirs=0) == 1 and b"directions" in err()
    assert fwd(dirs=4) == 1
    assert fwd(x=None) == 1 and b"null x or y" in err()
    assert fwd(y=None) == 1 and b"null x or y" in err()
    assert fwd(ixy=None) == 1 and b"null index" in err()
    assert fwd(iyx=None) == 1 and b"null index" in err()
    assert fwd(loss=None) == 1 and b"null loss" in err()
    assert fwd(ws=None) == 1 and b"workspace" in err()
    assert fwd(ws_bytes=need - 1) == 1 and b"workspace" in err()
    assert fwd(B=70000) == 1 and b"65535" in err()
    assert fwd(B=0) == 0  # nothing to do
    assert L.nr_chamfer_forward(p, p, -1, 2, 5, 7, 3, p, p, None, None, p, p, big, None) == 1 and b"stride" in err()

    def bwd(x=p, y=p, ixy=p, iyx=p, g=p, B=2, N=5, M=7, dirs=3, gx=p, gy=p):
        return L.nr_chamfer_backward(x, y, 21, ixy, iyx, g, B, N, M, dirs, gx, gy, None)

    assert bwd(N=0) == 1 and b"empty point set" in err()
    assert bwd(M=0) == 1 and b"empty point set" in err()
    assert bwd(x=None) == 1 and bwd(y=None) == 1 and bwd(g=None) == 1 and b"null x, y or grad_loss" in err()
    assert bwd(ixy=None) == 1 and b"null index" in err()
    assert bwd(iyx=None) == 1 and b"null index" in err()
    assert bwd(gx=None, gy=None) == 0 and bwd(B=0) == 0  # nothing to do

    assert L.nr_sample_points_workspace_bytes(0, 5) == 0 and L.nr_sample_points_workspace_bytes(2, 0) == 0
    assert L.nr_sample_points_workspace_bytes(3, 320) >= 3 * 320 * 4

    def sample(v=p, f=p, u=p, B=2, V=12, F=20, S=8, pts=p, face=p, w=p, ws=p, ws_bytes=big):
        return L.nr_sample_points_forward(v, f, u, B, V, F, S, pts, face, w, ws, ws_bytes, None)

    assert sample(S=0) == 1 and b"no samples" in err() and b"S=0" in err()
    assert sample(S=-1) == 1
    assert sample(F=0) == 1 and b"no faces" in err()
    assert sample(V=0) == 1 and b"no faces" in err()
    assert sample(B=-1) == 1 and b"bad sizes" in err()
    for name in ("v", "f", "u", "pts", "face", "w"):
        assert sample(**{name: None}) == 1 and b"null pointer" in err()
    assert sample(ws=None) == 1 and b"workspace" in err()
    assert sample(ws_bytes=2 * 20 * 4 - 1) == 1 and b"workspace" in err()
    assert sample(B=0) == 0

    def sample_bwd(f=p, face=p, w=p, g=p, B=2, V=12, F=20, S=8, gv=p):
        return L.nr_sample_points_backward(f, face, w, g, B, V, F, S, gv, None)

    assert sample_bwd(S=0) == 1 and b"no samples" in err()
    for name in ("f", "face", "w", "g", "gv"):
        assert sample_bwd(**{name: None}) == 1 and b"null pointer" in err()
    assert sample_bwd(B=0) == 0


def test_python_level_errors():
    x, y = (torch.as_tensor(t) for t in sets(2, 5, 7))
    for fn in (nr.chamfer_distance, nr.chamfer_distance_torch, nr.nearest_points, nr.nearest_points_torch):
        with pytest.raises(ValueError, match="empty"):
            fn(x[:, :0], y)
        with pytest.raises(ValueError, match="empty"):
            fn(x, y[:, :0])
        with pytest.raises(ValueError, match="empty"):
            fn(x, y[0, :0])
        with pytest.raises(ValueError):
            fn(x[..., :2], y)  # wrong last dimension
        with pytest.raises(ValueError):
            fn(x, torch.zeros(2, 7, 4, dtype=torch.float64))
        with pytest.raises(ValueError, match="batch sizes"):
            fn(x, torch.cat([y, y[:1]]))
        with pytest.raises(ValueError):
            fn(x[0], y)  # a single x against a batched y
        with pytest.raises(ValueError):
            fn(x.numpy(), y)
    for fn in (nr.chamfer_distance, nr.chamfer_distance_torch):
        with pytest.raises(ValueError, match="directions"):
            fn(x, y, "x_to_x")
    with pytest.raises(ValueError):
        nr.ChamferLoss(directions="neither")
    v, f = synthetic.icosphere(0)
    vt = torch.as_tensor(v.astype(np.float64))
    for fn in (nr.sample_points, nr.sample_points_torch):
        for bad in ([[0, 1, len(v)]], [[0, -1, 2]]):
            with pytest.raises(IndexError):
                fn(vt, np.concatenate([f, bad]).astype(np.int32), 4)
        with pytest.raises(ValueError):
            fn(vt, f, 0)
        with pytest.raises(ValueError):
            fn(vt, np.zeros((0, 3), np.int32), 4)
        with pytest.raises(ValueError):
            fn(vt[:, :2], f, 4)
        with pytest.raises(ValueError):
            fn(vt[None], f, 4, u=torch.zeros(1, 5, 3, dtype=torch.float64))
        with pytest.raises(ValueError):
            fn(vt[None].expand(2, -1, -1), f, 4, u=torch.zeros(4, 3, dtype=torch.float64))


def test_cpu_and_float64_run_the_composition(monkeypatch):
    """Dispatch: nothing on the CPU touches the HIP library."""
    def no_library():
        raise AssertionError("the HIP library was loaded")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(point_loss.ChamferFunction, "apply", lambda *a: no_library())
    monkeypatch.setattr(point_loss.SamplePointsFunction, "apply", lambda *a: no_library())
    v, f = grid_fin()
    for dtype in (torch.float32, torch.float64):
        x, y = (torch.as_tensor(t, dtype=dtype) for t in sets(2, 5, 7))
        x.requires_grad_(True)
        loss = nr.chamfer_distance(x, y)
        assert loss.dtype == dtype and torch.equal(loss, nr.chamfer_distance_torch(x, y))
        loss.sum().backward()
        assert bool(torch.isfinite(x.grad).all())
        assert nr.nearest_points(x, y)[0].dtype == dtype
        pts = nr.sample_points(torch.as_tensor(v, dtype=dtype), f, 9)
        assert pts.dtype == dtype and pts.shape == (9, 3)
    assert point_loss.CHAMFER_TILE == _lib.NR_CHAMFER_TILE and point_loss.CHAMFER_TILE > 0

"""edge_length_loss and cot_laplacian_loss on the host: the corner CSR against a loop over the faces,
the torch compositions against plain Python loops, the properties of the definitions (equal weights on
the regular icosahedron, scaling, the clamp, the zero-length edge) and the C entry points' argument
checks."""
import math
import os
import re

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import _lib, mesh_loss, synthetic, topology
from mesh_loss_cases import grid_fin, hinge, jitter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KITE_V = np.array([[0., 0., 0.], [1., 0., 0.], [0.5, 0.1, 0.], [0.5, -0.1, 0.02]])
KITE_F = np.array([[0, 1, 2], [1, 0, 3]], np.int32)


def corner_lists(t):
    """{(i, j): [corners]} of a topology's corner CSR, one entry per neighbour entry."""
    off, idx = t.nbr_offsets.numpy(), t.nbr_index.numpy()
    coff, corners = t.nbr_corner_offsets.numpy(), t.nbr_corners.numpy()
    assert coff.dtype == np.int32 and corners.dtype == np.int32
    assert coff.shape == (idx.shape[0] + 1,) and coff[0] == 0 and coff[-1] == corners.shape[0]
    rows = np.repeat(np.arange(t.num_vertices), np.diff(off))
    return {(int(i), int(j)): corners[coff[e]:coff[e + 1]].tolist() for e, (i, j) in enumerate(zip(rows, idx))}


def brute_corner_lists(faces):
    want = {}
    for f, face in enumerate(np.asarray(faces).tolist()):
        if len(set(face)) < 3:
            continue
        for k in range(3):
            i, j = face[(k + 1) % 3], face[(k + 2) % 3]
            want.setdefault((i, j), []).append(3 * f + k)
            want.setdefault((j, i), []).append(3 * f + k)
    return {e: sorted(c) for e, c in want.items()}


def test_corner_csr_of_grid_fin():
    v, f = grid_fin()
    t = nr.mesh_topology(f, 27)
    got = corner_lists(t)
    assert got == brute_corner_lists(f)
    assert len(got[(12, 13)]) == 3 and got[(12, 13)][-1] == 3 * 32 + 2  # the fin's corner at vertex 25
    off = t.nbr_offsets.numpy()
    assert off[27] == off[26]  # the isolated vertex: an empty row, so no entry and no corner
    sizes = [len(c) for c in got.values()]
    assert sizes.count(1) == 2 * t.num_boundary_edges and sizes.count(3) == 2 * t.num_nonmanifold_edges
    assert sizes.count(2) == 2 * t.num_edges
    for (i, j), c in got.items():
        assert c == sorted(c) and len(set(c)) == len(c) and got[(j, i)] == c
    assert t.num_all_edges == t.nbr_index.numel() // 2 == t.num_edges + t.num_boundary_edges + t.num_nonmanifold_edges


def test_corner_csr_special_inputs():
    none = nr.mesh_topology(np.zeros((0, 3), np.int32), 3)
    assert none.num_all_edges == 0 and none.nbr_corner_offsets.tolist() == [0] and none.nbr_corners.numel() == 0
    # one degenerate face in the middle: its corners 3, 4, 5 appear nowhere, the later faces keep their numbers
    f = np.array([[0, 1, 2], [3, 3, 5], [2, 1, 4], [5, 0, 2]], np.int32)
    t = nr.mesh_topology(f, 6)
    got = corner_lists(t)
    assert got == brute_corner_lists(f)
    assert not {3, 4, 5} & set(t.nbr_corners.tolist())
    assert got[(1, 2)] == [0, 8] and got[(0, 2)] == [1, 9]
    assert t.num_all_edges == t.nbr_index.numel() // 2 == 7
    assert (3, 5) not in got
    # the five arrays and what build_topology returns are what they were
    assert topology.MeshTopology.FIELDS == ("nbr_offsets", "nbr_index", "edges", "edge_offsets", "edge_slots")
    arrays, boundary, nonmanifold = topology.build_topology(f, 6)
    assert len(arrays) == 5 and (boundary, nonmanifold) == (5, 0)
    # built lazily, once, and shared by the copies; a topology without faces cannot build it
    assert t._corners is not None and nr.mesh_topology(f.copy(), 6)._corners is None
    bare = nr.MeshTopology(list(t), 6, boundary, nonmanifold)
    assert bare.num_all_edges == 7
    with pytest.raises(ValueError):
        bare.corner_csr()


def loop_edge_loss(x, faces, target):
    """Per item: the sum over the distinct undirected edges, as a Python loop."""
    edges = sorted({tuple(sorted((face[a], face[b]))) for face in np.asarray(faces).tolist() if len(set(face)) == 3
                    for a, b in ((0, 1), (1, 2), (2, 0))})
    return [sum((math.sqrt(sum((float(xb[i, k]) - float(xb[j, k])) ** 2 for k in range(3))) - target) ** 2 for i, j in edges)
            for xb in x], edges


def loop_cot_loss(x, faces, eps=1e-12, skip=()):
    """Per item: the cotangent Laplacian loss as a Python loop over faces, edges and vertices; `skip` names
    undirected edges left out of every row."""
    out = []
    for xb in x.numpy():
        cot = {}
        for face in np.asarray(faces).tolist():
            if len(set(face)) < 3:
                continue
            for k in range(3):
                p, q, r = xb[face[k]], xb[face[(k + 1) % 3]], xb[face[(k + 2) % 3]]
                a, b = q - p, r - p
                c = 0.5 * float(a @ b) / math.sqrt(float(np.cross(a, b) @ np.cross(a, b)) + eps)
                key = tuple(sorted((face[(k + 1) % 3], face[(k + 2) % 3])))
                cot[key] = cot.get(key, 0.) + c
        loss = 0.
        for i in range(xb.shape[0]):
            W, s = 0., np.zeros(3)
            for (a, b), c in sorted(cot.items()):
                if i in (a, b) and (a, b) not in skip:
                    w = max(0., c)
                    W += w
                    s += w * xb[b if i == a else a]
            if W > 1e-6:
                loss += float(((xb[i] - s / W) ** 2).sum())
        out.append(loss)
    return out


@pytest.mark.parametrize("name", ["hinge", "grid_fin"])
def test_compositions_match_python_loops(name):
    v, f = hinge(2.2) if name == "hinge" else grid_fin()
    x = torch.as_tensor(jitter(v, 2, 0.02, 5))
    for target in (0., 0.1):
        got = nr.edge_length_loss_torch(x, f, target)
        want, edges = loop_edge_loss(x, f, target)
        assert got.shape == (2,) and got.dtype == torch.float64
        assert len(edges) == nr.mesh_topology(f, v.shape[0]).num_all_edges
        assert np.allclose(got.numpy(), want, rtol=1e-12, atol=0)
    got = nr.cot_laplacian_loss_torch(x, f)
    assert got.shape == (2,) and got.dtype == torch.float64
    assert np.allclose(got.numpy(), loop_cot_loss(x, f), rtol=1e-11, atol=0)
    # the public names run the compositions off the GPU, for float32 too
    for dtype in (torch.float64, torch.float32):
        y = x.to(dtype)
        assert torch.equal(nr.edge_length_loss(y, f, 0.1), nr.edge_length_loss_torch(y, f, 0.1))
        assert torch.equal(nr.cot_laplacian_loss(y, f), nr.cot_laplacian_loss_torch(y, f))
        assert nr.cot_laplacian_loss(y, f).dtype == dtype


def test_edge_gradient_matches_the_formula():
    """grad v_i = 2 g sum_j (len - L) / len (v_i - v_j) over all of N(i)."""
    v, f = grid_fin()
    x = torch.as_tensor(jitter(v, 1, 0.02, 8)).requires_grad_(True)
    nr.edge_length_loss_torch(x, f, 0.1).sum().backward()
    _, edges = loop_edge_loss(x.detach(), f, 0.1)
    want = np.zeros((27, 3))
    xb = x.detach().numpy()[0]
    for i, j in edges:
        d = xb[i] - xb[j]
        n = math.sqrt(float(d @ d))
        want[i] += 2 * (n - 0.1) / n * d
        want[j] -= 2 * (n - 0.1) / n * d
    assert np.allclose(x.grad.numpy()[0], want, rtol=1e-10, atol=1e-14)
    assert float(x.grad[0, 26].abs().max()) == 0.


def test_cot_gradient_treats_the_weights_as_constants():
    """grad v_k = 2 (delta_k - sum_i w_ki Winv_i delta_i) with the forward's weights, on grid_fin."""
    v, f = grid_fin()
    x = torch.as_tensor(jitter(v, 1, 0.02, 8)).requires_grad_(True)
    nr.cot_laplacian_loss_torch(x, f).sum().backward()
    t = nr.mesh_topology(f, 27)
    rows, cols = (a.numpy() for a in t.composition_index()[:2])
    w = mesh_loss.cot_weights_torch(x.detach(), t)[0].numpy()
    xb = x.detach().numpy()[0]
    W = np.bincount(rows, w, 27)
    A = np.zeros((27, 27))
    A[rows, cols] = w
    ok = W > 1e-6
    M = (np.eye(27) - A / np.where(ok, W, 1.)[:, None]) * ok[:, None]  # delta = M v
    want = 2 * M.T @ (M @ xb)
    assert np.allclose(x.grad.numpy()[0], want, rtol=1e-10, atol=1e-14)
    assert not ok[26] and ok[:26].all() and float(x.grad[0, 26].abs().max()) == 0.


def test_regular_icosahedron_has_equal_weights():
    v, f = synthetic.icosphere(0)
    x = torch.as_tensor(np.asarray(v, np.float64))[None]
    w = mesh_loss.cot_weights_torch(x, nr.mesh_topology(f, 12))
    # 2 * 0.5 cot 60 = 0.577 on every edge, up to the float32 rounding of the vertices synthetic.icosphere returns
    assert float((w.max() - w.min()) / w.max()) <= 1e-6 and float(w.min()) > 0.5
    cot, uniform = nr.cot_laplacian_loss_torch(x, f), nr.laplacian_loss_torch(x, f)
    assert float(uniform) > 0.1 and abs(float(cot) - float(uniform)) <= 1e-12 * float(uniform)


def test_laplacians_scale_with_the_square():
    v, f = grid_fin()
    x = torch.as_tensor(jitter(v, 2, 0.02, 4))
    for s in (0.25, 3.):
        # eps scales with length^4; without that the definition is scale invariant only up to eps
        assert np.allclose(nr.cot_laplacian_loss_torch(s * x, f, eps=1e-12 * s ** 4).numpy(),
                           s * s * nr.cot_laplacian_loss_torch(x, f).numpy(), rtol=1e-12, atol=0)
        assert np.allclose(nr.cot_laplacian_loss_torch(s * x, f).numpy(), s * s * nr.cot_laplacian_loss_torch(x, f).numpy(),
                           rtol=1e-6, atol=0)  # eps against |a x b|^2 >= 1e-5 here
        assert np.allclose(nr.laplacian_loss_torch(s * x, f).numpy(), s * s * nr.laplacian_loss_torch(x, f).numpy(),
                           rtol=1e-12, atol=0)


def test_kite_clamps_the_obtuse_edge():
    """Both angles opposite edge 0-1 are about 157 degrees: its weight is clamped to 0, so the loss and the
    gradient are those of the composition with that edge taken out of the rows of 0 and 1."""
    t = nr.mesh_topology(KITE_F, 4)
    x = torch.as_tensor(KITE_V)[None].clone().requires_grad_(True)
    rows, cols = t.composition_index()[:2]
    raw = {}
    for (i, j), c in corner_lists(t).items():
        raw[(i, j)] = sum(loop_half_cot(KITE_V, KITE_F, corner) for corner in c)
    assert -2.6 < raw[(0, 1)] < -2.2 and raw[(0, 1)] == raw[(1, 0)]
    w = mesh_loss.cot_weights_torch(x.detach(), t)[0]
    e01 = int(((rows == 0) & (cols == 1)).nonzero())
    assert float(w[e01]) == 0. and int((w == 0).sum()) == 2 and float(w[w > 0].min()) > 0.1
    loss = nr.cot_laplacian_loss_torch(x, t)
    loss.sum().backward()
    # the same composition over the rows without 0-1
    keep = ~(((rows == 0) & (cols == 1)) | ((rows == 1) & (cols == 0)))
    y = torch.as_tensor(KITE_V)[None].clone().requires_grad_(True)
    r, c, wk = rows[keep], cols[keep], w[keep][None]
    W = torch.zeros((1, 4), dtype=torch.float64).index_add_(1, r, wk)
    total = torch.zeros_like(y).index_add_(1, r, wk[:, :, None] * y.index_select(1, c))
    delta = y - total / W[:, :, None]
    want = (delta * delta).sum((1, 2))
    want.sum().backward()
    assert torch.equal(loss, want) and torch.equal(x.grad, y.grad)
    assert np.allclose(loss.detach().numpy(), loop_cot_loss(x.detach(), KITE_F, skip={(0, 1)}), rtol=1e-12, atol=0)
    assert float(loss.detach()) > 0.1  # 0 and 1 are pulled toward 2 and 3: nothing like the unclamped mean


def loop_half_cot(v, faces, corner):
    f, k = divmod(corner, 3)
    p, q, r = (v[faces[f][(k + n) % 3]] for n in range(3))
    a, b = q - p, r - p
    n = np.cross(a, b)
    return 0.5 * float(a @ b) / math.sqrt(float(n @ n) + 1e-12)


def test_zero_length_edge():
    """Vertices 1 and 3 coincide and share an edge: it adds target^2 to the loss and nothing to the gradient."""
    v = np.array([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.], [1., 0., 0.]])
    f = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    x = torch.as_tensor(v).requires_grad_(True)
    loss = nr.edge_length_loss(x, f, 0.3)
    others = [(0, 1), (0, 2), (1, 2), (2, 3)]
    want = 0.09 + sum((float(np.linalg.norm(v[i] - v[j])) - 0.3) ** 2 for i, j in others)
    assert loss.ndim == 0 and abs(float(loss.detach()) - want) <= 1e-14
    loss.backward()
    assert bool(torch.isfinite(x.grad).all())
    grad = np.zeros((4, 3))
    for i, j in others:
        d = v[i] - v[j]
        n = float(np.linalg.norm(d))
        grad[i] += 2 * (n - 0.3) / n * d
        grad[j] -= 2 * (n - 0.3) / n * d
    assert np.allclose(x.grad.numpy(), grad, rtol=1e-12, atol=1e-15)
    with pytest.raises(ValueError):
        nr.edge_length_loss(x, f, -0.1)


def test_shapes_average_and_modules():
    v, f = synthetic.icosphere(1)
    V = v.shape[0]
    x = torch.as_tensor(jitter(v, 3, 0.02, 5))
    for fn, mod, kw in ((nr.edge_length_loss, nr.EdgeLengthLoss, {"target_length": 0.2}),
                        (nr.cot_laplacian_loss, nr.CotLaplacianLoss, {"eps": 1e-10})):
        per_item = fn(x, f, **kw)
        assert per_item.shape == (3,)
        assert fn(x[1], f, **kw).ndim == 0 and float(fn(x[1], f, **kw)) == float(per_item[1])
        avg = fn(x, f, average=True, **kw)
        assert avg.ndim == 0 and abs(float(avg) - float(per_item.mean())) <= 1e-15
        assert torch.equal(mod(f, V, **kw)(x), per_item)
        assert torch.equal(mod(f, V, average=True, **kw)(x), avg)
        assert not torch.equal(fn(x, f), per_item)  # the keyword reached the loss
        with pytest.raises(ValueError):
            fn(x, nr.mesh_topology(f, V + 1))
        y = x[:, :3].clone().requires_grad_(True)
        none = fn(y, np.zeros((0, 3), np.int32))
        assert none.tolist() == [0., 0., 0.]
        none.sum().backward()
        assert float(y.grad.abs().max()) == 0.


def test_cpu_runs_the_composition(monkeypatch):
    def no_library():
        raise AssertionError("the HIP library was loaded")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(mesh_loss.EdgeLengthFunction, "apply", lambda *a: no_library())
    monkeypatch.setattr(mesh_loss.CotLaplacianFunction, "apply", lambda *a: no_library())
    v, f = synthetic.icosphere(1)
    x = torch.as_tensor(jitter(v, 2, 0.02, 9), dtype=torch.float32).requires_grad_(True)
    (nr.edge_length_loss(x, f, 0.1) + nr.cot_laplacian_loss(x, f)).sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0.


def test_abi_rejects_bad_regularizer_arguments():
    """Argument validation of the C entry points runs before any launch (no GPU touched)."""
    L = _lib.lib()
    p = 4096  # a non-null pointer value; never dereferenced on these paths
    err = L.nr_last_error
    # edge length
    assert L.nr_edge_length_forward(p, p, p, -1, 3, 0.1, p, None, 0, None) == 1 and b"bad sizes" in err()
    assert L.nr_edge_length_forward(p, p, p, 1, 3, 0.1, None, None, 0, None) == 1 and b"null loss" in err()
    assert L.nr_edge_length_forward(p, p, p, 1, 3, -0.5, p, p, 256, None) == 1 and b"bad target_length" in err()
    assert L.nr_edge_length_forward(p, p, p, 1, 3, float("nan"), p, p, 256, None) == 1 and b"bad target_length" in err()
    assert L.nr_edge_length_forward(None, p, p, 1, 3, 0.1, p, p, 256, None) == 1 and b"null vertices" in err()
    assert L.nr_edge_length_forward(p, p, p, 1, 3, 0.1, p, None, 0, None) == 3
    assert L.nr_edge_length_forward(p, p, p, 1, 300, 0.1, p, p, 4, None) == 3  # two blocks need 8 bytes (256 aligned)
    assert L.nr_edge_length_forward(p, p, p, 2 ** 30, 2 ** 30, 0.1, p, p, 1 << 40, None) == 1 and b"too many" in err()
    assert L.nr_edge_length_forward(p, p, p, 0, 3, 0.1, None, None, 0, None) == 0  # B = 0: nothing to do
    assert L.nr_edge_length_backward(None, p, p, p, 1, 3, 0.1, p, None) == 1 and b"null pointer" in err()
    assert L.nr_edge_length_backward(p, p, p, p, 1, 3, 0.1, None, None) == 1
    assert L.nr_edge_length_backward(p, p, p, p, 1, 3, -1., p, None) == 1 and b"bad target_length" in err()
    assert L.nr_edge_length_backward(p, p, p, p, 1, -3, 0.1, p, None) == 1 and b"bad sizes" in err()
    assert L.nr_edge_length_backward(p, p, p, p, 0, 3, 0.1, p, None) == 0
    # cotangent Laplacian: the workspace is the partial sums [B][ceil(V / 256)], then [B][3 F] floats, each 256-aligned
    wb = L.nr_cot_laplacian_workspace_bytes
    assert wb(0, 5, 5) == 0 and wb(2, 0, 5) == 0 and wb(2, 5, -1) == 0
    assert wb(2, 257, 0) == 256 and wb(2, 257, 10) == 256 + 256 and wb(64, 25000, 50000) == 25088 + 64 * 50000 * 12
    big = 1 << 40

    def fwd(vertices=p, faces=p, off=p, idx=p, coff=p, corners=p, B=1, V=4, F=2, nnz=10, eps=1e-12, loss=p, ws=p, nbytes=big):
        return L.nr_cot_laplacian_forward(vertices, faces, off, idx, coff, corners, B, V, F, nnz, eps, None, None, None, loss,
                                          ws, nbytes, None)
    assert fwd(B=-1) == 1 and b"bad sizes" in err()
    assert fwd(F=-1) == 1 and b"bad sizes" in err()
    assert fwd(nnz=-1) == 1 and b"bad sizes" in err()
    assert fwd(F=2 ** 30) == 1 and b"2^31" in err()
    assert fwd(loss=None) == 1 and b"null loss" in err()
    assert fwd(eps=-1.) == 1 and b"bad eps" in err()
    assert fwd(eps=float("inf")) == 1 and b"bad eps" in err()
    assert fwd(V=0) == 1 and b"without vertices" in err()
    assert fwd(vertices=None) == 1 and b"null vertices" in err()
    assert fwd(corners=None) == 1 and fwd(coff=None) == 1 and fwd(idx=None) == 1 and fwd(faces=None) == 1
    assert fwd(F=0) == 1  # neighbours without faces
    assert fwd(ws=None, nbytes=0) == 3
    assert fwd(nbytes=wb(1, 4, 2) - 1) == 3
    assert fwd(B=0, loss=None) == 0
    assert L.nr_cot_laplacian_backward(None, p, p, p, p, p, 1, 4, 10, p, None) == 1 and b"null pointer" in err()
    assert L.nr_cot_laplacian_backward(p, p, None, p, p, p, 1, 4, 10, p, None) == 1
    assert L.nr_cot_laplacian_backward(p, None, p, p, p, p, 1, 4, 10, p, None) == 1 and b"null w" in err()
    assert L.nr_cot_laplacian_backward(p, p, p, p, p, p, 1, 4, -1, p, None) == 1 and b"bad sizes" in err()
    assert L.nr_cot_laplacian_backward(p, p, p, p, p, p, 0, 4, 10, p, None) == 0
    assert L.nr_cot_laplacian_backward(p, p, p, p, p, p, 1, 0, 0, p, None) == 0


def test_cot_min_weight_is_the_librarys():
    """The binding's NR_COT_MIN_WEIGHT is the value the library is compiled with: the header's."""
    header = open(os.path.join(ROOT, "include", "nr_raster.h")).read()
    value, = re.findall(r"^#define NR_COT_MIN_WEIGHT (\S+)f$", header, re.M)
    assert float(value) == _lib.NR_COT_MIN_WEIGHT == mesh_loss.COT_MIN_WEIGHT == 1e-6
    source = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "nr_mesh_loss.h")).read()
    assert "ML_COT_MIN_WEIGHT = NR_COT_MIN_WEIGHT;" in source


def test_example_flags():
    """The fitting examples take the new regularizers by flag, and do what they did without."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("example_scan_fit", os.path.join(ROOT, "examples", "example_scan_fit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parser().parse_args([])
    assert args.laplacian == "uniform" and args.edge_weight == 0.
    args = mod.parser().parse_args(["--laplacian", "cot", "--edge-weight", "0.5"])
    assert args.laplacian == "cot" and args.edge_weight == 0.5
    with pytest.raises(SystemExit):
        mod.parser().parse_args(["--laplacian", "umbrella"])
    source = open(os.path.join(ROOT, "examples", "example_chamfer.py")).read()
    assert "'--edge-weight'" in source and "'--laplacian'" in source

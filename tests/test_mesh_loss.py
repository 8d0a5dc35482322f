"""mesh_loss on the host: the topology (counts, CSR invariants, ignored faces), the torch compositions
against a dense restatement and torch's gradcheck, the hinge values, and the dispatch."""
import math

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import _lib, mesh_loss, synthetic
from mesh_loss_cases import fan, grid_fin, hinge, jitter, teapot


def counts(t):
    return t.num_edges, t.num_boundary_edges, t.num_nonmanifold_edges


def named_mesh(name):
    if name == "teapot":
        return teapot()
    if name == "grid_fin":
        return grid_fin()
    if name == "fan":
        return fan()
    return synthetic.icosphere(int(name[-1]))


def test_topology_counts():
    v, f = teapot()
    assert v.shape == (1292, 3) and f.shape == (2464, 3)
    assert counts(nr.mesh_topology(f, 1292)) == (3636, 120, 0)
    v, f = synthetic.icosphere(2)
    assert counts(nr.mesh_topology(f, v.shape[0])) == (480, 0, 0)


def test_grid_fin_topology():
    v, f = grid_fin()
    assert v.shape == (27, 3) and f.shape == (33, 3)
    t = nr.mesh_topology(f, 27)
    assert counts(t) == (39, 18, 1)
    edges = t.edges.numpy()
    assert not ((edges[:, 0] == 12) & (edges[:, 1] == 13)).any()  # the fin's edge has three faces
    assert int(t.nbr_offsets[27] - t.nbr_offsets[26]) == 0 and int(t.edge_offsets[27] - t.edge_offsets[26]) == 0
    # the isolated vertex: delta = 0, so it neither changes the loss nor takes a gradient
    x = torch.as_tensor(v)[None].clone().requires_grad_(True)
    loss = nr.laplacian_loss(x, t) + nr.flatten_loss(x, t)
    loss.sum().backward()
    assert float(x.grad[0, 26].abs().max()) == 0. and float(x.grad[0, :26].norm(dim=1).min()) > 0.
    moved = x.detach().clone()
    moved[0, 26] += 5.
    assert torch.equal(nr.laplacian_loss(moved, t), nr.laplacian_loss(x.detach(), t))


@pytest.mark.parametrize("name", ["teapot", "grid_fin", "ico2", "fan"])
def test_csr_invariants(name):
    v, f = named_mesh(name)
    V = v.shape[0]
    t = nr.mesh_topology(f, V)
    for x in t:
        assert x.dtype == torch.int32
    off, idx, edges, eoff, slots = (x.numpy().astype(np.int64) for x in t)
    assert off.shape == (V + 1,) and eoff.shape == (V + 1,) and edges.shape == (t.num_edges, 4)
    assert off[0] == 0 and off[-1] == idx.shape[0] and eoff[0] == 0 and eoff[-1] == 4 * t.num_edges
    # every slot once, and under the vertex it names, ascending
    assert np.array_equal(np.sort(slots), np.arange(4 * t.num_edges))
    owner = np.repeat(np.arange(V), np.diff(eoff))
    assert np.array_equal(edges.reshape(-1)[slots], owner)
    for i in range(V):
        assert (np.diff(slots[eoff[i]:eoff[i + 1]]) > 0).all()
    # edge rows: v0 < v1, sorted by (v0, v1), each of the two faces really holds (v0, v1, opposite)
    assert (edges[:, 0] < edges[:, 1]).all()
    assert (np.diff(edges[:, 0] * V + edges[:, 1]) > 0).all()
    face_sets = [frozenset(int(x) for x in row) for row in np.asarray(f)]
    for v0, v1, v2, v3 in edges[:: max(1, len(edges) // 200)]:
        lower = [i for i, s in enumerate(face_sets) if s == {v0, v1, v2}]
        upper = [i for i, s in enumerate(face_sets) if s == {v0, v1, v3}]
        assert lower and upper and min(lower) < max(upper)
    # neighbour lists: ascending without duplicates, no self, symmetric, and exactly the face edges
    rows = np.repeat(np.arange(V), np.diff(off))
    for i in range(V):
        assert (np.diff(idx[off[i]:off[i + 1]]) > 0).all()
    assert (rows != idx).all()
    pairs = set(zip(rows.tolist(), idx.tolist()))
    assert all((j, i) in pairs for i, j in pairs)
    want = set()
    for a, b, c in np.asarray(f).tolist():
        if len({a, b, c}) == 3:
            want |= {(a, b), (b, a), (b, c), (c, b), (a, c), (c, a)}
    assert pairs == want


def test_ignored_faces_and_index_errors():
    v, f = synthetic.icosphere(1)
    V = v.shape[0]
    base = nr.mesh_topology(f, V)
    # a face with a repeated index changes nothing, wherever it stands (the faces after it keep their order)
    extra = np.concatenate([f[:7], [[3, 3, 9]], f[7:], [[5, 2, 5]]]).astype(np.int32)
    t = nr.mesh_topology(extra, V)
    for a, b in zip(base, t):
        assert torch.equal(a, b)
    assert counts(t) == counts(base)
    x = torch.as_tensor(jitter(v, 2, 0.02, 0))
    assert torch.equal(nr.laplacian_loss(x, extra), nr.laplacian_loss(x, f))
    assert torch.equal(nr.flatten_loss(x, extra), nr.flatten_loss(x, f))
    # a duplicate face counts separately: its three edges now have three faces
    dup = nr.mesh_topology(np.concatenate([f, f[:1]]), V)
    assert counts(dup) == (base.num_edges - 3, 0, 3)
    for bad in ([[0, 1, V]], [[0, -1, 2]]):
        with pytest.raises(IndexError):
            nr.mesh_topology(np.concatenate([f, bad]).astype(np.int32), V)
        with pytest.raises(IndexError):
            nr.laplacian_loss(x, torch.as_tensor(np.concatenate([f, bad]).astype(np.int64)))


def test_topology_is_cached_per_tensor():
    v, f = synthetic.icosphere(1)
    ft = torch.as_tensor(f)
    t = nr.mesh_topology(ft, v.shape[0])
    assert nr.mesh_topology(ft, v.shape[0]) is t
    ft[0] = ft[0].flip(0).clone()  # an in-place edit bumps the version: rebuilt
    assert nr.mesh_topology(ft, v.shape[0]) is not t
    assert t.to("cpu") is t


def dense_laplacian_loss(x, faces):
    """|L v|^2 with the dense row-normalised umbrella Laplacian: -1 for every face edge in both
    directions, the row sum (negated) on the diagonal, each row divided by its diagonal."""
    V = x.shape[1]
    L = torch.zeros((V, V), dtype=x.dtype)
    for a, b, c in np.asarray(faces).tolist():
        if len({a, b, c}) == 3:
            for i, j in ((a, b), (b, c), (c, a)):
                L[i, j] = L[j, i] = -1.
    diag = -L.sum(1)
    L[range(V), range(V)] = diag
    L = torch.where(diag[:, None] > 0, L / diag.clamp(min=1)[:, None], torch.zeros_like(L))
    return (torch.matmul(L, x) ** 2).sum((1, 2))


@pytest.mark.parametrize("name", ["teapot", "grid_fin", "ico2"])
def test_composition_matches_dense_form(name):
    v, f = named_mesh(name)
    x = torch.as_tensor(jitter(v, 2, 0.002 if name == "teapot" else 0.02, 3))
    got = nr.laplacian_loss_torch(x, f)
    want = dense_laplacian_loss(x, f)
    assert got.shape == (2,) and got.dtype == torch.float64
    assert float(((got - want).abs() / want.abs()).max()) <= 1e-12


@pytest.mark.parametrize("mesh", ["ico0", "hinge"])
def test_gradcheck_of_the_compositions(mesh):
    v, f = synthetic.icosphere(0) if mesh == "ico0" else hinge(2.2)
    t = nr.mesh_topology(f, v.shape[0])
    x = torch.as_tensor(jitter(v, 2, 0.02, 11)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda y: nr.laplacian_loss_torch(y, t), (x,))
    assert torch.autograd.gradcheck(lambda y: nr.flatten_loss_torch(y, t), (x,))


@pytest.mark.parametrize("phi, want", [(math.pi, 0.), (math.pi / 2, 1.), (0., 4.), (2.0, None), (0.7, None)])
def test_hinge_values(phi, want):
    v, f = hinge(phi)
    want = (math.cos(phi) + 1.) ** 2 if want is None else want
    for dtype in (torch.float64, torch.float32):
        got = nr.flatten_loss(torch.as_tensor(v, dtype=dtype), f)
        assert got.ndim == 0 and got.dtype == dtype
        assert abs(float(got) - want) <= 1e-5
    assert counts(nr.mesh_topology(f, 4)) == (1, 4, 0)
    assert nr.mesh_topology(f, 4).edges.tolist() == [[0, 1, 2, 3]]


def test_shapes_average_and_modules():
    v, f = synthetic.icosphere(1)
    V = v.shape[0]
    x = torch.as_tensor(jitter(v, 3, 0.02, 5))
    for fn, mod in ((nr.laplacian_loss, nr.LaplacianLoss), (nr.flatten_loss, nr.FlattenLoss)):
        per_item = fn(x, f)
        assert per_item.shape == (3,)
        assert fn(x[1], f).ndim == 0 and float(fn(x[1], f)) == float(per_item[1])
        avg = fn(x, f, average=True)
        assert avg.ndim == 0 and abs(float(avg) - float(per_item.mean())) <= 1e-15
        assert torch.equal(mod(f, V)(x), per_item)
        assert torch.equal(mod(f, V, average=True)(x), avg)
    assert float(nr.FlattenLoss(f, V, eps=1e-3)(x)[0]) == float(nr.flatten_loss(x, f, eps=1e-3)[0])
    with pytest.raises(ValueError):
        nr.laplacian_loss(x, nr.mesh_topology(f, V + 1))
    # no faces: zeros, and a zero gradient
    y = x[:, :3].clone().requires_grad_(True)
    none = np.zeros((0, 3), np.int32)
    tot = nr.laplacian_loss(y, none) + nr.flatten_loss(y, none)
    assert tot.tolist() == [0., 0., 0.]
    tot.sum().backward()
    assert float(y.grad.abs().max()) == 0.


def test_abi_rejects_bad_mesh_loss_arguments():
    """Argument validation of the C entry points runs before any launch (no GPU touched)."""
    L = _lib.lib()
    p = 4096  # a non-null pointer value; never dereferenced on these paths
    assert L.nr_mesh_loss_workspace_bytes(0, 5) == 0 and L.nr_mesh_loss_workspace_bytes(2, 0) == 0
    assert L.nr_mesh_loss_workspace_bytes(2, 257) == 256 and L.nr_mesh_loss_workspace_bytes(64, 25000) == 25088
    assert L.nr_laplacian_forward(p, p, p, -1, 3, None, p, None, 0, None) == 1 and b"bad sizes" in L.nr_last_error()
    assert L.nr_laplacian_forward(p, p, p, 1, 3, None, None, None, 0, None) == 1 and b"null loss" in L.nr_last_error()
    assert L.nr_laplacian_forward(p, p, p, 1, 3, None, p, None, 0, None) == 3
    assert L.nr_laplacian_forward(p, p, p, 1, 300, None, p, p, 4, None) == 3  # two blocks need 8 bytes (256 aligned)
    assert L.nr_laplacian_backward(None, p, p, p, 1, 3, p, None) == 1
    assert L.nr_laplacian_backward(p, p, p, p, 0, 3, p, None) == 0  # B = 0: nothing to do
    assert L.nr_flatten_forward(p, p, 1, 4, 2 ** 29, 1e-6, None, p, p, 1 << 40, None) == 1 and b"2^31" in L.nr_last_error()
    assert L.nr_flatten_forward(p, p, 1, 4, 1, -1., None, p, p, 256, None) == 1 and b"bad eps" in L.nr_last_error()
    assert L.nr_flatten_forward(p, p, 1, 4, 1, 1e-6, None, p, None, 0, None) == 3
    assert L.nr_flatten_forward(p, p, 1, 0, 1, 1e-6, None, p, p, 256, None) == 1  # edges without vertices
    assert L.nr_flatten_backward(p, None, p, p, 1, 4, 1, p, None) == 1
    assert L.nr_flatten_backward(None, p, p, p, 1, 4, 1, p, None) == 1 and b"null records" in L.nr_last_error()


def test_cpu_and_float64_run_the_composition(monkeypatch):
    """Dispatch: nothing on the CPU touches the HIP library."""
    def no_library():
        raise AssertionError("the HIP library was loaded")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(mesh_loss.LaplacianFunction, "apply", lambda *a: no_library())
    monkeypatch.setattr(mesh_loss.FlattenFunction, "apply", lambda *a: no_library())
    v, f = synthetic.icosphere(1)
    for dtype in (torch.float32, torch.float64):
        x = torch.as_tensor(jitter(v, 2, 0.02, 9), dtype=dtype).requires_grad_(True)
        lap, flat = nr.laplacian_loss(x, f), nr.flatten_loss(x, f)
        assert lap.dtype == dtype and flat.dtype == dtype
        assert torch.equal(lap, nr.laplacian_loss_torch(x, f)) and torch.equal(flat, nr.flatten_loss_torch(x, f))
        (lap + flat).sum().backward()
        assert x.grad is not None and bool(torch.isfinite(x.grad).all())

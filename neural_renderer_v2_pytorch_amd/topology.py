"""What the package derives on the host from an index tensor (faces [F, 3], faces_textures,
faces_attributes), and the caches that make it a once-per-tensor cost: the range check (faces_i32),
the CSR lists the backward gathers walk (vertex_adjacency, normal_adjacency) and the mesh losses'
MeshTopology.  Every list is built with stable sorts, so each has one fixed, ascending order: the
summation order of every gather that walks it, which keeps those sums reproducible bit for bit.
A steady-state call (the same device int32 tensor again) is one key tuple and one cache lookup: no
device-to-host copy and no host synchronisation, so such a step can be captured in a HIP graph."""
import collections

import numpy as np
import torch


class TensorCache:
    """Small LRU of results derived from index tensors, keyed by `key(tensor, extra)`.  The storage
    address in a key identifies the tensor only while that storage cannot be freed and handed to
    another tensor, so `put` takes the key's tensors and the entry keeps them alive as long as it
    lives; the version counter in the key catches in-place edits.  A caller alternating a few
    meshes (several objects, or train / validation sets) keeps hitting."""

    def __init__(self, size=8):
        self.size = size
        self.entries = collections.OrderedDict()

    @staticmethod
    def key(t, extra=None):
        """The key of index tensor `t`; `extra` is whatever else the result depends on."""
        return (t.data_ptr(), t._version, t.shape[0], t.device, extra)

    def get(self, key):
        hit = self.entries.get(key)
        if hit is None:
            return None
        self.entries.move_to_end(key)
        return hit[0]

    def put(self, key, value, *pinned):
        """Store `value` (not None); `pinned` are the tensors whose addresses `key` holds."""
        self.entries[key] = (value, pinned)
        self.entries.move_to_end(key)
        while len(self.entries) > self.size:
            self.entries.popitem(last=False)


# one cache per derivation: a large topology entry must not evict a faces check
faces_checked, adjacency, normal_adj, topologies = TensorCache(), TensorCache(), TensorCache(), TensorCache()


def check_range(f, bound, what):
    if f.numel():
        lo, hi = int(f.min()), int(f.max())
        if lo < 0 or hi >= bound:
            raise IndexError("%s index out of range [0, %d): min %d max %d" % (what, bound, lo, hi))


def faces_i32(faces, device, bound, what):
    """[F,3] int32 on `device`, indices checked like the reference's IndexError on out-of-range
    indices (rasterize.py:232, :246).  CPU index tensors are checked on the host before the copy;
    device-resident int32 ones once per (storage, version), so steady-state calls never sync."""
    f = faces if isinstance(faces, torch.Tensor) else torch.as_tensor(faces)
    if f.ndim != 2 or f.shape[1] != 3:
        raise AssertionError("%s must be [F, 3]" % what)
    if f.is_cuda and f.dtype == torch.int32 and f.device == device and f.is_contiguous():
        # the steady-state case (a device int32 index tensor reused every step): no conversion calls
        key = TensorCache.key(f, bound)
        if f.numel() and faces_checked.get(key) is None:
            check_range(f, bound, what)
            faces_checked.put(key, True, f)
        return f
    if f.is_cuda:  # converted: the copy is a new tensor every call, so nothing to cache
        f = f.to(device=device, dtype=torch.int32).contiguous()
        check_range(f, bound, what)
        return f
    check_range(f, bound, what)
    return f.to(dtype=torch.int32).contiguous().to(device, non_blocking=False)


def csr_offsets(keys, n):
    """int32 offsets [n + 1] of the CSR rows of integer `keys` in [0, n): row r has count(keys == r) entries."""
    offsets = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(keys, minlength=n), out=offsets[1:])
    return offsets


def csr(keys, n):
    """(csr_offsets(keys, n), the stable order of `keys`): order[offsets[r]:offsets[r + 1]] are the
    positions of r in `keys`, ascending."""
    return csr_offsets(keys, n), np.argsort(keys, kind="stable")


def vertex_adjacency(faces_i32, V):
    """CSR vertex -> face corners (3 f + k) for the backward's vertex gather, as (offsets [V + 1],
    entries) int32 tensors on the faces' device, cached per faces tensor."""
    key = TensorCache.key(faces_i32, V)
    hit = adjacency.get(key)
    if hit is None:
        offsets, order = csr(faces_i32.reshape(-1).cpu().numpy().astype(np.int64), V)
        hit = (torch.as_tensor(offsets, device=faces_i32.device),
               torch.as_tensor(order.astype(np.int32), device=faces_i32.device))
        adjacency.put(key, hit, faces_i32)
    return hit


def normal_adjacency(faces_i32, V):
    """CSR vertex -> its distinct faces, ascending (the one-hot [F, V] matrix of
    rasterize.py:173-179: a face counts once per vertex), cached per faces tensor."""
    key = TensorCache.key(faces_i32, V)
    hit = normal_adj.get(key)
    if hit is None:
        f = faces_i32.cpu().numpy().astype(np.int64)
        pairs = np.unique(np.stack([f.reshape(-1), np.repeat(np.arange(f.shape[0]), 3)], 1), axis=0)  # sorted by (v, f)
        hit = (torch.as_tensor(csr_offsets(pairs[:, 0], V), device=faces_i32.device),
               torch.as_tensor(pairs[:, 1].astype(np.int32), device=faces_i32.device))
        normal_adj.put(key, hit, faces_i32)
    return hit


class MeshTopology:
    """What both mesh losses need of a faces tensor, as int32 tensors on one device:
      nbr_offsets [V + 1], nbr_index   CSR vertex -> its distinct neighbours, ascending
      edges [E2, 4]                    rows (v0, v1, v2, v3) of the two-face edges, sorted by (v0, v1)
      edge_offsets [V + 1], edge_slots [4 E2]
                                       CSR vertex -> the entries 4 e + k with edges[e, k] == vertex, ascending
    and the counts num_vertices, num_edges (E2), num_boundary_edges (one incident face),
    num_nonmanifold_edges (three or more) and num_all_edges (every distinct undirected edge).
    A topology that knows its faces ([F, 3] int32 on its device, as mesh_topology builds it) also gives,
    built on first use (corner_csr), what the cotangent Laplacian needs:
      nbr_corner_offsets [nnz + 1], nbr_corners
                                       CSR neighbour entry (i, j) -> the corners 3 f + k opposite the edge
                                       {i, j} in `faces` as given, ascending; (i, j) and (j, i) hold the same list"""
    FIELDS = ("nbr_offsets", "nbr_index", "edges", "edge_offsets", "edge_slots")

    def __init__(self, tensors, num_vertices, num_boundary_edges, num_nonmanifold_edges, faces=None):
        for name, t in zip(self.FIELDS, tensors):
            setattr(self, name, t)
        self.num_vertices = int(num_vertices)
        self.num_edges = int(self.edges.shape[0])
        self.num_boundary_edges = int(num_boundary_edges)
        self.num_nonmanifold_edges = int(num_nonmanifold_edges)
        self.num_all_edges = int(self.nbr_index.numel()) // 2
        self.faces = faces
        self._on = {self.device: self}
        self._host = {}  # shared by the copies on other devices: what corner_csr built on the host
        self._index = self._edge_index = self._corners = self._cot_index = None

    @property
    def device(self):
        return self.edges.device

    def __iter__(self):
        return iter(getattr(self, name) for name in self.FIELDS)

    def to(self, device):
        """This topology on `device` (copied once per device)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        hit = self._on.get(device)
        if hit is None:
            hit = MeshTopology([t.to(device) for t in self], self.num_vertices, self.num_boundary_edges,
                               self.num_nonmanifold_edges, None if self.faces is None else self.faces.to(device))
            hit._on, hit._host = self._on, self._host
            self._on[device] = hit
        return hit

    def composition_index(self):
        """int64 index tensors of the torch composition: the row and column of every neighbour entry,
        the neighbour counts, and the edge rows."""
        if self._index is None:
            deg = (self.nbr_offsets[1:] - self.nbr_offsets[:-1]).long()
            rows = torch.repeat_interleave(torch.arange(self.num_vertices, device=self.device), deg)
            self._index = (rows, self.nbr_index.long(), deg, self.edges.long())
        return self._index

    def edge_index(self):
        """int64 index tensors (i, j) of the distinct undirected edges: the neighbour entries with j > i."""
        if self._edge_index is None:
            rows, cols = self.composition_index()[:2]
            once = rows < cols
            self._edge_index = (rows[once], cols[once])
        return self._edge_index

    def corner_csr(self):
        """(nbr_corner_offsets, nbr_corners) on this device: built on the host at the first call on any
        device, copied once per device."""
        if self._corners is None:
            if self.faces is None:
                raise ValueError("this topology was built without its faces: use mesh_topology(faces, num_vertices)")
            if "corners" not in self._host:
                self._host["corners"] = build_corner_csr(self.faces.cpu().numpy(), self.num_vertices,
                                                         self.nbr_offsets.cpu().numpy(), self.nbr_index.cpu().numpy())
            self._corners = tuple(torch.as_tensor(x, device=self.device) for x in self._host["corners"])
        return self._corners

    @property
    def nbr_corner_offsets(self):
        return self.corner_csr()[0]

    @property
    def nbr_corners(self):
        return self.corner_csr()[1]

    def cot_composition_index(self):
        """int64 index tensors of the cotangent composition: the faces, and for every listed corner its
        neighbour entry and itself."""
        if self._cot_index is None:
            off, corners = self.corner_csr()
            count = (off[1:] - off[:-1]).long()
            entry = torch.repeat_interleave(torch.arange(count.numel(), device=self.device), count)
            self._cot_index = (self.faces.long(), entry, corners.long())
        return self._cot_index


def build_corner_csr(faces, V, nbr_offsets, nbr_index):
    """(nbr_corner_offsets [nnz + 1], nbr_corners) int32 numpy, for faces [F, 3] as given and the neighbour
    CSR build_topology made of them: corner 3 f + k is opposite the edge of face f's two other corners, and
    is listed under both directions of that edge.  Faces with a repeated vertex have no corner listed."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if 3 * f.shape[0] >= 2 ** 31:
        raise ValueError("mesh too large: 3 * F must stay below 2^31")
    keep = np.flatnonzero((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2]))
    f = f[keep]
    a, b = f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1)
    corner = (3 * keep[:, None] + np.arange(3)[None, :]).reshape(-1)
    key, corner = np.concatenate([a * V + b, b * V + a]), np.concatenate([corner, corner])
    if key.shape[0] >= 2 ** 31:
        raise ValueError("mesh too large: the corner lists (6 per face) must stay below 2^31 entries")
    order = np.lexsort((corner, key))  # by entry, ascending corners within one
    rows = np.repeat(np.arange(V, dtype=np.int64), np.diff(np.asarray(nbr_offsets, np.int64)))
    pair = rows * V + np.asarray(nbr_index, np.int64)  # ascending: the CSR's own order
    entry = np.searchsorted(pair, key[order])
    assert entry.size == 0 or np.array_equal(pair[entry], key[order])  # every face edge is a neighbour entry
    return csr_offsets(entry, pair.shape[0]), corner[order].astype(np.int32)


def build_topology(faces, V):
    """The five arrays of MeshTopology (int32 numpy) and the boundary / non-manifold edge counts, from
    faces [F, 3] with indices in [0, V).  Faces with a repeated vertex are ignored."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    W = max(V, 1)  # V = 0 leaves no face: every array is empty
    # distinct neighbours: every face edge in both directions, duplicates dropped (np.unique sorts)
    src = np.concatenate([f[:, 0], f[:, 1], f[:, 1], f[:, 2], f[:, 2], f[:, 0]])
    dst = np.concatenate([f[:, 1], f[:, 0], f[:, 2], f[:, 1], f[:, 0], f[:, 2]])
    pair = np.unique(src * V + dst)
    # undirected edges: corner k of a face is opposite the edge of its two other corners; face-major
    # order and a stable sort keep each edge's faces in ascending face order
    a, b, opp = f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1), f.reshape(-1)
    key = np.minimum(a, b) * V + np.maximum(a, b)
    order = np.argsort(key, kind="stable")
    uniq, start, count = np.unique(key[order], return_index=True, return_counts=True)
    two = count == 2
    first = start[two]
    edges = np.stack([uniq[two] // W, uniq[two] % W, opp[order[first]], opp[order[first + 1]]], 1).reshape(-1, 4)
    if 4 * edges.shape[0] >= 2 ** 31 or pair.shape[0] >= 2 ** 31:
        raise ValueError("mesh too large: 4 * E2 and the neighbour count must stay below 2^31")
    edge_offsets, edge_slots = csr(edges.reshape(-1), V)
    arrays = [csr_offsets(pair // W, V), pair % W, edges, edge_offsets, edge_slots]
    return [x.astype(np.int32) for x in arrays], int((count == 1).sum()), int((count > 2).sum())


def mesh_topology(faces, num_vertices, device=None):
    """The MeshTopology of faces [F, 3] (any integer tensor or array; indices outside [0, num_vertices)
    raise IndexError) on `device` (default: the faces' own, the CPU for arrays).  Built on the host once
    per (faces storage, version, shape, num_vertices, device) and cached: calls that pass the same
    device int32 tensor again issue no host synchronisation."""
    V = int(num_vertices)
    if V < 0:
        raise ValueError("num_vertices must not be negative")
    if device is None:
        device = faces.device if torch.is_tensor(faces) else torch.device("cpu")
    f = faces_i32(faces, torch.device(device), V, "faces")
    key = TensorCache.key(f, V)
    topo = topologies.get(key)
    if topo is None:
        arrays, boundary, nonmanifold = build_topology(f.cpu().numpy(), V)
        topo = MeshTopology([torch.as_tensor(x, device=f.device) for x in arrays], V, boundary, nonmanifold, f)
        topologies.put(key, topo, f)
    return topo

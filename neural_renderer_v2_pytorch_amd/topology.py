"""What the package derives on the host from an index tensor (faces [F, 3], faces_textures,
faces_attributes), and the caches that make it a once-per-tensor cost: the range check (faces_i32),
the CSR lists the backward gathers walk (vertex_adjacency, normal_adjacency), the mesh losses'
MeshTopology, and what skinning.py derives from a rig's parents and weights (Skeleton, SkinBinding).
Every list is built with stable sorts, so each has one fixed, ascending order: the summation order
of every gather that walks it, which keeps those sums reproducible bit for bit.
A steady-state call (the same device int32 tensor again) is one key tuple and one cache lookup: no
device-to-host copy and no host synchronisation, so such a step can be captured in a HIP graph."""
import collections

import numpy as np
import torch

from . import _lib


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


def _device_of(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class _PerDevice:
    """int32 / float32 tensors named by FIELDS on one device, copied once per further device (`to`)."""
    FIELDS = ()

    def _place(self, tensors):
        for name, t in zip(self.FIELDS, tensors):
            setattr(self, name, t)
        self._on = {self.device: self}

    @property
    def device(self):
        return getattr(self, self.FIELDS[0]).device

    def to(self, device):
        """This structure on `device` (copied once per device)."""
        device = _device_of(device)
        hit = self._on.get(device)
        if hit is None:
            hit = object.__new__(type(self))
            hit.__dict__.update(self.__dict__)
            for name in self.FIELDS:
                setattr(hit, name, getattr(self, name).to(device))
            self._on[device] = hit
        return hit


# ---- articulated meshes (skinning.py) ----
SKIN_MAX_JOINTS, SKIN_MAX_INFLUENCES, SKIN_CHUNK = _lib.NR_SKIN_MAX_JOINTS, _lib.NR_SKIN_MAX_INFLUENCES, _lib.NR_SKIN_CHUNK
skeletons, bindings = TensorCache(), TensorCache()


def build_skeleton(parents):
    """(level_offsets [L + 1], level_joints [J], child_offsets [J + 1], children) int32 numpy of parents [J]:
    the joints sorted by depth (ascending within a level) and the children CSR (ascending).  -1 marks a root;
    a cycle, an index outside [0, J) or J outside [1, SKIN_MAX_JOINTS] is a ValueError."""
    p = np.asarray(parents)
    if p.ndim != 1 or p.dtype.kind not in "iu":
        raise ValueError("parents must be a [J] integer tensor or array")
    p = p.astype(np.int64)
    J = p.shape[0]
    if J < 1 or J > SKIN_MAX_JOINTS:
        raise ValueError("a skeleton has 1 to %d joints, got %d" % (SKIN_MAX_JOINTS, J))
    bad = np.flatnonzero((p < -1) | (p >= J))
    if bad.size:
        raise ValueError("parents[%d] = %d is neither -1 nor a joint index in [0, %d)" % (bad[0], p[bad[0]], J))
    depth = np.where(p < 0, 0, -1)
    level = 0
    while True:  # a level per pass: the joints whose parent was placed by the pass before
        level += 1
        new = (depth < 0) & (depth[np.maximum(p, 0)] == level - 1)
        if not new.any():
            break
        depth[new] = level
    if (depth < 0).any():
        raise ValueError("parents hold a cycle (through joint %d)" % int(np.flatnonzero(depth < 0)[0]))
    level_offsets, level_joints = csr(depth, level)
    has = np.flatnonzero(p >= 0)
    child_offsets, order = csr(p[has], J)
    return level_offsets, level_joints.astype(np.int32), child_offsets, has[order].astype(np.int32)


class Skeleton(_PerDevice):
    """A joint tree (or forest), as int32 tensors on one device:
      parents [J]                       -1 for a root, else the parent's index; joints need not be parents-first
      level_offsets [L + 1], level_joints [J]
                                        the joints sorted by depth, ascending within a level
      child_offsets [J + 1], children   CSR joint -> its children, ascending
    and num_joints, num_levels, plus the host lists `parent_list` and `order` (level_joints) the torch
    composition walks.  Skeleton(parents) builds one from any [J] integer tensor, array or list; the functions
    of skinning.py go through skeleton(), which caches."""
    FIELDS = ("parents", "level_offsets", "level_joints", "child_offsets", "children")

    def __init__(self, parents, device=None):
        if isinstance(parents, Skeleton):
            self.__dict__.update(parents.to(parents.device if device is None else device).__dict__)
            return
        if device is None:
            device = parents.device if torch.is_tensor(parents) else torch.device("cpu")
        host = parents.detach().cpu().numpy() if torch.is_tensor(parents) else np.asarray(parents)
        arrays = build_skeleton(host)
        self.parent_list = [int(x) for x in host]
        self.order = [int(x) for x in arrays[1]]
        self.num_joints, self.num_levels = len(self.parent_list), int(arrays[0].shape[0]) - 1
        dev = _device_of(device)
        self._place([torch.as_tensor(x, device=dev) for x in (host.astype(np.int32),) + arrays])


def skeleton(parents, device=None):
    """The Skeleton of `parents` on `device` (default: the tensor's own, the CPU for arrays): a Skeleton is moved,
    a tensor is looked up by (storage, version) -- no device-to-host copy on a hit -- and an array or list by its
    values."""
    if isinstance(parents, Skeleton):
        return parents if device is None else parents.to(device)
    if torch.is_tensor(parents):
        key = TensorCache.key(parents)
    else:
        key = ("values", tuple(int(x) for x in np.asarray(parents).reshape(-1)))
    hit = skeletons.get(key)
    if hit is None:
        hit = Skeleton(parents)
        skeletons.put(key, hit, parents)
    return hit if device is None else hit.to(device)


def build_binding(weights, indices, num_joints):
    """The arrays of SkinBinding (numpy) from weights [V, K] with indices [V, K], or from dense weights [V, J]
    (indices None): (indices, weights, joint_offsets, entry_vertex, entry_slot, chunk_joint, chunk_begin,
    chunk_end, joint_chunk_offsets)."""
    w = np.ascontiguousarray(np.asarray(weights, np.float32))
    if w.ndim != 2:
        raise ValueError("weights must be [V, K] with indices, or dense [V, J]")
    V = w.shape[0]
    if indices is None:
        J = w.shape[1] if num_joints is None else int(num_joints)
        if w.shape[1] != J:
            raise ValueError("dense weights must be [V, %d], got %s" % (J, list(w.shape)))
        nz = w != 0
        count = nz.sum(1)
        over = np.flatnonzero(count > SKIN_MAX_INFLUENCES)
        if over.size:
            raise ValueError("row %d of the weights has %d non-zero entries; at most %d joints may influence a vertex"
                             % (over[0], count[over[0]], SKIN_MAX_INFLUENCES))
        K = max(int(count.max()) if V else 1, 1)
        # a row's non-zero columns first, ascending (stable), then zero columns: padding of weight 0
        idx = np.argsort(~nz, axis=1, kind="stable")[:, :K]
        w = np.take_along_axis(w, idx, 1)
    else:
        idx = np.asarray(indices)
        if idx.dtype.kind not in "iu" or idx.shape != w.shape:
            raise ValueError("indices must be integers of the weights' shape %s, got %s %s" % (list(w.shape), idx.dtype, list(idx.shape)))
        if num_joints is None:
            raise ValueError("weights with indices need num_joints")
        J, K = int(num_joints), w.shape[1]
        if K < 1 or K > SKIN_MAX_INFLUENCES:
            raise ValueError("a vertex takes 1 to %d influences, got K = %d" % (SKIN_MAX_INFLUENCES, K))
        idx = idx.astype(np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= J):
            raise ValueError("indices out of range [0, %d): min %d max %d" % (J, idx.min(), idx.max()))
    if J < 1 or J > SKIN_MAX_JOINTS:
        raise ValueError("a skeleton has 1 to %d joints, got %d" % (SKIN_MAX_JOINTS, J))
    if V * K >= 2 ** 31:
        raise ValueError("mesh too large: V * K must stay below 2^31")
    idx = np.ascontiguousarray(idx.astype(np.int32))
    # the joint CSR: the slots of non-zero weight, by (vertex, slot) within a joint (a stable sort of the flat order)
    slots = np.flatnonzero(w.reshape(-1) != 0)
    joint = idx.reshape(-1)[slots].astype(np.int64)
    joint_offsets, order = csr(joint, J)
    entries = slots[order]
    # the chunk table: each non-empty row cut into runs of at most SKIN_CHUNK entries
    rows = np.diff(joint_offsets.astype(np.int64))
    chunks = -(-rows // SKIN_CHUNK)
    joint_chunk_offsets = np.zeros(J + 1, np.int32)
    np.cumsum(chunks, out=joint_chunk_offsets[1:])
    chunk_joint = np.repeat(np.arange(J, dtype=np.int64), chunks)
    local = np.arange(chunk_joint.shape[0], dtype=np.int64) - joint_chunk_offsets[chunk_joint]
    chunk_begin = joint_offsets[chunk_joint] + local * SKIN_CHUNK
    chunk_end = np.minimum(chunk_begin + SKIN_CHUNK, joint_offsets[chunk_joint + 1])
    i32 = [x.astype(np.int32) for x in (joint_offsets, entries // K, entries % K, chunk_joint, chunk_begin, chunk_end,
                                        joint_chunk_offsets)]
    return (idx, w, *i32)


class SkinBinding(_PerDevice):
    """Skinning weights in the form the fused kernels read, on one device:
      indices [V, K] int32, weights [V, K] float32
                                        from a dense [V, J] matrix: each row's non-zero entries in ascending joint
                                        order, K the largest row count (at least 1), padded with slots of weight 0
      joint_offsets [J + 1], entry_vertex, entry_slot
                                        CSR joint -> the slots (vertex, slot) of non-zero weight that name it, ordered
                                        by (vertex, slot): zero-weight padding appears in no row
      chunk_joint, chunk_begin, chunk_end, joint_chunk_offsets [J + 1]
                                        the rows cut into runs of at most SKIN_CHUNK entries; a row of 0 entries has none
    and num_vertices, num_joints, num_influences (K), num_entries, num_chunks.  chunk_joint stays on the host (the
    kernels find a joint's chunks through joint_chunk_offsets).  skin_binding() builds and caches one."""
    FIELDS = ("indices", "weights", "joint_offsets", "entry_vertex", "entry_slot", "chunk_begin", "chunk_end",
              "joint_chunk_offsets")

    def __init__(self, arrays, num_joints, device):
        indices, weights, joint_offsets, entry_vertex, entry_slot, chunk_joint, chunk_begin, chunk_end, jco = arrays
        dev = _device_of(device)
        self._place([torch.as_tensor(x, device=dev) for x in (indices, weights, joint_offsets, entry_vertex, entry_slot,
                                                              chunk_begin, chunk_end, jco)])
        self.chunk_joint = torch.as_tensor(chunk_joint)
        self.num_vertices, self.num_influences = int(indices.shape[0]), int(indices.shape[1])
        self.num_joints = int(num_joints)
        self.num_entries, self.num_chunks = int(entry_vertex.shape[0]), int(chunk_begin.shape[0])
        self._gather = {}

    def gather_index(self):
        """(indices as int64, the mask of the slots of non-zero weight as float32) on this device: what reads a
        live dense matrix into the [V, K] form."""
        hit = self._gather.get(self.device)
        if hit is None:
            hit = self._gather[self.device] = (self.indices.long(), (self.weights != 0).to(torch.float32))
        return hit


def skin_binding(weights, indices=None, num_joints=None, device=None):
    """The SkinBinding of dense weights [V, J], or of weights [V, K] with integer indices [V, K] and num_joints, on
    `device` (default: the weights' own, the CPU for arrays).  More than SKIN_MAX_INFLUENCES non-zero entries in a
    row, an index outside [0, num_joints) or mismatched shapes raise ValueError.  Tensors are looked up by
    (storage, version) of both, so a steady-state call is one key and one lookup -- no device-to-host copy -- and an
    in-place edit (an optimiser's step on learned weights) rebuilds the binding at the next call."""
    if isinstance(weights, SkinBinding):
        return weights if device is None else weights.to(device)
    tensors = torch.is_tensor(weights) and (indices is None or torch.is_tensor(indices))
    if tensors:
        key = (TensorCache.key(weights, None if num_joints is None else int(num_joints)),
               None if indices is None else TensorCache.key(indices), tuple(weights.shape))
        hit = bindings.get(key)
    else:
        hit = None
    if hit is None:
        host = lambda x: x.detach().cpu().numpy() if torch.is_tensor(x) else x  # noqa: E731
        w, idx = host(weights), None if indices is None else host(indices)
        arrays = build_binding(w, idx, num_joints)
        J = np.asarray(w).shape[1] if indices is None else int(num_joints)
        hit = SkinBinding(arrays, J, weights.device if torch.is_tensor(weights) else "cpu")
        if tensors:
            bindings.put(key, hit, weights, indices)
    return hit if device is None else hit.to(device)


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

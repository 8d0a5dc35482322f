"""Rigs, bindings and poses shared by test_skinning.py and test_gpu_skinning.py, and the float64 reference of
each GPU case (computed once, on the CPU, by the torch composition)."""
import functools

import numpy as np
import torch

import neural_renderer_v2_pytorch_amd as nr

CHUNK = nr.NR_SKIN_CHUNK
CHUNK_ROWS = (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)  # entries of joints 0 .. 5 of chunk_rows_binding


def parents_of(kind, J, rng):
    """chain: j - 1; tree: each parent drawn from the four joints before; forest: a tree with two roots (joints 0
    and 1); children_first: the tree relabelled j -> J - 1 - j, so every child is listed before its parent; roots:
    every joint a root (unconnected rigid parts: one level, no child anywhere)."""
    if kind == "roots":
        return np.full(J, -1, np.int64)
    if kind == "chain":
        return np.arange(J, dtype=np.int64) - 1
    p = np.array([-1] + [rng.randint(max(0, j - 4), j) for j in range(1, J)], np.int64)
    if kind == "forest":
        p[1] = -1
    if kind == "children_first":
        p = np.where(p[::-1] < 0, -1, J - 1 - p[::-1])
    return p


def random_binding(V, J, K, rng):
    """indices [V, K] int32 and weights [V, K] float32: random joints (the last joint never named when J > 1: a
    joint with no vertices), positive weights summing to 1, then a fifth of the slots beyond the first zeroed
    (padding whose index stays in range) and vertex V // 2 zeroed altogether."""
    idx = rng.randint(0, max(J - 1, 1), size=(V, K)).astype(np.int32)
    w = rng.uniform(0.1, 1.0, size=(V, K))
    w /= w.sum(1, keepdims=True)
    if K > 1:
        w[:, 1:] *= rng.uniform(size=(V, K - 1)) > 0.2
    if V > 2:
        w[V // 2] = 0
    return idx, w.astype(np.float32)


def chunk_rows_binding(rng=None):
    """K = 1, J = 6: joint j is named by CHUNK_ROWS[j] vertices (in shuffled vertex order), every weight non-zero."""
    idx = np.repeat(np.arange(len(CHUNK_ROWS)), CHUNK_ROWS).astype(np.int32)
    rng = rng or np.random.RandomState(5)
    rng.shuffle(idx)
    return idx[:, None], rng.uniform(0.5, 1.5, size=(idx.shape[0], 1)).astype(np.float32)


def brute_levels(parents):
    """(depth of every joint, children lists) by Python loops."""
    J = len(parents)
    depth = []
    for j in range(J):
        d, k = 0, j
        while parents[k] >= 0:
            d, k = d + 1, parents[k]
        depth.append(d)
    return depth, [[c for c in range(J) if parents[c] == j] for j in range(J)]


# name: (kind, J, V, K, B, shared vertices, shared joints, matrix pose, pose sigma)
GPU_CASES = {
    "j1_v1_k1": ("chain", 1, 1, 1, 3, True, True, False, 1.0),
    "j2_v255_k4_matrix": ("chain", 2, 255, 4, 3, False, False, True, 1.0),
    "j24_tree_v256_k4": ("tree", 24, 256, 4, 3, True, True, False, 1.0),
    "j24_tree_v257_k8_b1": ("tree", 24, 257, 8, 1, False, True, False, 1.0),
    "j5_all_roots_v70_k2": ("roots", 5, 70, 2, 3, False, True, False, 1.0),  # the children list is empty
    "j24_forest_v300_k4": ("forest", 24, 300, 4, 3, False, False, False, 1.0),
    "j24_children_first_v300_k4": ("children_first", 24, 300, 4, 3, True, False, False, 1.0),
    "j65_chain_v700_k4": ("chain", 65, 700, 4, 3, False, False, False, 0.3),
    "j65_tree_v700_k8_matrix": ("tree", 65, 700, 8, 3, True, True, True, 0.3),
    "j256_chain_v64_k1": ("chain", 256, 64, 1, 3, False, False, False, 0.3),
    "chunk_rows": ("tree", 6, sum(CHUNK_ROWS), 1, 3, True, True, False, 1.0),
}


def special_poses(r):
    """Into item 0 of axis-angle pose r [B, J, 3] (float32 numpy), as far as it has the joints: an exact zero, one
    just below and one just above the series switch, and an angle above pi."""
    J = r.shape[1]
    unit = np.array([0.6, -0.64, 0.48], np.float32)
    for j, t2 in ((0, 0.), (1, 0.98 * nr.NR_RODRIGUES_SERIES), (2, 1.02 * nr.NR_RODRIGUES_SERIES), (3, 3.5 ** 2)):
        if j < J:
            r[0, j] = unit * np.float32(np.sqrt(t2))
    return r


@functools.lru_cache(maxsize=None)
def gpu_case(name):
    """A dict of float32-valued float64 CPU tensors: pose, joints, vertices, weights, indices (int32), parents
    (int64 numpy) and the upstream gradients g_out, g_posed, g_transforms; then the float64 composition's
    `ref` = dict(transforms, posed, out, pose, joints, vertices, weights: the gradients).  Left unchanged by the
    tests."""
    kind, J, V, K, B, shared_v, shared_j, matrix, sigma = GPU_CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    parents = parents_of(kind, J, rng)
    idx, w = chunk_rows_binding(rng) if name == "chunk_rows" else random_binding(V, J, K, rng)
    r = special_poses((rng.normal(size=(B, J, 3)) * sigma).astype(np.float32))
    f64 = lambda a: torch.as_tensor(np.asarray(a, np.float32)).double()  # noqa: E731
    pose = f64(r)
    if matrix:  # used as given: not orthonormal
        pose = f64((nr.rodrigues_torch(pose) + f64(rng.normal(size=(B, J, 3, 3)) * 0.01)).numpy())
    d = {"parents": parents, "pose": pose, "indices": torch.as_tensor(idx),
         "joints": f64(rng.uniform(-0.5, 0.5, size=(J, 3) if shared_j else (B, J, 3))),
         "vertices": f64(rng.uniform(-0.5, 0.5, size=(V, 3) if shared_v else (B, V, 3))),
         "weights": f64(w), "g_out": f64(rng.normal(size=(B, V, 3))), "g_posed": f64(rng.normal(size=(B, J, 3))),
         "g_transforms": f64(rng.normal(size=(B, J, 3, 4)))}
    d["ref"] = run(d, nr.pose_transforms_torch, nr.skin_vertices_torch, torch.float64, "cpu")
    return d


def run(d, pose_fn, skin_fn, dtype, device, weights_grad=True):
    """Forward and backward of pose_fn then skin_fn on the case's inputs in `dtype` on `device`: the outputs and
    the gradient of <out, g_out> + <posed, g_posed> + <transforms, g_transforms> to every input."""
    leaf = lambda k: d[k].detach().to(device=device, dtype=dtype, copy=True).requires_grad_(True)  # noqa: E731
    pose, joints, vertices = leaf("pose"), leaf("joints"), leaf("vertices")
    weights = leaf("weights") if weights_grad else d["weights"].to(device=device, dtype=dtype)
    transforms, posed = pose_fn(pose, joints, d["parents"])
    out = skin_fn(vertices, transforms, weights, d["indices"].to(device))
    up = lambda k: d[k].to(device=device, dtype=dtype)  # noqa: E731
    ((out * up("g_out")).sum() + (posed * up("g_posed")).sum() + (transforms * up("g_transforms")).sum()).backward()
    return {"transforms": transforms.detach(), "posed": posed.detach(), "out": out.detach(), "pose": pose.grad,
            "joints": joints.grad, "vertices": vertices.grad, "weights": weights.grad if weights_grad else None}

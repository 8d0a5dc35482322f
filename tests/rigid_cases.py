"""Inputs, the float64 reference and the closed-form backward (restated as torch ops) shared by test_rigid.py,
test_gpu_rigid.py and test_gpu_icp.py."""
import functools
import math

import numpy as np
import torch

import neural_renderer_v2_pytorch_amd as nr
from arap_cases import axis_rotation
from mesh_loss_cases import teapot

CHUNK = nr._lib.NR_RIGID_CHUNK  # points per block of the fused sums
assert CHUNK == 1024

# name: (B, N, far).  n1025 is just past one chunk; two_trips has more than 256 chunks, so every loop over partial
# sums (256 threads) takes a second trip; far has its centroids at 100 times the cloud's extent.
CASES = {
    "n1": (3, 1, False), "n2": (3, 2, False), "n3": (3, 3, False), "n63": (3, 63, False), "n65": (1, 65, False),
    "n257": (3, 257, False), "n1025": (3, CHUNK + 1, False), "two_trips": (1, 256 * CHUNK + CHUNK + 5, False),
    "far": (3, 257, True),
}
WEIGHTS = ("none", "random", "zeros")
VARIANTS = [(shared, scale, kind) for shared in (False, True) for scale in (False, True) for kind in WEIGHTS]
SURE = 0.1  # rotations (and what depends on them) are compared where the float64 reference's condition is at least this


def rotation(axis, angle):
    return torch.as_tensor(axis_rotation(axis, angle))


@functools.lru_cache(maxsize=None)
def pairs(name, shared):
    """float32 CPU tensors x [B, N, 3] and y ([N, 3] when shared): a uniform cloud of extent 1, and per item a
    rotated, scaled and shifted copy of it (of item 0's x when shared) plus N(0, 0.02) noise."""
    B, N, far = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    x = rng.uniform(-0.5, 0.5, (B, N, 3))
    y = np.empty_like(x)
    for b in range(B):
        R = axis_rotation(rng.normal(size=3), 0.4 + 0.5 * b)
        y[b] = (0.8 + 0.3 * b) * (x[0 if shared else b] @ R.T) + rng.uniform(-0.3, 0.3, 3)
    y += rng.normal(0., 0.02, y.shape)
    if shared:
        x = x[:1] @ np.stack([axis_rotation(rng.normal(size=3), 0.3 * b) for b in range(B)]).transpose(0, 2, 1) + rng.normal(0., 0.02, x.shape)
        y = y[0]
    if far:
        x = x + np.array([100., -70., 50.])
        y = y + np.array([-60., 100., 80.])
    return torch.as_tensor(x.astype(np.float32)), torch.as_tensor(y.astype(np.float32))


@functools.lru_cache(maxsize=None)
def weights(name, kind):
    """None, uniform (0, 1) float32 weights [B, N], or those with the block [N / 4, N / 2) set to 0."""
    B, N, _ = CASES[name]
    if kind == "none":
        return None
    w = np.random.RandomState(5 + N).uniform(0.05, 1., (B, N)).astype(np.float32)
    if kind == "zeros":
        w[:, N // 4:N // 2] = 0.
    return torch.as_tensor(w)


@functools.lru_cache(maxsize=None)
def upstream(name):
    """Random float64 gradients of R, t and s."""
    B = CASES[name][0]
    rng = np.random.RandomState(11)
    return tuple(torch.as_tensor(rng.normal(size=shape)) for shape in ((B, 3, 3), (B, 3), (B,)))


def wide(t):
    return None if t is None else t.double()


@functools.lru_cache(maxsize=None)
def reference(name, shared, scale, kind):
    """rigid_align_torch in float64 on the float32 values widened: dict of R, t, s, condition, and the gradients gx,
    gy (summed over the items for a shared y) for upstream(name)."""
    x, y = pairs(name, shared)
    a, b = x.double().requires_grad_(True), y.double().requires_grad_(True)
    R, t, s, c = nr.rigid_align_torch(a, b, wide(weights(name, kind)), scale, return_condition=True)
    gR, gt, gs = upstream(name)
    ((R * gR).sum() + (t * gt).sum() + (s * gs).sum()).backward()
    return dict(R=R.detach(), t=t.detach(), s=s.detach(), condition=c.detach(), gx=a.grad, gy=b.grad)


@functools.lru_cache(maxsize=None)
def float32_error(name):
    """What rigid_align_torch itself loses in float32 on the CPU against float64 on exactly these inputs: the
    largest |d| of R, t, s and condition over the items whose float64 condition is at least SURE, over VARIANTS."""
    err = dict(R=0., t=0., s=0., condition=0.)
    for shared, scale, kind in VARIANTS:
        x, y = pairs(name, shared)
        ref = reference(name, shared, scale, kind)
        R, t, s, c = nr.rigid_align_torch(x, y, weights(name, kind), scale, return_condition=True)
        sure = ref["condition"] >= SURE
        for key, got in (("R", R), ("t", t), ("s", s), ("condition", c)):
            if bool(sure.any()):
                err[key] = max(err[key], float((got.double() - ref[key])[sure].abs().max()))
    return err


def closed_form_backward(x, y, w, scale, gR, gt, gs):
    """The gradients of x and y [B, N, 3] from those of R, t and s, in closed form (float64 tensors; w [B, N]):
    the derivation of include/nr_raster.h done again.  R maximises tr(R^T A), so P = R^T A is symmetric; a
    perturbation keeps (R + dR)^T (A + dA) symmetric, which with dR = R [omega]x reads
    [omega]x P + P [omega]x = R^T dA - dA^T R, and the left side is [(tr(P) I - P) omega]x."""
    W = w.sum(1)
    xbar, ybar = (w[..., None] * x).sum(1) / W[:, None], (w[..., None] * y).sum(1) / W[:, None]
    xc, yc = x - xbar[:, None], y - ybar[:, None]
    A = torch.einsum("bn,bni,bnj->bij", w, yc, xc)
    var = (w * (xc * xc).sum(-1)).sum(1)
    R, t, s = nr.rigid_align_torch(x, y, w, scale)
    eye = torch.eye(3, dtype=x.dtype)
    # t = ybar - s R xbar
    g_s = gs - (gt * (R @ xbar[..., None])[..., 0]).sum(1)
    g_xbar = -s[:, None] * (R.transpose(1, 2) @ gt[..., None])[..., 0]
    G = gR - s[:, None, None] * gt[:, :, None] * xbar[:, None, :]
    # s = tr(R^T A) / var, and d tr(R^T A) = tr(R^T dA) because tr([omega]x^T P) = 0
    g_tau = g_s / var if scale else torch.zeros_like(W)
    g_var = -g_s * s / var if scale else torch.zeros_like(W)
    # dL = <G, R [omega]x> = omega . m with m = axial(M - M^T), M = R^T G; omega = K^{-1} axial(R^T dA - dA^T R), so
    # dL = u . axial(Z - Z^T) = <[u]x, Z> with u = K^{-1} m, Z = R^T dA: gA = R [u]x
    P = R.transpose(1, 2) @ A
    P = 0.5 * (P + P.transpose(1, 2))
    K = torch.einsum("bii->b", P)[:, None, None] * eye - P
    M = R.transpose(1, 2) @ G
    m = torch.stack([M[:, 2, 1] - M[:, 1, 2], M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1]], 1)
    u = torch.linalg.solve(K, m)
    z = torch.zeros_like(W)
    ux = torch.stack([torch.stack([z, -u[:, 2], u[:, 1]], 1), torch.stack([u[:, 2], z, -u[:, 0]], 1),
                      torch.stack([-u[:, 1], u[:, 0], z], 1)], 1)
    gA = g_tau[:, None, None] * R + R @ ux
    gx = w[..., None] * (torch.einsum("bij,bni->bnj", gA, yc) + 2 * g_var[:, None, None] * xc + (g_xbar / W[:, None])[:, None])
    gy = w[..., None] * (torch.einsum("bij,bnj->bni", gA, xc) + (gt / W[:, None])[:, None])
    return gx, gy


# ---- ICP ----
MOTIONS = [((1., 2., 3.), 0.3, (0.1, -0.15, 0.12)), ((-1., 0.5, 0.2), 0.5, (-0.2, 0.1, 0.15)), ((1., 2., 3.), 0.8, (0.15, 0.2, -0.1))]


@functools.lru_cache(maxsize=None)
def teapot_scan(dtype=torch.float32):
    """(x [3, N, 3], y [M, 3], R [3, 3, 3], t [3, 3], want [N]): y the teapot's vertices, x every third of them moved
    by the inverse of MOTIONS' motions, so that y[want] = R x + t; want is 3 arange, or the lower index where two
    vertices coincide."""
    v = torch.as_tensor(teapot()[0])
    picks = torch.arange(0, v.shape[0], 3)
    d = (v[picks, None] - v[None]).abs().sum(-1)
    want = (d == 0).to(torch.uint8).argmax(1)  # the first coincident vertex
    R = torch.stack([rotation(axis, angle) for axis, angle, _ in MOTIONS])
    t = torch.as_tensor([m[2] for m in MOTIONS], dtype=torch.float64)
    x = (v[picks][None] - t[:, None]) @ R  # R^T (y - t), row vectors
    return x.to(dtype), v.to(dtype), R, t, want


ICP_CASES = {  # name: (B, N, M, seed of x, seed of y); test_gpu_point_loss's seeds where the precondition holds
    "wave": (3, 65, 63, 103, 203), "partial_block": (3, 257, 300, 103, 203), "few_x": (2, 3, 2500, 103, 203),
    "three_ranges": (1, 5, 3074, 103, 203),
    # two query blocks per item: against two tiles of targets, which four blocks still split in two (103 / 203 leave
    # a gap of 5.7e-6 here; these 9.7e-5), and against fewer targets than a tile, unsplit (gap 1.4e-4)
    "two_query_blocks": (2, 1025, 2049, 116, 216), "two_query_blocks_one_tile": (2, 1025, 300, 107, 207),
}
ICP_SPLIT = ("few_x", "three_ranges", "two_query_blocks")  # the cases whose targets are split over several blocks
ICP_GAP = 1e-5


@functools.lru_cache(maxsize=None)
def icp_clouds(name):
    B, N, M, sx, sy = ICP_CASES[name]
    x = np.random.RandomState(sx).uniform(-1, 1, (B, N, 3)).astype(np.float32)
    y = np.random.RandomState(sy).uniform(-1, 1, (B, M, 3)).astype(np.float32)
    return torch.as_tensor(x), torch.as_tensor(y)


def icp_init(B):
    """A non-identity start, float64: rotations of 0.4 + 0.3 b rad about (1, 2, 3), t = (0.1, -0.2, 0.05), s = 1.1."""
    R = torch.stack([rotation((1., 2., 3.), 0.4 + 0.3 * b) for b in range(B)])
    return R, torch.tensor([0.1, -0.2, 0.05], dtype=torch.float64).expand(B, 3).clone(), torch.full((B,), 1.1, dtype=torch.float64)


def distance_gap(q, y):
    """The smallest (second-nearest - nearest) distance over the queries q [B, N, 3] against y [B, M, 3] (float64)."""
    worst = math.inf
    for i in range(0, q.shape[1], 256):
        two = torch.cdist(q[:, i:i + 256], y).topk(2, dim=2, largest=False)[0]
        worst = min(worst, float((two[..., 1] - two[..., 0]).min()))
    return worst


@functools.lru_cache(maxsize=None)
def icp_first_update(name):
    """The float64 reference of one update from icp_init: (index after the first pass, then R, t, s, condition of
    rigid_align_torch on the gathered pairs with scale on), and the distance gap under the start."""
    x, y = icp_clouds(name)
    x, y = x.double(), y.double()
    R, t, s = icp_init(x.shape[0])
    q = s[:, None, None] * (x @ R.transpose(1, 2)) + t[:, None]
    index = nr.nearest_points_torch(q, y)[1]
    out = nr.rigid_align_torch(x, y.gather(1, index.long()[..., None].expand(-1, -1, 3)), None, True, return_condition=True)
    return (index,) + tuple(out) + (distance_gap(q, y),)

"""Synthetic meshes and batched scenes for parity tests and the benchmark.

Meshes:
  * icosphere(level)  -- level 4: V=2562, F=5120 (the headline "~5k-face mesh"), radius 0.9
  * torus(nu, nv)     -- 250x100: V=25000, F=50000 (config 5)
  * subdivide(v, f, vt, ft) -- one midpoint subdivision (the ShapeNet car 3644 -> 14576 faces, config 3)
Scenes: per-item Gaussian vertex jitter (seed 1000+b) and per-item viewpoint
get_points_from_angles(2.732, U(-30,30), U(0,360)) (seed 2000+b); faces shared across the batch.
"""
import math

import numpy as np
import torch


def icosphere(level=4, radius=0.9):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t),
             (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    verts = [np.array(v, np.float64) / np.linalg.norm(v) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4),
             (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8),
             (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        cache = {}

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                cache[key] = len(verts) - 1
            return cache[key]

        nf = []
        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nf
    v = (np.stack(verts) * radius).astype(np.float32)
    f = np.asarray(faces, np.int32)
    return v, f


def torus(nu=250, nv=100, major=0.65, minor=0.25):
    u = np.arange(nu) * (2 * math.pi / nu)
    w = np.arange(nv) * (2 * math.pi / nv)
    uu, ww = np.meshgrid(u, w, indexing="ij")
    x = (major + minor * np.cos(ww)) * np.cos(uu)
    y = minor * np.sin(ww)
    z = (major + minor * np.cos(ww)) * np.sin(uu)
    v = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    i = np.arange(nu)[:, None]
    j = np.arange(nv)[None, :]
    a = i * nv + j
    b = ((i + 1) % nu) * nv + j
    c = ((i + 1) % nu) * nv + (j + 1) % nv
    d = i * nv + (j + 1) % nv
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)], 0)
    return v, f.astype(np.int32)


def rigged_tube(rings=16, segments=12, joints=4, radius=0.2, height=1.2):
    """A capped tube along y with a chain of `joints` joints on its axis: (vertices [V, 3] float32, faces
    [F, 3] int32 wound outwards, joint positions [J, 3] float32, parents [J] int32, weights [V, 2] float32,
    indices [V, 2] int32).  V = rings * segments + 2 (the cap centres last), F = 2 segments rings.  Joint j sits
    at y = -height / 2 + j height / joints with joint j - 1 its parent; a vertex between joints j and j + 1 is
    weighted linearly between the two (K = 2), one above the last joint follows that joint alone (its second
    slot is padding of weight 0)."""
    if rings < 2 or segments < 3 or joints < 1:
        raise ValueError("rigged_tube needs rings >= 2, segments >= 3 and joints >= 1")
    ys = -height / 2 + height * np.arange(rings) / (rings - 1)
    ang = np.arange(segments) * (2 * math.pi / segments)
    ring = np.stack([radius * np.cos(ang), np.zeros(segments), radius * np.sin(ang)], -1)
    v = (ring[None] + np.stack([np.zeros(rings), ys, np.zeros(rings)], -1)[:, None]).reshape(-1, 3)
    v = np.concatenate([v, [[0, -height / 2, 0], [0, height / 2, 0]]])
    i, j = np.arange(rings - 1)[:, None], np.arange(segments)[None, :]
    a, b = i * segments + j, i * segments + (j + 1) % segments
    c, d = a + segments, b + segments
    side = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)])
    s, top = np.arange(segments), (rings - 1) * segments
    bottom_c, top_c = rings * segments, rings * segments + 1
    caps = np.concatenate([np.stack([np.full(segments, bottom_c), s, (s + 1) % segments], -1),
                           np.stack([np.full(segments, top_c), top + (s + 1) % segments, top + s], -1)])
    f = np.concatenate([side, caps]).astype(np.int32)
    jy = -height / 2 + height * np.arange(joints) / joints
    c_j = np.stack([np.zeros(joints), jy, np.zeros(joints)], -1)
    parents = np.arange(joints, dtype=np.int32) - 1
    pos = np.clip((v[:, 1] + height / 2) / (height / joints), 0, None)  # in bone lengths above joint 0
    lo = np.minimum(pos.astype(np.int64), joints - 1)
    frac = np.where(lo < joints - 1, pos - lo, 0.)
    indices = np.stack([lo, np.minimum(lo + 1, joints - 1)], -1).astype(np.int32)
    weights = np.stack([1 - frac, frac], -1)
    return (v.astype(np.float32), f, c_j.astype(np.float32), parents, weights.astype(np.float32), indices)


def bent(vertices, angle=1.0):
    """`vertices` [V, 3] bent in the x-y plane about the z axis: the y axis becomes an arc that turns by
    `angle` rad over the mesh's height, the arc length kept, cross-sections staying rigid (float64 in, the
    input's dtype out).  A non-rigid deformation that is locally a rotation: what an ARAP term leaves alone."""
    v = np.asarray(vertices, np.float64)
    lo, hi = v[:, 1].min(), v[:, 1].max()
    if not angle or hi <= lo:
        return np.asarray(vertices).copy()
    k = angle / (hi - lo)  # curvature; the centre of the arc is at x = 1 / k
    t = k * (v[:, 1] - lo)
    r = 1. / k - v[:, 0]
    out = np.stack([1. / k - r * np.cos(t), lo + r * np.sin(t), v[:, 2]], -1)
    return out.astype(np.asarray(vertices).dtype)


def subdivide(v, f, vt=None, ft=None):
    """Midpoint subdivision: every triangle into 4 (shared edge midpoints, computed in float64);
    the same on the uv mesh when given.  SURVEY.md section 8d: the car 4e49873... (F=3644) once
    subdivided is the "ShapeNet car ~15k faces" of BASELINE config 3 (F=14576)."""
    def split(verts, faces):
        cache, out_v, nf = {}, [tuple(x) for x in verts], []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                out_v.append(tuple((np.asarray(out_v[a], np.float64) + np.asarray(out_v[b], np.float64)) / 2))
                cache[key] = len(out_v) - 1
            return cache[key]
        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        return np.asarray(out_v, np.float32), np.asarray(nf, np.int32)
    v2, f2 = split(v, f)
    if vt is None:
        return v2, f2
    vt2, ft2 = split(vt, ft)
    return v2, f2, vt2, ft2


def viewpoints(batch_size, distance=2.732, seed_base=2000):
    out = []
    for b in range(batch_size):
        r = np.random.RandomState(seed_base + b)
        el = r.uniform(-30, 30)
        az = r.uniform(0, 360)
        el, az = np.radians(el), np.radians(az)
        out.append((distance * np.cos(el) * np.sin(az), distance * np.sin(el),
                    -distance * np.cos(el) * np.cos(az)))
    return np.asarray(out, np.float32)


def jittered(vertices, batch_size, sigma=0.01, seed_base=1000):
    out = np.empty((batch_size,) + vertices.shape, np.float32)
    for b in range(batch_size):
        r = np.random.RandomState(seed_base + b)
        out[b] = vertices + r.normal(0, sigma, vertices.shape).astype(np.float32)
    return out


def project(vertices, eyes, viewing_angle=30.0):
    """look_at (at=0, up=+y) + perspective, per item, float32 torch ops on the input's device.
    Equivalent to the reference Renderer.transform_vertices (renderer.py:24-35) for B != 3."""
    from .look_at import look_at
    from .perspective import perspective
    return perspective(look_at(vertices, eyes), angle=viewing_angle)

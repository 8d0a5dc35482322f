"""Meshes shared by test_mesh_loss.py and test_gpu_mesh_loss.py."""
import math
import os

import numpy as np

from conftest import DATA


def grid_fin():
    """A 5x5 grid patch (vertices 0..24, 32 triangles), a fin face (12, 13, 25) on the interior edge
    12-13 (which then has three faces), and the isolated vertex 26: V 27, F 33."""
    faces = []
    for r in range(4):
        for c in range(4):
            a, b, d, e = 5 * r + c, 5 * r + c + 1, 5 * (r + 1) + c, 5 * (r + 1) + c + 1
            faces += [(a, b, e), (a, e, d)]
    faces.append((12, 13, 25))
    v = np.zeros((27, 3))
    for i in range(25):
        v[i] = (0.25 * (i % 5) - 0.5, 0.25 * (i // 5) - 0.5, 0.05 * math.sin(1.7 * i))
    v[25] = (0.12, 0.0, 0.3)
    v[26] = (0.9, 0.9, 0.9)
    return v, np.asarray(faces, np.int32)


def grid(n):
    """An n x n height-field patch over [-0.5, 0.5]^2, heights 0.05 sin(2 pi x) cos(3 pi y) (slopes below
    0.5: neither flat nor folded), every cell split into two triangles: V n^2, F 2 (n - 1)^2, and
    3 (n - 1)^2 - 2 (n - 1) edges with two faces."""
    c = np.linspace(-0.5, 0.5, n)
    x, y = np.meshgrid(c, c, indexing="xy")
    v = np.stack([x, y, 0.05 * np.sin(2 * math.pi * x) * np.cos(3 * math.pi * y)], -1).reshape(-1, 3)
    a = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([a, a + 1, a + n + 1], 1), np.stack([a, a + n + 1, a + n], 1)])
    return v, f.astype(np.int32)


def hinge(phi):
    """Two unit-sized triangles on the shared edge (0, 1); the opposite vertices 2 and 3 stand at the
    angle phi about that edge (phi = pi: flat)."""
    v = np.array([[0., 0., 0.], [1., 0., 0.], [0.5, 1., 0.], [0.5, math.cos(phi), math.sin(phi)]])
    return v, np.array([[0, 1, 2], [1, 0, 3]], np.int32)


def fan(n=70):
    """n triangles round vertex 0 (a closed cone): the centre's degree is above the wave width."""
    ang = np.arange(n) * (2 * math.pi / n)
    v = np.concatenate([[[0., 0., 0.4]], np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], 1)])
    rim = np.arange(n)
    return v, np.stack([np.zeros(n, np.int64), 1 + rim, 1 + (rim + 1) % n], 1).astype(np.int32)


def teapot():
    import neural_renderer_v2_pytorch_amd as nr
    v, f = nr.load_obj(os.path.join(DATA, "teapot.obj"))
    return np.asarray(v, np.float64), np.asarray(f, np.int32)


def jitter(v, B, sigma, seed):
    """[B, V, 3] float64: v plus N(0, sigma) noise from RandomState(seed)."""
    return np.asarray(v, np.float64)[None] + np.random.RandomState(seed).normal(0., sigma, (B,) + v.shape)

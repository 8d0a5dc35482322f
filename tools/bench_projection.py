"""Times one forward + backward of the calibrated camera: the fused path (camera.projection_transform)
against the torch composition (projection.projection) on the same float32 GPU tensors, at the teapot's
vertex count with B = 4 and the car's with B = 64.  Gradients go to vertices, K, R, t and dist_coeffs.

Per shape and path: wall-clock per step (host time of a synchronised loop) and GPU time per step (a pair
of events around each step: first kernel start to last kernel end), over 50 warm-up and 100 timed steps.
Prints one JSON line.

    python tools/bench_projection.py [--steps 100] [--warmup 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import neural_renderer_v2_pytorch_amd as nr  # noqa: E402
from neural_renderer_v2_pytorch_amd import camera  # noqa: E402

DATA = os.path.join(ROOT, "tests", "data")
S = 256


def inputs(path, B, dev):
    v = nr.load_obj(path)[0]
    r = np.random.RandomState(0)
    q = np.linalg.qr(r.normal(size=(B, 3, 3)))[0]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    K = np.tile(np.array([[2. * S, 0., S / 2.], [0., 2. * S, S / 2.], [0., 0., 1.]]), (B, 1, 1))
    t = np.concatenate((r.uniform(-0.2, 0.2, (B, 2)), r.uniform(2., 3., (B, 1))), 1)
    d = r.uniform(-0.05, 0.05, (B, 5))
    x = [np.tile(v[None], (B, 1, 1)), K, q, t, d]
    x = [torch.as_tensor(a, dtype=torch.float32, device=dev).requires_grad_(True) for a in x]
    g = torch.as_tensor(r.normal(size=(B, v.shape[0], 3)), dtype=torch.float32, device=dev)
    return x, g


def time_path(fn, x, g, warmup, steps):
    def step():
        for a in x:
            a.grad = None
        fn(*x, S).backward(g)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    starts = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    ends = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    t0 = time.perf_counter()
    for i in range(steps):
        starts[i].record()
        step()
        ends[i].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps * 1e3
    gpu = float(np.mean([a.elapsed_time(b) for a, b in zip(starts, ends)]))
    return {"wall_ms": round(wall, 4), "gpu_ms": round(gpu, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    shapes = {"teapot_b4": (os.path.join(DATA, "teapot.obj"), 4),
              "car_b64": (os.path.join(DATA, "4e49873292196f02574b5684eaec43e9", "model.obj"), 64)}
    res = {"steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for name, (path, B) in shapes.items():
        x, g = inputs(path, B, dev)
        fused = time_path(camera.projection_transform, x, g, a.warmup, a.steps)
        composed = time_path(nr.projection, x, g, a.warmup, a.steps)
        res[name] = {"B": B, "V": int(x[0].shape[1]), "fused": fused, "composition": composed,
                     "wall_ratio": round(composed["wall_ms"] / fused["wall_ms"], 2),
                     "gpu_ratio": round(composed["gpu_ms"] / fused["gpu_ms"], 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Times one forward + backward (to vertices and attributes) of the vertex-attribute renderer: the fused path
(nr.rasterize_attributes) against the composition from the Level-1 bindings and torch ops
(nr.rasterize_attributes_torch) on the same float32 GPU tensors, each eager and as a torch.cuda.CUDAGraph
replay, on

  headline_c3    ico-sphere level 4 (5120 faces), B = 64, 256^2 with anti-aliasing, per-item attributes, C = 3
  headline_c16   the same with C = 16
  teapot_c3      tests/data/teapot.obj, B = 4, 256^2 with anti-aliasing, C = 3

Every (shape, path) cell runs in a child process of its own under `timeout`; the first cell that fails ends
the run.  Per cell, over --reps repeats of --steps steps each: eager wall-clock per step (host time of a
synchronised loop), eager GPU time per step (median of the events around each step) and graph-replay GPU
time per step; each as the median of the repeats with their min and max.  The fused cells also time the two
new entry points alone (nr_attributes_forward, nr_attributes_backward: back-to-back calls between two
events) and set them against their kernels' algorithmic bytes and the 8 TB/s HBM roof.  The JSON lines go to
--out (default profiles/attributes_bench.jsonl) and to stdout; the last line holds the acceptance cells:
fused not slower than the composition beyond the spread (max - min of the repeats, the larger of the two
paths') measured in this run.

    python tools/bench_attributes.py [--steps 50] [--warmup 10] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # name: (mesh, B, image size, C)
    "headline_c3": ("ico4", 64, 256, 3),
    "headline_c16": ("ico4", 64, 256, 16),
    "teapot_c3": ("teapot", 4, 256, 3),
}
PATHS = ("fused", "composition")
MODES = ("eager_gpu_ms", "eager_wall_ms", "graph_ms")
HBM_ROOF = 8.0e12  # bytes / s


def entry_bytes(B, F, V, Va, C, S, s, fg):
    """Algorithmic bytes of the two entry points: every array read or written once (4-byte elements); fg =
    foreground internal pixels, which alone read a face record (64 B) and gather 3 rows of C attributes."""
    px = B * S * S
    fwd = 4 * px + fg * (64 + 12 + 12 * C) + 4 * px * C + 4 * B * C * s * s
    rec = 4 * B * F * 3 * (3 + C)
    bwd = (4 * px + fg * (64 + 12 + 12 * C) + 4 * px * C + 4 * B * C * s * s  # k_attr_bwd: maps, image, upstream
           + 2 * rec                                                          # zero fill, atomics
           + rec + 12 * B * V + 4 * B * Va * C)                               # the two sums
    return {"nr_attributes_forward": fwd, "nr_attributes_backward": bwd}


def stats(values):
    import numpy as np
    return {"median": round(float(np.median(values)), 5), "min": round(min(values), 5), "max": round(max(values), 5)}


def cell(shape, path, warmup, steps, reps):
    import numpy as np
    import torch
    import neural_renderer_v2_pytorch_amd as nr
    from neural_renderer_v2_pytorch_amd import _lib, synthetic
    from neural_renderer_v2_pytorch_amd.topology import vertex_adjacency

    mesh, B, s, C = SHAPES[shape]
    dev = torch.device("cuda:0")
    if mesh == "ico4":
        v, f = synthetic.icosphere(4)
    else:
        v, f = nr.load_obj(os.path.join(ROOT, "tests", "data", "teapot.obj"))
        v, f = np.asarray(v, np.float32), np.asarray(f)
    vb = torch.as_tensor(synthetic.jittered(np.asarray(v, np.float32), B))
    proj = synthetic.project(vb, torch.as_tensor(synthetic.viewpoints(B))).contiguous().to(dev)
    faces = torch.as_tensor(np.asarray(f), device=dev).int()
    V, F = proj.shape[1], faces.shape[0]
    rs = np.random.RandomState(0)
    pv = proj.clone().requires_grad_(True)
    at = torch.as_tensor(rs.normal(size=(B, V, C)).astype(np.float32), device=dev).requires_grad_(True)
    g = torch.as_tensor(rs.normal(size=(B, C, s, s)).astype(np.float32), device=dev)
    hp = nr.RasterizeHyperparam(image_size=s)
    fn = nr.rasterize_attributes if path == "fused" else nr.rasterize_attributes_torch

    def note(what):
        print("[%s %s] %s" % (shape, path, what), file=sys.stderr, flush=True)

    def step():
        pv.grad = at.grad = None
        out = fn(pv, faces, at, hp)
        out.backward(g)
        return out.detach()

    # warm-up on a side stream, then the capture straight after it (the order of the graph-capture tests)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    note("warm-up done")
    graph = torch.cuda.CUDAGraph()
    pv.grad = at.grad = None
    with torch.cuda.graph(graph):
        gimg = step()
    note("captured")
    for _ in range(warmup):
        graph.replay()
    torch.cuda.synchronize()
    graph_ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        graph_ms.append(a.elapsed_time(b) / steps)
    graph_img = gimg.clone()
    note("replayed")

    starts = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    ends = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    wall_ms, gpu_ms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        for i in range(steps):
            starts[i].record()
            eager_img = step()
            ends[i].record()
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t0) / steps * 1e3)
        gpu_ms.append(float(np.median([a.elapsed_time(b) for a, b in zip(starts, ends)])))
    note("eager done")
    row = {"shape": shape, "path": path, "B": B, "F": F, "V": V, "C": C, "image_size": s, "steps": steps, "reps": reps,
           "eager_gpu_ms": stats(gpu_ms), "eager_wall_ms": stats(wall_ms), "graph_ms": stats(graph_ms),
           "graph_image_equals_eager": bool(torch.equal(graph_img, eager_img)),
           "grad_abs_max": [float(pv.grad.abs().max()), float(at.grad.abs().max())],
           "device": torch.cuda.get_device_name(0)}
    if path != "fused":
        return row

    # the two new entry points alone, on the state a forward leaves (its silhouette-only rasterizer pass is
    # not part of them), back to back on the stream between two events
    L = _lib.lib()
    out = fn(pv, faces, at, hp)
    a_args, fim, frec, internal, vadj, aadj = out.grad_fn.state
    fg = int((fim >= 0).sum())
    S = 2 * s
    images = torch.empty_like(out)
    gv, ga = torch.empty_like(pv), torch.empty_like(at)
    ws = torch.empty(L.nr_attributes_backward_workspace_bytes(B, F, C), dtype=torch.uint8, device=dev)
    st = _lib.stream_of(pv)

    def fwd():
        return L.nr_attributes_forward(a_args, images.data_ptr(), st)

    def bwd():
        return L.nr_attributes_backward(a_args, g.data_ptr(), gv.data_ptr(), ga.data_ptr(), vadj[0].data_ptr(), vadj[1].data_ptr(),
                                        aadj[0].data_ptr(), aadj[1].data_ptr(), ws.data_ptr(), ws.numel(), st)
    nbytes = entry_bytes(B, F, V, V, C, S, s, fg)
    row["foreground_pixels"] = fg
    row["saved_internal_bytes"] = out.grad_fn.internal_bytes
    row["entry_points"] = {}
    for name, call in (("nr_attributes_forward", fwd), ("nr_attributes_backward", bwd)):
        for _ in range(warmup):
            _lib.check(call(), name)
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                call()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) / steps)
        t = stats(times)
        row["entry_points"][name] = {"ms": t, "bytes": nbytes[name],
                                     "tb_per_s": round(nbytes[name] / (t["median"] * 1e-3) / 1e12, 3),
                                     "fraction_of_hbm_roof": round(nbytes[name] / (t["median"] * 1e-3) / HBM_ROOF, 3)}
    note("entry points done")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attributes_bench.jsonl"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per cell")
    ap.add_argument("--cell", nargs=2, metavar=("SHAPE", "PATH"), help="run one cell in this process")
    a = ap.parse_args()
    if a.cell:
        print(json.dumps(cell(a.cell[0], a.cell[1], a.warmup, a.steps, a.reps)))
        return 0
    rows = {}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for shape in SHAPES:
            for path in PATHS:
                cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--steps", str(a.steps),
                       "--warmup", str(a.warmup), "--reps", str(a.reps), "--cell", shape, path]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                if p.returncode != 0:
                    print("cell %s %s ended with status %d: stopping" % (shape, path, p.returncode), file=sys.stderr)
                    return p.returncode
                line = p.stdout.strip().splitlines()[-1]
                rows[(shape, path)] = json.loads(line)
                out.write(line + "\n")
                out.flush()
                print(line, flush=True)
        summary = {"summary": {}, "entry_points": {}}
        for shape in SHAPES:
            fused, comp = rows[(shape, "fused")], rows[(shape, "composition")]
            for mode in MODES:
                f, c = fused[mode], comp[mode]
                spread = max(f["max"] - f["min"], c["max"] - c["min"])
                summary["summary"]["%s/%s" % (shape, mode)] = {
                    "fused": f["median"], "composition": c["median"], "spread": round(spread, 5),
                    "speedup": round(c["median"] / f["median"], 2), "not_slower": f["median"] <= c["median"] + spread}
            summary["entry_points"][shape] = fused["entry_points"]
        line = json.dumps(summary)
        out.write(line + "\n")
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Times one forward + backward of the image losses: the fused path against the torch composition on the same
float32 GPU tensors, each eager and as a torch.cuda.CUDAGraph replay, on

  headline_sq    squared error of images [64, 5, 256, 256] against per-item targets
  headline_iou   IoU of the silhouette channel rgba[:, 3] of [64, 4, 256, 256] (a strided view, read in place)
  torus_sq       squared error of [1, 256, 256] silhouettes (the loss of examples/example2.py)

Every (shape, path) cell runs in a child process of its own under `timeout`; the first cell that fails ends
the run.  Per cell, over --reps repeats of --steps steps each: eager wall-clock per step (host time of a
synchronised loop), eager GPU time per step (median of the events around each step) and graph-replay GPU
time per step; each as the median of the repeats with their min and max.  The fused cells also time the
library's forward and backward entry points alone (back-to-back calls between two events) and set them
against each kernel's algorithmic bytes and the 8 TB/s HBM roof.  The JSON lines go to --out (default
profiles/image_loss_bench.jsonl) and to stdout; the last line holds the acceptance cells: fused not slower
than the composition beyond the spread (max - min of the repeats, the larger of the two paths') measured
in this run.

    python tools/bench_image_loss.py [--steps 200] [--warmup 50] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # name: (leaf shape, loss)
    "headline_sq": ((64, 5, 256, 256), "squared"),
    "headline_iou": ((64, 4, 256, 256), "iou"),
    "torus_sq": ((1, 256, 256), "squared"),
}
PATHS = ("fused", "composition")
MODES = ("eager_gpu_ms", "eager_wall_ms", "graph_ms")
HBM_ROOF = 8.0e12  # bytes / s


def kernel_bytes(loss, B, N):
    """Algorithmic bytes of each fused kernel: every array read or written once (4-byte elements)."""
    chunks = -(-N // 4096)
    if loss == "iou":
        return {"k_iou_fwd": 4 * (2 * B * N + 2 * B * chunks), "k_iou_bwd": 4 * (2 * B * N + 3 * B)}
    return {"k_pointwise_fwd": 4 * (2 * B * N + B * chunks), "k_pointwise_bwd": 4 * (3 * B * N + B)}


def stats(values):
    import numpy as np
    return {"median": round(float(np.median(values)), 5), "min": round(min(values), 5), "max": round(max(values), 5)}


def cell(shape, path, warmup, steps, reps):
    import numpy as np
    import torch
    import neural_renderer_v2_pytorch_amd as nr
    from neural_renderer_v2_pytorch_amd import _lib, image_loss

    leaf_shape, loss = SHAPES[shape]
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    leaf = torch.as_tensor(rs.uniform(0, 1, leaf_shape).astype(np.float32), device=dev).requires_grad_(True)
    view = (lambda a: a[:, 3]) if shape == "headline_iou" else (lambda a: a)
    B = leaf_shape[0]
    N = int(view(leaf)[0].numel())
    tshape = tuple(view(leaf).shape)
    if loss == "iou":
        t = torch.as_tensor((rs.uniform(0, 1, tshape) < 0.4).astype(np.float32), device=dev)
        fn = nr.iou_loss if path == "fused" else nr.iou_loss_torch
    else:
        t = torch.as_tensor(rs.uniform(0, 1, tshape).astype(np.float32), device=dev)
        fn = nr.squared_error_loss if path == "fused" else nr.squared_error_loss_torch
    g = torch.as_tensor(rs.normal(size=B).astype(np.float32), device=dev)

    def note(what):
        print("[%s %s] %s" % (shape, path, what), file=sys.stderr, flush=True)

    def step():
        # returns the detached loss: no reference to the autograd graph outlives a step (tools/bench_mesh_loss.py)
        leaf.grad = None
        out = fn(view(leaf), t)
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
    leaf.grad = None
    with torch.cuda.graph(graph):
        gloss = step()
    ggrad = leaf.grad
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
    graph_loss, graph_grad = gloss.clone(), ggrad.clone()
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
            eager_loss = step()
            ends[i].record()
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t0) / steps * 1e3)
        gpu_ms.append(float(np.median([a.elapsed_time(b) for a, b in zip(starts, ends)])))
    eager_grad = leaf.grad
    note("eager done")
    same = bool(torch.equal(graph_loss, eager_loss) and torch.equal(graph_grad, eager_grad))
    row = {"shape": shape, "path": path, "loss": loss, "B": B, "N": N, "steps": steps, "reps": reps,
           "eager_gpu_ms": stats(gpu_ms), "eager_wall_ms": stats(wall_ms), "graph_ms": stats(graph_ms),
           "graph_equals_eager": same, "loss_values": [float(v) for v in eager_loss[:2]],
           "device": torch.cuda.get_device_name(0)}
    if path != "fused":
        return row

    # the library's entry points alone: the forward's two launches (chunks, then the per-item sum), the
    # backward's one, back to back on the stream between two events
    L = _lib.lib()
    x = view(leaf).detach()
    istride = x.stride(0) if B > 1 else 0
    tstride = t.stride(0) if B > 1 else 0
    out = torch.empty(B, device=dev)
    sums = torch.empty((B, 2), device=dev)
    grad = torch.empty(tshape, device=dev)
    ws = torch.empty(L.nr_image_loss_workspace_bytes(B, N), dtype=torch.uint8, device=dev)
    st = _lib.stream_of(x)
    if loss == "iou":
        def fwd():
            return L.nr_iou_loss_forward(_lib.ptr(x), istride, _lib.ptr(t), tstride, 1e-6, B, N, _lib.ptr(out), _lib.ptr(sums),
                                         _lib.ptr(ws), ws.numel(), st)

        def bwd():
            return L.nr_iou_loss_backward(_lib.ptr(t), tstride, _lib.ptr(sums), 1e-6, B, N, _lib.ptr(g), _lib.ptr(grad), st)
    else:
        head = (_lib.ptr(x), istride, _lib.ptr(t), tstride, None, 0, 1, _lib.NR_LOSS_SQUARED, 1.0, B, N)

        def fwd():
            return L.nr_pointwise_loss_forward(*head, _lib.ptr(out), _lib.ptr(ws), ws.numel(), st)

        def bwd():
            return L.nr_pointwise_loss_backward(*head, _lib.ptr(g), _lib.ptr(grad), st)
    names = list(kernel_bytes(loss, B, N))
    row["kernels"] = {}
    for name, call in zip(names, (fwd, bwd)):
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
        nbytes = kernel_bytes(loss, B, N)[name]
        s = stats(times)
        row["kernels"][name] = {"ms": s, "bytes": nbytes, "tb_per_s": round(nbytes / (s["median"] * 1e-3) / 1e12, 3),
                                "fraction_of_hbm_roof": round(nbytes / (s["median"] * 1e-3) / HBM_ROOF, 3)}
    assert image_loss._fusable(x, t)
    note("kernels done")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_loss_bench.jsonl"))
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
        summary = {"summary": {}, "kernels": {}}
        for shape in SHAPES:
            fused, comp = rows[(shape, "fused")], rows[(shape, "composition")]
            for mode in MODES:
                f, c = fused[mode], comp[mode]
                spread = max(f["max"] - f["min"], c["max"] - c["min"])
                summary["summary"]["%s/%s" % (shape, mode)] = {
                    "fused": f["median"], "composition": c["median"], "spread": round(spread, 5),
                    "speedup": round(c["median"] / f["median"], 2), "not_slower": f["median"] <= c["median"] + spread}
            summary["kernels"][shape] = fused["kernels"]
        line = json.dumps(summary)
        out.write(line + "\n")
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())

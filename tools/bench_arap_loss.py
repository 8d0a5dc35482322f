"""Times one forward + backward of the ARAP energy (arap_loss with cotangent weights against a fixed rest
shape, gradient to the vertices): the fused path (nr.ArapLoss: weights formed once, then k_arap_fwd,
k_mesh_loss_sum and k_arap_bwd per step) against the torch composition on the same float32 GPU tensors
(nr.arap_loss_torch with the same precomputed weights: index_select / index_add_ and torch.linalg.svd on
[B, V, 3, 3], what a user writes from public torch ops), on the icosphere L4 (V 2562, B 64) and the teapot
(tests/data/teapot.obj, B 4).

tools/bench_mesh_loss.py's protocol: every (shape, path) cell runs in a child process of its own under
`timeout`, and the first cell that fails ends the run.  Per cell: eager wall-clock per step (host time of a
synchronised loop), eager GPU time per step (events around each step, the median) and, for the fused path,
graph-replay GPU time per step; the composition is timed eagerly only (its batched SVD is a library call
that is not relied on to capture).  A cell whose steps are slow is cut to the steps that fit --budget seconds
(at least 5), and says so in "steps".  The JSON lines go to --out (default profiles/arap_loss_bench.jsonl) and
to stdout; the last line holds both times and their ratio per shape.  A record, not a gate.

    python tools/bench_arap_loss.py [--steps 200] [--warmup 50] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"ico4_b64": ("ico4", 64), "teapot_b4": ("teapot", 4)}
PATHS = ("fused", "composition")


def mesh(kind):
    import numpy as np
    import neural_renderer_v2_pytorch_amd as nr
    from neural_renderer_v2_pytorch_amd import synthetic
    if kind == "ico4":
        return synthetic.icosphere(4)
    v, f = nr.load_obj(os.path.join(ROOT, "tests", "data", "teapot.obj"))
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def kernel_bytes(B, V, NN):
    """Algorithmic bytes of each fused kernel: every array read or written once (4-byte elements)."""
    csr = (V + 1) + NN
    return {
        "k_arap_fwd": 4 * (B * V * 3 + V * 3 + NN + csr + B * V * 4 + B * -(-V // 256)),
        "k_arap_bwd": 4 * (B * V * 3 * 2 + V * 3 + NN + csr + B * V * 4 + B),
    }


def cell(shape, path, warmup, steps, budget):
    import numpy as np
    import torch
    import neural_renderer_v2_pytorch_amd as nr
    from neural_renderer_v2_pytorch_amd import synthetic

    kind, B = SHAPES[shape]
    dev = torch.device("cuda:0")
    v, f = mesh(kind)
    faces = torch.as_tensor(f, device=dev)
    topo = nr.mesh_topology(faces, v.shape[0])
    rest = torch.as_tensor(v, device=dev, dtype=torch.float32)
    # the deformed batch: the rest shape bent (locally a rotation) and jittered
    bent = synthetic.bent(np.asarray(v, np.float32), 0.8)
    x = torch.as_tensor(synthetic.jittered(bent, B, sigma=0.005), device=dev, dtype=torch.float32).requires_grad_(True)
    g = torch.as_tensor(np.random.RandomState(0).normal(size=B).astype(np.float32), device=dev)
    weights = nr.cot_weights(rest, topo)  # once, outside the timed step, for both paths
    module = nr.ArapLoss(rest, topo.faces, weights=weights)
    if path == "fused":
        loss_fn = module
    else:
        loss_fn = lambda y: nr.arap_loss_torch(y, rest, topo, weights)  # noqa: E731

    def note(what):
        print("[%s %s] %s" % (shape, path, what), file=sys.stderr, flush=True)

    def step():
        # returns the detached loss: no reference to the autograd graph outlives a step (tools/bench_mesh_loss.py)
        x.grad = None
        loss = loss_fn(x)
        loss.backward(g)
        return loss.detach()

    # three steps tell how many fit the budget
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    per_step = time.perf_counter() - t0
    fit = max(5, int(budget / max(per_step, 1e-6) / 3))
    warmup, steps = min(warmup, fit), min(steps, fit)
    note("%.3f ms per step: %d warm-up + %d timed steps" % (per_step * 1e3, warmup, steps))

    graph_ms = graph_min = same = None
    if path == "fused":
        # warm-up on a side stream, then the capture straight after it (the order of the graph-capture tests)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        x.grad = None
        with torch.cuda.graph(graph):
            gloss = step()
        ggrad = x.grad
        note("captured")
        for _ in range(warmup):
            graph.replay()
        torch.cuda.synchronize()
        reps = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                graph.replay()
            b.record()
            torch.cuda.synchronize()
            reps.append(a.elapsed_time(b) / steps)
        graph_loss, graph_grad = gloss.clone(), ggrad.clone()
        graph_ms, graph_min = round(float(np.median(reps)), 4), round(min(reps), 4)
        note("replayed")

    starts = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    ends = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        starts[i].record()
        eager_loss = step()
        ends[i].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps * 1e3
    gpu = float(np.median([a.elapsed_time(b) for a, b in zip(starts, ends)]))
    note("eager done")
    if path == "fused":
        same = bool(torch.equal(graph_loss, eager_loss) and torch.equal(graph_grad, x.grad))
    return {"shape": shape, "path": path, "B": B, "V": int(v.shape[0]), "F": int(f.shape[0]),
            "neighbours": int(topo.nbr_index.shape[0]), "steps": steps, "warmup": warmup, "eager_wall_ms": round(wall, 4),
            "eager_gpu_ms": round(gpu, 4), "graph_ms": graph_ms, "graph_ms_min": graph_min, "graph_equals_eager": same,
            "loss": [float(t) for t in eager_loss[:2]], "finite": bool(torch.isfinite(x.grad).all()),
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--budget", type=float, default=45., help="seconds of timed and warm-up steps per cell, about")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arap_loss_bench.jsonl"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per cell")
    ap.add_argument("--cell", nargs=2, metavar=("SHAPE", "PATH"), help="run one cell in this process")
    a = ap.parse_args()
    if a.cell:
        print(json.dumps(cell(a.cell[0], a.cell[1], a.warmup, a.steps, a.budget)))
        return 0
    rows = {}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for shape in SHAPES:
            for path in PATHS:
                cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--steps", str(a.steps),
                       "--warmup", str(a.warmup), "--budget", str(a.budget), "--cell", shape, path]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                if p.returncode != 0:
                    print("cell %s %s ended with status %d: stopping" % (shape, path, p.returncode), file=sys.stderr)
                    return p.returncode
                line = p.stdout.strip().splitlines()[-1]
                rows[(shape, path)] = json.loads(line)
                out.write(line + "\n")
                out.flush()
                print(line, flush=True)
        summary = {"summary": {}, "kernel_bytes": {}}
        for shape in SHAPES:
            fused, comp = rows[(shape, "fused")], rows[(shape, "composition")]
            for mode in ("eager_gpu_ms", "eager_wall_ms"):
                summary["summary"]["%s/%s" % (shape, mode)] = {
                    "fused": fused[mode], "composition": comp[mode], "ratio": round(comp[mode] / fused[mode], 2)}
            summary["summary"]["%s/graph_ms" % shape] = {"fused": fused["graph_ms"]}
            summary["kernel_bytes"][shape] = kernel_bytes(fused["B"], fused["V"], fused["neighbours"])
        line = json.dumps(summary)
        out.write(line + "\n")
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())

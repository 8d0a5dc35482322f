"""Times one forward + backward of both mesh regularizers (laplacian_loss + 0.1 flatten_loss, gradient
to the vertices): the fused path against the torch composition on the same float32 GPU tensors, each
eager and as a torch.cuda.CUDAGraph replay, on the torus (V 25000, F 50000, B 1) and the icosphere L4
(V 2562, F 5120, B 64).

Every (shape, path) cell runs in a child process of its own under `timeout`; the first cell that fails
ends the run.  Per cell: eager wall-clock per step (host time of a synchronised loop), eager GPU time
per step (events around each step) and graph-replay GPU time per step.  The JSON lines go to --out
(default profiles/mesh_loss_bench.jsonl) and to stdout; the last line holds the four acceptance cells
(fused not slower than the composition) and each kernel's algorithmic bytes.

    python tools/bench_mesh_loss.py [--steps 200] [--warmup 50] [--out FILE]

--losses edge_cot times cot_laplacian_loss + 0.1 edge_length_loss (target: the mesh's mean edge length)
instead, on the same meshes and in the same way (default --out profiles/mesh_regularizers_bench.jsonl).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"torus_b1": ("torus", 1), "ico4_b64": ("ico4", 64)}
PATHS = ("fused", "composition")


def mesh(kind):
    from neural_renderer_v2_pytorch_amd import synthetic
    return synthetic.torus() if kind == "torus" else synthetic.icosphere(4)


def kernel_bytes(B, V, E2, NN):
    """Algorithmic bytes of each fused kernel: every array read or written once (4-byte elements)."""
    return {
        "k_lap_fwd": 4 * (B * V * 3 * 2 + (V + 1) + NN + B * -(-V // 256)),
        "k_lap_bwd": 4 * (B * V * 3 * 2 + (V + 1) + NN + B),
        "k_flat_fwd<records>": 4 * (B * V * 3 + E2 * 4 + B * E2 * 12 + B * -(-E2 // 256)),
        "k_flat_bwd_gather": 4 * (B * E2 * 12 + (V + 1) + 4 * E2 + B * V * 3 + B),
    }


def kernel_bytes_edge_cot(B, V, F, NN):
    """As kernel_bytes, for the edge-length and cotangent Laplacian kernels (corner lists: 6 F entries)."""
    csr = (V + 1) + NN
    return {
        "k_edge_fwd": 4 * (B * V * 3 + csr + B * -(-V // 256)),
        "k_edge_bwd": 4 * (B * V * 3 * 2 + csr + B),
        "k_cot_face": 4 * (B * V * 3 + F * 3 + B * F * 3),
        "k_cotlap_fwd<saved>": 4 * (B * V * 3 * 2 + csr + (NN + 1) + 6 * F + B * F * 3 + B * NN + B * V + B * -(-V // 256)),
        "k_cotlap_bwd": 4 * (B * V * 3 * 2 + csr + B * NN + B * V + B),
    }


def cell(shape, path, warmup, steps, losses="laplacian_flatten"):
    import numpy as np
    import torch
    import neural_renderer_v2_pytorch_amd as nr
    from neural_renderer_v2_pytorch_amd import synthetic

    kind, B = SHAPES[shape]
    dev = torch.device("cuda:0")
    v, f = mesh(kind)
    faces = torch.as_tensor(f, device=dev)
    topo = nr.mesh_topology(faces, v.shape[0])
    x = torch.as_tensor(synthetic.jittered(v, B, sigma=0.005), device=dev).requires_grad_(True)
    g = torch.as_tensor(np.random.RandomState(0).normal(size=B).astype(np.float32), device=dev)
    if path == "composition":
        lap_fn, flat_fn = nr.laplacian_loss_torch, nr.flatten_loss_torch
    else:
        lap_fn, flat_fn = nr.laplacian_loss, nr.flatten_loss
    if losses == "edge_cot":
        rows, cols = topo.composition_index()[:2]
        target = float((x.detach()[0, rows] - x.detach()[0, cols]).norm(dim=-1).mean())
        edge_fn = nr.edge_length_loss_torch if path == "composition" else nr.edge_length_loss
        lap_fn = nr.cot_laplacian_loss_torch if path == "composition" else nr.cot_laplacian_loss
        flat_fn = lambda y, t: edge_fn(y, t, target)  # noqa: E731
        topo.corner_csr()

    def note(what):
        print("[%s %s] %s" % (shape, path, what), file=sys.stderr, flush=True)

    def step():
        # returns the detached loss: no reference to the autograd graph (and so to the leaf's
        # AccumulateGrad node, which is bound to the stream it was made on) outlives a step.  A step kept
        # alive from the eager loop on the default stream made the capture below synchronise the
        # capturing stream with the default stream.
        x.grad = None
        loss = lap_fn(x, topo) + 0.1 * flat_fn(x, topo)
        loss.backward(g)
        return loss.detach()

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
    eager_grad = x.grad
    note("eager done")
    same = bool(torch.equal(graph_loss, eager_loss) and torch.equal(graph_grad, eager_grad))
    return {"shape": shape, "path": path, "B": B, "V": int(v.shape[0]), "F": int(f.shape[0]), "E2": topo.num_edges,
            "neighbours": int(topo.nbr_index.shape[0]), "eager_wall_ms": round(wall, 4), "eager_gpu_ms": round(gpu, 4),
            "graph_ms": round(float(np.median(reps)), 4), "graph_ms_min": round(min(reps), 4),
            "graph_equals_eager": same, "loss": [float(t) for t in eager_loss[:2]],
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--losses", choices=("laplacian_flatten", "edge_cot"), default="laplacian_flatten")
    ap.add_argument("--out", default=None, help="default: profiles/mesh_loss_bench.jsonl, or "
                    "profiles/mesh_regularizers_bench.jsonl with --losses edge_cot")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per cell")
    ap.add_argument("--cell", nargs=2, metavar=("SHAPE", "PATH"), help="run one cell in this process")
    a = ap.parse_args()
    edge_cot = a.losses == "edge_cot"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "mesh_regularizers_bench.jsonl" if edge_cot else "mesh_loss_bench.jsonl")
    if a.cell:
        row = cell(a.cell[0], a.cell[1], a.warmup, a.steps, a.losses)
        if edge_cot:
            row["losses"] = a.losses
        print(json.dumps(row))
        return 0
    rows = {}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for shape in SHAPES:
            for path in PATHS:
                cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--steps", str(a.steps),
                       "--warmup", str(a.warmup), "--losses", a.losses, "--cell", shape, path]
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
            for mode in ("eager_gpu_ms", "eager_wall_ms", "graph_ms"):
                summary["summary"]["%s/%s" % (shape, mode)] = {
                    "fused": fused[mode], "composition": comp[mode],
                    "speedup": round(comp[mode] / fused[mode], 2), "not_slower": fused[mode] <= comp[mode]}
            if edge_cot:
                summary["kernel_bytes"][shape] = kernel_bytes_edge_cot(fused["B"], fused["V"], fused["F"], fused["neighbours"])
            else:
                summary["kernel_bytes"][shape] = kernel_bytes(fused["B"], fused["V"], fused["E2"], fused["neighbours"])
        line = json.dumps(summary)
        out.write(line + "\n")
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())

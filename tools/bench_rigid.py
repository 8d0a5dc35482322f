"""Times rigid registration: rigid_align (scale=True), forward + backward with gradients to x, between a jittered
copy of a mesh's vertices and a rotated, shifted and differently jittered copy of them, and a 20-iteration icp of the
one onto the other, each on tools/bench_point_loss.py's shapes: the icosphere L4 (V 2562, B 64) and the torus
(V 25000, B 1).  The fused path against the torch composition (rigid_align_torch / icp_torch) on the same float32
GPU tensors.

Every (cell, path) runs in a child process of its own under `timeout`; the first one that fails ends the run.  Per
cell: eager wall-clock per step (host time of a synchronised loop), eager GPU time per step (the median of events
around each step), the peak device memory of the eager loop, and for the fused path the GPU time per step of a
torch.cuda.CUDAGraph replay (the composition is not captured: torch.linalg.svd is not, and its icp runs a hundred
chunks an update).  The icp composition runs 3 timed steps after 1 warm-up.  The JSON lines go to --out (default
profiles/rigid_bench.jsonl) and to stdout; the last line holds the ratios, the fused kernels' algorithmic bytes per
step (rigid_align) and per update (icp), and icp's nearest-neighbour pairs per second.

    python tools/bench_rigid.py [--steps 100] [--warmup 20] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"ico4_b64": ("ico4", 64), "torus_b1": ("torus", 1)}
CELLS = [(what, s) for what in ("rigid_align", "icp") for s in SHAPES]
PATHS = ("fused", "composition")
ICP_ITERATIONS = 20
ICP_COMPOSITION_STEPS, ICP_COMPOSITION_WARMUP = 3, 1


def kernel_bytes(B, N, M):
    """Algorithmic bytes of the fused kernels, every array read or written once (4-byte elements): rigid_align's
    forward and backward, and one icp update (the targets' re-reads by further query blocks are not counted)."""
    chunks = (N + 1023) // 1024
    moments = 4 * (2 * B * N * 3 + B * chunks * (8 + 12))
    return {
        "rigid_align": {"k_rigid_sums": 4 * (2 * B * N * 3 + B * chunks * 8), "k_rigid_moments": moments,
                        "k_rigid_solve": 4 * B * (chunks * 20 + 9 + 3 + 1 + 1 + 32), "k_rigid_bwd_item": 4 * B * (32 + 13 + 16),
                        "k_rigid_bwd_points": 4 * (2 * B * N * 3 + B * N * 3 + B * (32 + 16))},
        "icp_update": {"k_icp_nn": 4 * (B * N * 3 + B * M * 3 + 2 * B * N + 13 * B),
                       "k_rigid_sums": 4 * (2 * B * N * 3 + 2 * B * N + B * chunks * 8), "k_rigid_moments": moments + 4 * 2 * B * N,
                       "k_rigid_solve": 4 * B * (chunks * 20 + 13 + 1)},
    }


def cell(what, shape, path, warmup, steps):
    import numpy as np
    import torch
    import neural_renderer_v2_pytorch_amd as nr
    from neural_renderer_v2_pytorch_amd import synthetic

    kind, B = SHAPES[shape]
    fused = path == "fused"
    if what == "icp" and not fused:
        warmup, steps = min(warmup, ICP_COMPOSITION_WARMUP), min(steps, ICP_COMPOSITION_STEPS)
    dev = torch.device("cuda:0")
    v, _ = synthetic.torus() if kind == "torus" else synthetic.icosphere(4)
    V = int(v.shape[0])
    x = torch.as_tensor(synthetic.jittered(v, B, sigma=0.005), device=dev)
    other = torch.as_tensor(synthetic.jittered(v, B, sigma=0.005, seed_base=2000), device=dev)
    c, s = float(np.cos(0.2)), float(np.sin(0.2))
    R0 = torch.tensor([[c, -s, 0.], [s, c, 0.], [0., 0., 1.]], device=dev)
    y = (1.1 * other @ R0.t() + torch.tensor([0.05, -0.02, 0.03], device=dev)).contiguous()
    rng = np.random.RandomState(0)
    gR, gt, gs = (torch.as_tensor(rng.normal(size=shape_).astype(np.float32), device=dev) for shape_ in ((B, 3, 3), (B, 3), (B,)))
    if what == "rigid_align":
        x.requires_grad_(True)
        fn = nr.rigid_align if fused else nr.rigid_align_torch
    else:
        fn = nr.icp if fused else nr.icp_torch

    def note(msg):
        print("[%s %s %s] %s" % (what, shape, path, msg), file=sys.stderr, flush=True)

    def step():
        if what == "icp":
            res = fn(x, y, iterations=ICP_ITERATIONS)
            return torch.cat([res.R.reshape(B, 9), res.t, res.rmse[:, -1:]], 1)
        x.grad = None
        R, t, sc = fn(x, y, None, True)
        torch.autograd.backward((R, t, sc), (gR, gt, gs))
        return torch.cat([R.detach().reshape(B, 9), t.detach(), sc.detach()[:, None]], 1)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    note("warm-up done")
    reps, same = [], None
    if fused:
        graph = torch.cuda.CUDAGraph()
        x.grad = None
        with torch.cuda.graph(graph):
            gout = step()
        ggrad = x.grad
        for _ in range(warmup):
            graph.replay()
        torch.cuda.synchronize()
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                graph.replay()
            b.record()
            torch.cuda.synchronize()
            reps.append(a.elapsed_time(b) / steps)
        graph_out, graph_grad = gout.clone(), None if ggrad is None else ggrad.clone()
        note("replayed")

    starts = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    ends = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for i in range(steps):
        starts[i].record()
        eager_out = step()
        ends[i].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps * 1e3
    gpu = float(np.median([a.elapsed_time(b) for a, b in zip(starts, ends)]))
    peak = torch.cuda.max_memory_allocated() - base
    note("eager done")
    if fused:  # no float atomics anywhere: bitwise
        same = bool(torch.equal(graph_out, eager_out) and (graph_grad is None or torch.equal(graph_grad, x.grad)))
    return {"cell": what, "shape": shape, "path": path, "B": B, "N": V, "M": V, "steps": steps,
            "eager_wall_ms": round(wall, 4), "eager_gpu_ms": round(gpu, 4),
            "graph_ms": round(float(np.median(reps)), 4) if reps else None, "graph_ms_min": round(min(reps), 4) if reps else None,
            "peak_step_bytes": int(peak), "graph_equals_eager": same, "out": [float(t) for t in eager_out.reshape(-1)[:13]],
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rigid_bench.jsonl"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per cell")
    ap.add_argument("--cell", nargs=3, metavar=("WHAT", "SHAPE", "PATH"), help="run one cell in this process")
    a = ap.parse_args()
    if a.cell:
        print(json.dumps(cell(a.cell[0], a.cell[1], a.cell[2], a.warmup, a.steps)))
        return 0
    rows = {}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for what, shape in CELLS:
            for path in PATHS:
                cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--steps", str(a.steps),
                       "--warmup", str(a.warmup), "--cell", what, shape, path]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                if p.returncode != 0:
                    print("cell %s %s %s ended with status %d: stopping" % (what, shape, path, p.returncode), file=sys.stderr)
                    return p.returncode
                line = p.stdout.strip().splitlines()[-1]
                rows[(what, shape, path)] = json.loads(line)
                out.write(line + "\n")
                out.flush()
                print(line, flush=True)
        summary = {"summary": {}, "icp_pairs_per_s": {}, "peak_step_bytes": {}, "kernel_bytes": {}}
        for what, shape in CELLS:
            fused, comp = rows[(what, shape, "fused")], rows[(what, shape, "composition")]
            name = "%s/%s" % (what, shape)
            for mode in ("eager_gpu_ms", "eager_wall_ms"):
                summary["summary"]["%s/%s" % (name, mode)] = {"fused": fused[mode], "composition": comp[mode],
                                                              "speedup": round(comp[mode] / fused[mode], 2)}
            summary["summary"][name + "/graph_ms"] = {"fused": fused["graph_ms"]}
            summary["peak_step_bytes"][name] = {"fused": fused["peak_step_bytes"], "composition": comp["peak_step_bytes"]}
            summary["kernel_bytes"][shape] = kernel_bytes(fused["B"], fused["N"], fused["M"])
            if what == "icp":
                pairs = 1.0 * (ICP_ITERATIONS + 1) * fused["B"] * fused["N"] * fused["M"]
                summary["icp_pairs_per_s"][name] = round(pairs / (fused["graph_ms"] * 1e-3), 1)
        line = json.dumps(summary)
        out.write(line + "\n")
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Times the point losses, forward + backward: chamfer_distance (both directions, gradient to x) between
two jittered copies of a mesh's vertices, and sample_points (S = 10000, gradient to the vertices), each on
the icosphere L4 (V 2562, F 5120, B 64) and the torus (V 25000, F 50000, B 1): the fused path against
the torch composition on the same float32 GPU tensors, each eager and as a torch.cuda.CUDAGraph replay.
The point-mesh cells time point_mesh_distance (gradient to the vertices) from N scan points (surface
samples of a differently jittered copy, moved by N(0, 0.01)) to the icosphere L4 at N = 25000, B = 1 and
16, and to the torus at N = 100000, B = 1.  Their composition tests B N F point-face pairs in chunks of
2^20, several seconds a step on the torus: it runs 3 timed steps after 1 warm-up, eager only.
The mesh-point cells time mesh_point_distance (the opposite direction, gradient to the vertices) on the same
three shapes and scan points and on examples/example_scan_fit.py's own (icosphere L3, F 1280, N 5000, B 1), with
the same protocol; the summary gives their point-face tests per second beside the point-mesh cell of the same
shape (the arithmetic per test is identical) and the ratio of the two.

Every (cell, path) runs in a child process of its own under `timeout`; the first one that fails ends the
run.  Per cell: eager wall-clock per step (host time of a synchronised loop), eager GPU time per step
(events around each step), graph-replay GPU time per step, and the peak device memory of the eager loop.
The JSON lines go to --out (default profiles/point_loss_bench.jsonl) and to stdout; the last line holds
the acceptance cells (fused not slower than the composition), the pair rate of the fused chamfer cells
(both directions: 2 B N M pairs per step over the graph-replay time, which also holds the backward), each
kernel's algorithmic bytes and the registers the compiler reports for it; for the point-mesh cells also the
point-face tests per second (B N F over the fused graph-replay time, backward included).

    python tools/bench_point_loss.py [--steps 100] [--warmup 20] [--out FILE] [--only chamfer|sample|point_mesh|mesh_point]

With --only the rows and a summary of those cells alone are appended to --out; without it the file is rewritten.
--only mesh_point runs the point_mesh cells again as well, so that both rates come from one run: the file then
holds a second set of point_mesh rows, and the ones to read beside the mesh_point rows are those just before them.
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
PM_SHAPES = {"ico4_n25k_b1": ("ico4", 1, 25000), "ico4_n25k_b16": ("ico4", 16, 25000), "torus_n100k_b1": ("torus", 1, 100000)}
# the point-mesh shapes and examples/example_scan_fit.py's own (icosphere L3: V 642, F 1280; 5000 scan points)
MP_SHAPES = dict(PM_SHAPES, ico3_n5k_b1=("ico3", 1, 5000))
PAIR_SHAPES = {"point_mesh": PM_SHAPES, "mesh_point": MP_SHAPES}  # the cells that test B N F point-face pairs
CELLS = ([("chamfer", s) for s in SHAPES] + [("sample", s) for s in SHAPES] + [("point_mesh", s) for s in PM_SHAPES] +
         [("mesh_point", s) for s in MP_SHAPES])
PM_COMPOSITION_STEPS, PM_COMPOSITION_WARMUP = 3, 1
# VALU instructions of k_point_face_nn's inner loop per point-face test: 230 per face and four queries in the gfx950
# assembly (hipcc -S with the build's flags; tools/isa_cost.py weighs the same block)
PM_LOOP_VALU_PER_TEST = 57.5
# the same for k_face_point_nn: 229 per four points of its unrolled loop (bc = ac - ab is loop-invariant there)
FP_LOOP_VALU_PER_TEST = 57.25
PATHS = ("fused", "composition")
SAMPLES = 10000
# VGPRs per lane of each kernel as hipcc reports them for gfx950 (-Rpass-analysis=kernel-resource-usage on
# csrc/nr_raster.hip with the build's flags); 78 allocates 80: 6 waves per SIMD, the rest run at 8
KERNEL_VGPRS = {"k_chamfer_nn": 78, "k_chamfer_combine": 10, "k_chamfer_sum": 18, "k_chamfer_bwd": 32,
                "k_sample_scan": 56, "k_sample_points": 26, "k_sample_points_bwd": 19,
                "k_point_face_records": 52, "k_point_face_nn": 66, "k_point_face_finish": 100, "k_point_mesh_bwd": 30,
                "k_face_point_nn": 50, "k_face_point_finish": 100, "k_face_point_bwd_vertices": 36, "k_face_point_bwd_points": 24}


def mesh(kind):
    from neural_renderer_v2_pytorch_amd import synthetic
    return synthetic.torus() if kind == "torus" else synthetic.icosphere(3 if kind == "ico3" else 4)


def kernel_bytes(B, N, M, F, S):
    """Algorithmic bytes of each fused kernel: every array read or written once (4-byte elements; the
    split path's partials and the targets' re-reads by further blocks are not counted)."""
    return {
        "k_chamfer_nn": 4 * (2 * B * (N + M) * 3 + 2 * B * (N + M)),
        "k_chamfer_sum": 4 * (B * (N + M) + B),
        "k_chamfer_bwd(grad x)": 4 * (B * (N + M) * 3 + B * (N + M) + B * N * 3 + B),
        "k_sample_scan": 4 * (B * F * 3 * 3 + F * 3 + B * F),
        "k_sample_points": 4 * (B * S * (3 + 3 + 1 + 3) + B * S * 9),
        "k_sample_points_bwd": 4 * (B * S * (3 + 1 + 3 + 3) + B * S * 9),
    }


def point_mesh_bytes(B, N, F):
    """The same for the point-mesh kernels (records of 24 floats; the backward's atomics as one read and one write)."""
    return {
        "k_point_face_records": 4 * (B * F * 9 + F * 3 + B * F * 24),
        "k_point_face_nn": 4 * (B * N * 3 + B * F * 24 + 2 * B * N),
        "k_point_face_finish": 4 * (B * N * (1 + 3 + 3 + 9) + B * N * (1 + 1 + 3)),
        "k_point_mesh_bwd": 4 * (B * N * (3 + 1 + 3 + 3 + 9) + B + 2 * B * N * 9),
    }


def face_point_bytes(B, N, F, V):
    """The same for the mesh-point kernels (the vertex gather reads a face's arrays once per corner)."""
    return {
        "k_point_face_records": 4 * (B * F * 9 + F * 3 + B * F * 24),
        "k_face_point_nn": 4 * (B * N * 3 + B * F * 24 + 2 * B * F),
        "k_face_point_finish": 4 * (B * F * (1 + 3 + 3 + 9) + B * F * (1 + 1 + 3)),
        "k_face_point_bwd_vertices": 4 * (V + 1 + 3 * F + 3 * B * F * (1 + 3 + 3 + 3 + 9) + B + B * V * 3),
    }


def cell(what, shape, path, warmup, steps):
    import numpy as np
    import torch
    import neural_renderer_v2_pytorch_amd as nr
    from neural_renderer_v2_pytorch_amd import synthetic

    pairs = what in PAIR_SHAPES
    kind, B = (PAIR_SHAPES[what] if pairs else SHAPES)[shape][:2]
    composed_pm = pairs and path == "composition"
    if composed_pm:
        warmup, steps = min(warmup, PM_COMPOSITION_WARMUP), min(steps, PM_COMPOSITION_STEPS)
    dev = torch.device("cuda:0")
    v, f = mesh(kind)
    V, F = int(v.shape[0]), int(f.shape[0])
    faces = torch.as_tensor(f, device=dev)
    x = torch.as_tensor(synthetic.jittered(v, B, sigma=0.005), device=dev).requires_grad_(True)
    if what == "chamfer":
        y = torch.as_tensor(synthetic.jittered(v, B, sigma=0.005, seed_base=2000), device=dev)
        g = torch.as_tensor(np.random.RandomState(0).normal(size=B).astype(np.float32), device=dev)
        fn = nr.chamfer_distance if path == "fused" else nr.chamfer_distance_torch
    elif pairs:
        N = PAIR_SHAPES[what][shape][2]
        u = torch.as_tensor(np.random.RandomState(1).uniform(0, 1, (B, N, 3)).astype(np.float32), device=dev)
        other = torch.as_tensor(synthetic.jittered(v, B, sigma=0.005, seed_base=2000), device=dev)
        noise = torch.as_tensor(np.random.RandomState(2).normal(scale=0.01, size=(B, N, 3)).astype(np.float32), device=dev)
        y = (nr.sample_points(other, faces, N, u=u) + noise).contiguous()
        g = torch.as_tensor(np.random.RandomState(0).normal(size=B).astype(np.float32), device=dev)
        if what == "point_mesh":
            fn = nr.point_mesh_distance if path == "fused" else nr.point_mesh_distance_torch
        else:
            fn = nr.mesh_point_distance if path == "fused" else nr.mesh_point_distance_torch
    else:
        u = torch.as_tensor(np.random.RandomState(1).uniform(0, 1, (B, SAMPLES, 3)).astype(np.float32), device=dev)
        g = torch.as_tensor(np.random.RandomState(0).normal(size=(B, SAMPLES, 3)).astype(np.float32), device=dev)
        fn = nr.sample_points if path == "fused" else nr.sample_points_torch

    def note(msg):
        print("[%s %s %s] %s" % (what, shape, path, msg), file=sys.stderr, flush=True)

    def step():
        # returns a detached result: no reference to the autograd graph outlives a step (bench_mesh_loss.py)
        x.grad = None
        out = (fn(x, y) if what == "chamfer" else fn(y, x, faces) if what == "point_mesh" else fn(x, faces, y) if what == "mesh_point"
               else fn(x, faces, SAMPLES, u=u))
        out.backward(g)
        return out.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    note("warm-up done")
    reps = []
    if not composed_pm:  # thousands of chunks a step: not captured
        graph = torch.cuda.CUDAGraph()
        x.grad = None
        with torch.cuda.graph(graph):
            gout = step()
        ggrad = x.grad
        note("captured")
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
        graph_out, graph_grad = gout.clone(), ggrad.clone()
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
    # the sampling backward adds with float atomics: its gradient is compared to a tolerance, not bitwise
    # (so does the point-mesh backward to the vertices; the mesh-point backward gathers them: bitwise)
    if composed_pm:
        same = None
    elif what in ("chamfer", "mesh_point"):
        same = bool(torch.equal(graph_out, eager_out) and torch.equal(graph_grad, x.grad))
    else:
        same = bool(torch.equal(graph_out, eager_out) and torch.allclose(graph_grad, x.grad, rtol=1e-4, atol=1e-6))
    return {"cell": what, "shape": shape, "path": path, "B": B, "N": PAIR_SHAPES[what][shape][2] if pairs else V, "M": V, "F": F,
            "S": SAMPLES if what == "sample" else 0, "steps": steps,
            "eager_wall_ms": round(wall, 4), "eager_gpu_ms": round(gpu, 4),
            "graph_ms": round(float(np.median(reps)), 4) if reps else None,
            "graph_ms_min": round(min(reps), 4) if reps else None, "peak_step_bytes": int(peak), "graph_equals_eager": same,
            "out": [float(t) for t in eager_out.reshape(-1)[:2]], "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_loss_bench.jsonl"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per cell")
    ap.add_argument("--only", choices=("chamfer", "sample", "point_mesh", "mesh_point"),
                    help="these cells alone, appended to --out (mesh_point also runs the point_mesh cells, its yardstick)")
    ap.add_argument("--cell", nargs=3, metavar=("WHAT", "SHAPE", "PATH"), help="run one cell in this process")
    a = ap.parse_args()
    if a.cell:
        print(json.dumps(cell(a.cell[0], a.cell[1], a.cell[2], a.warmup, a.steps)))
        return 0
    rows = {}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    # the mesh_point cells are read beside the point_mesh cell of the same shape from the same run
    wanted = (None, a.only, "point_mesh") if a.only == "mesh_point" else (None, a.only)
    cells = [c for c in CELLS if a.only is None or c[0] in wanted]
    with open(a.out, "a" if a.only else "w") as out:
        for what, shape in cells:
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
        summary = {"summary": {}, "pairs_per_s": {}, "point_face_tests_per_s": {}, "mesh_point_rate_over_point_mesh": {},
                   "peak_step_bytes": {}, "kernel_bytes": {},
                   "kernel_vgprs": KERNEL_VGPRS, "point_face_loop_valu_per_test": PM_LOOP_VALU_PER_TEST,
                   "face_point_loop_valu_per_test": FP_LOOP_VALU_PER_TEST}
        for what, shape in cells:
            fused, comp = rows[(what, shape, "fused")], rows[(what, shape, "composition")]
            name = "%s/%s" % (what, shape)
            for mode in ("eager_gpu_ms", "eager_wall_ms", "graph_ms"):
                if comp[mode] is None:
                    continue
                summary["summary"]["%s/%s" % (name, mode)] = {
                    "fused": fused[mode], "composition": comp[mode],
                    "speedup": round(comp[mode] / fused[mode], 2), "not_slower": fused[mode] <= comp[mode]}
            summary["peak_step_bytes"][name] = {"fused": fused["peak_step_bytes"], "composition": comp["peak_step_bytes"]}
            if what == "chamfer":
                summary["pairs_per_s"][name] = round(2.0 * fused["B"] * fused["N"] * fused["M"] / (fused["graph_ms"] * 1e-3), 1)
                summary["kernel_bytes"][shape] = kernel_bytes(fused["B"], fused["N"], fused["M"], fused["F"], SAMPLES)
            if what == "point_mesh":
                summary["point_face_tests_per_s"][name] = round(1.0 * fused["B"] * fused["N"] * fused["F"] / (fused["graph_ms"] * 1e-3), 1)
                summary["kernel_bytes"][shape] = point_mesh_bytes(fused["B"], fused["N"], fused["F"])
            if what == "mesh_point":
                rate = round(1.0 * fused["B"] * fused["N"] * fused["F"] / (fused["graph_ms"] * 1e-3), 1)
                summary["point_face_tests_per_s"][name] = rate
                sibling = summary["point_face_tests_per_s"].get("point_mesh/%s" % shape)
                if sibling:
                    summary["mesh_point_rate_over_point_mesh"][shape] = round(rate / sibling, 3)
                summary["kernel_bytes"]["mesh_point/" + shape] = face_point_bytes(fused["B"], fused["N"], fused["F"], fused["M"])
        line = json.dumps(summary)
        out.write(line + "\n")
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())

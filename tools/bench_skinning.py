"""Times one forward + backward of pose_transforms then skin_vertices (gradients to the pose, the joints and the
vertices): the fused path against the torch composition given dense [V, J] weights -- what a user writes today --
on the same float32 GPU tensors, each eager and as a torch.cuda.CUDAGraph replay, on random rigs of a body's
shape (V 6890, J 24, K 4; B 1 and B 64) and a hand's (V 778, J 16, K 4; B 64).  The rigs come from a fixed seed
(each parent drawn from the four joints before, K distinct joints per vertex): no model file is needed.  Joints
and vertices are per item, as they are after a body model's blend shapes and joint regression.

Every (shape, path, repeat) cell runs in a child process of its own under `timeout`; the first cell that fails
ends the run.  Per cell: eager wall-clock per step (host time of a synchronised loop), eager GPU time per step
(events around each step) and graph-replay GPU time per step.  The JSON lines go to --out (default
profiles/skinning_bench.jsonl) and to stdout; the last line holds, per shape and mode, the three repeats of both
paths, and for the graph replay whether the fused path is faster by more than the spread of the repeats, and each
fused kernel's algorithmic bytes beside the composition's blended [B, V, 3, 4] intermediate.

    python tools/bench_skinning.py [--steps 200] [--warmup 50] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"body_b1": (6890, 24, 4, 1), "body_b64": (6890, 24, 4, 64), "hand_b64": (778, 16, 4, 64)}  # V, J, K, B
PATHS = ("fused", "composition")
MODES = ("eager_gpu_ms", "eager_wall_ms", "graph_ms")


def rig(V, J, K, seed=0):
    """parents [J], indices [V, K] (distinct joints per vertex), weights [V, K] summing to 1, dense [V, J]."""
    import numpy as np
    rng = np.random.RandomState(seed)
    parents = np.array([-1] + [rng.randint(max(0, j - 4), j) for j in range(1, J)], np.int32)
    indices = np.stack([rng.permutation(J)[:K] for _ in range(V)]).astype(np.int32)
    weights = rng.uniform(0.1, 1.0, size=(V, K))
    weights = (weights / weights.sum(1, keepdims=True)).astype(np.float32)
    dense = np.zeros((V, J), np.float32)
    np.put_along_axis(dense, indices.astype(np.int64), weights, 1)
    return parents, indices, weights, dense


def traffic(B, V, J, K, chunks):
    """Algorithmic bytes (every array read or written once, 4-byte elements) of the fused skinning kernels, and of
    the composition's blended-transform intermediate."""
    shared = 4 * (V * K * 2 + B * J * 12)  # indices + weights, and the transforms
    return {
        "k_skin_fwd": shared + 4 * B * V * 3 * 2,
        "k_skin_fwd/shared_inputs": shared,
        "k_skin_fwd/output": 4 * B * V * 3,
        "k_skin_bwd_vertices": shared + 4 * B * V * 3 * 3,
        "k_skin_bwd_transforms": 4 * (B * V * K * (3 + 3) + V * K * 3 + B * chunks * 12),
        "composition/blended_transforms": 4 * B * V * 12,
    }


def cell(shape, path, warmup, steps):
    import numpy as np
    import torch
    import neural_renderer_v2_pytorch_amd as nr

    V, J, K, B = SHAPES[shape]
    dev = torch.device("cuda:0")
    parents, indices, weights, dense = rig(V, J, K)
    rng = np.random.RandomState(1)
    f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=dev)  # noqa: E731
    pose = f32(rng.normal(size=(B, J, 3)) * 0.3).requires_grad_(True)
    joints = f32(rng.uniform(-0.5, 0.5, size=(B, J, 3))).requires_grad_(True)
    vertices = f32(rng.uniform(-0.5, 0.5, size=(B, V, 3))).requires_grad_(True)
    g_out, g_posed = f32(rng.normal(size=(B, V, 3))), f32(rng.normal(size=(B, J, 3)))
    leaves = (pose, joints, vertices)
    chunks = 0
    if path == "composition":
        skel, w = nr.skeleton(parents), f32(dense)
        pose_fn, skin_fn = nr.pose_transforms_torch, nr.skin_vertices_torch
    else:
        skel = nr.skeleton(parents, dev)
        w = nr.skin_binding(f32(weights), torch.as_tensor(indices, device=dev), J)
        chunks = w.num_chunks
        pose_fn, skin_fn = nr.pose_transforms, nr.skin_vertices

    def note(what):
        print("[%s %s] %s" % (shape, path, what), file=sys.stderr, flush=True)

    def step():
        # returns detached outputs only: no reference to the autograd graph outlives a step (bench_mesh_loss.py)
        for t in leaves:
            t.grad = None
        transforms, posed = pose_fn(pose, joints, skel)
        out = skin_fn(vertices, transforms, w)
        torch.autograd.backward((out, posed), (g_out, g_posed))
        return out.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    note("warm-up done")
    graph = torch.cuda.CUDAGraph()
    for t in leaves:
        t.grad = None
    with torch.cuda.graph(graph):
        gout = step()
    ggrads = [t.grad for t in leaves]
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
    graph_out, graph_grads = gout.clone(), [g.clone() for g in ggrads]
    note("replayed")

    starts = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    ends = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        starts[i].record()
        eager_out = step()
        ends[i].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps * 1e3
    gpu = float(np.median([a.elapsed_time(b) for a, b in zip(starts, ends)]))
    note("eager done")
    same = bool(torch.equal(graph_out, eager_out) and all(torch.equal(a, t.grad) for a, t in zip(graph_grads, leaves)))
    return {"shape": shape, "path": path, "B": B, "V": V, "J": J, "K": K, "levels": skel.num_levels, "chunks": chunks,
            "eager_wall_ms": round(wall, 4), "eager_gpu_ms": round(gpu, 4), "graph_ms": round(float(np.median(reps)), 4),
            "graph_ms_min": round(min(reps), 4), "graph_equals_eager": same,
            "out_norm": float(eager_out.double().norm()), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skinning_bench.jsonl"))
    ap.add_argument("--timeout", type=int, default=120, help="seconds per cell")
    ap.add_argument("--cell", nargs=2, metavar=("SHAPE", "PATH"), help="run one cell in this process")
    a = ap.parse_args()
    if a.cell:
        print(json.dumps(cell(a.cell[0], a.cell[1], a.warmup, a.steps)))
        return 0
    rows = {}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for shape in SHAPES:
            for path in PATHS:
                for repeat in range(a.repeats):
                    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--steps",
                           str(a.steps), "--warmup", str(a.warmup), "--cell", shape, path]
                    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                    if p.returncode != 0:
                        print("cell %s %s ended with status %d: stopping" % (shape, path, p.returncode), file=sys.stderr)
                        return p.returncode
                    row = dict(json.loads(p.stdout.strip().splitlines()[-1]), repeat=repeat)
                    rows.setdefault((shape, path), []).append(row)
                    line = json.dumps(row)
                    out.write(line + "\n")
                    out.flush()
                    print(line, flush=True)
        summary = {"summary": {}, "kernel_bytes": {}}
        for shape in SHAPES:
            for mode in MODES:
                fused, comp = ([r[mode] for r in rows[(shape, path)]] for path in PATHS)
                spread = max(max(fused) - min(fused), max(comp) - min(comp))
                entry = {"fused": fused, "composition": comp, "spread": round(spread, 4),
                         "speedup": round(sorted(comp)[len(comp) // 2] / sorted(fused)[len(fused) // 2], 2)}
                if mode == "graph_ms":  # the acceptance: faster by more than the spread of the repeats
                    entry["fused_faster_beyond_spread"] = min(comp) - max(fused) > spread
                summary["summary"]["%s/%s" % (shape, mode)] = entry
            V, J, K, B = SHAPES[shape]
            summary["kernel_bytes"][shape] = traffic(B, V, J, K, rows[(shape, "fused")][0]["chunks"])
        line = json.dumps(summary)
        out.write(line + "\n")
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())

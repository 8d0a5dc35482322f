"""Times one forward + backward of the SSIM loss: the fused path against the torch composition on the same
float32 GPU tensors, each eager and as a torch.cuda.CUDAGraph replay, on

  headline   images [64, 3, 256, 256] against per-item targets, window 11, padding 'same'
  rgb_view   the colour channels rgba[:, :3] of [64, 4, 256, 256] (a strided view, read in place)
  single     images [1, 3, 256, 256]

Every (shape, path) cell runs in a child process of its own under `timeout`; the first cell that fails ends
the run.  Per cell, over --reps repeats of --steps steps each: eager wall-clock per step (host time of a
synchronised loop), eager GPU time per step (median of the events around each step) and graph-replay GPU
time per step; each as the median of the repeats with their min and max.  The fused cells also time the
library's entry points alone (back-to-back calls between two events): the forward without and with the
saved maps, and the backward, each set against its algorithmic bytes and the 8 TB/s HBM roof.  The JSON
lines go to --out (default profiles/ssim_loss_bench.jsonl) and to stdout; the last line holds the acceptance
cells: fused not slower than the composition beyond the spread (max - min of the repeats, the larger of the
two paths') measured in this run.

    python tools/bench_ssim_loss.py [--steps 200] [--warmup 50] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # name: leaf shape
    "headline": (64, 3, 256, 256),
    "rgb_view": (64, 4, 256, 256),
    "single": (1, 3, 256, 256),
}
WINDOW, SIGMA, PADDING = 11, 1.5, "same"
PATHS = ("fused", "composition")
MODES = ("eager_gpu_ms", "eager_wall_ms", "graph_ms")
HBM_ROOF = 8.0e12  # bytes / s


def kernel_bytes(B, N, M):
    """Algorithmic bytes of each fused launch: every array read or written once (4-byte elements); N image
    and M map elements per item."""
    return {"k_ssim_fwd": 4 * (2 * B * N), "k_ssim_fwd_save": 4 * (2 * B * N + 3 * B * M),
            "k_ssim_bwd": 4 * (2 * B * N + 3 * B * M + B * N)}


def stats(values):
    import numpy as np
    return {"median": round(float(np.median(values)), 5), "min": round(min(values), 5), "max": round(max(values), 5)}


def cell(shape, path, warmup, steps, reps):
    import numpy as np
    import torch
    import neural_renderer_v2_pytorch_amd as nr
    from neural_renderer_v2_pytorch_amd import _lib, image_loss

    leaf_shape = SHAPES[shape]
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    leaf = torch.as_tensor(rs.uniform(0, 1, leaf_shape).astype(np.float32), device=dev).requires_grad_(True)
    view = (lambda a: a[:, :3]) if shape == "rgb_view" else (lambda a: a)
    B, C, H, W = view(leaf).shape
    t = torch.as_tensor(rs.uniform(0, 1, (B, C, H, W)).astype(np.float32), device=dev)
    g = torch.as_tensor(rs.normal(size=B).astype(np.float32), device=dev)
    fn = nr.ssim_loss if path == "fused" else nr.ssim_loss_torch

    def note(what):
        print("[%s %s] %s" % (shape, path, what), file=sys.stderr, flush=True)

    def step():
        # returns the detached loss: no reference to the autograd graph outlives a step (tools/bench_mesh_loss.py)
        leaf.grad = None
        out = fn(view(leaf), t, WINDOW, SIGMA, 1.0, PADDING)
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
    row = {"shape": shape, "path": path, "B": B, "C": C, "H": H, "W": W, "window": WINDOW, "padding": PADDING, "steps": steps,
           "reps": reps, "eager_gpu_ms": stats(gpu_ms), "eager_wall_ms": stats(wall_ms), "graph_ms": stats(graph_ms),
           "graph_equals_eager": same, "loss_values": [float(v) for v in eager_loss[:2]],
           "device": torch.cuda.get_device_name(0)}
    if path != "fused":
        return row

    # the library's entry points alone, back to back on the stream between two events: the forward's two
    # launches (tiles, then the per-item sum) without and with the saved maps, and the backward's one
    L = _lib.lib()
    x = view(leaf).detach()
    assert image_loss._fusable(x, t) and image_loss._item_contiguous(x, 1)
    istride = x.stride(0) if B > 1 else 0
    tstride = t.stride(0) if B > 1 else 0
    pad = _lib.NR_SSIM_SAME if PADDING == "same" else _lib.NR_SSIM_VALID
    R = WINDOW // 2
    mh, mw = (H, W) if PADDING == "same" else (H - 2 * R, W - 2 * R)
    N, M = C * H * W, C * mh * mw
    win = (_lib.c_float * WINDOW)(*image_loss._ssim_window(WINDOW, SIGMA).to(torch.float32).tolist())
    out = torch.empty(B, device=dev)
    saved = torch.empty((3, B, C, mh, mw), device=dev)
    grad = torch.empty((B, C, H, W), device=dev)
    ws = torch.empty(L.nr_ssim_loss_workspace_bytes(B, C, H, W, WINDOW, pad), dtype=torch.uint8, device=dev)
    st = _lib.stream_of(x)
    head = (_lib.ptr(x), istride, _lib.ptr(t), tstride)

    def fwd(save):
        return L.nr_ssim_loss_forward(*head, B, C, H, W, WINDOW, win, 1e-4, 9e-4, pad, _lib.ptr(out), _lib.ptr(saved if save else None),
                                      _lib.ptr(ws), ws.numel(), st)

    def bwd():
        return L.nr_ssim_loss_backward(*head, _lib.ptr(saved), B, C, H, W, WINDOW, win, pad, _lib.ptr(g), _lib.ptr(grad), st)
    calls = {"k_ssim_fwd": lambda: fwd(False), "k_ssim_fwd_save": lambda: fwd(True), "k_ssim_bwd": bwd}
    row["kernels"] = {}
    for name, call in calls.items():
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
        nbytes = kernel_bytes(B, N, M)[name]
        s = stats(times)
        row["kernels"][name] = {"ms": s, "bytes": nbytes, "tb_per_s": round(nbytes / (s["median"] * 1e-3) / 1e12, 3),
                                "fraction_of_hbm_roof": round(nbytes / (s["median"] * 1e-3) / HBM_ROOF, 3)}
    note("kernels done")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_loss_bench.jsonl"))
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

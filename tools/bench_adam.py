"""Times one optimiser step: nr.Adam (the fused HIP launch pair) against torch.optim.Adam as the project's
loops used it before (default in eager steps, capturable=True under a graph) and against
torch.optim.Adam(fused=True), the nearest competitor, on

  torus_vertices  one [1, 25000, 3] tensor (the vertices of tools/bench_configs.py cfg5)
  atlas           the car's texture atlas with the gradient of one real backward of the car scene of
                  tools/bench_configs.py (cfg3); its share of exact zeros is printed
  atlas_skip      the same, nr.Adam with skip_zero_grad=True (the torch paths as in `atlas`: they have no skip)
  camera_group    K, R, t and the distortion coefficients: four tiny tensors in one launch

Every (cell, path) runs in a child process of its own under `timeout`; the first one that fails ends the
run.  Per cell, over --reps repeats of --steps steps each: eager GPU time per step (median of the events
around each step), eager wall-clock per step (host time of a synchronised loop) and graph-replay GPU time
per step; each as the median of the repeats with their min and max.  Each row also carries the number of
kernel nodes its captured graph holds.  The nr.Adam rows time nr_adam_step alone (tick + update, back to
back between two events) against the update kernel's algorithmic bytes and the 8 TB/s HBM roof; with
skip_zero_grad the bytes come from the measured gradient: 4 per element, plus 24 per element of every
4-element group that holds a nonzero gradient.  Unless --no-variant is given, the skipping cell is timed a
second time as `atlas_skip_loads_all`, through a build of the library with -DNR_ADAM_SKIP_LOADS_ALL (the
skipping kernel loads everything and only stores conditionally; built next to the library when missing).

A second section times the cfg5 torus step (camera, rasterize, loss, backward, optimiser) as a graph with
torch.optim.Adam(capturable=True) and with nr.Adam, built from bench_configs.cfg5_step's parts: per repeat,
from the initial torus and a zeroed optimiser state, --torus-warmup replays and then --torus-steps timed ones,
once with a synchronisation after every replay (bench_configs.median_step, the protocol of its
graph_ms_per_step) and once back to back between two events.

The JSON lines go to --out (default profiles/adam_bench.jsonl) and to stdout; the last line holds the
acceptance cells: nr.Adam not slower than torch.optim.Adam (the parent's path) beyond the spread (max - min
of the repeats, the larger of the two paths') measured in this run.

    python tools/bench_adam.py [--steps 200] [--warmup 50] [--reps 5] [--out FILE] [--no-variant]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CELLS = ("torus_vertices", "atlas", "atlas_skip", "camera_group")
PATHS = ("nr", "torch", "torch_fused")
MODES = ("eager_gpu_ms", "eager_wall_ms", "graph_ms")
HBM_ROOF = 8.0e12  # bytes / s
VARIANT_LIB = os.path.join(ROOT, "neural_renderer_v2_pytorch_amd", "_lib", "libnr_raster_adam_loads_all.so")
VARIANT_FLAG = "-DNR_ADAM_SKIP_LOADS_ALL"


def stats(values):
    import numpy as np
    return {"median": round(float(np.median(values)), 5), "min": round(min(values), 5), "max": round(max(values), 5)}


def graph_kernel_nodes(graph):
    """Kernel nodes of a captured torch.cuda.CUDAGraph (made with keep_graph=True), or None when this
    torch or HIP build does not expose the graph."""
    import torch
    try:
        raw = graph.raw_cuda_graph()
        hip = None
        for name in (os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"), "libamdhip64.so"):
            try:
                hip = ctypes.CDLL(name)
                break
            except OSError:
                continue
        if hip is None:
            return None
        n = ctypes.c_size_t(0)
        if hip.hipGraphGetNodes(ctypes.c_void_p(raw), None, ctypes.byref(n)) != 0:
            return None
        nodes = (ctypes.c_void_p * n.value)()
        if hip.hipGraphGetNodes(ctypes.c_void_p(raw), nodes, ctypes.byref(n)) != 0:
            return None
        kernels = 0
        for node in nodes:
            kind = ctypes.c_int(-1)
            if hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(kind)) != 0:
                return None
            kernels += kind.value == 0  # hipGraphNodeTypeKernel
        return int(kernels)
    except Exception as e:  # noqa: BLE001 -- a report, not a requirement
        print("graph nodes unavailable: %r" % (e,), file=sys.stderr)
        return None


def count_kernel_nodes(step):
    """Kernel nodes of one captured `step`: a second capture that keeps its graph and is never replayed (the
    timed graph is an ordinary torch.cuda.CUDAGraph)."""
    import torch
    try:
        graph = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        return None
    with torch.cuda.graph(graph):
        step()
    return graph_kernel_nodes(graph)


def atlas_and_gradient(dev):
    """The car's atlas [3, H, W] and its gradient from one real backward of the car scene (cfg3's scene,
    rebuilt from the parts of tools/bench_configs.py)."""
    import numpy as np
    import torch
    import bench_configs as bc
    import neural_renderer_v2_pytorch_amd as nr
    v, f, vt, ft, tex = nr.load_obj(os.path.join(bc.DATA, "4e49873292196f02574b5684eaec43e9", "model.obj"), load_textures=True)
    v, f, vt, ft = bc.subdivide(v, f, vt, ft)
    B, s = 64, 256
    proj = bc.scene(v, f, B, dev)
    tex = torch.as_tensor(np.ascontiguousarray(tex), device=dev).float()
    if tex.shape[0] != 3:
        tex = tex.permute(2, 0, 1).contiguous()
    tex.requires_grad_(True)
    params = nr.RasterizeParam(vertices_textures=torch.as_tensor(vt, device=dev)[None].expand(B, -1, -1),
                               faces_textures=torch.as_tensor(ft, device=dev), textures=tex[None].expand(B, -1, -1, -1))
    torch.manual_seed(0)
    g = torch.randn((B, 4, s, s), device=dev)
    nr.rasterize_rgba(proj, torch.as_tensor(f, device=dev), params, nr.RasterizeHyperparam(image_size=s)).backward(g)
    return tex.detach().clone(), tex.grad.detach().clone().contiguous()


def make_tensors(cell_name, dev):
    """[(initial value, gradient)] of the cell, float32 on the device."""
    import numpy as np
    import torch
    rs = np.random.RandomState(0)
    mk = lambda *shape: torch.as_tensor(rs.normal(size=shape).astype(np.float32), device=dev)
    if cell_name == "torus_vertices":
        return [(mk(1, 25000, 3), mk(1, 25000, 3))]
    if cell_name == "camera_group":
        return [(mk(1, 3, 3), mk(1, 3, 3)), (mk(1, 3, 3), mk(1, 3, 3)), (mk(1, 1, 3), mk(1, 1, 3)), (mk(1, 5), mk(1, 5))]
    return [atlas_and_gradient(dev)]


def cell(cell_name, path, warmup, steps, reps):
    import numpy as np
    import torch
    import neural_renderer_v2_pytorch_amd as nr
    from neural_renderer_v2_pytorch_amd import _lib

    dev = torch.device("cuda:0")
    skip = cell_name.startswith("atlas_skip")
    tensors = make_tensors(cell_name, dev)
    initial = [p.clone() for p, _ in tensors]
    params = [torch.nn.Parameter(p) for p, _ in tensors]
    for p, (_, g) in zip(params, tensors):
        p.grad = g
    numel = sum(p.numel() for p in params)
    row = {"cell": cell_name, "path": path, "tensors": len(params), "numel": numel, "skip_zero_grad": skip, "steps": steps,
           "reps": reps, "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH)}
    if cell_name.startswith("atlas"):
        g = tensors[0][1].reshape(-1)
        zero = float((g == 0).float().mean())
        pad = (-g.numel()) % 4
        groups = torch.nn.functional.pad(g, (0, pad)).reshape(-1, 4)
        live = float((groups != 0).any(1).float().mean())
        row.update(atlas_shape=list(tensors[0][0].shape), zero_share=round(zero, 6), live_group_share=round(live, 6))
        print("[%s %s] atlas %s: %.4f of the gradient is exactly zero, %.4f of the 4-element groups hold a nonzero"
              % (cell_name, path, tuple(tensors[0][0].shape), zero, live), file=sys.stderr, flush=True)

    def make(capturable):
        if path == "nr":
            return nr.Adam(params, skip_zero_grad=skip)
        if path == "torch":  # as the project's loops used it: the default in eager steps, capturable under a graph
            return torch.optim.Adam(params, capturable=True) if capturable else torch.optim.Adam(params)
        return torch.optim.Adam(params, fused=True, capturable=capturable)

    def reset(opt):
        with torch.no_grad():
            for p, p0 in zip(params, initial):
                p.copy_(p0)
            for st in opt.state.values():
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()

    def note(what):
        print("[%s %s] %s" % (cell_name, path, what), file=sys.stderr, flush=True)

    # ---- graph replay: warm-up on a side stream, then the capture straight after it ----
    gopt = make(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            gopt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    reset(gopt)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gopt.step()
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
    row["graph_kernel_nodes"] = count_kernel_nodes(gopt.step)
    note("replayed")

    # ---- eager ----
    eopt = make(False)
    reset(eopt)
    starts = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    ends = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    for _ in range(warmup):
        eopt.step()
    torch.cuda.synchronize()
    wall_ms, gpu_ms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        for i in range(steps):
            starts[i].record()
            eopt.step()
            ends[i].record()
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t0) / steps * 1e3)
        gpu_ms.append(float(np.median([a.elapsed_time(b) for a, b in zip(starts, ends)])))
    note("eager done")
    row.update(eager_gpu_ms=stats(gpu_ms), eager_wall_ms=stats(wall_ms), graph_ms=stats(graph_ms),
               finite=bool(all(torch.isfinite(p).all() for p in params)))
    if path != "nr":
        return row

    # ---- nr_adam_step alone: the tick and the update launch back to back between two events ----
    L = _lib.lib()
    n = len(params)
    state = [[p.detach(), p.grad, torch.zeros_like(p), torch.zeros_like(p), torch.zeros((), device=dev)] for p in params]
    arr = (_lib.NrAdamTensor * n)()
    for d, (p, g, m, v, step) in zip(arr, state):
        d.param, d.grad, d.exp_avg, d.exp_avg_sq, d.step = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr()
        d.numel, d.lr_scale = p.numel(), 1.0
    scratch = torch.empty(L.nr_adam_scratch_bytes(n), dtype=torch.uint8, device=dev)
    args = _lib.NrAdamArgs()
    args.num_tensors = args.tensors_capacity = n
    args.tensors = arr
    args.lr, args.beta1, args.beta2, args.eps = 1e-3, 0.9, 0.999, 1e-8
    args.skip_zero_grad = int(skip)
    args.scratch, args.scratch_bytes = scratch.data_ptr(), scratch.numel()
    st = _lib.stream_of(params[0])
    for _ in range(warmup):
        _lib.check(L.nr_adam_step(ctypes.byref(args), st), "nr_adam_step")
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            L.nr_adam_step(ctypes.byref(args), st)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / steps)
    nbytes = 4 * numel + int(round(24 * numel * row["live_group_share"])) if skip else 28 * numel
    s = stats(times)
    row["nr_adam_step"] = {"ms": s, "update_bytes": nbytes, "tb_per_s": round(nbytes / (s["median"] * 1e-3) / 1e12, 3),
                           "fraction_of_hbm_roof": round(nbytes / (s["median"] * 1e-3) / HBM_ROOF, 3)}
    note("entry point done")
    return row


def torus(optimizer, warmup, steps, reps):
    """The cfg5 torus step as a graph, with the parent's optimiser ('torch': capturable Adam) or nr.Adam."""
    import torch
    import bench_configs as bc
    import neural_renderer_v2_pytorch_amd as nr
    dev = torch.device("cuda:0")
    _, v, f, s, faces, ren, target, verts = bc.cfg5_step(dev)
    ren.viewpoints = torch.as_tensor(ren.viewpoints, dtype=torch.float32, device=dev)
    opt = nr.Adam([verts], lr=0.001) if optimizer == "nr" else torch.optim.Adam([verts], lr=0.001, capturable=True)

    def step():
        loss = ((ren.render_silhouettes(verts, faces) - target) ** 2).sum()
        loss.backward()
        opt.step()
    opt.zero_grad(set_to_none=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    # the vertices move with every step and the step's cost moves with them: every repeat starts from the
    # initial torus and a zeroed optimiser state, so both optimisers are timed over the same steps
    initial = torch.as_tensor(v[None], device=dev)

    def restart():
        with torch.no_grad():
            verts.copy_(initial)
            for st in opt.state.values():
                for x in st.values():
                    if torch.is_tensor(x):
                        x.zero_()
    synced, events = [], []
    for _ in range(reps):
        restart()
        synced.append(bc.median_step(graph.replay, steps, warmup) * 1e3)
        restart()
        for _ in range(warmup):
            graph.replay()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        events.append(a.elapsed_time(b) / steps)
    nodes = count_kernel_nodes(step)
    return {"section": "torus_step", "optimizer": optimizer, "faces": int(f.shape[0]), "image_size": s, "steps": steps,
            "warmup": warmup, "reps": reps,
            "graph_kernel_nodes": nodes, "graph_synced_ms_per_step": stats(synced), "graph_ms": stats(events),
            "finite": bool(torch.isfinite(verts).all()), "device": torch.cuda.get_device_name(0)}


def build_variant():
    """The library with the skipping kernel's load-everything variant, next to the product library."""
    import __graft_entry__ as ge
    ge._build_one(VARIANT_LIB, [VARIANT_FLAG], False, True)
    return VARIANT_LIB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torus-steps", type=int, default=50, help="timed steps of a torus repeat (tools/bench_configs.py's default)")
    ap.add_argument("--torus-warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_bench.jsonl"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per cell")
    ap.add_argument("--no-variant", action="store_true", help="skip the load-everything variant of the skipping kernel")
    ap.add_argument("--cell", nargs=2, metavar=("CELL", "PATH"), help="run one cell in this process")
    ap.add_argument("--torus", metavar="OPTIMIZER", help="run the torus step with this optimiser in this process")
    a = ap.parse_args()
    if a.cell:
        print(json.dumps(cell(a.cell[0], a.cell[1], a.warmup, a.steps, a.reps)))
        return 0
    if a.torus:
        print(json.dumps(torus(a.torus, a.torus_warmup, a.torus_steps, a.reps)))
        return 0
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--reps", str(a.reps)]
    jobs = [((c, p), ["--cell", c, p], {}) for c in CELLS for p in PATHS if not (c == "atlas_skip" and p != "nr")]
    if not a.no_variant:
        jobs.append((("atlas_skip_loads_all", "nr"), ["--cell", "atlas_skip_loads_all", "nr"], {"NR_LIB_PATH": build_variant()}))
    jobs += [(("torus_step", o), ["--torus", o, "--torus-steps", str(a.torus_steps), "--torus-warmup", str(a.torus_warmup)], {})
             for o in ("torch", "nr")]
    rows = {}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for key, extra, env in jobs:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + common + extra
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=dict(os.environ, **env))
            if p.returncode != 0:
                print("%s %s ended with status %d: stopping" % (key + (p.returncode,)), file=sys.stderr)
                return p.returncode
            line = p.stdout.strip().splitlines()[-1]
            rows[key] = json.loads(line)
            out.write(line + "\n")
            out.flush()
            print(line, flush=True)
        summary = {"summary": {}, "nr_adam_step": {}, "graph_kernel_nodes": {}}
        for c in CELLS:
            base = "atlas" if c == "atlas_skip" else c
            mine, parent, rival = rows[(c, "nr")], rows[(base, "torch")], rows[(base, "torch_fused")]
            for mode in MODES:
                f, t = mine[mode], parent[mode]
                spread = max(f["max"] - f["min"], t["max"] - t["min"])
                summary["summary"]["%s/%s" % (c, mode)] = {
                    "nr": f["median"], "torch": t["median"], "torch_fused": rival[mode]["median"], "spread": round(spread, 5),
                    "speedup": round(t["median"] / f["median"], 2), "not_slower": f["median"] <= t["median"] + spread}
            summary["nr_adam_step"][c] = mine["nr_adam_step"]
            summary["graph_kernel_nodes"][c] = {"nr": mine["graph_kernel_nodes"], "torch": parent["graph_kernel_nodes"],
                                                "torch_fused": rival["graph_kernel_nodes"]}
        if ("atlas_skip_loads_all", "nr") in rows:
            summary["nr_adam_step"]["atlas_skip_loads_all"] = rows[("atlas_skip_loads_all", "nr")]["nr_adam_step"]
        f, t = rows[("torus_step", "nr")], rows[("torus_step", "torch")]
        summary["torus_step"] = {k: {"nr": f[k]["median"], "torch": t[k]["median"],
                                     "spread": round(max(f[k]["max"] - f[k]["min"], t[k]["max"] - t[k]["min"]), 5),
                                     "not_slower": f[k]["median"] <= t[k]["median"] + max(f[k]["max"] - f[k]["min"], t[k]["max"] - t[k]["min"])}
                                 for k in ("graph_synced_ms_per_step", "graph_ms")}
        summary["torus_step"]["graph_kernel_nodes"] = {"nr": f["graph_kernel_nodes"], "torch": t["graph_kernel_nodes"]}
        line = json.dumps(summary)
        out.write(line + "\n")
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())

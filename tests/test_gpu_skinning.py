"""The fused pose_transforms and skin_vertices on the GPU (float32) against the torch composition in float64 on
the CPU.

Tolerances and helpers are test_gpu_mesh_loss's: outputs rtol = atol = 1e-5, gradients 1e-4 of the reference
gradient's largest magnitude plus 1e-4 relative.  The cases (skinning_cases.GPU_CASES) draw joints and vertices
uniformly in +-0.5 and the pose with sigma 1.0 up to 24 joints and 0.3 from 65 joints on; every seed is the sum
of the case name's characters, none was picked.  What the composition alone loses in float32 on the CPU against
float64, as the worst share of a tolerance over the committed cases: 0.17 of the output tolerance (the 256-joint
chain's skinned vertices; the 24- and 65-joint cases stay below 0.07) and 0.009 of a gradient tolerance (the same
chain's pose gradient).  tests/test_skinning.py::test_float32_headroom_of_the_gpu_cases recomputes both figures
from the committed cases and asserts that no case uses more than half a tolerance."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from conftest import ROOT
from skinning_cases import GPU_CASES, gpu_case, run
from test_gpu_mesh_loss import close_grads, close_out

pytestmark = pytest.mark.gpu

OUTPUTS, GRADS = ("transforms", "posed", "out"), ("pose", "joints", "vertices", "weights")


def fused(d, dev, **kw):
    return run(d, nr.pose_transforms, nr.skin_vertices, torch.float32, dev, **kw)


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_fused_matches_float64(dev, name):
    d = gpu_case(name)
    got, ref = fused(d, dev), d["ref"]
    for k in OUTPUTS + GRADS:
        assert got[k].dtype == torch.float32 and got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        print("%s %s: max |d| %.3g of scale %.3g" % (name, k, float((got[k].cpu().double() - ref[k]).abs().max()),
                                                     float(ref[k].abs().max())))
    for k in OUTPUTS:
        close_out(got[k], ref[k], "%s %s" % (name, k))
    for k in GRADS:
        close_grads(got[k], ref[k], "%s grad %s" % (name, k))
    J = d["pose"].shape[1]
    if J > 1 and name != "chunk_rows":  # the last joint has no vertices: only g_transforms reaches its transform
        alone = dict(d, g_posed=d["g_posed"] * 0, g_transforms=d["g_transforms"] * 0)
        pose = alone["pose"].to(device=dev, dtype=torch.float32)
        transforms, _ = nr.pose_transforms(pose, alone["joints"].to(device=dev, dtype=torch.float32), d["parents"])
        transforms = transforms.detach().requires_grad_(True)
        out = nr.skin_vertices(d["vertices"].to(device=dev, dtype=torch.float32), transforms,
                               d["weights"].to(device=dev, dtype=torch.float32), d["indices"].to(dev))
        out.backward(d["g_out"].to(device=dev, dtype=torch.float32))
        assert float(transforms.grad[:, J - 1].abs().max()) == 0. and float(transforms.grad.abs().max()) > 0.
    if d["weights"].shape[0] > 2 and name != "chunk_rows":  # the vertex whose weights are all 0 maps to 0
        assert float(got["out"][:, d["weights"].shape[0] // 2].abs().max()) == 0.


def test_dense_learned_weights(dev):
    """A dense [V, J] matrix that requires grad: the same output as its [V, K] form, and its gradient is the
    composition's on the non-zero entries and zero elsewhere."""
    d = gpu_case("j24_tree_v256_k4")
    V, J = d["weights"].shape[0], d["pose"].shape[1]
    idx = d["indices"].long()
    dense64 = torch.zeros((V, J), dtype=torch.float64)
    keep = torch.zeros((V, J), dtype=torch.bool)
    for v in range(V):  # distinct joints only: a joint named twice in a row would add up in the dense form
        seen = set()
        for k in range(idx.shape[1]):
            j = int(idx[v, k])
            if j not in seen and float(d["weights"][v, k]) != 0:
                seen.add(j)
                dense64[v, j] = d["weights"][v, k]
                keep[v, j] = True
    dd = dict(d, weights=dense64, indices=None)

    def with_dense(pose_fn, skin_fn, dtype, device):
        pose = dd["pose"].to(device=device, dtype=dtype)
        w = dd["weights"].detach().to(device=device, dtype=dtype, copy=True).requires_grad_(True)
        transforms, _ = pose_fn(pose, dd["joints"].to(device=device, dtype=dtype), dd["parents"])
        out = skin_fn(dd["vertices"].to(device=device, dtype=dtype), transforms, w)
        out.backward(dd["g_out"].to(device=device, dtype=dtype))
        return out.detach(), w.grad

    out64, gw64 = with_dense(nr.pose_transforms_torch, nr.skin_vertices_torch, torch.float64, "cpu")
    out, gw = with_dense(nr.pose_transforms, nr.skin_vertices, torch.float32, dev)
    close_out(out, out64, "dense out")
    assert gw.shape == (V, J)
    close_grads(gw.cpu() * keep, gw64 * keep, "dense weight grad")
    assert float((gw.cpu() * ~keep).abs().max()) == 0.
    # a step on the weights (their version changes): the next call reads the new values, not a stale copy
    w = dd["weights"].detach().to(device=dev, dtype=torch.float32, copy=True).requires_grad_(True)
    transforms = nr.pose_transforms(dd["pose"].to(device=dev, dtype=torch.float32),
                                    dd["joints"].to(device=dev, dtype=torch.float32), dd["parents"])[0]
    x = dd["vertices"].to(device=dev, dtype=torch.float32)
    first = nr.skin_vertices(x, transforms, w).detach().clone()
    with torch.no_grad():
        w.mul_(0.5)
    assert torch.allclose(nr.skin_vertices(x, transforms, w).detach(), 0.5 * first, rtol=1e-6, atol=1e-7)
    sparse = d["weights"].detach().to(device=dev, dtype=torch.float32, copy=True).requires_grad_(True)
    first = nr.skin_vertices(x, transforms, sparse, d["indices"].to(dev)).detach().clone()
    with torch.no_grad():
        sparse.mul_(0.5)
    assert torch.allclose(nr.skin_vertices(x, transforms, sparse, d["indices"].to(dev)).detach(), 0.5 * first,
                          rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("name", ["j24_forest_v300_k4", "j65_tree_v700_k8_matrix", "chunk_rows"])
def test_runs_are_bitwise_reproducible(dev, name):
    d = gpu_case(name)
    first = fused(d, dev)
    again = fused(d, dev)
    for k in OUTPUTS + GRADS:
        assert torch.equal(first[k], again[k]), k


@pytest.mark.parametrize("name", ["j24_forest_v300_k4", "j65_chain_v700_k4", "j24_tree_v256_k4"])
def test_an_item_does_not_depend_on_its_batch(dev, name):
    """Item b of the batch, bit for bit, is the B = 1 run of that item: outputs and every per-item gradient (the
    gradients of shared inputs and of the weights are sums over the batch and are left out)."""
    d = gpu_case(name)
    whole = fused(d, dev, weights_grad=False)
    per_item = ["pose"] + [k for k in ("joints", "vertices") if d[k].ndim == 3]
    for b in range(d["pose"].shape[0]):
        one = dict(d)
        for k in ("pose", "g_out", "g_posed", "g_transforms") + tuple(per_item[1:]):
            one[k] = d[k][b:b + 1]
        got = fused(one, dev, weights_grad=False)
        for k in OUTPUTS + tuple(per_item):
            assert torch.equal(got[k][0], whole[k][b]), (k, b)


def test_an_item_of_the_item_walking_backward_does_not_depend_on_its_batch(dev):
    """With a weight gradient asked for, batched vertices take their gradient from the kernel whose threads walk the
    items (as shared vertices do): item b's vertex gradient is still, bit for bit, that of its B = 1 run, through
    that kernel and through the one-thread-per-(item, vertex) kernel alike."""
    d = gpu_case("j24_forest_v300_k4")
    assert d["vertices"].ndim == 3
    whole = fused(d, dev, weights_grad=True)
    assert torch.equal(whole["vertices"], fused(d, dev, weights_grad=False)["vertices"])
    for b in range(d["pose"].shape[0]):
        one = dict(d)
        for k in ("pose", "g_out", "g_posed", "g_transforms", "joints", "vertices"):
            one[k] = d[k][b:b + 1]
        for weights_grad in (True, False):
            got = fused(one, dev, weights_grad=weights_grad)
            for k in OUTPUTS + ("pose", "joints", "vertices"):
                assert torch.equal(got[k][0], whole[k][b]), (k, b, weights_grad)


def test_one_hot_zero_pose_is_exact(dev):
    """Zero pose and one weight of exactly 1 per vertex: transforms == [I | 0], posed_joints == joints and
    out == vertices, exactly.  The joints are rounded to multiples of 1/64, where the chain's c_p + (c_j - c_p) is
    exactly c_j (for arbitrary joints it is c_j to within an ulp: test_skinning.py says the same of the composition)."""
    d = gpu_case("j24_forest_v300_k4")
    f32 = lambda k: d[k].to(device=dev, dtype=torch.float32)  # noqa: E731
    pose, joints, vertices = torch.zeros_like(f32("pose")), torch.round(f32("joints") * 64) / 64, f32("vertices")
    transforms, posed = nr.pose_transforms(pose, joints, d["parents"])
    assert torch.equal(transforms, torch.eye(3, 4, device=dev).expand_as(transforms)) and torch.equal(posed, joints)
    weights = torch.zeros_like(f32("weights"))
    weights[:, 1] = 1
    assert torch.equal(nr.skin_vertices(vertices, transforms, weights, d["indices"].to(dev)), vertices)


def test_graph_capture_matches_eager(dev):
    """Forward plus backward of both calls captured once in a HIP graph and replayed after the pose changed in
    place: bit for bit the eager results."""
    d = gpu_case("j24_forest_v300_k4")
    f32 = lambda k: d[k].to(device=dev, dtype=torch.float32)  # noqa: E731
    pose, joints, vertices = f32("pose").requires_grad_(True), f32("joints").requires_grad_(True), f32("vertices").requires_grad_(True)
    weights, indices = f32("weights"), d["indices"].to(dev)
    skel, bind = nr.skeleton(d["parents"], dev), nr.skin_binding(weights, indices, pose.shape[1])
    g_out, g_posed = f32("g_out"), f32("g_posed")
    leaves = (pose, joints, vertices)

    def step(pose, joints, vertices):
        transforms, posed = nr.pose_transforms(pose, joints, skel)
        out = nr.skin_vertices(vertices, transforms, bind)
        ((out * g_out).sum() + (posed * g_posed).sum()).backward()
        return out.detach(), posed.detach()

    def clear():
        for t in leaves:
            t.grad = None

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            clear()
            before = step(*leaves)[0].clone()
    torch.cuda.current_stream().wait_stream(side)
    clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, posed = step(*leaves)
    moved = (0.5 * f32("pose")).contiguous()
    with torch.no_grad():
        pose.copy_(moved)
    graph.replay()
    torch.cuda.synchronize()
    got = [out.clone(), posed.clone()] + [t.grad.clone() for t in leaves]
    eager = (moved.clone().requires_grad_(True), f32("joints").requires_grad_(True), f32("vertices").requires_grad_(True))
    want = list(step(*eager)) + [t.grad for t in eager]
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert not torch.equal(got[0], before)  # the replay saw the new pose


def test_module_and_fallbacks(dev):
    """nr.Skinning gives what the two functions give; float64 GPU inputs take the composition."""
    d = gpu_case("j24_tree_v256_k4")
    f32 = lambda k: d[k].to(device=dev, dtype=torch.float32)  # noqa: E731
    rig = nr.Skinning(d["joints"].float(), d["parents"], d["weights"].float(), d["indices"]).to(dev)
    out, posed = rig(f32("pose"), f32("vertices"))
    transforms, want_posed = nr.pose_transforms(f32("pose"), f32("joints"), d["parents"])
    want = nr.skin_vertices(f32("vertices"), transforms, f32("weights"), d["indices"].to(dev))
    assert torch.equal(out, want) and torch.equal(posed, want_posed)
    t64, p64 = nr.pose_transforms(d["pose"].to(dev), d["joints"].to(dev), d["parents"])
    assert t64.dtype == torch.float64
    close_out(t64, d["ref"]["transforms"], "float64 fallback")
    o64 = nr.skin_vertices(d["vertices"].to(dev), t64, d["weights"].to(dev), d["indices"].to(dev))
    close_out(o64, d["ref"]["out"], "float64 fallback out")


def test_pose_fit_descends(dev):
    """examples/example_pose_fit.py's model at 32 x 32 and 25 steps: the last loss is below the first."""
    spec = importlib.util.spec_from_file_location("example_pose_fit", os.path.join(ROOT, "examples", "example_pose_fit.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    model = example.PoseFit(dev, image_size=32)
    losses = example.optimize(model, 25)
    assert len(losses) == 25 and np.isfinite(losses).all()
    assert losses[-1] < losses[0], losses

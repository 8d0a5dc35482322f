"""The fused icp on the GPU (float32): recovery of known motions on the teapot, one update from a non-identity start
against the float64 composition, rejection, graph capture and reproducibility.

Recovery.  The target is the teapot's 1292 vertices (two LDS tiles), the source every third vertex moved by the
inverse of rigid_cases.MOTIONS (0.3, 0.5 and 0.8 rad).  On the CPU the composition icp_torch reaches exact
correspondences after 10, 14 and 19 updates, in float64 and float32 alike; after 30 its float32 result is off the
known motion by 3.97e-7 in R and 5.36e-8 in t (TEAPOT_FLOAT32_ERROR).  The fused result is allowed 4x that.  Twenty of
the 431 sampled vertices coincide with an earlier vertex: the lower index is the expected one.

One update.  Uniform clouds in [-1, 1]^3 (rigid_cases.ICP_CASES: test_gpu_point_loss's seeds, and for the two cases with
two query blocks seeds whose gap passes), from rigid_cases.icp_init (s = 1.1).  Asserted first, on the float64
reference: under the start every query's nearest and second-nearest distances differ by more than 1e-5 (measured:
6.7e-4, 2.3e-5, 7.3e-3, 5.8e-3, 9.7e-5 and 1.4e-4), which float32 cannot bridge, so the indices must EQUAL the reference's.
R, t and s are compared with rigid_align_torch in float64 on the reference's gathered pairs, by test_gpu_rigid's
protocol: the float32 composition on the CPU is off by at most 3.59e-7 in R, 1.62e-7 in t and 2.14e-7 in s over
these six cases (ONE_UPDATE_FLOAT32_ERROR; items whose float64 condition is at least 0.1), and the fused path is
allowed 4x that."""
import os
import sys

import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import _lib
from conftest import ROOT
from rigid_cases import ICP_CASES, ICP_GAP, ICP_SPLIT, SURE, icp_clouds, icp_first_update, icp_init, teapot_scan

pytestmark = pytest.mark.gpu

TEAPOT_FLOAT32_ERROR = dict(R=3.97e-7, t=5.36e-8)  # measured: float32 icp_torch on the CPU against the known motion
ONE_UPDATE_FLOAT32_ERROR = dict(R=3.59e-7, t=1.62e-7, s=2.14e-7)  # measured: the module docstring


QUERY_ERROR = 2e-6  # see dist2_bound


def dist2_bound(d2):
    """How far a float32 squared distance of a transformed query may be from the reference's d2.  A coordinate of
    s R x + t is at most 2.2 here (|x| <= sqrt(3), s = 1.1, |t| <= 0.2) and comes from some seven float32 operations on
    values no larger, each within half an ulp (1.2e-7) of exact, and from a start rounded to float32: under 1e-6 per
    coordinate, QUERY_ERROR for the vector.  A distance d then moves by at most that, d^2 by 2 d e + e^2, and the
    difference form itself adds five roundings of non-negative terms (test_gpu_point_loss's DIST_RTOL, 1e-6)."""
    return 2 * d2.sqrt() * QUERY_ERROR + QUERY_ERROR ** 2 + 1e-6 * d2


def f32(dev, *tensors):
    return tuple(t.to(device=dev, dtype=torch.float32) for t in tensors)


def test_recovers_the_teapot_motions(dev):
    x, y, R, t, want = teapot_scan()
    assert int((want != torch.arange(0, y.shape[0], 3)).sum()) == 20 and bool((want <= torch.arange(0, y.shape[0], 3)).all())
    res = nr.icp(x.to(dev), y.to(dev), iterations=30)
    assert isinstance(res, nr.ICPResult) and res.rmse.shape == (3, 31) and res.index.dtype == torch.int32
    assert not any(v.requires_grad for v in res)
    err_R, err_t = float((res.R.cpu().double() - R).abs().max()), float((res.t.cpu().double() - t).abs().max())
    print("teapot: R off by %.3g (allowed %.3g), t by %.3g (allowed %.3g), rmse %s" % (
        err_R, 4 * TEAPOT_FLOAT32_ERROR["R"], err_t, 4 * TEAPOT_FLOAT32_ERROR["t"], res.rmse[:, -1].tolist()))
    assert err_R <= 4 * TEAPOT_FLOAT32_ERROR["R"] and err_t <= 4 * TEAPOT_FLOAT32_ERROR["t"]
    assert torch.equal(res.s, torch.ones_like(res.s))
    assert float(res.rmse[:, -1].max()) < 1e-6 and bool((res.rmse[:, 0] > 0.01).all())
    assert torch.equal(res.index.cpu().long(), want[None].expand(3, -1))
    assert float(res.dist2.max()) < 1e-12
    # a single scan against the same target: unbatched results, the same bits
    one = nr.icp(x[1].to(dev), y.to(dev), iterations=30)
    assert one.R.shape == (3, 3) and one.rmse.shape == (31,) and one.index.shape == (x.shape[1],)
    assert torch.equal(one.R, res.R[1]) and torch.equal(one.t, res.t[1]) and torch.equal(one.rmse, res.rmse[1])


@pytest.mark.parametrize("name", list(ICP_CASES))
def test_one_update_from_a_start(dev, name):
    x, y = icp_clouds(name)
    B = x.shape[0]
    index, R, t, s, condition, gap = icp_first_update(name)
    print("%s: distance gap %.3g, condition %s" % (name, gap, condition.tolist()))
    assert gap > ICP_GAP, gap
    init = icp_init(B)
    res = nr.icp(x.to(dev), y.to(dev), iterations=1, scale=True, init=f32(dev, *init))
    split = _lib.last_launch("k_icp_nn")
    assert split[0] == 256 and bool(split[1] & _lib.NR_LAUNCH_SPLIT_TARGETS) == (name in ICP_SPLIT)
    # the first pass's indices, under init: iterations=0 returns init and that pass
    first = nr.icp(x.to(dev), y.to(dev), iterations=0, scale=True, init=f32(dev, *init))
    assert torch.equal(first.index.cpu(), index)
    for got, want in zip(first[:3], f32(dev, *init)):
        assert torch.equal(got, want)
    assert first.rmse.shape == (B, 1)
    q = init[2][:, None, None] * (x.double() @ init[0].transpose(1, 2)) + init[1][:, None]
    d2 = ((q - y.double().gather(1, index.long()[..., None].expand(-1, -1, 3))) ** 2).sum(-1)
    assert bool(((first.dist2.cpu().double() - d2).abs() <= dist2_bound(d2)).all())
    assert float((first.rmse[:, 0].cpu().double() - d2.mean(1).sqrt()).abs().max()) <= 1e-5
    assert torch.equal(first.rmse[:, 0], res.rmse[:, 0])
    # the update
    sure = condition >= SURE
    assert bool(sure.any())
    err = dict(R=float((res.R.cpu().double() - R)[sure].abs().max()), t=float((res.t.cpu().double() - t)[sure].abs().max()),
               s=float((res.s.cpu().double() - s)[sure].abs().max()))
    print("%s: %s allowed 4 x %s" % (name, {k: "%.3g" % v for k, v in err.items()}, ONE_UPDATE_FLOAT32_ERROR))
    for k in err:
        assert err[k] <= 4 * ONE_UPDATE_FLOAT32_ERROR[k], (name, k, err[k])
    Rd = res.R.cpu().double()
    assert float((Rd @ Rd.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-5
    assert bool((torch.linalg.det(Rd) > 0).all())
    # index and dist2 belong to the returned transform
    q = res.s[:, None, None] * (x.to(dev) @ res.R.transpose(1, 2)) + res.t[:, None]
    d2, j = nr.nearest_points(q, y.to(dev))
    close = (res.dist2 - d2).abs() <= 2 * dist2_bound(d2)  # two float32 paths
    assert bool(close.all()) and bool(((res.index == j) | close).all())


def test_shared_target_and_batch_independence(dev):
    x, y = icp_clouds("partial_block")
    init = f32(dev, *icp_init(3))
    shared = nr.icp(x.to(dev), y[0].to(dev), iterations=3, init=init)
    expanded = nr.icp(x.to(dev), y[:1].expand(3, -1, -1).to(dev).contiguous(), iterations=3, init=init)
    alone = nr.icp(x[2:].to(dev), y[0].to(dev), iterations=3, init=tuple(v[2:] for v in init))
    for a, b, c in zip(shared, expanded, alone):
        assert torch.equal(a, b) and torch.equal(a[2:], c)


def test_rejection(dev):
    x, y, R, t, want = teapot_scan()
    x, y = x.to(dev), y.to(dev)
    outliers = torch.cat([x, x[:, :50] + 10.], 1)
    a = nr.icp(x, y, iterations=30, max_distance=0.5)
    b = nr.icp(outliers, y, iterations=30, max_distance=0.5)
    assert float((a.R - b.R).abs().max()) <= 4 * TEAPOT_FLOAT32_ERROR["R"] and float((a.t - b.t).abs().max()) <= 4 * TEAPOT_FLOAT32_ERROR["t"]
    assert float((a.R.cpu().double() - R).abs().max()) <= 4 * TEAPOT_FLOAT32_ERROR["R"]
    assert bool((b.dist2[:, -50:] > 0.25).all()) and torch.equal(b.index[:, :-50].cpu().long(), want[None].expand(3, -1))
    assert float((a.rmse - b.rmse).abs().max()) <= 1e-6 and float(b.rmse[:, -1].max()) < 1e-6
    # every weight 0: the transform stays at init bit for bit and rmse is 0
    init = f32(dev, *icp_init(3))
    none = nr.icp(x + 5., y, iterations=4, scale=True, max_distance=1e-3, init=init)
    for got, start in zip(none[:3], init):
        assert torch.equal(got, start)
    assert torch.equal(none.rmse, torch.zeros_like(none.rmse)) and none.rmse.shape == (3, 5)
    assert bool((none.dist2 > 1e-6).all())


def test_graph_capture_and_reproducibility(dev):
    x, y = (v.to(dev) for v in icp_clouds("partial_block"))
    init = f32(dev, *icp_init(3))

    def step():
        return nr.icp(x, y, iterations=5, scale=True, max_distance=0.8, init=init)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    eager, again = step(), step()
    for a, b in zip(eager, again):
        assert torch.equal(a, b)
    for _ in range(2):
        for v in out:
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(a, b)
    assert bool((eager.rmse[:, -1] < eager.rmse[:, 0]).all())


def test_example_icp(dev):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import example_icp
    out = example_icp.run(example_icp.parser().parse_args([]))
    print("example_icp: rmse %s" % " ".join("%.2e" % r for r in out["rmse"]))
    assert len(out["rmse"]) == 31 and out["rmse"][-1] < 1e-5 and out["rmse"][0] > 0.01
    assert float((out["R"] - out["R0"]).abs().max()) <= 1e-5 and float((out["t"] - out["t0"]).abs().max()) <= 1e-5

"""nr.Adam without a GPU: the torch composition of the rule against a plain numpy restatement and
against torch.optim.Adam, the optimiser's behaviour on CPU tensors (which take the composition), the
zero-gradient skip, the state_dict interchange with torch.optim.Adam, and the C ABI's argument checks
(which return before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import _lib, optimizers
from adam_cases import BETA1, BETA2, EPS, LR, STEPS, inputs, np_trajectory


def run_composition(p0, grads, scale, skip):
    p = torch.as_tensor(p0).clone()
    m, v, step = torch.zeros_like(p), torch.zeros_like(p), torch.zeros((), dtype=torch.float32)
    out = []
    for g in grads:
        nr.adam_step_torch([p], [torch.as_tensor(g)], [m], [v], [step], lr=LR, lr_scales=[scale], beta1=BETA1, beta2=BETA2,
                           eps=EPS, skip_zero_grad=skip)
        out.append(p.numpy().copy())
    assert float(step) == len(grads)
    return np.stack(out), m.numpy(), v.numpy()


def torch_adam_trajectory(p0, grads, dtype=torch.float64):
    p = torch.nn.Parameter(torch.as_tensor(p0, dtype=dtype).clone())
    opt = torch.optim.Adam([p])
    out = []
    for g in grads:
        p.grad = torch.as_tensor(g, dtype=dtype)
        opt.step()
        out.append(p.detach().numpy().copy())
    return np.stack(out)


@pytest.mark.parametrize("skip", [False, True])
def test_composition_matches_numpy(skip):
    """adam_step_torch in float64 against the numpy loop: 30 steps of 5000 elements, gradients over
    10^[-4, 2] with 30 % exact zeros, two tensors with different lr_scales in one call."""
    p0, grads = inputs()
    pa, pb = torch.as_tensor(p0).clone(), torch.as_tensor(p0[::-1].copy())
    state = [torch.zeros_like(pa) for _ in range(4)]
    steps = [torch.zeros((), dtype=torch.float32) for _ in range(2)]
    want_a = np_trajectory(p0, grads, scale=1., skip=skip)
    want_b = np_trajectory(p0[::-1], grads[:, ::-1], scale=0.25, skip=skip)
    for t, g in enumerate(grads):
        nr.adam_step_torch([pa, pb], [torch.as_tensor(g), torch.as_tensor(g[::-1].copy())], state[:2], state[2:], steps, lr=LR,
                           lr_scales=[1., 0.25], beta1=BETA1, beta2=BETA2, eps=EPS, skip_zero_grad=skip)
        np.testing.assert_allclose(pa.numpy(), want_a[0][t], rtol=1e-12, atol=0)
        np.testing.assert_allclose(pb.numpy(), want_b[0][t], rtol=1e-12, atol=0)
    for got, want in ((state[0], want_a[1]), (state[2], want_a[2]), (state[1], want_b[1]), (state[3], want_b[2])):
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=0)
    assert (grads == 0).mean() > 0.25 and np.abs(grads).max() > 50 and np.abs(grads[grads != 0]).min() < 2e-4
    if skip:  # the skip changes the trajectory
        assert np.abs(want_a[0][-1] - np_trajectory(p0, grads)[0][-1]).max() > 1e-6


def test_composition_matches_torch_adam_with_the_defaults():
    """Without the skip and with lr_scale 1 the rule is torch.optim.Adam's: float64 trajectories within
    1e-14 on values of order 1 (the two differ in the order of a few roundings; measured: some 1e-16)."""
    p0, grads = inputs()
    got = run_composition(p0, grads, 1., False)[0]
    want = torch_adam_trajectory(p0, grads)
    err = np.abs(got - want).max()
    print("composition against torch.optim.Adam, float64: max |diff| %.3g" % err)
    assert err <= 1e-14
    assert np.abs(np_trajectory(p0, grads)[0] - want).max() <= 1e-14


@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the fused path was taken")
    monkeypatch.setattr(optimizers._lib, "lib", boom)


def test_cpu_tensors_take_the_composition(no_library):
    p0, grads = inputs()
    for dtype, tol in ((torch.float64, 1e-14), (torch.float32, None)):  # float32: that it runs, and its state
        p = torch.nn.Parameter(torch.as_tensor(p0, dtype=dtype).clone())
        opt = nr.Adam([p])
        got = []
        for g in grads:
            p.grad = torch.as_tensor(g, dtype=dtype)
            opt.step()
            got.append(p.detach().numpy().copy())
        if tol is not None:
            assert np.abs(np.stack(got) - torch_adam_trajectory(p0, grads, dtype)).max() <= tol
        st = opt.state[p]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["step"].dtype == torch.float32 and st["step"].ndim == 0 and float(st["step"]) == STEPS
        assert st["exp_avg"].dtype == dtype


def test_param_groups_take_their_own_options():
    p0, grads = inputs()
    a = torch.nn.Parameter(torch.as_tensor(p0).clone())
    b = torch.nn.Parameter(torch.as_tensor(p0).clone())
    opt = nr.Adam([{"params": [a]}, {"params": [b], "lr": 5e-3, "betas": (0.8, 0.99), "eps": 1e-6, "skip_zero_grad": True}])
    assert opt.param_groups[0]["lr"] == LR and opt.param_groups[0]["skip_zero_grad"] is False
    for g in grads[:10]:
        a.grad, b.grad = torch.as_tensor(g), torch.as_tensor(g)
        opt.step()
    np.testing.assert_allclose(a.detach().numpy(), np_trajectory(p0, grads[:10])[0][-1], rtol=1e-12)
    want_b = np_trajectory(p0, grads[:10], lr=5e-3, beta1=0.8, beta2=0.99, eps=1e-6, skip=True)[0][-1]
    np.testing.assert_allclose(b.detach().numpy(), want_b, rtol=1e-12)


def test_missing_gradient_leaves_the_step_alone():
    a, b = torch.nn.Parameter(torch.ones(4)), torch.nn.Parameter(torch.ones(4))
    opt = nr.Adam([a, b])
    for with_b in (True, False, True):
        a.grad = torch.ones(4)
        b.grad = torch.ones(4) if with_b else None
        before = b.detach().clone()
        opt.step()
        if not with_b:
            assert torch.equal(b.detach(), before)
    assert float(opt.state[a]["step"]) == 3 and float(opt.state[b]["step"]) == 2


def test_param_lr_scales_the_rate_and_zero_freezes():
    p0, grads = inputs()
    a = torch.nn.Parameter(torch.as_tensor(p0).clone())
    b = torch.nn.Parameter(torch.as_tensor(p0).clone())
    a.lr, b.lr = 0.25, 0.
    opt = nr.Adam([a, b])
    for g in grads[:5]:
        a.grad, b.grad = torch.as_tensor(g), torch.as_tensor(g)
        opt.step()
    np.testing.assert_allclose(a.detach().numpy(), np_trajectory(p0, grads[:5], scale=0.25)[0][-1], rtol=1e-12)
    assert np.array_equal(b.detach().numpy(), p0) and len(opt.state[b]) == 0
    b.lr = 1.  # read at every step: the parameter starts moving, from step 1
    b.grad = torch.as_tensor(grads[5])
    opt.step()
    np.testing.assert_allclose(b.detach().numpy(), np_trajectory(p0, grads[5:6])[0][-1], rtol=1e-12)
    assert float(opt.state[b]["step"]) == 1


def test_sparse_gradient_raises():
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        nr.Adam([p]).step()


def test_step_with_closure_returns_the_loss():
    p = torch.nn.Parameter(torch.full((3,), 2., dtype=torch.float64))
    opt = nr.Adam([p], lr=0.1)

    def closure():
        opt.zero_grad()
        loss = (p * p).sum()
        loss.backward()
        return loss
    loss = opt.step(closure)
    assert float(loss.detach()) == 12. and loss.requires_grad
    assert bool((p.detach() < 2).all())


def test_invalid_options_raise():
    p = torch.nn.Parameter(torch.ones(2))
    for kw in ({"lr": -1.}, {"lr": float("nan")}, {"betas": (1., 0.9)}, {"betas": (0.9, -0.1)}, {"eps": -1.}):
        with pytest.raises(ValueError):
            nr.Adam([p], **kw)


def test_skip_semantics():
    """An element with a nonzero gradient at step 1 and zero afterwards keeps moving under the default;
    under skip_zero_grad its p, m and v stay bitwise where step 1 left them.  -0.0 counts as zero; a NaN
    gradient propagates."""
    g1 = torch.tensor([1., -2., 0.5, 3.])
    later = [torch.tensor([0., -0., 0.5, float("nan")]), torch.tensor([-0., 0., 0.25, 0.])]
    result = {}
    for skip in (False, True):
        p = torch.nn.Parameter(torch.ones(4))
        opt = nr.Adam([p], lr=0.1, skip_zero_grad=skip)
        p.grad = g1.clone()
        opt.step()
        st = opt.state[p]
        first = [p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
        for g in later:
            p.grad = g.clone()
            opt.step()
        result[skip] = (first, [p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()])
        assert float(st["step"]) == 3  # the step advances per tensor either way
    first, last = result[False]
    assert bool((last[0][:2] != first[0][:2]).all())  # stale momentum keeps moving the unseen elements
    assert bool((last[1][:2].abs() < first[1][:2].abs()).all())
    first, last = result[True]
    for a, b in zip(first, last):
        assert a[:2].numpy().tobytes() == b[:2].numpy().tobytes()
        assert bool((a[2] != b[2]))  # the element that kept a gradient moved on
    for skip in (False, True):  # NaN is not zero: it reaches p, m and v under both settings
        assert all(bool(torch.isnan(t[3])) for t in result[skip][1])


def _three_steps(opt, p, grads):
    for g in grads:
        p.grad = torch.as_tensor(g)
        opt.step()


def test_state_dict_moves_between_nr_adam_and_torch_adam():
    """Both directions on CPU tensors, against torch.optim.Adam as it keeps its state there (a 0-dim
    float32 `step` on the parameter's device; capturable=True, which torch refuses for CPU parameters,
    is the GPU test's)."""
    p0, grads = inputs()
    uninterrupted = np_trajectory(p0, grads[:4])[0][-1]
    # nr.Adam -> torch.optim.Adam
    p = torch.nn.Parameter(torch.as_tensor(p0).clone())
    opt = nr.Adam([p])
    _three_steps(opt, p, grads[:3])
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and sd["state"][0]["step"].dtype == torch.float32
    other = torch.optim.Adam([p])
    other.load_state_dict(sd)
    _three_steps(other, p, grads[3:4])
    assert np.abs(p.detach().numpy() - uninterrupted).max() <= 1e-14
    # torch.optim.Adam -> nr.Adam, which keeps its own skip_zero_grad
    p = torch.nn.Parameter(torch.as_tensor(p0).clone())
    opt = torch.optim.Adam([p])
    _three_steps(opt, p, grads[:3])
    mine = nr.Adam([p], skip_zero_grad=True)
    mine.load_state_dict(opt.state_dict())
    assert mine.param_groups[0]["skip_zero_grad"] is True
    mine.param_groups[0]["skip_zero_grad"] = False
    _three_steps(mine, p, grads[3:4])
    assert float(mine.state[p]["step"]) == 4
    assert np.abs(p.detach().numpy() - uninterrupted).max() <= 1e-14


# ---- the C ABI, without a launch ----
ARGS, WORKSPACE = 1, 3  # NR_ERR_ARGS, NR_ERR_WORKSPACE
P = 4096  # a non-null address that is never dereferenced


def adam_call(n=1, capacity=None, length=2, param=P, step=P, numel=8, lr_scale=1., lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
              scratch=P, scratch_bytes=1 << 10, null_args=False):
    L = _lib.lib()
    tensors = (_lib.NrAdamTensor * length)()
    for t in tensors:
        t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.step, t.numel, t.lr_scale = param, P, P, P, step, numel, lr_scale
    a = _lib.NrAdamArgs()
    a.num_tensors, a.tensors_capacity, a.tensors = n, length if capacity is None else capacity, tensors
    a.lr, a.beta1, a.beta2, a.eps = lr, beta1, beta2, eps
    a.scratch, a.scratch_bytes = scratch, scratch_bytes
    status = L.nr_adam_step(None if null_args else ctypes.byref(a), None)
    if status != 0:
        assert len(L.nr_last_error()) > 0
    return status


def test_abi_sizes():
    L = _lib.lib()
    assert L.nr_adam_args_size() == ctypes.sizeof(_lib.NrAdamArgs)
    assert _lib.NR_ADAM_CHUNK == 4096 and _lib.NR_ADAM_MAX_TENSORS == 24
    assert L.nr_adam_scratch_bytes(0) == 0 and L.nr_adam_scratch_bytes(-3) == 0
    sizes = [L.nr_adam_scratch_bytes(n) for n in range(1, 100)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and all(s >= 8 * n for n, s in enumerate(sizes, 1))


def test_abi_rejects_bad_arguments():
    """nr_adam_step validates before any launch (no GPU needed: every call here returns from the checks)."""
    L = _lib.lib()
    assert adam_call(null_args=True) == ARGS
    assert adam_call(n=-1) == ARGS
    assert adam_call(n=3, length=2) == ARGS  # more than the host array holds
    assert b"holds" in L.nr_last_error()
    assert adam_call(param=None) == ARGS and adam_call(step=None) == ARGS  # null with numel > 0
    assert adam_call(numel=-1) == ARGS and adam_call(numel=2 ** 31 - 1) == ARGS  # past INT_MAX - chunk
    assert adam_call(beta1=1.) == ARGS and adam_call(beta2=1.) == ARGS and adam_call(beta1=-0.1) == ARGS
    assert adam_call(eps=-1e-8) == ARGS and adam_call(eps=float("nan")) == ARGS
    assert adam_call(lr=float("nan")) == ARGS and adam_call(lr=float("inf")) == ARGS
    assert adam_call(lr_scale=float("nan")) == ARGS
    assert adam_call(scratch=None) == WORKSPACE and adam_call(n=2, scratch_bytes=8) == WORKSPACE
    assert b"scratch" in L.nr_last_error()
    # nothing to do: no pointer is needed
    assert adam_call(n=0, scratch=None) == 0

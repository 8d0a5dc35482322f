"""Adam for the optimisation loop around the renderer, with the two rules of the reference's optimiser
(neural_renderer_torch/optimizers.py:1-37): "do not update a weight if the gradient is zero"
(skip_zero_grad) and "use parameter-wise learning rate specified by param.lr".  Float32 GPU parameters of a
group are updated together by one fused HIP launch pair per 24 tensors (nr_adam_step,
include/nr_raster.h); everything else takes the same rule as torch ops (adam_step_torch).

The rule, for every element of a parameter whose gradient is present, at the parameter's step t (after
the increment):

    step_size = lr * lr_scale / (1 - beta1^t)        inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t)
    if skip_zero_grad and g == 0: leave p, m, v as they are      (both zeros count; NaN does not)
    m = m + (1 - beta1) * (g - m)
    v = v + (1 - beta2) * (g * g - v);   v = max(v, 0)
    p = p - step_size * (m / (sqrt(v) * inv_sqrt_bc2 + eps))

With skip_zero_grad=False and no param.lr this is torch.optim.Adam's rule (amsgrad=False, no weight decay,
maximize=False) up to rounding.  No host synchronisation on the fused path, so a step can be captured in a
HIP graph with no flag to set, and no float atomics: updates are bitwise identical from run to run."""
import ctypes
import math

import torch

from . import _lib


def adam_step_torch(params, grads, exp_avgs, exp_avg_sqs, steps, *, lr, lr_scales, beta1, beta2, eps, skip_zero_grad):
    """One Adam step of the module's rule as torch ops, in place, for any device and dtype: the fallback
    of Adam, the tests' second opinion and the benchmark's companion.  steps: one 0-dim tensor per
    parameter, advanced here; lr: a float or a one-element tensor; lr_scales: one float per parameter."""
    for p, g, m, v, step, scale in zip(params, grads, exp_avgs, exp_avg_sqs, steps, lr_scales):
        step += 1
        if torch.is_tensor(lr) or step.is_cuda:  # the factors as device tensors: nothing is read back to the host
            t = step.to(torch.float64)
            rate = lr.to(device=step.device, dtype=torch.float64).reshape(()) if torch.is_tensor(lr) else lr
            step_size = (rate * scale / (1 - beta1 ** t)).to(device=p.device, dtype=p.dtype)
            inv_sqrt_bc2 = (1 / (1 - beta2 ** t).sqrt()).to(device=p.device, dtype=p.dtype)
        else:
            t = float(step)
            step_size = lr * scale / (1 - beta1 ** t)
            inv_sqrt_bc2 = 1 / math.sqrt(1 - beta2 ** t)
        m2 = m + (1 - beta1) * (g - m)
        v2 = v + (1 - beta2) * (g * g - v)
        v2 = torch.where(v2 < 0, torch.zeros_like(v2), v2)
        p2 = p - step_size * (m2 / (v2.sqrt() * inv_sqrt_bc2 + eps))
        if skip_zero_grad:
            zero = g == 0
            m2, v2, p2 = torch.where(zero, m, m2), torch.where(zero, v, v2), torch.where(zero, p, p2)
        m.copy_(m2)
        v.copy_(v2)
        p.copy_(p2)


def _nr_adam_step(args, stream):
    """The one place the optimiser enters the library (the tests count the calls here)."""
    _lib.check(_lib.lib().nr_adam_step(ctypes.byref(args), stream), "nr_adam_step")


def _dense(t):
    return t.dtype == torch.float32 and t.is_contiguous()


class Adam(torch.optim.Optimizer):
    """Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, skip_zero_grad=False).

    Param groups are supported and every option is per group.  lr is a float, or a 0-dim float32 tensor
    on the parameters' device that the update reads on the device (a schedule can change it between
    replays of a captured step).  A parameter's `lr` attribute (the reference's param.lr, mesh.py:35-37)
    multiplies its group's rate: it is read at every step() in eager use and baked in when a step is
    captured in a graph; a param.lr of 0 leaves the parameter and its state untouched.

    skip_zero_grad=True leaves every element whose gradient is exactly zero (+0 or -0; NaN is not zero)
    as it is: parameter, exp_avg and exp_avg_sq.  The step count still advances per tensor, and a skipped
    element's moments do not decay while it is skipped (lazy Adam): when its gradient returns, the
    update continues from the moments it had when it was last seen, with the tensor's bias corrections.

    State per parameter: `step` (0-dim float32 on the parameter's device), `exp_avg`, `exp_avg_sq`: the
    keys and dtypes of torch.optim.Adam(capturable=True), so a state_dict moves between the two in both
    directions.  Parameters whose .grad is None are skipped and their step does not advance; sparse
    gradients raise.  Float32 parameters on a GPU with contiguous data take the fused kernels (a
    non-contiguous gradient is made contiguous); every other parameter takes adam_step_torch."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, skip_zero_grad=False):
        if torch.is_tensor(lr):
            if lr.numel() != 1:
                raise ValueError("a tensor lr must have one element")
        elif not (lr >= 0.0 and math.isfinite(lr)):
            raise ValueError("invalid learning rate: %r" % (lr,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid betas: %r" % (betas,))
        if not eps >= 0.0:
            raise ValueError("invalid eps: %r" % (eps,))
        # weight_decay / amsgrad / maximize: the keys torch.optim.Adam reads from a loaded state_dict's
        # groups; this optimiser implements none of them
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False,
                        skip_zero_grad=bool(skip_zero_grad))
        super().__init__(params, defaults)
        self._scratch = {}

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("skip_zero_grad", False)
        self._scratch = {}

    def load_state_dict(self, state_dict):
        """A torch.optim.Adam state_dict loads too; its groups carry no skip_zero_grad, so each group keeps
        the setting it has."""
        keep = [g["skip_zero_grad"] for g in self.param_groups]
        super().load_state_dict(state_dict)
        saved = state_dict["param_groups"]
        for group, old, s in zip(self.param_groups, keep, saved):
            if "skip_zero_grad" not in s:
                group["skip_zero_grad"] = old

    def _state_of(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        step = st["step"]
        if not torch.is_tensor(step) or step.dtype != torch.float32 or step.device != p.device or step.ndim != 0:
            # a state loaded from a torch.optim.Adam that kept its steps on the host
            st["step"] = torch.as_tensor(float(step), dtype=torch.float32).to(p.device)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            if group.get("weight_decay", 0) != 0 or group.get("amsgrad", False) or group.get("maximize", False):
                raise RuntimeError("nr.Adam implements no weight decay, amsgrad or maximize")
            fused, rest = {}, []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("nr.Adam does not support sparse gradients")
                scale = float(getattr(p, "lr", 1.0))
                if scale == 0:
                    continue
                st = self._state_of(p)
                item = (p, g, st["exp_avg"], st["exp_avg_sq"], st["step"], scale)
                if (p.is_cuda and _dense(p) and g.device == p.device and g.dtype == torch.float32 and g.layout == torch.strided
                        and _dense(st["exp_avg"]) and _dense(st["exp_avg_sq"])):
                    fused.setdefault(p.device, []).append(item)
                else:
                    rest.append(item)
            for dev, items in fused.items():
                self._fused_step(gi, group, dev, items)
            if rest:
                beta1, beta2 = group["betas"]
                adam_step_torch(*[[it[k] for it in rest] for k in range(5)], lr=group["lr"], lr_scales=[it[5] for it in rest],
                                beta1=beta1, beta2=beta2, eps=group["eps"], skip_zero_grad=group["skip_zero_grad"])
        return loss

    def _fused_step(self, gi, group, dev, items):
        """One nr_adam_step for the fusable parameters of group gi on device dev (the library takes
        NR_ADAM_MAX_TENSORS of them per launch pair)."""
        L = _lib.lib()
        n = len(items)
        # the factor scratch of this (group, device): calls of different groups may sit in one graph.  Sized
        # for the whole group at once, so a captured step's scratch is never replaced by a larger one
        key = (gi, dev)
        scratch = self._scratch.get(key)
        need = L.nr_adam_scratch_bytes(len(group["params"]))
        if scratch is None or scratch.numel() < need:
            scratch = self._scratch[key] = torch.empty(need, dtype=torch.uint8, device=dev)
        tensors = (_lib.NrAdamTensor * n)()
        hold = []
        for d, (p, g, m, v, step, scale) in zip(tensors, items):
            if not g.is_contiguous():
                g = g.contiguous()
                hold.append(g)
            d.param, d.grad, d.exp_avg, d.exp_avg_sq, d.step = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr()
            d.numel, d.lr_scale = p.numel(), scale
        a = _lib.NrAdamArgs()
        a.num_tensors = a.tensors_capacity = n
        a.tensors = tensors
        lr = group["lr"]
        if torch.is_tensor(lr):
            if lr.device != dev or lr.dtype != torch.float32:
                raise RuntimeError("nr.Adam: a tensor lr must be float32 on the parameters' device (%s), got %s on %s"
                                   % (dev, lr.dtype, lr.device))
            a.lr, a.lr_device = 0.0, lr.data_ptr()
        else:
            a.lr, a.lr_device = float(lr), None
        a.beta1, a.beta2 = group["betas"]
        a.eps = group["eps"]
        a.skip_zero_grad = 1 if group["skip_zero_grad"] else 0
        a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
        with _lib.on_device(dev):
            _nr_adam_step(a, _lib.stream_of(items[0][0]))

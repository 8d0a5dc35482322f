"""Per-item image losses for the optimisation loop around the renderer: the weighted squared error, the
Huber loss, the silhouette IoU loss and the structural-similarity (SSIM) loss, each one fused HIP launch
pair forward and one launch backward (nr_pointwise_loss_* / nr_iou_loss_* / nr_ssim_loss_*,
include/nr_raster.h) for float32 GPU images, and a torch composition (squared_error_loss_torch /
huber_loss_torch / iou_loss_torch / ssim_loss_torch) for everything else.

Definitions, for images [B, ...] with N elements per item (all the trailing dimensions):

  squared error: loss_b = sum_i w_i (x_i - t_i)^2                      (no 1/2)
  Huber:         loss_b = sum_i w_i h(x_i - t_i),  h(d) = d^2 / 2 if |d| < delta else delta (|d| - delta / 2)
                 (torch.nn.functional.huber_loss with reduction='none', weighted and summed per item)
  IoU:           loss_b = 1 - sum_i p_i t_i / (sum_i (p_i + t_i - p_i t_i) + eps)
  SSIM:          loss_b = 1 - mean of S over the item's map; images [B, C, H, W] or [B, H, W] (ssim_loss)

targets have the images' shape, or are shared by the items: a leading 1, no batch dimension, or a
batch-expanded view; a shared target is read at stride 0 and never expanded in memory.  weights are None,
shaped like the images, or for [B, C, H, W] images a per-pixel mask [B or 1, 1, H, W] applied to every
channel; each per item or shared like the targets.  Gradients reach the images only on the fused path.

The fused path runs when images is a float32 GPU tensor and targets / weights are float32 tensors on
its device that take no gradient; every other combination takes the composition.  Each item must be
one contiguous run of N floats (rgba[:, 3], rgba[:, :3] and the [:, 0] view of rasterize_silhouettes
are: the kernels take an item stride); any other layout is made contiguous first.  No host
synchronisation, so a step can be captured in a HIP graph, and no float atomics: losses and gradients
are bitwise identical from run to run."""
import functools

import torch
from torch.autograd.function import once_differentiable

from . import _lib


# ---- shapes ----
def _item_dims(images):
    if not torch.is_tensor(images) or images.ndim < 2:
        raise ValueError("images must be a [B, ...] tensor with at least two dimensions")
    return tuple(range(1, images.ndim))


def _shared(t, images):
    """Whether operand t (already known to fit) is one item shared by the batch; None when it does not fit."""
    item = tuple(images.shape[1:])
    if tuple(t.shape) == tuple(images.shape):
        return False
    if tuple(t.shape) == item or tuple(t.shape) == (1,) + item:
        return True
    return None


def _check_targets(images, targets):
    if not torch.is_tensor(targets) or _shared(targets, images) is None:
        raise ValueError("targets %s fit neither the images %s nor one item of them" % (
            tuple(targets.shape) if torch.is_tensor(targets) else type(targets).__name__, tuple(images.shape)))


def _mask_like(images):
    """A stand-in with the shape a per-pixel mask takes for these images, or None."""
    if images.ndim != 4:
        return None
    return images[:, :1]


def _check_weights(images, weights):
    """Whether the weights are a per-pixel mask (True) or full weights (False)."""
    if not torch.is_tensor(weights):
        raise ValueError("weights must be a tensor or None")
    if _shared(weights, images) is not None:
        return False
    mask = _mask_like(images)
    if mask is not None and _shared(weights, mask) is not None:
        return True
    raise ValueError("weights %s fit neither the images %s nor a per-pixel mask of them" % (
        tuple(weights.shape), tuple(images.shape)))


def _finish(loss, average):
    return loss.mean() if average else loss


# ---- the torch composition: reference of the tests, baseline of tools/bench_image_loss.py ----
def _weighted_sum(term, images, weights):
    if weights is not None:
        _check_weights(images, weights)
        term = term * weights
    return term.sum(_item_dims(images))


def squared_error_loss_torch(images, targets, weights=None, average=False):
    """The weighted squared error as torch ops; any device and dtype, gradients to every operand."""
    _item_dims(images)
    _check_targets(images, targets)
    d = images - targets
    return _finish(_weighted_sum(d * d, images, weights), average)


def huber_loss_torch(images, targets, delta=1.0, weights=None, average=False):
    """The weighted Huber loss as torch ops; any device and dtype, gradients to every operand."""
    _item_dims(images)
    _check_targets(images, targets)
    if not delta > 0:
        raise ValueError("delta must be positive")
    d = images - targets
    a = d.abs()
    term = torch.where(a < delta, 0.5 * d * d, delta * (a - 0.5 * delta))
    return _finish(_weighted_sum(term, images, weights), average)


def iou_loss_torch(silhouettes, targets, eps=1e-6, average=False):
    """The silhouette IoU loss as torch ops; any device and dtype, gradients to both operands."""
    dims = _item_dims(silhouettes)
    _check_targets(silhouettes, targets)
    pt = silhouettes * targets
    inter = pt.sum(dims)
    union = (silhouettes + targets - pt).sum(dims)
    return _finish(1 - inter / (union + eps), average)


# ---- SSIM: definition and composition ----
_SSIM_PADDINGS = ("same", "valid")


def _ssim_window(window_size, sigma):
    """The 1-D Gaussian window exp(-k^2 / 2 sigma^2), k = -R .. R, normalised to sum 1: a float64 tensor."""
    R = window_size // 2
    k = torch.arange(-R, R + 1, dtype=torch.float64)
    g = torch.exp(-(k * k) / (2.0 * float(sigma) ** 2))
    return g / g.sum()


@functools.lru_cache(maxsize=64)
def _ssim_window_on(window_size, sigma, dtype, device):
    """The window in the composition's dtype on its device, kept: a step that was run once makes no host-to-device
    copy again, so it can be captured in a graph."""
    return _ssim_window(window_size, sigma).to(dtype=dtype, device=device)


def _ssim_check(images, targets, window_size, sigma, data_range, padding):
    """The argument errors of both paths; returns (images, targets) as 4-D [B, C, H, W] / [B or 1, C, H, W] views."""
    if not torch.is_tensor(images) or images.ndim not in (3, 4):
        raise ValueError("images must be a [B, C, H, W] or [B, H, W] tensor")
    _check_targets(images, targets)
    if not isinstance(window_size, int) or window_size < 1 or window_size % 2 == 0:
        raise ValueError("window_size must be a positive odd integer, not %r" % (window_size,))
    if padding not in _SSIM_PADDINGS:
        raise ValueError("padding must be 'same' or 'valid', not %r" % (padding,))
    if not (0 < sigma < float("inf")) or not (0 < data_range < float("inf")):
        raise ValueError("sigma and data_range must be positive and finite")
    if padding == "valid" and images.numel() and (images.shape[-2] < window_size or images.shape[-1] < window_size):
        raise ValueError("padding='valid' needs images of at least %d x %d pixels, not %d x %d"
                         % (window_size, window_size, images.shape[-2], images.shape[-1]))
    t = targets if targets.ndim == images.ndim else targets[None]
    if images.ndim == 3:
        images, t = images[:, None], t[:, None]
    return images, t


def ssim_loss_torch(images, targets, window_size=11, sigma=1.5, data_range=1.0, padding="same", average=False):
    """The SSIM loss as torch ops (two grouped 1-D convolutions per filtered quantity); any device and dtype,
    gradients to both operands.  The definition: ssim_loss."""
    x, t = _ssim_check(images, targets, window_size, sigma, data_range, padding)
    dtype = torch.result_type(x, t)  # mixed operands promote, as in the pointwise compositions
    x, t = x.to(dtype), t.to(dtype)
    C, R = x.shape[1], window_size // 2
    g = _ssim_window_on(window_size, float(sigma), x.dtype, x.device)
    row, col = g.reshape(1, 1, 1, -1).repeat(C, 1, 1, 1), g.reshape(1, 1, -1, 1).repeat(C, 1, 1, 1)
    pad = R if padding == "same" else 0
    conv2d = torch.nn.functional.conv2d

    def G(a):
        return conv2d(conv2d(a, row, padding=(0, pad), groups=C), col, padding=(pad, 0), groups=C)

    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mu1, mu2 = G(x), G(t)
    mu11, mu22, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11, s22, s12 = G(x * x) - mu11, G(t * t) - mu22, G(x * t) - mu12
    S = ((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu11 + mu22 + c1) * (s11 + s22 + c2))
    return _finish(1 - S.mean((1, 2, 3)), average)


# ---- the fused path ----
def _item_contiguous(t, start):
    """Whether dimensions start.. of t are laid out as one contiguous run."""
    expect = 1
    for size, stride in zip(reversed(t.shape[start:]), reversed(t.stride()[start:])):
        if size != 1 and stride != expect:
            return False
        expect *= size
    return True


def _image_items(images):
    """images with every item one contiguous run (a copy only when they are not), and the item stride."""
    if images.numel() == 0 or not _item_contiguous(images, 1):
        images = images.contiguous()
    return images, (images.stride(0) if images.shape[0] > 1 else 0)


def _items(t, shared):
    """Target or weight operand t as (tensor whose data_ptr is item 0, item stride in elements): each item
    one contiguous run, without expanding a shared or batch-expanded operand."""
    if not shared and t.shape[0] > 1 and t.stride(0) == 0:
        t, shared = t[0], True
    if shared:
        return (t if t.is_contiguous() else t.contiguous()), 0
    return _image_items(t)


def _fusable(images, *others):
    if not (torch.is_tensor(images) and images.is_cuda and images.dtype == torch.float32):
        return False
    for t in others:
        if t is None:
            continue
        if not torch.is_tensor(t) or t.device != images.device or t.dtype != torch.float32 or t.requires_grad:
            return False
    return True


def _sizes(images):
    B = images.shape[0]
    N = 1
    for s in images.shape[1:]:
        N *= s
    return B, N


def _workspace(L, B, N, dev):
    return torch.empty(L.nr_image_loss_workspace_bytes(B, N), dtype=torch.uint8, device=dev)


class PointwiseLossFunction(torch.autograd.Function):
    """images [B, ...] float32 on the GPU, every item contiguous -> loss [B].  The backward recomputes from
    images, targets and weights, which are saved by reference."""

    @staticmethod
    def forward(ctx, images, istride, targets, tstride, weights, wstride, period, kind, delta):
        B, N = _sizes(images)
        dev = images.device
        L = _lib.lib()
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        ws = _workspace(L, B, N, dev)
        with _lib.on_device(dev):
            _lib.check(L.nr_pointwise_loss_forward(_lib.ptr(images), istride, _lib.ptr(targets), tstride, _lib.ptr(weights), wstride,
                                                   period, kind, delta, B, N, _lib.ptr(loss), _lib.ptr(ws), ws.numel(),
                                                   _lib.stream_of(images)), "nr_pointwise_loss_forward")
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(images, targets, weights)
            ctx.args = (istride, tstride, wstride, period, kind, delta)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return (None,) * 9
        images, targets, weights = ctx.saved_tensors
        istride, tstride, wstride, period, kind, delta = ctx.args
        B, N = _sizes(images)
        g = grad_loss.to(torch.float32).contiguous()
        grad = torch.empty(images.shape, dtype=torch.float32, device=images.device)
        with _lib.on_device(images.device):
            _lib.check(_lib.lib().nr_pointwise_loss_backward(_lib.ptr(images), istride, _lib.ptr(targets), tstride,
                                                             _lib.ptr(weights), wstride, period, kind, delta, B, N, _lib.ptr(g),
                                                             _lib.ptr(grad), _lib.stream_of(images)), "nr_pointwise_loss_backward")
        return (grad,) + (None,) * 8


class IoULossFunction(torch.autograd.Function):
    """silhouettes [B, ...] float32 on the GPU, every item contiguous -> loss [B].  The forward keeps the
    intersection and union sums [B, 2]; the backward reads them and the targets (the gradient does not
    depend on the silhouettes' own values)."""

    @staticmethod
    def forward(ctx, images, istride, targets, tstride, eps):
        B, N = _sizes(images)
        dev = images.device
        L = _lib.lib()
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        sums = torch.empty((B, 2), dtype=torch.float32, device=dev)
        ws = _workspace(L, B, N, dev)
        with _lib.on_device(dev):
            _lib.check(L.nr_iou_loss_forward(_lib.ptr(images), istride, _lib.ptr(targets), tstride, eps,
                                             B, N, _lib.ptr(loss), _lib.ptr(sums), _lib.ptr(ws), ws.numel(),
                                             _lib.stream_of(images)), "nr_iou_loss_forward")
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(targets, sums)
            ctx.args = (tuple(images.shape), tstride, eps)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        targets, sums = ctx.saved_tensors
        shape, tstride, eps = ctx.args
        g = grad_loss.to(torch.float32).contiguous()
        grad = torch.empty(shape, dtype=torch.float32, device=sums.device)
        B = shape[0]
        with _lib.on_device(sums.device):
            _lib.check(_lib.lib().nr_iou_loss_backward(_lib.ptr(targets), tstride, _lib.ptr(sums), eps, B,
                                                       grad.numel() // B if B else 0, _lib.ptr(g), _lib.ptr(grad),
                                                       _lib.stream_of(sums)), "nr_iou_loss_backward")
        return grad, None, None, None, None


class SSIMLossFunction(torch.autograd.Function):
    """images [B, C, H, W] float32 on the GPU, every item contiguous -> loss [B].  When the images take a
    gradient the forward keeps the three maps [3, B, C, H', W'] of include/nr_raster.h; the backward
    filters them and reads images and targets, which are saved by reference."""

    @staticmethod
    def forward(ctx, images, istride, targets, tstride, window, c1, c2, padding):
        B, C, H, W = images.shape
        dev = images.device
        L = _lib.lib()
        K = len(window)
        R = K // 2
        win = (_lib.c_float * K)(*window)
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        ws = torch.empty(L.nr_ssim_loss_workspace_bytes(B, C, H, W, K, padding), dtype=torch.uint8, device=dev)
        saved = None
        if ctx.needs_input_grad[0]:
            mh, mw = (H - 2 * R, W - 2 * R) if padding == _lib.NR_SSIM_VALID else (H, W)
            saved = torch.empty((3, B, C, max(mh, 0), max(mw, 0)), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.nr_ssim_loss_forward(_lib.ptr(images), istride, _lib.ptr(targets), tstride, B, C, H, W, K, win, c1, c2,
                                              padding, _lib.ptr(loss), _lib.ptr(saved), _lib.ptr(ws), ws.numel(),
                                              _lib.stream_of(images)), "nr_ssim_loss_forward")
        if saved is not None:
            ctx.save_for_backward(images, targets, saved)
            ctx.args = (istride, tstride, win, padding)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        images, targets, saved = ctx.saved_tensors
        istride, tstride, win, padding = ctx.args
        B, C, H, W = images.shape
        g = grad_loss.to(torch.float32).contiguous()
        grad = torch.empty(images.shape, dtype=torch.float32, device=images.device)
        with _lib.on_device(images.device):
            _lib.check(_lib.lib().nr_ssim_loss_backward(_lib.ptr(images), istride, _lib.ptr(targets), tstride, _lib.ptr(saved),
                                                        B, C, H, W, len(win), win, padding, _lib.ptr(g), _lib.ptr(grad),
                                                        _lib.stream_of(images)), "nr_ssim_loss_backward")
        return (grad,) + (None,) * 7


def _pointwise(images, targets, weights, kind, delta):
    _check_targets(images, targets)
    x, istride = _image_items(images)
    t, tstride = _items(targets, _shared(targets, images))
    w, wstride, period = None, 0, 1
    if weights is not None:
        mask = _check_weights(images, weights)
        like = _mask_like(images) if mask else images
        w, wstride = _items(weights, _shared(weights, like))
        period = max(images.shape[2] * images.shape[3] if mask else _sizes(images)[1], 1)
    return PointwiseLossFunction.apply(x, istride, t, tstride, w, wstride, period, kind, float(delta))


def squared_error_loss(images, targets, weights=None, average=False):
    """sum_i w_i (x_i - t_i)^2 per item (no 1/2): [B] for images [B, ...], or with average=True the 0-dim
    mean over the items.  Target and weight forms, dispatch and layout: the module docstring."""
    _item_dims(images)
    if not _fusable(images, targets, weights):
        return squared_error_loss_torch(images, targets, weights, average)
    return _finish(_pointwise(images, targets, weights, _lib.NR_LOSS_SQUARED, 1.0), average)


def huber_loss(images, targets, delta=1.0, weights=None, average=False):
    """sum_i w_i h(x_i - t_i) per item, h the Huber function of torch.nn.functional.huber_loss with this
    delta: shapes, dispatch and gradient as squared_error_loss."""
    _item_dims(images)
    if not _fusable(images, targets, weights):
        return huber_loss_torch(images, targets, delta, weights, average)
    if not delta > 0 or delta == float("inf"):
        raise ValueError("delta must be positive and finite")
    return _finish(_pointwise(images, targets, weights, _lib.NR_LOSS_HUBER, delta), average)


def iou_loss(silhouettes, targets, eps=1e-6, average=False):
    """1 - sum(p t) / (sum(p + t - p t) + eps) per item, the silhouette loss of the Neural Mesh Renderer
    paper: shapes, dispatch and gradient as squared_error_loss (no weights)."""
    _item_dims(silhouettes)
    if not _fusable(silhouettes, targets):
        return iou_loss_torch(silhouettes, targets, eps, average)
    _check_targets(silhouettes, targets)
    x, istride = _image_items(silhouettes)
    t, tstride = _items(targets, _shared(targets, silhouettes))
    return _finish(IoULossFunction.apply(x, istride, t, tstride, float(eps)), average)


def ssim_loss(images, targets, window_size=11, sigma=1.5, data_range=1.0, padding="same", average=False):
    """1 - the mean structural similarity (Wang et al. 2004) per item: [B] for images [B, C, H, W] or
    [B, H, W] (C = 1), or with average=True the 0-dim mean over the items.  Targets as the other losses take.

    g is the window exp(-k^2 / 2 sigma^2), k = -R .. R, R = window_size // 2, computed in float64,
    normalised to sum 1 and cast to the images' dtype; G = g (x) g filters each channel.  With
    C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2, mu1 = G*x, mu2 = G*t, s11 = G*x^2 - mu1^2,
    s22 = G*t^2 - mu2^2, s12 = G*(x t) - mu1 mu2 (no variance clamp):

      S = (2 mu1 mu2 + C1) (2 s12 + C2) / ((mu1^2 + mu2^2 + C1) (s11 + s22 + C2))
      loss_b = 1 - mean of S over the item's map (all channels and map pixels)

    padding='same' pads with R zeros, the map is H x W (the Gaussian-splatting loss); padding='valid' does
    not pad, the map is (H - 2R) x (W - 2R) (pytorch-msssim, skimage) and H, W >= window_size.

    The fused path (module docstring) also needs window_size in 3, 5, 7, 9, 11; anything else runs
    ssim_loss_torch.  An even window, an unknown padding, a non-positive sigma or data_range and targets
    that do not fit raise ValueError on both paths."""
    x, t = _ssim_check(images, targets, window_size, sigma, data_range, padding)
    if not _fusable(images, targets) or not 3 <= window_size <= _lib.NR_SSIM_MAX_WINDOW:
        return ssim_loss_torch(images, targets, window_size, sigma, data_range, padding, average)
    window = _ssim_window(window_size, sigma).to(torch.float32).tolist()
    x, istride = _image_items(x)
    t, tstride = _items(t, _shared(targets, images))
    loss = SSIMLossFunction.apply(x, istride, t, tstride, tuple(window), (0.01 * data_range) ** 2, (0.03 * data_range) ** 2,
                                  _lib.NR_SSIM_VALID if padding == "valid" else _lib.NR_SSIM_SAME)
    return _finish(loss, average)


class _TargetLoss(torch.nn.Module):
    def __init__(self, targets, weights, average):
        super().__init__()
        self.register_buffer("targets", targets)
        self.register_buffer("weights", weights)
        self.average = average


class SquaredErrorLoss(_TargetLoss):
    """squared_error_loss with the targets (and weights) held as buffers of the module."""

    def __init__(self, targets, weights=None, average=False):
        super().__init__(targets, weights, average)

    def forward(self, images):
        return squared_error_loss(images, self.targets, self.weights, self.average)


class HuberLoss(_TargetLoss):
    """huber_loss with the targets (and weights) held as buffers of the module."""

    def __init__(self, targets, delta=1.0, weights=None, average=False):
        super().__init__(targets, weights, average)
        self.delta = delta

    def forward(self, images):
        return huber_loss(images, self.targets, self.delta, self.weights, self.average)


class IoULoss(_TargetLoss):
    """iou_loss with the targets held as a buffer of the module."""

    def __init__(self, targets, eps=1e-6, average=False):
        super().__init__(targets, None, average)
        self.eps = eps

    def forward(self, silhouettes):
        return iou_loss(silhouettes, self.targets, self.eps, self.average)


class SSIMLoss(_TargetLoss):
    """ssim_loss with the targets held as a buffer of the module."""

    def __init__(self, targets, window_size=11, sigma=1.5, data_range=1.0, padding="same", average=False):
        super().__init__(targets, None, average)
        self.window_size, self.sigma, self.data_range, self.padding = window_size, sigma, data_range, padding

    def forward(self, images):
        return ssim_loss(images, self.targets, self.window_size, self.sigma, self.data_range, self.padding, self.average)

import torch


def _batched(x, like, tail):
    """x as a [1 or B, *tail] tensor of `like`'s dtype and device."""
    if not torch.is_tensor(x):
        x = torch.as_tensor(x, dtype=like.dtype)
    x = x.to(device=like.device, dtype=like.dtype)
    if x.ndim == len(tail):
        x = x[None]
    if tuple(x.shape[1:]) != tuple(tail):
        raise ValueError("expected a [B or 1, %s] tensor, got %s" % (", ".join(map(str, tail)), list(x.shape)))
    return x


def projection(vertices, K, R, t, dist_coeffs=None, orig_size=1024, eps=1e-9):
    """Calibrated pinhole camera with OpenCV's distortion model, mapped to the y-up normalised
    coordinates that `perspective` produces.

    vertices [B, V, 3]; K [B or 1, 3, 3] (row 2 is not read); R [B or 1, 3, 3]; t [B or 1, 3] or
    [B or 1, 1, 3]; dist_coeffs [B or 1, 5] = (k1, k2, p1, p2, k3), None = no distortion; orig_size S:
    the (square) image size in pixels that K refers to.  Per vertex:

        p = R v + t = (x, y, z);  x' = x / (z + eps), y' = y / (z + eps), r2 = x'^2 + y'^2
        rad = 1 + k1 r2 + k2 r2^2 + k3 r2^3
        x'' = x' rad + 2 p1 x' y' + p2 (r2 + 2 x'^2);  y'' = y' rad + p1 (r2 + 2 y'^2) + 2 p2 x' y'
        u = K00 x'' + K01 y'' + K02;  v = K10 x'' + K11 y'' + K12
        out = (2 (u - S/2) / S, 2 ((S - v) - S/2) / S, z)

    A composition of torch ops for any device and dtype (r2 takes no square root: the gradient at the
    optical axis is finite); camera.projection_transform is the fused GPU path."""
    assert vertices.ndim == 3
    K = _batched(K, vertices, (3, 3))
    R = _batched(R, vertices, (3, 3))
    if torch.is_tensor(t) and t.ndim == 3:
        t = t.reshape(t.shape[0], 3) if t.shape[1:] == (1, 3) else t
    t = _batched(t, vertices, (3,))
    if dist_coeffs is None:
        dist_coeffs = torch.zeros((1, 5), dtype=vertices.dtype, device=vertices.device)
    d = _batched(dist_coeffs, vertices, (5,))
    S = orig_size

    p = torch.matmul(vertices, R.transpose(1, 2)) + t[:, None, :]
    x, y, z = p[:, :, 0], p[:, :, 1], p[:, :, 2]
    x_ = x / (z + eps)
    y_ = y / (z + eps)
    k1, k2, p1, p2, k3 = (d[:, None, i] for i in range(5))
    r2 = x_ ** 2 + y_ ** 2
    rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    x__ = x_ * rad + 2 * p1 * x_ * y_ + p2 * (r2 + 2 * x_ ** 2)
    y__ = y_ * rad + p1 * (r2 + 2 * y_ ** 2) + 2 * p2 * x_ * y_
    u = K[:, None, 0, 0] * x__ + K[:, None, 0, 1] * y__ + K[:, None, 0, 2]
    v = K[:, None, 1, 0] * x__ + K[:, None, 1, 1] * y__ + K[:, None, 1, 2]
    u = 2 * (u - S / 2.) / S
    v = 2 * ((S - v) - S / 2.) / S
    return torch.stack((u, v, z), 2)

"""Rigid registration before a fit: a partial scan of the teapot, moved by a known rotation and translation, is
brought back onto the teapot with nr.icp.

The scan is every third vertex of the teapot, rotated by --angle rad (0.5 by default) about (1, 2, 3) and shifted
by (0.15, -0.1, 0.2).  nr.icp runs --iterations updates on the device -- the nearest teapot vertex of every moved
scan point, then the closed-form rigid alignment of the original scan onto those -- with no host
synchronisation; its rmse history shows the convergence, and the recovered motion is printed beside the known
one.  Every non-rigid term of the package (point_mesh_distance, mesh_point_distance, arap_loss) assumes that the
scan and the template already share a frame: this is the step that finds it.

With --then-fit the aligned scan goes to example_scan_fit.py's exact losses: an icosphere is fitted to it with
nr.PointMeshLoss, nr.MeshPointLoss and a small nr.laplacian_loss for --fit-iters steps of nr.Adam.

    python examples/example_icp.py [--iterations 30] [--angle 0.5] [--max-distance D] [--then-fit] [--fit-iters 100]

The mesh defaults to tests/data/teapot.obj.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import neural_renderer_v2_pytorch_amd as nr  # noqa: E402
from neural_renderer_v2_pytorch_amd import synthetic  # noqa: E402

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'data')
AXIS, SHIFT = (1., 2., 3.), (0.15, -0.1, 0.2)


def axis_rotation(axis, angle):
    """The rotation by `angle` rad about `axis` (Rodrigues), [3, 3] float64."""
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0., -a[2], a[1]], [a[2], 0., -a[0]], [-a[1], a[0], 0.]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * K + (1. - math.cos(angle)) * (K @ K)


def fit(scan, device, iters, level=3, smoothness=0.01):
    """An icosphere fitted to the aligned scan with example_scan_fit.py's exact losses; the scan -> mesh loss of the
    first and the last step."""
    sphere, sphere_faces = synthetic.icosphere(level, radius=0.5)
    faces = torch.as_tensor(sphere_faces).to(device).int()
    vertices = torch.nn.Parameter(torch.as_tensor(sphere).float().to(device))
    topology = nr.mesh_topology(faces, sphere.shape[0])
    to_mesh, to_scan = nr.PointMeshLoss(scan), nr.MeshPointLoss(scan)
    opt = nr.Adam([vertices], lr=0.01)
    history = []
    for _ in range(iters):
        opt.zero_grad()
        first = to_mesh(vertices, faces)
        (first + to_scan(vertices, faces) + smoothness * nr.laplacian_loss(vertices, topology)).backward()
        opt.step()
        history.append(float(first.detach()))
    return history[0], history[-1]


def run(args):
    """Returns the rmse history (a list), the recovered R [3, 3] and t [3] (float64, CPU) and the known ones."""
    device = torch.device('cuda', args.gpu)
    vertices, _ = nr.load_obj(args.obj)
    target = torch.as_tensor(vertices).float().to(device)
    # the scan: x = R0^T (y - t0) of every third vertex y, so that y = R0 x + t0
    R0, t0 = axis_rotation(AXIS, args.angle), torch.tensor(SHIFT, dtype=torch.float64)
    scan = ((target[::3].double().cpu() - t0) @ R0).float().to(device)
    result = nr.icp(scan, target, iterations=args.iterations, max_distance=args.max_distance)
    out = dict(rmse=result.rmse.tolist(), R=result.R.double().cpu(), t=result.t.double().cpu(), R0=R0, t0=t0)
    if args.then_fit:
        aligned = scan @ result.R.t() + result.t
        out['fit'] = fit(aligned, device, args.fit_iters)
    return out


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--obj', default=os.path.join(DATA, 'teapot.obj'))
    ap.add_argument('--iterations', type=int, default=30)
    ap.add_argument('--angle', type=float, default=0.5, help='the known rotation, rad about (1, 2, 3)')
    ap.add_argument('--max-distance', type=float, default=None, help='reject pairs farther apart than this')
    ap.add_argument('--then-fit', action='store_true', help='fit an icosphere to the aligned scan')
    ap.add_argument('--fit-iters', type=int, default=100)
    ap.add_argument('--gpu', type=int, default=0)
    return ap


def main():
    args = parser().parse_args()
    out = run(args)
    print('rmse: ' + ' '.join('%.2e' % r for r in out['rmse']))
    print('rotation error %.2e, translation error %.2e (known: %.2f rad about %s, t = %s)'
          % (float((out['R'] - out['R0']).abs().max()), float((out['t'] - out['t0']).abs().max()), args.angle, AXIS, SHIFT))
    if 'fit' in out:
        print('scan -> mesh after the alignment: first %.5f, last %.5f after %d steps' % (out['fit'] + (args.fit_iters,)))


if __name__ == '__main__':
    main()

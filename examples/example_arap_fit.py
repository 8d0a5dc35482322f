"""Non-rigid registration: a straight tube is deformed onto a scan of a bent copy of itself, and keeps its shape.

example_scan_fit.py's exact scan terms with the regularizer a template needs.  The Laplacian, flatten and
edge-length losses pull towards "smooth", "flat" or "equal edges"; none of them says "stay, locally, a rotated
copy of the rest shape".  nr.ArapLoss says exactly that: around every vertex it finds the rotation that best
takes the rest shape's edges onto the deformed ones and charges what that rotation leaves over, so a bend
costs (almost) nothing while stretching, shearing and collapsing do.  Per step:

  scan -> mesh   nr.PointMeshLoss(target): every scan point to its closest point on the mesh;
  mesh -> scan   nr.MeshPointLoss(target): every triangle to its nearest scan point;
  ARAP           nr.ArapLoss(rest, faces): cotangent weights of the rest shape, formed once;

stepped by nr.Adam: every operation of the step is a fused HIP kernel.

    python examples/example_arap_fit.py [--iters 300] [--samples 4000] [--angle 1.2] [--arap-weight 1.0]
                                        [--weights cotangent|uniform] [--out fitted.obj]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import neural_renderer_v2_pytorch_amd as nr  # noqa: E402
from neural_renderer_v2_pytorch_amd import synthetic  # noqa: E402


class ArapFit(torch.nn.Module):
    def __init__(self, samples, angle, arap_weight, device, weights='cotangent', seed=0):
        super().__init__()
        rest, faces = synthetic.rigged_tube(rings=24, segments=16)[:2]
        self.faces = torch.as_tensor(faces).to(device).int()
        rest = torch.as_tensor(rest).float().to(device)
        bent = torch.as_tensor(synthetic.bent(rest.cpu().numpy(), angle)).float().to(device)
        with torch.no_grad():  # the scan: points on the bent copy's surface
            target = nr.sample_points(bent, self.faces, samples, generator=torch.Generator(device=device).manual_seed(seed))
        self.scan_to_mesh, self.mesh_to_scan = nr.PointMeshLoss(target), nr.MeshPointLoss(target)
        self.arap = nr.ArapLoss(rest, self.faces, weights=weights)
        self.arap_weight = arap_weight
        self.vertices = torch.nn.Parameter(rest.clone())

    def forward(self):
        return (self.scan_to_mesh(self.vertices, self.faces), self.mesh_to_scan(self.vertices, self.faces),
                self.arap_weight * self.arap(self.vertices))


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--samples', type=int, default=4000)
    ap.add_argument('--angle', type=float, default=1.2, help='how far the scanned copy is bent, rad over its height')
    ap.add_argument('--arap-weight', type=float, default=1.0)
    ap.add_argument('--weights', choices=('cotangent', 'uniform'), default='cotangent')
    ap.add_argument('--gpu', type=int, default=0)
    ap.add_argument('--out', default=None, help='write the fitted mesh as an .obj file')
    return ap


def fit(args):
    """The history of (scan -> mesh, mesh -> scan, weighted ARAP term) per step, and the model."""
    model = ArapFit(args.samples, args.angle, args.arap_weight, torch.device('cuda', args.gpu), weights=args.weights)
    opt = nr.Adam(model.parameters(), lr=0.005)
    history = []
    for _ in range(args.iters):
        opt.zero_grad()
        to_mesh, to_scan, arap = model()
        (to_mesh + to_scan + arap).backward()
        opt.step()
        history.append((float(to_mesh.detach()), float(to_scan.detach()), float(arap.detach())))
    return history, model


def main():
    args = parser().parse_args()
    history, model = fit(args)
    print('scan -> mesh: first %.6f, last %.6f; mesh -> scan: first %.6f, last %.6f; ARAP: first %.6f, largest %.6f, '
          'last %.6f after %d steps' % (history[0][0], history[-1][0], history[0][1], history[-1][1], history[0][2],
                                        max(h[2] for h in history), history[-1][2], len(history)))
    if args.out:
        nr.save_obj(args.out, model.vertices.detach().cpu().numpy(), model.faces.cpu().numpy())


if __name__ == '__main__':
    main()

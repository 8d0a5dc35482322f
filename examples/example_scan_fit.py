"""Fitting a mesh to a scan: an icosphere's vertices move until its surface passes through a point cloud
drawn from the teapot, and covers it.

example_chamfer.py's loop with an exact scan -> mesh term.  There both terms go through fresh samples of the
current mesh, so a scan point between two samples pulls towards the nearest sample, along the surface, and
the loss carries sampling noise of the order of the sample spacing.  Here

  scan -> mesh   nr.PointMeshLoss(target): the squared distance from every scan point to its closest point
                 on its closest triangle, with the gradient to that triangle's corners: no sampling, no noise;
  mesh -> scan   keeps the mesh from growing surface where the scan has no points.  --mesh-to-scan sampled (the
                 default), as before: fresh area-weighted samples of the current mesh (nr.sample_points, with
                 the gradient back to the vertices) and nr.chamfer_distance(..., directions="x_to_y") to the
                 scan.  --mesh-to-scan exact: nr.MeshPointLoss(target), the squared distance from every
                 triangle to its nearest scan point: no samples are drawn, and the whole scan loss is exact;

plus a small nr.laplacian_loss that keeps the surface smooth, stepped by nr.Adam: every operation of the
step is a fused HIP kernel.  --laplacian cot takes nr.cot_laplacian_loss instead (it leaves an irregular
triangulation of a flat patch alone), and --edge-weight W adds W * nr.edge_length_loss towards the
icosphere's mean initial edge length, which keeps the triangles from stretching and collapsing.

    python examples/example_scan_fit.py [--iters 300] [--samples 5000] [--level 3] [--mesh-to-scan sampled|exact]
                                        [--laplacian uniform|cot] [--edge-weight 0] [--out fitted.obj]

The target mesh defaults to tests/data/teapot.obj.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import neural_renderer_v2_pytorch_amd as nr  # noqa: E402
from neural_renderer_v2_pytorch_amd import synthetic  # noqa: E402

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'data')


class ScanFit(torch.nn.Module):
    def __init__(self, obj_file, level, samples, smoothness, device, seed=0, mesh_to_scan='sampled', laplacian='uniform',
                 edge_weight=0.):
        super().__init__()
        self.generator = torch.Generator(device=device).manual_seed(seed)
        vertices, faces = nr.load_obj(obj_file)
        target_vertices = torch.as_tensor(vertices).float().to(device)
        with torch.no_grad():
            target = nr.sample_points(target_vertices, torch.as_tensor(faces).to(device).int(), samples,
                                      generator=self.generator)
        self.scan_to_mesh = nr.PointMeshLoss(target)
        self.exact = mesh_to_scan == 'exact'
        self.mesh_to_scan = nr.MeshPointLoss(target) if self.exact else nr.ChamferLoss(target, directions="x_to_y")
        sphere, sphere_faces = synthetic.icosphere(level, radius=0.5)
        self.faces = torch.as_tensor(sphere_faces).to(device).int()
        self.vertices = torch.nn.Parameter(torch.as_tensor(sphere).float().to(device))
        self.topology = nr.mesh_topology(self.faces, sphere.shape[0])
        self.samples, self.smoothness = samples, smoothness
        self.laplacian = nr.cot_laplacian_loss if laplacian == 'cot' else nr.laplacian_loss
        self.edge_weight = edge_weight
        corners = torch.as_tensor(sphere)[torch.as_tensor(sphere_faces).long()]  # [F, 3, 3]
        self.edge_length = float((corners - corners.roll(1, 1)).norm(dim=-1).mean())  # a closed mesh: every edge twice

    def regularizer(self):
        """The weighted regularizers: the Laplacian loss, and the edge-length loss if asked for."""
        total = self.smoothness * self.laplacian(self.vertices, self.topology)
        if self.edge_weight:
            total = total + self.edge_weight * nr.edge_length_loss(self.vertices, self.topology, self.edge_length)
        return total

    def forward(self):
        if self.exact:
            return (self.scan_to_mesh(self.vertices, self.faces), self.mesh_to_scan(self.vertices, self.faces),
                    self.regularizer())
        points = nr.sample_points(self.vertices, self.faces, self.samples, generator=self.generator)
        return self.scan_to_mesh(self.vertices, self.faces), self.mesh_to_scan(points), self.regularizer()


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--obj', default=os.path.join(DATA, 'teapot.obj'))
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--samples', type=int, default=5000)
    ap.add_argument('--level', type=int, default=3, help='icosphere subdivision level')
    ap.add_argument('--smoothness', type=float, default=0.01, help='weight of the Laplacian loss')
    ap.add_argument('--gpu', type=int, default=0)
    ap.add_argument('--mesh-to-scan', choices=('sampled', 'exact'), default='sampled',
                    help="the mesh -> scan term: fresh surface samples and a one-sided chamfer term, or nr.MeshPointLoss")
    ap.add_argument('--laplacian', choices=('uniform', 'cot'), default='uniform',
                    help='nr.laplacian_loss (every neighbour weighs the same) or nr.cot_laplacian_loss')
    ap.add_argument('--edge-weight', type=float, default=0., help='weight of nr.edge_length_loss (0: not computed)')
    ap.add_argument('--out', default=None, help='write the fitted mesh as an .obj file')
    return ap


def main():
    args = parser().parse_args()
    model = ScanFit(args.obj, args.level, args.samples, args.smoothness, torch.device('cuda', args.gpu),
                    mesh_to_scan=args.mesh_to_scan, laplacian=args.laplacian, edge_weight=args.edge_weight)
    opt = nr.Adam(model.parameters(), lr=0.01)
    history = []
    for _ in range(args.iters):
        opt.zero_grad()
        to_mesh, to_scan, regularizer = model()
        (to_mesh + to_scan + regularizer).backward()
        opt.step()
        history.append((float(to_mesh.detach()), float(to_scan.detach())))
    print('scan -> mesh: first %.5f, last %.5f; mesh -> scan: first %.5f, last %.5f after %d steps'
          % (history[0][0], history[-1][0], history[0][1], history[-1][1], len(history)))
    if args.out:
        nr.save_obj(args.out, model.vertices.detach().cpu().numpy(), model.faces.cpu().numpy())


if __name__ == '__main__':
    main()

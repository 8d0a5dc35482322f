"""Fitting a mesh to a point cloud: an icosphere's vertices move until points sampled on its surface match
points sampled on the teapot.

The target is a fixed cloud drawn once from the teapot with nr.sample_points.  Every step draws fresh
points on the current icosphere (area-weighted, with the gradient back to the vertices), takes
nr.chamfer_distance against the target plus a small nr.laplacian_loss that keeps the surface smooth, and
steps nr.Adam: every operation of the step is a fused HIP kernel.  --laplacian cot takes
nr.cot_laplacian_loss instead (it leaves an irregular triangulation of a flat patch alone), and
--edge-weight W adds W * nr.edge_length_loss towards the icosphere's mean initial edge length, which keeps
the triangles from stretching and collapsing.

    python examples/example_chamfer.py [--iters 300] [--samples 5000] [--level 3] [--laplacian uniform|cot]
                                       [--edge-weight 0] [--out fitted.obj]

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


class CloudFit(torch.nn.Module):
    def __init__(self, obj_file, level, samples, smoothness, device, seed=0, laplacian='uniform', edge_weight=0.):
        super().__init__()
        self.generator = torch.Generator(device=device).manual_seed(seed)
        vertices, faces = nr.load_obj(obj_file)
        target_vertices = torch.as_tensor(vertices).float().to(device)
        with torch.no_grad():
            target = nr.sample_points(target_vertices, torch.as_tensor(faces).to(device).int(), samples,
                                      generator=self.generator)
        self.loss = nr.ChamferLoss(target)
        sphere, sphere_faces = synthetic.icosphere(level, radius=0.5)
        self.faces = torch.as_tensor(sphere_faces).to(device).int()
        self.vertices = torch.nn.Parameter(torch.as_tensor(sphere).float().to(device))
        self.topology = nr.mesh_topology(self.faces, sphere.shape[0])
        self.samples, self.smoothness = samples, smoothness
        self.laplacian = nr.cot_laplacian_loss if laplacian == 'cot' else nr.laplacian_loss
        self.edge_weight = edge_weight
        corners = torch.as_tensor(sphere)[torch.as_tensor(sphere_faces).long()]  # [F, 3, 3]
        self.edge_length = float((corners - corners.roll(1, 1)).norm(dim=-1).mean())  # a closed mesh: every edge twice

    def forward(self):
        """The chamfer distance, and the weighted regularizers."""
        points = nr.sample_points(self.vertices, self.faces, self.samples, generator=self.generator)
        regularizer = self.smoothness * self.laplacian(self.vertices, self.topology)
        if self.edge_weight:
            regularizer = regularizer + self.edge_weight * nr.edge_length_loss(self.vertices, self.topology, self.edge_length)
        return self.loss(points), regularizer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--obj', default=os.path.join(DATA, 'teapot.obj'))
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--samples', type=int, default=5000)
    ap.add_argument('--level', type=int, default=3, help='icosphere subdivision level')
    ap.add_argument('--smoothness', type=float, default=0.01, help='weight of the Laplacian loss')
    ap.add_argument('--laplacian', choices=('uniform', 'cot'), default='uniform',
                    help='nr.laplacian_loss (every neighbour weighs the same) or nr.cot_laplacian_loss')
    ap.add_argument('--edge-weight', type=float, default=0., help='weight of nr.edge_length_loss (0: not computed)')
    ap.add_argument('--gpu', type=int, default=0)
    ap.add_argument('--out', default=None, help='write the fitted mesh as an .obj file')
    args = ap.parse_args()
    model = CloudFit(args.obj, args.level, args.samples, args.smoothness, torch.device('cuda', args.gpu),
                     laplacian=args.laplacian, edge_weight=args.edge_weight)
    opt = nr.Adam(model.parameters(), lr=0.01)
    history = []
    for _ in range(args.iters):
        opt.zero_grad()
        chamfer, regularizer = model()
        (chamfer + regularizer).backward()
        opt.step()
        history.append(float(chamfer.detach()))
    print('chamfer distance: first %.5f, last %.5f after %d steps' % (history[0], history[-1], len(history)))
    if args.out:
        nr.save_obj(args.out, model.vertices.detach().cpu().numpy(), model.faces.cpu().numpy())


if __name__ == '__main__':
    main()

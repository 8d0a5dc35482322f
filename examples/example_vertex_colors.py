"""Vertex-colour fitting: optimise per-vertex colours until the rendered images match target images.

The shape of the reference's examples_pytorch/example3.py (texture optimisation), with per-vertex colours
in place of a texture atlas: the teapot's colours [V, 3] are the parameter, shared by a batch of views;
every step renders them with Renderer.render_attributes (nr.rasterize_attributes: the fused HIP
interpolation, gradients back to the colours), takes nr.squared_error_loss against the targets and steps
nr.Adam.  The targets are renders of the same mesh coloured by its vertex positions, from the same views.

    python examples/example_vertex_colors.py [--iters 200] [--views 8] [--out result.png]

The mesh defaults to tests/data/teapot.obj.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import neural_renderer_v2_pytorch_amd as nr  # noqa: E402

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'data')
CAMERA_DISTANCE, ELEVATION = 2.732, 30


class ColourFit(torch.nn.Module):
    def __init__(self, obj_file, views, device):
        super().__init__()
        vertices, faces = nr.load_obj(obj_file)
        self.vertices = torch.as_tensor(vertices[None]).to(device).expand(views, -1, -1).contiguous()
        self.faces = torch.as_tensor(faces).to(device).int()
        self.colours = torch.nn.Parameter(torch.full((vertices.shape[0], 3), 0.5, device=device))
        self.renderer = nr.Renderer()
        eyes = [nr.get_points_from_angles(CAMERA_DISTANCE, ELEVATION, 360.0 * i / views) for i in range(views)]
        self.renderer.viewpoints = torch.as_tensor(np.asarray(eyes, np.float32), device=device)
        with torch.no_grad():  # the targets: colours = vertex positions mapped to [0, 1]
            truth = self.vertices[0] * 0.5 + 0.5
            self.targets = self.renderer.render_attributes(self.vertices, self.faces, truth)

    def render(self):
        return self.renderer.render_attributes(self.vertices, self.faces, self.colours)

    def forward(self):
        return nr.squared_error_loss(self.render(), self.targets, average=True)


def save_image(image, path):
    from PIL import Image
    a = image.detach().clamp(0, 1).permute(1, 2, 0).cpu().numpy()
    Image.fromarray((a * 255).astype(np.uint8)).save(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--obj', default=os.path.join(DATA, 'teapot.obj'))
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--gpu', type=int, default=0)
    ap.add_argument('--out', default=None, help='write view 0 of the result as an image')
    args = ap.parse_args()
    model = ColourFit(args.obj, args.views, torch.device('cuda', args.gpu))
    opt = nr.Adam(model.parameters(), lr=0.05)
    losses = []
    for _ in range(args.iters):
        opt.zero_grad()
        loss = model()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print('loss: first %.2f, last %.2f after %d steps' % (losses[0], losses[-1], len(losses)))
    if args.out:
        save_image(model.render()[0], args.out)


if __name__ == '__main__':
    main()

"""Fitting the pose of a rigged mesh: a tube with a chain of four joints is bent until its silhouettes from two
views, and the projections of its joints, match those of a hidden pose.

The rig is an nr.Skinning module (forward kinematics and linear blend skinning, one fused HIP launch each); the
pose -- axis-angle, [1, 4, 3] -- is the only parameter and starts at zero.  The loss is

  silhouettes   nr.iou_loss of Renderer.render_silhouettes from azimuth 0 and 90, against the hidden pose's;
  keypoints     nr.squared_error_loss of the posed joints seen through the same two cameras
                (Renderer.transform_vertices) against the hidden pose's: 2-D keypoints need nothing new;

stepped by nr.Adam: every operation of the step is a fused HIP kernel.

    python examples/example_pose_fit.py [--iters 200] [--image-size 64] [--keypoint-weight 1.0] [--out posed.obj]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import neural_renderer_v2_pytorch_amd as nr  # noqa: E402
from neural_renderer_v2_pytorch_amd import synthetic  # noqa: E402

CAMERA_DISTANCE, ELEVATION, AZIMUTHS = 2.732, 0, (0, 90)
HIDDEN_POSE = [[0., 0., 0.25], [0.3, 0., 0.45], [0., 0., -0.6], [-0.4, 0., 0.3]]


class PoseFit(torch.nn.Module):
    def __init__(self, device, image_size=64, keypoint_weight=1.0):
        super().__init__()
        vertices, faces, joints, parents, weights, indices = synthetic.rigged_tube(rings=16, segments=12, joints=4)
        self.rig = nr.Skinning(joints, parents, weights, indices).to(device)
        self.vertices = torch.as_tensor(vertices).to(device)
        self.faces = torch.as_tensor(faces).to(device)
        self.keypoint_weight = keypoint_weight
        self.renderers = []
        for azimuth in AZIMUTHS:
            renderer = nr.Renderer()
            renderer.image_size = image_size
            renderer.viewpoints = nr.get_points_from_angles(CAMERA_DISTANCE, ELEVATION, azimuth)
            self.renderers.append(renderer)
        self.pose = torch.nn.Parameter(torch.zeros((1, len(HIDDEN_POSE), 3), device=device))
        with torch.no_grad():
            self.targets = self.observe(torch.tensor([HIDDEN_POSE], device=device))

    def observe(self, pose):
        """Per view: (silhouettes [1, s, s], the joints' image coordinates [1, J, 2])."""
        posed_vertices, posed_joints = self.rig(pose, self.vertices)
        return [(renderer.render_silhouettes(posed_vertices, self.faces), renderer.transform_vertices(posed_joints)[..., :2])
                for renderer in self.renderers]

    def forward(self):
        """(the silhouette loss, the keypoint loss), each summed over the views."""
        silhouette = keypoints = 0.
        for (image, points), (target_image, target_points) in zip(self.observe(self.pose), self.targets):
            silhouette = silhouette + nr.iou_loss(image, target_image).sum()
            keypoints = keypoints + nr.squared_error_loss(points, target_points).sum()
        return silhouette, self.keypoint_weight * keypoints


def optimize(model, iters, lr=0.05):
    """nr.Adam over the pose; returns the loss of every step."""
    opt = nr.Adam(model.parameters(), lr=lr)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        silhouette, keypoints = model()
        loss = silhouette + keypoints
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--image-size', type=int, default=64)
    ap.add_argument('--keypoint-weight', type=float, default=1.0)
    ap.add_argument('--gpu', type=int, default=0)
    ap.add_argument('--out', default=None, help='write the posed mesh as an .obj file')
    args = ap.parse_args()
    model = PoseFit(torch.device('cuda', args.gpu), args.image_size, args.keypoint_weight)
    losses = optimize(model, args.iters)
    error = float((model.pose.detach() - torch.tensor([HIDDEN_POSE], device=model.pose.device)).abs().max())
    print('loss: first %.5f, last %.5f after %d steps; largest pose error %.4f' % (losses[0], losses[-1], len(losses), error))
    if args.out:
        with torch.no_grad():
            posed = model.rig(model.pose, model.vertices)[0][0]
        nr.save_obj(args.out, posed.cpu().numpy(), model.faces.cpu().numpy())


if __name__ == '__main__':
    main()

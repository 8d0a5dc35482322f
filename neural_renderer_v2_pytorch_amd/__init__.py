"""neural_renderer_v2_pytorch_amd -- MI355X-native drop-in for neural_renderer_torch's rasterize path.

Public surface mirrors the reference's neural_renderer_torch/__init__.py:1-14 (minus Mesh; the
reference's chainer-based Adam is optimizers.Adam here).  Compute runs in hand-written HIP kernels for
gfx950 (csrc/nr_raster.hip) behind the C ABI of include/nr_raster.h; there is no CPU fallback.
"""
from .lights import AmbientLight, DirectionalLight, Light, SpecularLight
from .load_obj import load_obj
from .look import look
from .look_at import look_at
from .perspective import perspective
from .projection import projection
from .rasterize import rasterize_core, rasterize_depth, rasterize_rgb, rasterize_rgba, rasterize_silhouettes
from .rasterize_param import RasterizeHyperparam, RasterizeParam
from .renderer import Renderer
from .save_obj import save_obj
from .utils import create_textures, get_points_from_angles, imread, make_gif, to_gpu
from .differentiation import differentiation
from .camera import camera_transform, projection_transform
from .mesh_loss import (ArapLoss, CotLaplacianLoss, EdgeLengthLoss, FlattenLoss, LaplacianLoss, MeshTopology, arap_loss,
                        arap_loss_torch, arap_rotations, arap_rotations_torch, cot_laplacian_loss, cot_laplacian_loss_torch,
                        cot_weights, cot_weights_torch, edge_length_loss, edge_length_loss_torch, flatten_loss,
                        flatten_loss_torch, laplacian_loss, laplacian_loss_torch, mesh_topology)
from .image_loss import (HuberLoss, IoULoss, SquaredErrorLoss, SSIMLoss, huber_loss, huber_loss_torch, iou_loss, iou_loss_torch,
                         squared_error_loss, squared_error_loss_torch, ssim_loss, ssim_loss_torch)
from .optimizers import Adam, adam_step_torch
from .attributes import (NR_ATTR_MAX_CHANNELS, attributes_from_maps_torch, rasterize_attributes,
                         rasterize_attributes_torch)
from .point_loss import (ChamferLoss, MeshPointLoss, PointMeshLoss, chamfer_distance, chamfer_distance_torch,
                         closest_points_on_mesh, closest_points_on_mesh_torch, closest_points_to_faces,
                         closest_points_to_faces_torch, mesh_point_distance, mesh_point_distance_torch, nearest_points,
                         nearest_points_torch, point_mesh_distance, point_mesh_distance_torch, sample_points,
                         sample_points_torch)
from .skinning import (NR_RODRIGUES_SERIES, NR_SKIN_CHUNK, NR_SKIN_MAX_INFLUENCES, NR_SKIN_MAX_JOINTS, Skeleton, SkinBinding,
                       Skinning, pose_transforms, pose_transforms_torch, rodrigues_torch, skeleton, skin_binding,
                       skin_vertices, skin_vertices_torch)
from .rigid import NR_RIGID_MIN_CONDITION, ICPResult, icp, icp_torch, rigid_align, rigid_align_torch

__version__ = '2.0.2+mi355x.1'

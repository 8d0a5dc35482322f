"""ctypes binding of the HIP library (include/nr_raster.h -> _lib/libnr_raster.so).

The library is loaded on first use.  There is no CPU fallback: if the shared object is missing or
a call fails, a RuntimeError is raised.  Build it with `python -c "import __graft_entry__ as g;
g.build()"` from the repository root (hipcc --offload-arch=gfx950).
"""
import ctypes
import os

import torch

LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib")
# NR_LIB_PATH: developer override used by the timing-variant scripts in tools/
LIB_PATH = os.environ.get("NR_LIB_PATH") or os.path.join(LIB_DIR, "libnr_raster.so")

NR_DRAW_RGB = 1
NR_DRAW_SILHOUETTES = 2
NR_DRAW_DEPTH = 4

ABI_VERSION = 6  # include/nr_raster.h NR_ABI_VERSION

NR_LAUNCH_FUSED_SHADE, NR_LAUNCH_STATIC_CHANNELS, NR_LAUNCH_TWO_PX_PER_LANE, NR_LAUNCH_DEEP_FIRST, NR_LAUNCH_SPLIT = 1, 2, 4, 8, 16
NR_LAUNCH_HOT_WINDOWS, NR_LAUNCH_DEALT_QUARTERS, NR_LAUNCH_QUADRANTS = 32, 64, 128
NR_LAUNCH_LIGHTS, NR_LAUNCH_BACKGROUNDS, NR_LAUNCH_SIL_ONLY = 256, 512, 1024  # k_raster_bwd's feature instantiation
NR_LAUNCH_SPLIT_X_TO_Y, NR_LAUNCH_SPLIT_Y_TO_X = 2048, 4096  # k_chamfer_nn: a direction's targets split over several blocks
NR_LAUNCH_SPLIT_FACES = 8192  # k_point_face_nn: the faces split over several blocks
NR_LAUNCH_SPLIT_POINTS = 16384  # k_face_point_nn: the points split over several blocks
NR_LAUNCH_SPLIT_TARGETS = 32768  # k_icp_nn: the targets split over several blocks
NR_HOT_MAX, NR_HOT_COPIES = 256, 32

c_int, c_float, c_void_p, c_size_t, c_ll = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_longlong


class NrRasterArgs(ctypes.Structure):
    _fields_ = [
        ("batch_size", c_int), ("num_vertices", c_int), ("num_faces", c_int), ("image_size", c_int),
        ("anti_aliasing", c_int), ("draw_backside", c_int), ("draw_flags", c_int),
        ("near", c_float), ("far", c_float), ("eps", c_float), ("depth_min_delta", c_float),
        ("vertices", c_void_p), ("faces", c_void_p),
        ("vertices_textures", c_void_p), ("vt_batch_stride", c_ll), ("num_vertices_textures", c_int),
        ("faces_textures", c_void_p), ("textures", c_void_p),
        ("tex_stride_b", c_ll), ("tex_stride_c", c_ll), ("tex_stride_p", c_ll),
        ("tex_height", c_int), ("tex_width", c_int),
        ("face_records", c_void_p), ("face_uv", c_void_p), ("face_index", c_void_p),
        ("workspace", c_void_p), ("workspace_bytes", c_size_t),
        ("vertex_offsets", c_void_p), ("vertex_faces", c_void_p), ("halo", c_void_p),
        ("num_lights", c_int), ("lights", c_void_p), ("face_normals", c_void_p), ("vertex_normals", c_void_p),
        ("normal_offsets", c_void_p), ("normal_faces", c_void_p),
        ("backgrounds", c_void_p), ("bg_stride_b", c_ll), ("bg_stride_c", c_ll), ("bg_stride_y", c_ll),
        ("grad_backgrounds", c_void_p), ("textures_packed", c_void_p),
        ("bwd_workspace", c_void_p), ("bwd_workspace_bytes", c_size_t), ("face_index_sparse", c_int),
        ("face_hot", c_void_p), ("num_hot", c_int), ("hot_acc", c_void_p),
    ]

NR_LIGHT_AMBIENT, NR_LIGHT_DIRECTIONAL, NR_LIGHT_SPECULAR, NR_LIGHT_FLOATS = 0, 1, 2, 8
NR_CAMERA_NONE, NR_CAMERA_LOOK_AT, NR_CAMERA_LOOK = 0, 1, 2
NR_LOSS_SQUARED, NR_LOSS_HUBER = 0, 1
NR_SSIM_SAME, NR_SSIM_VALID = 0, 1
NR_SSIM_TILE, NR_SSIM_MAX_WINDOW = 32, 11  # csrc/nr_ssim_loss.h SS_TILE (output tile edge of a block), 2 SS_MAX_R + 1
NR_ADAM_MAX_TENSORS, NR_ADAM_CHUNK = 24, 4096  # tensors per launch pair, elements of one tensor per block
NR_ATTR_MAX_CHANNELS = 64
NR_CHAMFER_X_TO_Y, NR_CHAMFER_Y_TO_X = 1, 2
NR_CHAMFER_TILE = 1024  # csrc/nr_point_loss.h PL_TILE: targets staged in LDS at a time
NR_POINT_MESH_TILE, NR_POINT_MESH_QBLOCK = 256, 1024  # csrc/nr_point_mesh.h PM_TILE (face records in LDS), PM_QBLOCK (queries per block)
NR_POINT_MESH_SPLIT_BLOCKS = 4096  # PM_SPLIT_BLOCKS: the faces are split over further blocks while a launch has fewer
NR_FACE_POINT_TILE, NR_FACE_POINT_FBLOCK = 64, 256  # csrc/nr_face_point.h FP_TILE (points in LDS), FP_FBLOCK (faces per block)
NR_FACE_POINT_SPLIT_BLOCKS = 4096  # FP_SPLIT_BLOCKS: the points are split over further blocks while a launch has fewer
NR_COT_MIN_WEIGHT = 1e-6  # include/nr_raster.h: a vertex whose cotangent weights sum to no more has delta = 0
# include/nr_raster.h: at or below this condition rigid_align's rotation passes no gradient; floats of its saved
# per-item record and of a transform (R, t, s) in device memory; csrc/nr_rigid.h RG_CHUNK: points per block of its sums
NR_RIGID_MIN_CONDITION, NR_RIGID_RECORD_FLOATS, NR_RIGID_TRANSFORM_FLOATS, NR_RIGID_CHUNK = 1e-6, 32, 13, 1024
# include/nr_raster.h: joints of a skeleton, influences per vertex, entries of a joint's CSR row per block of
# k_skin_bwd_transforms, and the |r|^2 below which Rodrigues' coefficients come from their series
NR_SKIN_MAX_JOINTS, NR_SKIN_MAX_INFLUENCES, NR_SKIN_CHUNK, NR_RODRIGUES_SERIES = 256, 8, 256, 1e-4


class NrCameraArgs(ctypes.Structure):  # include/nr_raster.h
    _fields_ = [
        ("batch_size", c_int), ("num_vertices", c_int), ("vertices", c_void_p), ("v_batch_stride", c_ll),
        ("eye", c_void_p), ("eye_batch_stride", c_ll), ("mode", c_int), ("at", c_float * 3), ("up", c_float * 3),
        ("perspective", c_int), ("width", c_float),
    ]


class NrProjectionArgs(ctypes.Structure):  # include/nr_raster.h
    _fields_ = [
        ("batch_size", c_int), ("num_vertices", c_int), ("vertices", c_void_p), ("v_batch_stride", c_ll),
        ("K", c_void_p), ("k_batch_stride", c_ll), ("R", c_void_p), ("r_batch_stride", c_ll),
        ("t", c_void_p), ("t_batch_stride", c_ll), ("dist", c_void_p), ("dist_batch_stride", c_ll),
        ("orig_size", c_float), ("eps", c_float),
    ]


class NrAdamTensor(ctypes.Structure):  # include/nr_raster.h
    _fields_ = [
        ("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p), ("step", c_void_p),
        ("numel", c_ll), ("lr_scale", ctypes.c_double),
    ]


class NrAdamArgs(ctypes.Structure):  # include/nr_raster.h
    _fields_ = [
        ("num_tensors", c_int), ("tensors_capacity", c_int), ("tensors", ctypes.POINTER(NrAdamTensor)),
        ("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
        ("lr_device", c_void_p), ("skip_zero_grad", c_int), ("scratch", c_void_p), ("scratch_bytes", c_size_t),
    ]


class NrAttributeArgs(ctypes.Structure):  # include/nr_raster.h
    _fields_ = [
        ("batch_size", c_int), ("num_faces", c_int), ("num_vertices", c_int), ("num_attributes", c_int),
        ("num_channels", c_int), ("image_size", c_int), ("anti_aliasing", c_int), ("perspective_correct", c_int),
        ("face_index", c_void_p), ("face_records", c_void_p), ("faces", c_void_p), ("faces_attributes", c_void_p),
        ("attributes", c_void_p), ("attr_batch_stride", c_ll), ("internal", c_void_p),
    ]


_P, _args = c_void_p, ctypes.POINTER
_pointwise = [_P, c_ll, _P, c_ll, _P, c_ll, c_int, c_int, c_float, c_int, c_int]

# every symbol declared in include/nr_raster.h: name -> (restype, argtypes)
SIGNATURES = {
    "nr_last_error": (ctypes.c_char_p, []),
    "nr_version": (c_int, []),
    "nr_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "nr_face_index_map_forward_safe": (c_int, [_P, _P, c_int, c_int, c_int, c_float, c_float, c_int, c_float, c_float, _P,
                                               c_size_t, _P]),
    "nr_compute_weight_map": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P]),
    "nr_mask_foreground_forward": (c_int, [_P, _P, _P, c_ll, c_int, _P]),
    "nr_mask_foreground_backward": (c_int, [_P, _P, _P, c_ll, c_int, _P]),
    "nr_differentiation_backward": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "nr_num_channels": (c_int, [c_int]),
    "nr_rasterize_forward": (c_int, [_args(NrRasterArgs), _P, _P]),
    "nr_rasterize_backward": (c_int, [_args(NrRasterArgs), _P, _P, _P, _P, c_size_t, c_int, _P]),
    "nr_backward_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "nr_profile_enable": (c_int, [c_int]),
    "nr_profile_read": (c_int, [ctypes.c_char_p, ctypes.POINTER(c_float)]),
    "nr_selftest_division": (c_int, [_P, _P, _P, _P, c_ll, _P]),
    "nr_halo_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "nr_raster_args_size": (c_size_t, []),
    "nr_rasterize_backward_params": (c_int, [_args(NrRasterArgs), _P, _P, _P, _P]),
    "nr_camera_forward": (c_int, [_args(NrCameraArgs), _P, _P]),
    "nr_camera_backward": (c_int, [_args(NrCameraArgs), _P, _P, _P, _P, c_size_t, _P]),
    "nr_camera_workspace_bytes": (c_size_t, [c_int]),
    "nr_texture_packed_bytes": (c_size_t, [c_int, c_int, c_int]),
    "nr_last_launch": (c_int, [ctypes.c_char_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "nr_tile_order": (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_uint16)]),
    "nr_hot_acc_bytes": (c_size_t, [c_int]),
    "nr_projection_args_size": (c_size_t, []),
    "nr_projection_forward": (c_int, [_args(NrProjectionArgs), _P, _P]),
    "nr_projection_workspace_bytes": (c_size_t, [c_int, c_int]),
    "nr_projection_backward": (c_int, [_args(NrProjectionArgs), _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "nr_mesh_loss_workspace_bytes": (c_size_t, [c_int, c_int]),
    "nr_laplacian_forward": (c_int, [_P, _P, _P, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "nr_laplacian_backward": (c_int, [_P, _P, _P, _P, c_int, c_int, _P, _P]),
    "nr_flatten_forward": (c_int, [_P, _P, c_int, c_int, c_int, c_float, _P, _P, _P, c_size_t, _P]),
    "nr_flatten_backward": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, _P]),
    "nr_edge_length_forward": (c_int, [_P, _P, _P, c_int, c_int, c_float, _P, _P, c_size_t, _P]),
    "nr_edge_length_backward": (c_int, [_P, _P, _P, _P, c_int, c_int, c_float, _P, _P]),
    "nr_cot_laplacian_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "nr_cot_laplacian_forward": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P, _P, _P, _P, _P, c_size_t,
                                         _P]),
    "nr_cot_laplacian_backward": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P, _P]),
    "nr_cot_weights_workspace_bytes": (c_size_t, [c_int, c_int]),
    "nr_cot_weights": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P, _P, c_size_t, _P]),
    "nr_arap_workspace_bytes": (c_size_t, [c_int, c_int]),
    "nr_arap_forward": (c_int, [_P, _P, c_ll, _P, c_ll, _P, _P, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "nr_arap_backward": (c_int, [_P, _P, c_ll, _P, c_ll, _P, _P, _P, _P, c_int, c_int, c_int, _P, _P]),
    "nr_pose_transforms_forward": (c_int, [_P, c_int, _P, c_ll, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P]),
    "nr_pose_transforms_backward": (c_int, [_P, c_int, _P, c_ll, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P]),
    "nr_skin_workspace_bytes": (c_size_t, [c_int, c_int]),
    "nr_skin_forward": (c_int, [_P, c_ll, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "nr_skin_backward": (c_int, [_P, c_ll, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P,
                                 c_size_t, _P]),
    "nr_image_loss_workspace_bytes": (c_size_t, [c_int, c_int]),
    "nr_pointwise_loss_forward": (c_int, _pointwise + [_P, _P, c_size_t, _P]),
    "nr_pointwise_loss_backward": (c_int, _pointwise + [_P, _P, _P]),
    "nr_iou_loss_forward": (c_int, [_P, c_ll, _P, c_ll, c_float, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "nr_iou_loss_backward": (c_int, [_P, c_ll, _P, c_float, c_int, c_int, _P, _P, _P]),
    "nr_ssim_loss_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "nr_ssim_loss_forward": (c_int, [_P, c_ll, _P, c_ll, c_int, c_int, c_int, c_int, c_int, _P, c_float, c_float, c_int, _P, _P, _P,
                                     c_size_t, _P]),
    "nr_ssim_loss_backward": (c_int, [_P, c_ll, _P, c_ll, _P, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, _P]),
    "nr_adam_args_size": (c_size_t, []),
    "nr_adam_scratch_bytes": (c_size_t, [c_int]),
    "nr_adam_step": (c_int, [_args(NrAdamArgs), _P]),
    "nr_attribute_args_size": (c_size_t, []),
    "nr_attributes_forward": (c_int, [_args(NrAttributeArgs), _P, _P]),
    "nr_attributes_backward_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "nr_attributes_backward": (c_int, [_args(NrAttributeArgs), _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "nr_chamfer_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "nr_chamfer_forward": (c_int, [_P, _P, c_ll, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "nr_chamfer_backward": (c_int, [_P, _P, c_ll, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "nr_sample_points_workspace_bytes": (c_size_t, [c_int, c_int]),
    "nr_sample_points_forward": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "nr_sample_points_backward": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "nr_point_mesh_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "nr_point_mesh_forward": (c_int, [_P, c_ll, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, c_size_t, _P]),
    "nr_point_mesh_backward": (c_int, [_P, c_ll, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "nr_face_point_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "nr_face_point_forward": (c_int, [_P, c_ll, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, c_size_t, _P]),
    "nr_face_point_backward": (c_int, [_P, c_ll, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "nr_rigid_workspace_bytes": (c_size_t, [c_int, c_int]),
    "nr_rigid_align_forward": (c_int, [_P, _P, c_ll, _P, c_ll, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "nr_rigid_align_backward": (c_int, [_P, _P, c_ll, _P, c_ll, _P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "nr_icp_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "nr_icp": (c_int, [_P, _P, c_ll, c_int, c_int, c_int, c_int, c_int, c_float, _P, _P, _P, _P, _P, c_size_t, _P]),
}
EXPORTS = list(SIGNATURES)

# the library's sizeof of each argument struct against its ctypes mirror
STRUCT_SIZES = [("nr_projection_args_size", NrProjectionArgs), ("nr_adam_args_size", NrAdamArgs),
                ("nr_attribute_args_size", NrAttributeArgs), ("nr_raster_args_size", NrRasterArgs)]

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("neural_renderer_v2_pytorch_amd: HIP library %s is missing; build it with "
                           "__graft_entry__.build() (there is no CPU fallback)" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    # additions within one ABI version (the nr_projection_*, mesh-loss, image-loss, nr_ssim_loss_*, nr_adam_*, nr_attributes_*,
    # point-loss entry points, the two point / mesh distance directions, nr_point_mesh_* and nr_face_point_*, and the
    # articulated-mesh entry points, nr_pose_transforms_* and nr_skin_*, nr_cot_weights and nr_arap_*, nr_rigid_* and nr_icp):
    # a library built before them still reports the version this binding expects
    missing = [name for name in EXPORTS if not hasattr(L, name)]
    if missing:
        raise RuntimeError("neural_renderer_v2_pytorch_amd: %s lacks %s; this binding needs a newer build of the "
                           "library (rebuild with __graft_entry__.build())" % (LIB_PATH, ", ".join(missing)))
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    # a library of another ABI revision (an NR_LIB_PATH override, a stale build) would misread the
    # arguments (e.g. an older nr_rasterize_backward takes its stream where workspace_zeroed is now)
    for size_fn, struct in STRUCT_SIZES:
        if getattr(L, size_fn)() != ctypes.sizeof(struct):
            raise RuntimeError("neural_renderer_v2_pytorch_amd: %s has a %d-byte %s; this binding needs %d bytes "
                               "(rebuild with __graft_entry__.build())"
                               % (LIB_PATH, getattr(L, size_fn)(), struct.__name__, ctypes.sizeof(struct)))
    if L.nr_version() != ABI_VERSION:
        raise RuntimeError("neural_renderer_v2_pytorch_amd: %s has ABI version %d; this binding needs version %d "
                           "(rebuild with __graft_entry__.build())" % (LIB_PATH, L.nr_version(), ABI_VERSION))
    _lib = L
    return L


def last_launch(kernel):
    """(threads per block, NR_LAUNCH_* flags) of the latest launch of `kernel` in this process: the variant the
    library actually ran.  kernel: "k_raster_fwd", "k_raster_bwd", "k_chamfer_nn", or the nearest-neighbour loop of a
    point / mesh distance direction, "k_point_face_nn" or "k_face_point_nn", or the ICP's, "k_icp_nn"."""
    t, f = c_int(), c_int()
    check(lib().nr_last_launch(kernel.encode(), ctypes.byref(t), ctypes.byref(f)), "nr_last_launch")
    return t.value, f.value


def check(status, what):
    if status != 0:
        raise RuntimeError("%s failed (status %d): %s" % (what, status, lib().nr_last_error().decode()))


def stream_of(t):
    """The raw hipStream_t of the current stream on t's device (what torch launches on)."""
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(t.device.index))


class on_device:
    """`with torch.cuda.device(dev)` that costs nothing when dev is already the current device
    (the usual case: the per-call exchange of the current device was a few microseconds of host
    time per launch call)."""
    __slots__ = ("idx", "prev")

    def __init__(self, dev):
        self.idx = dev.index

    def __enter__(self):
        cur = torch._C._cuda_getDevice()
        self.prev = None if cur == self.idx else torch.cuda._exchange_device(self.idx)

    def __exit__(self, *exc):
        if self.prev is not None:
            torch.cuda._exchange_device(self.prev)
        return False


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda):
            raise RuntimeError("neural_renderer_v2_pytorch_amd runs on the GPU only (no CPU fallback); "
                               "got a %s" % ("CPU tensor" if torch.is_tensor(t) else type(t).__name__))

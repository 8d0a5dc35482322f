"""The workspace sizes of the two point / mesh distance directions (no GPU needed): nr_point_mesh_workspace_bytes
and nr_face_point_workspace_bytes are cut by one layout function from a direction descriptor, and the entry points
point into the caller's buffer by it.  The values were recorded from the library before the two layouts became one
and must not move: a caller may size its buffer once and keep it."""
import pytest

from neural_renderer_v2_pytorch_amd import _lib

T, Q, S = _lib.NR_POINT_MESH_TILE, _lib.NR_POINT_MESH_QBLOCK, _lib.NR_POINT_MESH_SPLIT_BLOCKS
TP, FQ, SP = _lib.NR_FACE_POINT_TILE, _lib.NR_FACE_POINT_FBLOCK, _lib.NR_FACE_POINT_SPLIT_BLOCKS

# (B, N, F): (point -> face bytes, face -> point bytes).  The queries are the N points in the first direction (blocks
# of Q, the F faces in ranges of at least T) and the F faces in the second (blocks of FQ, the N points in ranges of
# at least TP); a launch splits its targets while it has fewer than S (SP) blocks.
RECORDED = {
    (2, 10, 7): (2304, 2304),                               # neither splits
    (1, 5, 3 * T + 2): (75264, 83968),                      # the cap F // T = 3 ranges; the other way unsplit
    (1, 3 * TP + 2, 5): (3584, 1792),                       # unsplit; the cap N // TP = 3 ranges
    (1, 2048 * Q, 1000): (58816256, 8300288),               # exactly two ranges (2048 blocks, F // T = 3); 1024 ranges
    (1, 200, 2048 * FQ): (53611520, 65011712),              # the cap F // T = 2048; exactly two ranges (N // TP = 3)
    (1, (S - 1) * Q + 1, 3 * T + 2): (50394112, 6391808),   # S query blocks: the first shape that no longer splits
    (1, (S - 1) * Q, 3 * T + 2): (117485824, 6391808),      # S - 1 query blocks: the last that does (two ranges)
    (1, 3 * TP + 2, (SP - 1) * FQ + 1): (106997504, 113219584),  # the same pair in the other direction
    (1, 3 * TP + 2, (SP - 1) * FQ): (106997248, 129991680),
    (3, 257, 300): (96512, 127232),                         # B > 1: one range; the cap N // TP = 4
    (2, Q + 1, 2 * T + 1): (157184, 243200),                # B > 1: two ranges by the cap; 16 ranges
    (2, 2 * TP + 1, FQ + 1): (53248, 65024),                # B > 1: one range; two by the cap
    (16, 20000, 5120): (44984320, 17367040),                # a scan against an icosphere of level 4, 16 items
    (0, 5, 5): (0, 0), (5, 0, 5): (0, 0), (5, 5, 0): (0, 0), (-1, 5, 5): (0, 0),  # nothing to do
}


def test_constants_are_the_recorded_ones():
    assert (T, Q, S, TP, FQ, SP) == (256, 1024, 4096, 64, 256, 4096)


@pytest.mark.parametrize("shape", list(RECORDED))
def test_workspace_bytes_are_the_recorded_ones(shape):
    L = _lib.lib()
    assert (L.nr_point_mesh_workspace_bytes(*shape), L.nr_face_point_workspace_bytes(*shape)) == RECORDED[shape]

"""Vertex-attribute rendering (rasterize_attributes) where tests/test_gpu_attributes.py's one centred scene
never goes: foreground on the image borders, more faces in a wave than a handful, k_attr_vertex_sum past its
first block, the anti-aliased instantiations at an odd output size, a shared table over three items,
attribute rows that no face references, an item whose upstream gradient is 0, and a strided upstream
gradient.  Same reference (the float32 composition on the CPU from the oracle's pieces), helpers and
tolerances as that file: images 1e-5 + 1e-5 |ref|; gradients 1e-4 max|ref| + 1e-4 |ref| with the vertex
gradient's x, y and its z scaled separately.

Scenes, all from synthetic: proj = synthetic.project(jittered(v, B, sigma), viewpoints(B)), then
proj[..., :2] scaled and shifted.

  dense      icosphere(level=3), 1,280 faces, 642 vertices, B = 2, sigma 0.002, unscaled: up to 51 distinct faces
             in one wave's 8x8 pixels (the segmented reduction of k_attr_bwd loops that often), faces that own a
             single pixel, and more than 780 faces that own none (their records stay at the zero fill);
             B V = 1284 is six blocks of k_attr_vertex_sum
  border     icosphere(level=1), B = 2, sigma 0.02, x and y times 2.0, then x + 0.05, y - 0.08: the sphere runs
             past all four image sides (diff_stencil's four guards are false in lanes that compute a gradient,
             `up` reads pool row and column 0 and s - 1); the four corners stay background
  border-L2  the same transform of icosphere(level=2), 320 faces, 162 vertices, sigma 0.002, B = 3 (B V = 486: two
             blocks of k_attr_vertex_sum)
  cover      icosphere(level=1), B = 2, sigma 0.02, x and y times 2.8: every pixel is foreground -- no
             silhouette, no background wave, every corner pixel live

Cases (scene, s, anti-aliasing, C, perspective-correct, seed); attributes, then the upstream gradient, N(0, 1)
from np.random.RandomState(seed).  The counts are the oracle's, pinned by the tests; "border fg" counts the
foreground pixels of the four border rows and columns of every item (a corner in both of its lines).

  case  scene      s   AA  C   pc   seed   fg px  border fg  max faces per 8x8  faces with a pixel
  1     dense      33  no  3   yes  10     610    0          50                 466 of 1280
  2     dense      17  yes 22  no   11     664    0          51                 497
  3     dense      17  yes 21  yes  12     664    0          51                 497
  4     border     33  no  3   yes  13     1990   160        6                  48 of 80
  5     border     17  yes 5   yes  14     2115   166        6                  47
  6     border-L2  40  no  43  no   15     4522   328        12                 206 of 320
  7     cover      17  yes 3   yes  16     2312   272        6                  26

  1: k_attr_vertex_sum's blocks 1 to 5.  2: S = 34 is a partial tile of k_attr_bwd together with the `>> aa`
  read, 17^2 = 289 a partial second block of k_attr_fwd<true> (its `o >= s*s` exit), C = 22 a second atomic
  flush of one channel.  3: the same shapes with the depth term and exactly one full flush of 63 lanes.
  4, 5: the borders without and with the pool.  6: B = 3, three flushes (21 + 21 + 1 channels).  7: all
  4 * 68 border pixels are foreground.

Conditioning (the rule of test_gpu_attributes.py's docstring): on the CPU the float32 composition against the
same composition in float64 on the same maps stays, over the seven cases, at or under 1.3 % of the image
tolerance (case 6), 0.40 % of the vertex gradient's x, y tolerance (case 4), 0.21 % of its z tolerance (case 5;
the linear cases 2 and 6 have a z gradient of exactly 0 on both sides) and 0.22 % of the attribute gradient's
(case 4), so no soft-gradient selection flips.  The variants, as images / x, y / z / attributes: the shared
table of case 6 1.5 % / 0.27 % / exactly 0 / 0.15 %, case 4 with V + 7 rows 1.1 % / 0.31 % / 0.18 % / 0.21 %,
case 4 with an unreferenced row 0 1.1 % / 0.45 % / 0.14 % / 0.18 %, and case 4 with g[1] = 0 1.1 % / 0.53 % /
0.18 % / 0.16 %: all under the 10 % that keeps a seed."""
import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import synthetic

from test_gpu_attributes import close_grad, close_images, close_vertex_grad, reference, run_gpu

pytestmark = pytest.mark.gpu

# name: (icosphere level, B, jitter sigma, x and y scale, (x shift, y shift))
SCENES = {
    "dense": (3, 2, 0.002, 1.0, (0.0, 0.0)),
    "border": (1, 2, 0.02, 2.0, (0.05, -0.08)),
    "border-L2": (2, 3, 0.002, 2.0, (0.05, -0.08)),
    "cover": (1, 2, 0.02, 2.8, (0.0, 0.0)),
}
# (scene, image size, anti-aliasing, C, perspective-correct, seed)
CASES = {
    1: ("dense", 33, False, 3, True, 10),
    2: ("dense", 17, True, 22, False, 11),
    3: ("dense", 17, True, 21, True, 12),
    4: ("border", 33, False, 3, True, 13),
    5: ("border", 17, True, 5, True, 14),
    6: ("border-L2", 40, False, 43, False, 15),
    7: ("cover", 17, True, 3, True, 16),
}
# (foreground pixels, foreground pixels on the border lines, most faces in an aligned 8x8 block, faces with a pixel)
COUNTS = {
    1: (610, 0, 50, 466),
    2: (664, 0, 51, 497),
    3: (664, 0, 51, 497),
    4: (1990, 160, 6, 48),
    5: (2115, 166, 6, 47),
    6: (4522, 328, 12, 206),
    7: (2312, 272, 6, 26),
}


def scene(name):
    level, B, sigma, scale, (dx, dy) = SCENES[name]
    v, f = synthetic.icosphere(level=level)
    vb = torch.as_tensor(synthetic.jittered(v, B, sigma=sigma))
    proj = synthetic.project(vb, torch.as_tensor(synthetic.viewpoints(B))).clone()
    proj[..., :2] *= scale
    proj[..., 0] += dx
    proj[..., 1] += dy
    return proj.contiguous(), torch.as_tensor(f).long()


def case_data(case, Va=None):
    name, s, aa, C, pc, seed = CASES[case]
    rs = np.random.RandomState(seed)
    proj, f = scene(name)
    B = proj.shape[0]
    attrs = torch.as_tensor(rs.normal(size=(B, Va or proj.shape[1], C)).astype(np.float32))
    g = torch.as_tensor(rs.normal(size=(B, C, s, s)).astype(np.float32))
    return proj, f, attrs, g


_refs = {}


def case_reference(oracle, case):
    """Computed once per case, shared by the tests, never modified."""
    if case not in _refs:
        _, s, aa, C, pc, _ = CASES[case]
        proj, f, attrs, g = case_data(case)
        _refs[case] = reference(oracle, proj, f, attrs, g, s, aa, pc)
    return _refs[case]


def hyper(case):
    return nr.RasterizeHyperparam(image_size=CASES[case][1], anti_aliasing=CASES[case][2])


def border_lines(fg):
    """fg [B, S, S] bool -> [B, 4, S]: the top and bottom rows and the left and right columns."""
    return torch.stack([fg[:, 0, :], fg[:, -1, :], fg[:, :, 0], fg[:, :, -1]], 1)


def scene_counts(fim):
    fg = fim >= 0
    S = fim.shape[1]
    most = 0
    for b in range(fim.shape[0]):
        for y0 in range(0, S, 8):  # aligned to 8, as k_attr_bwd's waves are
            for x0 in range(0, S, 8):
                blk = fim[b, y0:y0 + 8, x0:x0 + 8]
                most = max(most, int(torch.unique(blk[blk >= 0]).numel()))
    return int(fg.sum()), int(border_lines(fg).sum()), most, int(torch.unique(fim[fg]).numel())


def check_scene(case, fim, F):
    """The scene is what its name claims (with margins, on the oracle's map), and the exact counts."""
    name = CASES[case][0]
    fg = fim >= 0
    S = fim.shape[1]
    counts = scene_counts(fim)
    print("case %d: fg %d, border fg %d, most faces per 8x8 %d, faces with a pixel %d of %d" % ((case,) + counts + (F,)))
    if name == "dense":
        assert counts[2] >= 40 and F - counts[3] >= 300
        owned = torch.bincount(fim[fg].long(), minlength=F)
        assert int((owned == 1).sum()) >= 1  # a face that covers a single pixel
    elif name.startswith("border"):
        assert int(border_lines(fg).sum(-1).min()) * 4 >= S  # every side of every item
        assert not fg[:, [0, 0, -1, -1], [0, -1, 0, -1]].any()
    else:
        assert bool(fg.all())
    assert counts == COUNTS[case]


@pytest.mark.parametrize("case", sorted(CASES))
def test_parity(oracle_mod, dev, case):
    """Images, the face-index map (bit-exact), grad_vertices and grad_attributes of the seven cases."""
    _, s, aa, C, pc, _ = CASES[case]
    proj, f, attrs, g = case_data(case)
    img_r, fim_r, gv_r, ga_r = case_reference(oracle_mod, case)
    check_scene(case, fim_r, f.shape[0])
    img, node, gv, ga = run_gpu(dev, proj, f, attrs, g, hyper(case), pc)
    assert img.shape == (proj.shape[0], C, s, s)
    assert torch.equal(node.face_index_map.cpu(), fim_r.int())
    close_images(img, img_r, "images")
    close_vertex_grad(gv, gv_r, "grad vertices")
    close_grad(ga, ga_r, "grad attributes")


@pytest.mark.parametrize("case", [1, 4, 7])
def test_composition_parity(oracle_mod, dev, case):
    """rasterize_attributes_torch on the dense, the border and the cover scene: the Level-1 k_diff_bwd meets
    the image border through the same diff_stencil."""
    pc = CASES[case][4]
    proj, f, attrs, g = case_data(case)
    img_r, _, gv_r, ga_r = case_reference(oracle_mod, case)
    pv = proj.to(dev).requires_grad_(True)
    at = attrs.to(dev).requires_grad_(True)
    img_t = nr.rasterize_attributes_torch(pv, f.to(dev).int(), at, hyper(case), None, pc)
    img_t.backward(g.to(dev))
    close_images(img_t, img_r, "composition images")
    close_vertex_grad(pv.grad, gv_r, "composition grad vertices")
    close_grad(at.grad, ga_r, "composition grad attributes")


def test_shared_table_over_three_items(oracle_mod, dev):
    """Case 6 with attrs[0] as one [Va, C] leaf for its three items: the image of the per-item call with the
    table repeated bit for bit, the gradient [Va, C] against the CPU composition with the shared table and
    against the sum of the three per-item GPU gradients (k_attr_row_sum's item loop to B = 3)."""
    _, s, aa, C, pc, _ = CASES[6]
    proj, f, attrs, g = case_data(6)
    B = proj.shape[0]
    assert B == 3
    table = attrs[0].contiguous()
    img_rep, _, gv_rep, ga_rep = run_gpu(dev, proj, f, table[None].repeat(B, 1, 1), g, hyper(6), pc)
    img, node, gv, ga = run_gpu(dev, proj, f, table, g, hyper(6), pc)
    assert torch.equal(img, img_rep)
    assert ga.shape == table.shape
    img_r, fim_r, gv_r, ga_r = reference(oracle_mod, proj, f, table, g, s, aa, pc)
    assert torch.equal(node.face_index_map.cpu(), fim_r.int())
    close_images(img, img_r, "images")
    close_grad(ga, ga_r, "shared grad attributes vs reference")
    close_vertex_grad(gv, gv_r, "grad vertices vs reference")
    assert float(ga_rep[2].abs().max()) > 0  # the third item has something to add
    close_grad(ga, ga_rep.sum(0), "shared grad attributes vs the per-item sum")
    close_vertex_grad(gv, gv_rep, "grad vertices vs the per-item call")


def test_rows_past_the_vertices_take_zero_gradient(oracle_mod, dev):
    """Case 4 with a table of V + 7 rows and faces_attributes=None: the faces index the first V rows, the
    other seven are `e0 == e1` rows of the CSR.  grad_attributes comes from torch.empty, so k_attr_row_sum alone
    makes them 0: the call runs twice into fresh tensors, the first one's result overwritten with ones before
    its memory is released, so that an allocation that happens to hold zeros does not hide an unwritten
    row."""
    _, s, aa, C, pc, _ = CASES[4]
    V = scene(CASES[4][0])[0].shape[1]
    proj, f, attrs, g = case_data(4, Va=V + 7)
    assert attrs.shape[1] == V + 7
    img_r, fim_r, gv_r, ga_r = reference(oracle_mod, proj, f, attrs, g, s, aa, pc)
    assert torch.all(ga_r[:, V:] == 0) and float(ga_r[:, :V].abs().max()) > 0
    for run in range(2):
        img, node, gv, ga = run_gpu(dev, proj, f, attrs, g, hyper(4), pc)
        assert torch.equal(node.face_index_map.cpu(), fim_r.int())
        assert ga.shape == attrs.shape
        assert torch.all(ga[:, V:] == 0), "run %d: a row that no face references" % run
        close_images(img, img_r, "images")
        close_grad(ga, ga_r, "grad attributes")
        close_vertex_grad(gv, gv_r, "grad vertices")
        ga.fill_(1.0)
        gv.fill_(1.0)
        torch.cuda.synchronize()
        del img, node, gv, ga


def test_unreferenced_first_row_takes_zero_gradient(oracle_mod, dev):
    """Case 4 with a per-item table of V + 1 rows and faces_attributes = faces + 1 given explicitly: row 0 is
    referenced by no face (an empty CSR row in front of the others) and its gradient is exactly 0."""
    _, s, aa, C, pc, _ = CASES[4]
    V = scene(CASES[4][0])[0].shape[1]
    proj, f, attrs, g = case_data(4, Va=V + 1)
    fa = f + 1
    assert int(fa.min()) == 1 and int(fa.max()) == V
    img_r, fim_r, gv_r, ga_r = reference(oracle_mod, proj, f, attrs, g, s, aa, pc, fa=fa)
    assert torch.all(ga_r[:, 0] == 0)
    for run in range(2):
        img, node, gv, ga = run_gpu(dev, proj, f, attrs, g, hyper(4), pc, fa=fa)
        assert torch.equal(node.face_index_map.cpu(), fim_r.int())
        assert torch.all(ga[:, 0] == 0), "run %d: row 0, which no face references" % run
        close_images(img, img_r, "images")
        close_grad(ga, ga_r, "grad attributes")
        close_vertex_grad(gv, gv_r, "grad vertices")
        ga.fill_(1.0)
        torch.cuda.synchronize()
        del img, node, gv, ga


def test_item_with_zero_upstream_gradient(oracle_mod, dev):
    """Case 4 with g[1] = 0: every sum of item 1 fails k_attr_bwd's `mine != 0.f` and its records stay at
    their zero fill, so its gradients are exactly 0; nothing is NaN and item 0 matches the reference."""
    _, s, aa, C, pc, _ = CASES[4]
    proj, f, attrs, g = case_data(4)
    g = g.clone()
    g[1] = 0
    img_r, _, gv_r, ga_r = reference(oracle_mod, proj, f, attrs, g, s, aa, pc)
    assert torch.all(gv_r[1] == 0) and torch.all(ga_r[1] == 0)
    img, _, gv, ga = run_gpu(dev, proj, f, attrs, g, hyper(4), pc)
    assert torch.all(gv[1] == 0) and torch.all(ga[1] == 0)
    assert not torch.isnan(img).any() and not torch.isnan(gv).any() and not torch.isnan(ga).any()
    close_images(img, img_r, "images")
    close_vertex_grad(gv[0], gv_r[0], "item 0 grad vertices")
    close_grad(ga[0], ga_r[0], "item 0 grad attributes")


def test_strided_upstream_gradient(oracle_mod, dev):
    """Case 4's upstream gradient handed to backward as a permuted view with the same values: the gradients
    of the contiguous run within the tolerance (float atomics keep them from being bit-equal), and the
    reference's."""
    pc = CASES[4][4]
    proj, f, attrs, g = case_data(4)
    _, _, gv_r, ga_r = case_reference(oracle_mod, 4)
    img_c, _, gv_c, ga_c = run_gpu(dev, proj, f, attrs, g, hyper(4), pc)
    view = g.to(dev).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not view.is_contiguous() and torch.equal(view.cpu(), g)
    img, _, gv, ga = run_gpu(dev, proj, f, attrs, view, hyper(4), pc)
    assert torch.equal(img, img_c)
    close_vertex_grad(gv, gv_c, "grad vertices vs the contiguous run")
    close_grad(ga, ga_c, "grad attributes vs the contiguous run")
    close_vertex_grad(gv, gv_r, "grad vertices")
    close_grad(ga, ga_r, "grad attributes")

"""The interleaved forward's table order (bins nearest the raster centre first, nr_tile_order) against
the CPU oracle: a permutation of which block takes which bin must leave every result as it was.

Small cases at B = 8 (one interleave group, G = 8) on ico-spheres of 80 or 320 faces, every item
compared: face-index map bit-exact, images by close_images, gradients within the atomic-order
tolerance (the helpers of test_gpu_bwd_variants.py and test_gpu_bwd_warmup.py):

  * 32^2 anti-aliased (S = 64): 2 x 2 forward bins, 2 x 4 backward tiles, the smallest table;
  * 40^2 anti-aliased (S = 80): 3 x 3 bins and 3 x 5 tiles, both counts odd, the last column and row
    ragged;
  * 64^2 without anti-aliasing: the unfused forward and the run-time-channel instantiations;
  * 384^2 anti-aliased (S = 768): 24 x 24 = 576 bins by the table, and 24 x 48 = 1152 backward tiles
    (9216 blocks: two pixels per lane), more than a table holds;
  * the mesh shrunk into one corner of the 40^2 scene: foreground only at the highest ranks.

And the smallest 2-pixel backward grid, Scene("rgbsd", True, 256, 16): 16 x 16 bins by the table in
groups of 16 items, 16 x 32 = 512 backward tiles per item; the launch record is unchanged, and a
poisoned workspace (halo cache NaN, face-index map pre-filled with face 7, sparse forward) gives what a
zero-filled one gives.  The oracle runs once per scene.
"""
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import synthetic
from test_gpu_parity import close_images
from test_gpu_bwd_variants import DRAW, STATIC, TWO_PX, Scene, _grads, _shared_pairs, gpu_scene, oracle_scene
from test_gpu_bwd_warmup import _sparse_run, compare, vacuous_guard

pytestmark = pytest.mark.gpu


class SmallScene(Scene):
    """Scene without its 8192-tile grid: an ico-sphere of the given level at any size and batch, shrunk
    and moved on the screen by (scale, shift)."""

    def __init__(self, draw, aa, image_size, B, level, scale=1.0, shift=0.0, seed=0):
        self.draw, self.aa, self.image_size, self.B = draw, aa, image_size, B
        self.rgb, self.sil, self.depth = DRAW[draw]
        self.S = image_size * (2 if aa else 1)
        v, f = synthetic.icosphere(level)
        self.f = f
        proj = synthetic.project(torch.as_tensor(synthetic.jittered(v, B)), torch.as_tensor(synthetic.viewpoints(B))).clone()
        proj[..., :2] = proj[..., :2] * scale + shift
        self.proj = proj.contiguous()
        gen = torch.Generator().manual_seed(2000 + seed)
        C = 3 * self.rgb + self.sil + self.depth
        self.g = torch.randn((B, C, image_size, image_size), generator=gen)
        self.per_item_tex = False
        self.bgs = self.lights = None
        vt, ft, tex = nr.create_textures(f.shape[0], texture_size=4)
        self.vt, self.ft = torch.as_tensor(vt), ft
        self.tex = torch.rand(tex.shape, generator=gen)


def some_foreground(sc, ref):
    """vacuous_guard, with any foreground at all (an object in a corner covers little)."""
    assert int((ref["fim"] >= 0).sum()) > 0
    for i in range(sc.B):
        assert int((ref["fim"][i] >= 0).sum()) > 0, "item %d: no foreground" % i
        assert float(ref["gv"][i].abs().max()) > 0, "item %d: zero reference vertex gradient" % i
    for what, _, r in _shared_pairs(sc, ref, ref, ""):
        assert float(r.abs().max()) > 0, what


# (draw, anti-aliasing, image size, ico-sphere level, scale, shift, backward launch record)
CASES = {
    "aa32": ("rgbsd", True, 32, 2, 1.0, 0.0, (512, 0)),
    "aa40_odd_ragged": ("rgbsd", True, 40, 2, 1.0, 0.0, (512, 0)),
    "noaa64": ("rgbsd", False, 64, 2, 1.0, 0.0, (512, 0)),
    "aa384_bwd_above_cap": ("rgbsd", True, 384, 1, 1.0, 0.0, (256, TWO_PX)),
    "aa40_corner": ("rgbsd", True, 40, 2, 0.2, 0.78, (512, 0)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_tile_order_small_vs_oracle(oracle_mod, dev, name):
    draw, aa, size, level, scale, shift, launch = CASES[name]
    sc = SmallScene(draw, aa, size, 8, level, scale, shift, seed=len(name))
    ref = oracle_scene(oracle_mod, sc)
    if name == "aa40_corner":
        some_foreground(sc, ref)
        # the object lies inside one corner bin of the 3 x 3 (the last ranks): no foreground in the pixel
        # rows or columns 16 .. 63 of any item (whichever way the image is flipped)
        fg = ref["fim"] >= 0
        assert int(fg[:, 16:64, :].sum()) == 0 and int(fg[:, :, 16:64].sum()) == 0
    else:
        vacuous_guard(sc, ref)
    got = gpu_scene(dev, sc)
    assert got["launch"] == launch, got["launch"]
    compare(sc, got, ref)


@pytest.fixture(scope="module")
def grid_end(oracle_mod, dev):
    sc = Scene("rgbsd", True, 256, 16, seed=12)
    ref = oracle_scene(oracle_mod, sc)
    vacuous_guard(sc, ref)
    return sc, ref


def test_tile_order_two_px_grid_vs_oracle(grid_end, dev):
    sc, ref = grid_end
    got = gpu_scene(dev, sc)
    assert got["launch"] == (256, TWO_PX | STATIC), got["launch"]
    compare(sc, got, ref)


def test_tile_order_poisoned_workspace(grid_end, dev):
    sc, ref = grid_end
    bad = _sparse_run(dev, sc, float("nan"), 7)
    zero = _sparse_run(dev, sc, 0.0, 0)
    for r in (bad, zero):
        assert r["launch"][0] == 256 and r["launch"][1] & (TWO_PX | STATIC) == TWO_PX | STATIC, r["launch"]
        for k in ("img", "gv", "gt"):
            assert bool(torch.isfinite(r[k]).all()), k
    assert torch.equal(bad["img"], zero["img"])
    _grads(bad["gv"], zero["gv"], "poisoned vs zero-filled: grad vertices")
    _grads(bad["gt"], zero["gt"], "poisoned vs zero-filled: grad textures")
    for i in range(sc.B):
        close_images(bad["img"][i:i + 1], ref["img"][i:i + 1], "poisoned: item %d images" % i)
    _grads(bad["gv"], ref["gv"], "poisoned vs oracle: grad vertices")
    _grads(bad["gt"], ref["gt"], "poisoned vs oracle: grad textures")

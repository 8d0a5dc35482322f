"""The cases an L2 warm-up of k_raster_bwd's 2-pixel-per-lane variant has to survive: a foreground
block touching, with loads it discards, the face-id and upstream-gradient rows of the tile a later
block (linear id L + D) will take.  The warm-up was measured and not kept (DESIGN.md section 4
"Round 7"; it lives on as tools/ablations/bwd_l2_warmup.patch, which passes these cases); the cases
stay, for the shipped kernel and for the next attempt at its first loads.  Every case renders the
1280-face ico-sphere at the smallest 2-pixel grid (exactly 8192 tiles of 32x16 pixels), asserts
NR_LAUNCH_TWO_PX_PER_LANE from the launch record and compares ALL items with the CPU oracle, with the
tolerances of test_gpu_parity.py (helpers of test_gpu_bwd_variants.py):

  * grid end: 256^2 anti-aliased (S = 512), B = 16, rgb + silhouettes + depth.  With D near 1024 the
    last D blocks have no look-ahead tile, and the blocks before them look D / 16 tiles further on in
    the centre-out order of the same 16 items (B = 16 is one interleave group);
  * a raster that is no multiple of 32 or 16 with B no multiple of 8: 505^2 anti-aliased (S = 1010:
    18 live columns in the last tile column, 2 live rows in the last tile row), B = 4, i.e. 32 x 64
    tiles per item dealt by xcd_tile's bands (no item interleave): clamped rows and columns, and an
    item dealing that does not follow the XCDs;
  * the grid-end case with the halo cache off (the backward re-shades its halos and gets no bin
    flags): images bit-equal to the cached run, gradients within tolerance of it;
  * the grid-end case from a poisoned workspace: halo cache NaN, face-index map pre-filled, with the
    sparse forward (empty bins leave their face-index rows unwritten, and a look-ahead would read
    such rows): nothing of the fill reaches an output, and the gradients equal those from a
    zero-filled workspace within the atomic-order tolerance.  No other test runs the sparse forward
    at a 2-pixel grid.

The oracle reference and the cached GPU run of the grid-end scene are computed once per module.
"""
import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import rasterize as nrr
from neural_renderer_v2_pytorch_amd import _lib
from test_gpu_parity import close_images
from test_gpu_bwd_variants import STATIC, TWO_PX, Scene, _grads, _leaf, _shared_pairs, gpu_scene, oracle_scene

pytestmark = pytest.mark.gpu


def compare(sc, got, ref, tag=""):
    """Every item of `got` against `ref`: face-index map bit-exact, images, per-item vertex gradients,
    the shared texture and vertices_textures gradients."""
    worst = [0.0, ""]
    try:
        for i in range(sc.B):
            nbad = int((got["fim"][i] != ref["fim"][i]).sum())
            assert nbad == 0, "%sitem %d fim: %d px" % (tag, i, nbad)
            close_images(got["img"][i:i + 1], ref["img"][i:i + 1], "%sitem %d images" % (tag, i))
            _grads(got["gv"][i:i + 1], ref["gv"][i:i + 1], "%sitem %d grad vertices" % (tag, i), worst)
    finally:
        print("%sper-item gradients: largest max |d| / tolerance %.3f (%s)" % (tag, *worst))
    for what, a, r in _shared_pairs(sc, got, ref, tag):
        _grads(a, r, what)


def vacuous_guard(sc, ref):
    assert int((ref["fim"] >= 0).sum()) > 0.2 * ref["fim"].size
    for i in range(sc.B):
        assert float(ref["gv"][i].abs().max()) > 0, "item %d: zero reference vertex gradient" % i
    for what, _, r in _shared_pairs(sc, ref, ref, ""):
        assert float(r.abs().max()) > 0, what


@pytest.fixture(scope="module")
def grid_end(oracle_mod, dev):
    """The grid-end scene, its oracle reference and its GPU run (halo cache on), each computed once."""
    sc = Scene("rgbsd", True, 256, 16, seed=10)
    ref = oracle_scene(oracle_mod, sc)
    vacuous_guard(sc, ref)
    got = gpu_scene(dev, sc)
    return sc, ref, got


def test_warmup_grid_end_vs_oracle(grid_end):
    """k_raster_bwd<0, 2, 5>: exactly 8192 blocks, the last D without a look-ahead tile."""
    sc, ref, got = grid_end
    assert got["launch"] == (256, TWO_PX | STATIC), got["launch"]
    compare(sc, got, ref)


def test_warmup_ragged_raster_odd_batch_vs_oracle(oracle_mod, dev):
    """k_raster_bwd<0, 2, 0>: S = 1010 (no multiple of 32 or 16), B = 4 (no item interleave)."""
    sc = Scene("rgbsd", True, 505, 4, seed=11)
    ref = oracle_scene(oracle_mod, sc)
    vacuous_guard(sc, ref)
    got = gpu_scene(dev, sc)
    assert got["launch"] == (256, TWO_PX), got["launch"]
    compare(sc, got, ref)


def test_warmup_halo_cache_off(grid_end, dev):
    """The grid-end scene with the backward re-shading its halos (NrRasterArgs.halo NULL)."""
    sc, ref, got = grid_end
    nrr._HALO_CACHE = False
    try:
        again = gpu_scene(dev, sc)
    finally:
        nrr._HALO_CACHE = True
    assert again["launch"] == (256, TWO_PX | STATIC), again["launch"]
    assert torch.equal(again["img"], got["img"]) and np.array_equal(again["fim"], got["fim"])
    compare(sc, again, ref, "halo cache off vs oracle: ")
    _grads(again["gv"], got["gv"], "halo cache off: grad vertices")
    for what, a, r in _shared_pairs(sc, again, got, "halo cache off: "):
        _grads(a, r, what)


def _sparse_run(dev, sc, halo_fill, fim_fill):
    """Forward + backward with the sparse face-index map (no map returned, no vertices_textures
    gradient) from a workspace pre-filled with (halo_fill, fim_fill); results on the CPU."""
    pv, tex = _leaf(sc.proj, dev), _leaf(sc.tex, dev)
    params = nr.RasterizeParam(vertices_textures=sc.vt.to(dev)[None].expand(sc.B, -1, -1),
                               faces_textures=torch.as_tensor(sc.ft, device=dev),
                               textures=tex[None].expand(sc.B, -1, -1, -1))
    hp = nr.RasterizeHyperparam(image_size=sc.image_size, **sc.hyperparams())
    nrr._HALO_FILL, nrr._FIM_FILL = halo_fill, fim_fill
    try:
        img = nrr.rasterize_core(pv, torch.as_tensor(sc.f, device=dev), params, hp)
        img.backward(sc.g.to(dev))
        torch.cuda.synchronize()
    finally:
        nrr._HALO_FILL = nrr._FIM_FILL = None
    return dict(launch=_lib.last_launch("k_raster_bwd"), img=img.detach().cpu(), gv=pv.grad.cpu(), gt=tex.grad.cpu())


def test_warmup_poisoned_workspace(grid_end, dev):
    """Halo cache NaN and face-index map pre-filled with face 7 (a valid id, as test_gpu_parity's
    _FIM_FILL cases: an entry read by mistake shows in the gradients) against a zero-filled workspace
    (halo 0, face 0), and both against the oracle."""
    sc, ref, _ = grid_end
    bad = _sparse_run(dev, sc, float("nan"), 7)
    zero = _sparse_run(dev, sc, 0.0, 0)
    for r in (bad, zero):
        # (without a vertices_textures gradient the shared-window instantiation may be the one launched)
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

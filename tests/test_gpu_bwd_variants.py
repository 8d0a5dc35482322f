"""k_raster_bwd's 2-pixel-per-lane instantiations beyond the plain textured headline / car renders,
and k_param_bwd and the unfused forward on a large grid, against the CPU oracle.

The backward takes two pixels per lane (256 threads, rows ly0 and ly0 + 4 of a wave's 16x8 region)
once its grid has 8192 blocks of 32x16 pixels (launch_bwd_v, nr_bwd.h).  The rest of the suite renders
lights, backgrounds, parameter gradients, per-item textures and odd sizes at B <= 4 and sizes <= 70,
i.e. with one pixel per lane.  Every case here renders an ico-sphere (1280 faces) at the smallest
batch whose backward grid ceil(S / 32) ceil(S / 16) B is exactly 8192, asserts from the library's
launch record (nr_last_launch) which instantiation ran, and compares ALL items with the oracle:

  * face-index map bit-exact; images; per-item vertex gradients;
  * texture gradients (the batch sum for a shared atlas, per item for per-item textures);
  * vertices_textures gradients through an expanded [1, Vt, 2] leaf (k_param_bwd<UV>);
  * lit renders: light colour, direction and specular-exponent gradients, per item (k_param_bwd<LGT>
    and the [L][B][8] light records); renders with backgrounds: the background gradients;
  * lit / background renders a second time with the halo cache off (the backward re-shades its tile
    halos): bit-equal images, gradients within the tolerance of the cached run's.

Tolerances as in test_gpu_parity.py: face-index map bit-exact; images |d| <= 1e-5 + 1e-5 |ref|;
gradients |d| <= 1e-4 max|ref| + 1e-4 |ref|.  The oracle runs 8 items per call with one leaf per
shared tensor, as test_gpu_parity.oracle_batch does.
"""
import numpy as np
import pytest
import torch

import neural_renderer_v2_pytorch_amd as nr
from neural_renderer_v2_pytorch_amd import rasterize as nrr
from neural_renderer_v2_pytorch_amd import synthetic
from neural_renderer_v2_pytorch_amd import _lib
from test_gpu_parity import GRAD_TOL, close_grads, close_images, oracle_batch  # noqa: F401  (oracle_batch: the sibling below follows it)

pytestmark = pytest.mark.gpu

TWO_PX = _lib.NR_LAUNCH_TWO_PX_PER_LANE
STATIC = _lib.NR_LAUNCH_STATIC_CHANNELS
LIGHTS = _lib.NR_LAUNCH_LIGHTS
BACKGROUNDS = _lib.NR_LAUNCH_BACKGROUNDS
SIL_ONLY = _lib.NR_LAUNCH_SIL_ONLY

DRAW = {"rgbsd": (True, True, True), "rgb": (True, False, False), "rgba": (True, True, False),
        "sil": (False, True, False), "depth": (False, False, True)}


class Scene:
    """One case's inputs, all on the CPU, drawn from seeded CPU generators."""

    def __init__(self, draw, aa, image_size, B, lights=False, backgrounds=False, per_item_tex=False, texture_size=4,
                 seed=0):
        self.draw, self.aa, self.image_size, self.B = draw, aa, image_size, B
        self.rgb, self.sil, self.depth = DRAW[draw]
        self.S = image_size * (2 if aa else 1)
        # the smallest 2-pixel grid: launch_bwd_v's threshold, in 32x16 tiles
        assert ((self.S + 31) // 32) * ((self.S + 15) // 16) * B == 8192
        v, f = synthetic.icosphere(3)
        assert f.shape[0] == 1280
        self.f = f
        self.proj = synthetic.project(torch.as_tensor(synthetic.jittered(v, B)),
                                      torch.as_tensor(synthetic.viewpoints(B))).contiguous()
        gen = torch.Generator().manual_seed(1000 + seed)
        C = 3 * self.rgb + self.sil + self.depth
        self.g = torch.randn((B, C, image_size, image_size), generator=gen)
        self.per_item_tex = per_item_tex
        self.tex = self.vt = self.ft = self.bgs = self.lights = None
        if self.rgb:
            vt, ft, tex = nr.create_textures(f.shape[0], texture_size=texture_size)
            self.vt, self.ft = torch.as_tensor(vt), ft
            self.tex = torch.rand(((B,) if per_item_tex else ()) + tex.shape, generator=gen)
        if backgrounds:
            self.bgs = torch.rand((B, 3, self.S, self.S), generator=gen)
        if lights:
            # ambient, directional (backside), specular: colours, directions and exponents differ per item
            d = torch.tensor([0.3, -0.5, 0.81]) + 0.4 * torch.randn((B, 3), generator=gen)
            self.lights = dict(amb_color=0.2 + 0.3 * torch.rand((B, 3), generator=gen),
                               dir_color=0.3 + 0.5 * torch.rand((B, 3), generator=gen),
                               dir_direction=d / d.norm(dim=1, keepdim=True),
                               spec_color=0.2 + 0.4 * torch.rand((B, 3), generator=gen),
                               spec_alpha=1.5 + 2.0 * torch.rand((B,), generator=gen))

    def hyperparams(self):
        return dict(anti_aliasing=self.aa, draw_rgb=self.rgb, draw_silhouettes=self.sil, draw_depth=self.depth)


LIGHT_KEYS = ("amb_color", "dir_color", "dir_direction", "spec_color", "spec_alpha")


def _light_objects(t):
    return [nr.AmbientLight(t["amb_color"]),
            nr.DirectionalLight(t["dir_color"], t["dir_direction"], backside=True),
            nr.SpecularLight(t["spec_color"], alpha=t["spec_alpha"])]


def _leaf(t, dev=None):
    if t is None:
        return None
    return (t.clone() if dev is None else t.to(dev)).requires_grad_(True)


def oracle_scene(oracle_mod, sc, chunk=8):
    """The CPU oracle over every item of the scene, `chunk` items per call, with one leaf per tensor
    (oracle_batch with lights, backgrounds, per-item textures and a vertices_textures leaf): a shared
    texture and the [1, Vt, 2] table are expanded over each chunk, so their gradients accumulate over
    the batch; per-item tensors are sliced, so each item's gradient lands in its own rows."""
    B = sc.B
    tex, vt, bgs = _leaf(sc.tex), _leaf(sc.vt[None] if sc.vt is not None else None), _leaf(sc.bgs)
    lt = {k: _leaf(v) for k, v in sc.lights.items()} if sc.lights else None
    imgs, fims, gvs = [], [], []
    for c in range(0, B, chunk):
        idx = list(range(c, min(c + chunk, B)))
        n = len(idx)
        pc = sc.proj[idx].clone().requires_grad_(True)
        extra = {}
        if sc.rgb:
            extra = dict(vertices_textures=vt.expand(n, -1, -1), faces_textures=sc.ft,
                         textures=tex[idx] if sc.per_item_tex else tex[None].expand(n, -1, -1, -1))
            if lt:
                extra["lights"] = _light_objects({k: v[idx] for k, v in lt.items()})
            if bgs is not None:
                extra["backgrounds"] = bgs[idx]
        ref, internals = oracle_mod.rasterize_core(pc, sc.f, image_size=sc.image_size, return_internals=True,
                                                   **sc.hyperparams(), **extra)
        ref.backward(sc.g[idx])
        imgs.append(ref.detach())
        fims.append(internals["fim"].numpy())
        gvs.append(pc.grad)
    out = dict(img=torch.cat(imgs), fim=np.concatenate(fims), gv=torch.cat(gvs))
    if sc.rgb:
        out["gt"], out["gvt"] = tex.grad, vt.grad
    if bgs is not None:
        out["gbg"] = bgs.grad
    if lt:
        out.update({"g_" + k: v.grad for k, v in lt.items()})
    return out


def gpu_scene(dev, sc):
    """The scene in one batched forward + backward through the HIP path; the results on the CPU, with
    the backward's launch record."""
    pv = _leaf(sc.proj, dev)
    params = nr.RasterizeParam()
    tex = vt = bgs = lt = None
    if sc.rgb:
        tex, vt, bgs = _leaf(sc.tex, dev), _leaf(sc.vt[None], dev), _leaf(sc.bgs, dev)
        lt = {k: _leaf(v, dev) for k, v in sc.lights.items()} if sc.lights else None
        params = nr.RasterizeParam(vertices_textures=vt.expand(sc.B, -1, -1), faces_textures=torch.as_tensor(sc.ft, device=dev),
                                   textures=tex if sc.per_item_tex else tex[None].expand(sc.B, -1, -1, -1),
                                   backgrounds=bgs, lights=_light_objects(lt) if lt else None)
    hp = nr.RasterizeHyperparam(image_size=sc.image_size, **sc.hyperparams())
    img, fim = nrr.rasterize_core(pv, torch.as_tensor(sc.f, device=dev), params, hp, return_face_index=True)
    img.backward(sc.g.to(dev))
    torch.cuda.synchronize()
    out = dict(launch=_lib.last_launch("k_raster_bwd"), img=img.detach().cpu(), fim=fim.cpu().numpy(), gv=pv.grad.cpu())
    if sc.rgb:
        out["gt"], out["gvt"] = tex.grad.cpu(), vt.grad.cpu()
    if bgs is not None:
        out["gbg"] = bgs.grad.cpu()
    if lt:
        out.update({"g_" + k: v.grad.cpu() for k, v in lt.items()})
    return out


def _light_grad_pairs(got, ref):
    """(what, got, ref) as test_param_grads_golden compares them: the colours stacked over the lights,
    each directional light's direction, the specular exponents stacked."""
    return [("grad light colours", torch.stack([got["g_amb_color"], got["g_dir_color"], got["g_spec_color"]]),
             torch.stack([ref["g_amb_color"], ref["g_dir_color"], ref["g_spec_color"]])),
            ("grad light direction 1", got["g_dir_direction"], ref["g_dir_direction"]),
            ("grad specular alpha", torch.stack([got["g_spec_alpha"]]), torch.stack([ref["g_spec_alpha"]]))]


def _shared_pairs(sc, got, ref, tag):
    """The gradients that are one tensor for the batch (or are compared whole): (what, got, ref)."""
    pairs = []
    if sc.rgb:
        if not sc.per_item_tex:
            pairs.append((tag + "grad textures (batch sum)", got["gt"], ref["gt"]))
        pairs.append((tag + "grad vertices_textures", got["gvt"], ref["gvt"]))
    if sc.lights:
        pairs += [(tag + w, a, b) for w, a, b in _light_grad_pairs(got, ref)]
    return pairs


def _grads(a, b, what, worst=None):
    """close_grads, after noting the comparison's largest error as a share of its tolerance."""
    a64, b64 = a.detach().cpu().double(), b.detach().cpu().double()
    tol = GRAD_TOL * float(b64.abs().max()) + GRAD_TOL * b64.abs()
    share = float(((a64 - b64).abs() / tol).max())
    if worst is None:
        print("%s: max |d| / tolerance %.3f" % (what, share))
    elif share > worst[0]:
        worst[:] = [share, what]
    close_grads(a, b, what)


def check_scene(oracle_mod, dev, sc, bits, halo_rerun=False):
    ref = oracle_scene(oracle_mod, sc)
    B = sc.B
    # guards against a vacuous pass, on the oracle's results only
    assert int((ref["fim"] >= 0).sum()) > 0.2 * ref["fim"].size
    for i in range(B):
        assert float(ref["gv"][i].abs().max()) > 0, "item %d: zero reference vertex gradient" % i
        if sc.per_item_tex:
            assert float(ref["gt"][i].abs().max()) > 0, "item %d: zero reference texture gradient" % i
        if sc.bgs is not None:
            assert float(ref["gbg"][i].abs().max()) > 0, "item %d: zero reference background gradient" % i
    for what, _, r in _shared_pairs(sc, ref, ref, ""):
        assert float(r.abs().max()) > 0, what
    if sc.lights:
        for k in ("amb_color", "dir_color", "spec_color", "dir_direction"):
            assert bool((ref["g_" + k] != 0).any(1).all()), "an item's %s gradient is all zero" % k
        assert bool((ref["g_spec_alpha"] != 0).all()), "an item's specular alpha gradient is zero"

    got = gpu_scene(dev, sc)
    assert got["launch"] == (256, TWO_PX | bits), got["launch"]
    worst = [0.0, ""]
    try:
        for i in range(B):
            nbad = int((got["fim"][i] != ref["fim"][i]).sum())
            assert nbad == 0, "item %d fim: %d px" % (i, nbad)
            close_images(got["img"][i:i + 1], ref["img"][i:i + 1], "item %d images" % i)
            _grads(got["gv"][i:i + 1], ref["gv"][i:i + 1], "item %d grad vertices" % i, worst)
            if sc.per_item_tex:
                _grads(got["gt"][i], ref["gt"][i], "item %d grad textures" % i, worst)
    finally:
        print("per-item gradients: largest max |d| / tolerance %.3f (%s)" % tuple(worst))
    if sc.bgs is not None:
        _grads(got["gbg"], ref["gbg"], "grad backgrounds")
    for what, a, r in _shared_pairs(sc, got, ref, ""):
        _grads(a, r, what)

    if halo_rerun:
        # the same render with the backward re-shading its tile halos (NrRasterArgs.halo NULL)
        nrr._HALO_CACHE = False
        try:
            again = gpu_scene(dev, sc)
        finally:
            nrr._HALO_CACHE = True
        assert again["launch"] == (256, TWO_PX | bits), again["launch"]
        assert torch.equal(again["img"], got["img"]) and np.array_equal(again["fim"], got["fim"])
        _grads(again["gv"], got["gv"], "halo cache off: grad vertices")
        if sc.per_item_tex:
            _grads(again["gt"], got["gt"], "halo cache off: grad textures")
        if sc.bgs is not None:
            _grads(again["gbg"], got["gbg"], "halo cache off: grad backgrounds")
        for what, a, r in _shared_pairs(sc, again, got, "halo cache off: "):
            _grads(a, r, what)


def test_bwd2_lights_vs_oracle(oracle_mod, dev):
    """k_raster_bwd<1, 2, 0> (lights, 2 pixels per lane, its 3-waves-per-SIMD budget and 24-float
    records with two records per lane in the gather): rgb + silhouettes + depth, 256^2 anti-aliased
    (S = 512), B = 16, an ambient, a directional (backside) and a specular light whose colours,
    directions and exponents differ per item and all require a gradient (the [L][B][8] record stride,
    k_param_bwd<true, true>), through the unfused forward (k_raster_fwd + k_shade).  Every item against
    the oracle, and the halo-cache-off backward against the cached one."""
    sc = Scene("rgbsd", True, 256, 16, lights=True, seed=1)
    check_scene(oracle_mod, dev, sc, LIGHTS, halo_rerun=True)


def test_bwd2_backgrounds_per_item_textures_vs_oracle(oracle_mod, dev):
    """k_raster_bwd<2, 2, 0> (backgrounds, 2 pixels per lane; it never skips a background tile):
    rgb + silhouettes + depth, 256^2 anti-aliased (S = 512), B = 16, backgrounds [B, 3, S, S] with a
    gradient, per-item textures (bt = b) of 8x8 texels per face (direct texel samples outside the 4x4
    face window).  Every item against the oracle, and the halo-cache-off backward against the cached one."""
    sc = Scene("rgbsd", True, 256, 16, backgrounds=True, per_item_tex=True, texture_size=8, seed=2)
    check_scene(oracle_mod, dev, sc, BACKGROUNDS, halo_rerun=True)


def test_bwd2_lights_backgrounds_ragged_vs_oracle(oracle_mod, dev):
    """k_raster_bwd<3, 2, 0> (lights + backgrounds) without anti-aliasing on a 250^2 raster, B = 64:
    the last tile row has 10 live rows, so lanes of wave 1 hold the pixel pairs (8, 12) and (9, 13)
    with one pixel inside the image and one outside; the last tile column has 26 live pixels;
    step = 2 / 250 takes div_step's true division.  Every item against the oracle, and the
    halo-cache-off backward against the cached one."""
    sc = Scene("rgbsd", False, 250, 64, lights=True, backgrounds=True, seed=3)
    check_scene(oracle_mod, dev, sc, LIGHTS | BACKGROUNDS, halo_rerun=True)


def test_bwd2_rgb_only_vs_oracle(oracle_mod, dev):
    """k_raster_bwd<0, 2, 0> with C = 3 (rgb only: no compile-time-channel instantiation), 256^2
    anti-aliased, B = 16."""
    check_scene(oracle_mod, dev, Scene("rgb", True, 256, 16, seed=4), 0)


def test_bwd2_non_pow2_antialiased_vs_oracle(oracle_mod, dev):
    """k_raster_bwd<0, 2, 0> with all five channels but a 500^2 raster (250^2 anti-aliased): the
    static instantiation needs a power-of-two raster, so the runtime-channel kernel runs with
    div_step's true division and partial edge tiles (20 live pixels in the last tile column, 4 live
    rows in the last tile row), B = 16."""
    check_scene(oracle_mod, dev, Scene("rgbsd", True, 250, 16, seed=5), 0)


def test_bwd2_rgba_no_antialiasing_vs_oracle(oracle_mod, dev):
    """k_raster_bwd<0, 2, 0> without anti-aliasing (rgb + silhouettes, 256^2, B = 64): the static
    4-channel instantiation needs anti-aliasing; the forward does not fuse its shading."""
    check_scene(oracle_mod, dev, Scene("rgba", False, 256, 64, seed=6), 0)


def test_bwd2_silhouettes_odd_raster_vs_oracle(oracle_mod, dev):
    """k_raster_bwd<4, 2, 0> (silhouettes only: weights after the stencil, sparse gather) without
    anti-aliasing on an odd 251^2 raster, B = 64."""
    check_scene(oracle_mod, dev, Scene("sil", False, 251, 64, seed=7), SIL_ONLY)


def test_bwd2_depth_only_vs_oracle(oracle_mod, dev):
    """k_raster_bwd<0, 2, 0> with C = 1 (depth only), 250^2 anti-aliased (S = 500), B = 16."""
    check_scene(oracle_mod, dev, Scene("depth", True, 250, 16, seed=8), 0)


def test_bwd2_per_item_textures_static_channels_vs_oracle(oracle_mod, dev):
    """k_raster_bwd<0, 2, 5> (compile-time channels, no shared-window flush) with per-item textures
    (bt = b) of 8x8 texels per face: direct texel samples (step 5's four-samples-per-atomic flush with
    two records per lane) without the HOT instantiation; 256^2 anti-aliased, B = 16."""
    sc = Scene("rgbsd", True, 256, 16, per_item_tex=True, texture_size=8, seed=9)
    check_scene(oracle_mod, dev, sc, STATIC)

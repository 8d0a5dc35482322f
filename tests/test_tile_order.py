"""nr_tile_order: the order in which an interleaved raster launch hands out an item's tiles (nearest the
raster centre first), checked on the host without a GPU.

  * the table is a permutation of the raster's tiles, the squared pixel distance of the tile centres
    from the raster centre never decreases along the ranks, and the order is symmetric: the ranks of a
    tile's four mirror images lie within their tie group (the tiles of the same distance);
  * a raster of more than 1024 tiles is an error (such a launch keeps the arithmetic order);
  * the property the order exists for, on the headline's geometry (ico-sphere level 4, 256^2
    anti-aliased: 16 x 16 bins of 32 x 32 pixels) and the bench's first 16 items: by distance the last
    bin with a candidate face has rank <= 112 for every item, where the arithmetic order (rows from
    the middle row outwards, each row from its middle outwards; computed here from its formula) gives
    >= 148.  A bin counts as non-empty when a face's conservative pixel bounding box (the setup's
    pix_range) overlaps it.
"""
import ctypes

import numpy as np
import pytest
import torch

from neural_renderer_v2_pytorch_amd import _lib
from neural_renderer_v2_pytorch_amd import synthetic

GEOMETRIES = [(16, 16, 32, 32), (16, 32, 32, 16), (3, 3, 32, 32), (3, 5, 32, 16), (1, 1, 32, 32), (1, 1, 32, 16),
              (32, 32, 32, 32)]


def tile_order(nx, ny, tw, th):
    out = (ctypes.c_uint16 * (nx * ny))()
    _lib.check(_lib.lib().nr_tile_order(nx, ny, tw, th, out), "nr_tile_order")
    e = np.frombuffer(out, dtype=np.uint16).astype(np.int64)
    return e & 0xff, e >> 8


def dist2(tx, ty, nx, ny, tw, th):
    return ((2 * tx + 1 - nx) * tw) ** 2 + ((2 * ty + 1 - ny) * th) ** 2


@pytest.mark.parametrize("nx,ny,tw,th", GEOMETRIES)
def test_permutation_by_distance(nx, ny, tw, th):
    tx, ty = tile_order(nx, ny, tw, th)
    assert tx.min() >= 0 and tx.max() < nx and ty.min() >= 0 and ty.max() < ny
    assert sorted((ty * nx + tx).tolist()) == list(range(nx * ny))
    d = dist2(tx, ty, nx, ny, tw, th)
    assert (np.diff(d) >= 0).all()
    # the stated key (d2, ty, tx), by an independent sort
    want = sorted((int(dist2(x, y, nx, ny, tw, th)), y, x) for y in range(ny) for x in range(nx))
    assert [(int(a), int(b), int(c)) for a, b, c in zip(d, ty, tx)] == want


@pytest.mark.parametrize("nx,ny,tw,th", GEOMETRIES)
def test_symmetric(nx, ny, tw, th):
    tx, ty = tile_order(nx, ny, tw, th)
    d = dist2(tx, ty, nx, ny, tw, th)
    rank = {(int(x), int(y)): t for t, (x, y) in enumerate(zip(tx, ty))}
    for (x, y), t in rank.items():
        lo, hi = np.searchsorted(d, d[t], "left"), np.searchsorted(d, d[t], "right")  # the tie group's ranks
        for m in ((x, y), (nx - 1 - x, y), (x, ny - 1 - y), (nx - 1 - x, ny - 1 - y)):
            assert lo <= rank[m] < hi, ((x, y), m)


@pytest.mark.parametrize("nx,ny", [(32, 33), (24, 48), (1025, 1), (1, 1025), (0, 4), (4, 0)])
def test_above_the_cap_is_an_error(nx, ny):
    out = (ctypes.c_uint16 * max(nx * ny, 1))()
    assert _lib.lib().nr_tile_order(nx, ny, 32, 16, out) == 1  # NR_ERR_ARGS
    assert b"nr_tile_order" in _lib.lib().nr_last_error()
    assert _lib.lib().nr_tile_order(32, 32, 32, 32, None) == 1


def centre_out(k, n):
    d = (k + 1) >> 1
    return (n >> 1) + (-d if k & 1 else d)


def test_headline_last_nonempty_bin_rank():
    S, NB = 512, 16
    v, f = synthetic.icosphere(4)
    tx, ty = tile_order(NB, NB, 32, 32)
    by_distance = list(zip(tx.tolist(), ty.tolist()))
    by_rows = [(centre_out(t % NB, NB), centre_out(t // NB, NB)) for t in range(NB * NB)]
    assert sorted(by_rows) == sorted(by_distance)

    def pix_range(lo, hi):
        a = np.clip((lo * S + S - 1) * 0.5, -2.0, S + 2.0)
        b = np.clip((hi * S + S - 1) * 0.5, -2.0, S + 2.0)
        return np.maximum(np.ceil(a).astype(int) - 1, 0), np.minimum(np.floor(b).astype(int) + 1, S - 1)

    for i in range(16):  # bench.workload's items
        vb = synthetic.jittered(v, 1, seed_base=1000 + i)
        eye = synthetic.viewpoints(1, seed_base=2000 + i)
        fv = synthetic.project(torch.as_tensor(vb), torch.as_tensor(eye))[0].numpy()[f].astype(np.float64)
        x0, x1 = pix_range(fv[:, :, 0].min(1), fv[:, :, 0].max(1))
        y0, y1 = pix_range(fv[:, :, 1].min(1), fv[:, :, 1].max(1))
        occ = np.zeros((NB, NB), bool)
        for k in np.nonzero((x0 <= x1) & (y0 <= y1))[0]:
            occ[y0[k] // 32:y1[k] // 32 + 1, x0[k] // 32:x1[k] // 32 + 1] = True
        assert 60 < occ.sum() < 130, occ.sum()
        last_distance = max(t for t, (x, y) in enumerate(by_distance) if occ[y, x])
        last_rows = max(t for t, (x, y) in enumerate(by_rows) if occ[y, x])
        print("item %d: %d non-empty bins, last at rank %d by distance, %d by rows" % (i, occ.sum(), last_distance, last_rows))
        assert last_distance <= 112, (i, last_distance)
        assert last_rows >= 148, (i, last_rows)

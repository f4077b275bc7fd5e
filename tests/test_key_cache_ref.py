"""The numpy restatement of the key cache's totals (tests/key_cache_ref.py) on
its own, on the meshes of the GPU test (tests/test_key_cache_gpu.py): a slot per
owned tile with a kept pair, an item per owned tile, and the two cases the
restatement has to get right -- a tile whose kept pairs win nothing inside it
(cached all the same) and a frame without any kept pair."""
import numpy as np
import pytest

import key_cache_ref as K
import scenes
import visible_plan_ref as P
import visible_ref as V

W, H = 640, 400
SMALL, BIG = (60, 200), (250, 700)
_MESH = {}


def _mesh(name):
    if name not in _MESH:
        _MESH[name] = scenes.sphere_mesh(W, H, *name)
    return _MESH[name]


@pytest.mark.parametrize("mesh,shard", [(SMALL, None), (SMALL, (2, 1)), (SMALL, (8, 3)), (BIG, None), (BIG, (8, 3))])
def test_totals_of_the_spheres(oracle, mesh, shard):
    xy, z, _ = _mesh(mesh)
    t, s = K.scene_totals(xy, z, (W, H), shard)
    owned = s["owned"]
    assert t["items"] == owned.sum() and t["bytes"] == t["tiles"] * K.TH * K.TW * 8
    assert 0 < t["tiles"] < t["items"]                      # the sphere leaves the frame's corners empty
    assert t["tiles"] == ((s["kept"] > 0) & owned).sum()
    # every tile with a winning pixel keeps a pair (the winner's), so it is cached
    wt = K.winner_tiles(xy, z, (W, H), shard)
    assert not (wt & ~(s["kept"] > 0)).any()
    assert t["tiles"] >= wt.sum()
    # never more than a third of the f64 framebuffer's bytes (3 doubles per pixel against one key)
    assert t["bytes"] <= owned.sum() * K.TH * K.TW * 8
    cls = K.item_order(s["kept"], owned)
    assert (cls > 0).sum() == t["tiles"] and cls.max() == K.KEY_NB


def test_a_tile_whose_kept_pairs_win_nothing_inside_it(oracle):
    """A sliver between two pixel columns right of a tile edge: the binning's
    rectangle (two columns of margin) reaches the tile to its left, where it
    covers nothing.  It wins a pixel elsewhere, so it is kept, and the left tile
    is cached with all ids zero."""
    size = (128, 32)
    xy = np.array([[64.6, 2.0, 70.4, 2.0, 67.0, 20.0]])
    z = np.full((1, 3), 0.5)
    assert list(V.winners(xy, z, size)) == [0]
    t, s = K.scene_totals(xy, z, size)
    assert list(s["kept"]) == [1, 1] and t == {"tiles": 2, "items": 2, "bytes": 2 * K.KEY_BYTES}
    assert list(K.winner_tiles(xy, z, size)) == [False, True]


def test_a_fully_empty_frame(oracle):
    """Triangles that cover no pixel centre: pairs, but no winner, so nothing
    is kept and nothing cached -- every owned tile is an empty item."""
    size = (128, 64)
    k = np.arange(3)[:, None] * np.array([7.0, 3.0])
    xy = (np.array([[90.2, 40.2], [90.4, 40.2], [90.3, 41.3]])[None] + k[:, None, :]).reshape(3, 6)
    z = np.full((3, 3), 0.5)
    assert len(V.winners(xy, z, size)) == 0 and P.tile_counts(xy, size).sum() == 3
    t, s = K.scene_totals(xy, z, size)
    assert t == {"tiles": 0, "items": 4, "bytes": 0}
    assert (K.item_order(s["kept"], s["owned"]) == 0).all()
    t2, _ = K.scene_totals(xy, z, size, shard=(2, 1))
    assert t2 == {"tiles": 0, "items": 2, "bytes": 0}


def test_random_counts():
    g = scenes.rng(5)
    for _ in range(50):
        n = int(g.integers(1, 400))
        kept = g.integers(0, 3000, n) * (g.uniform(size=n) < 0.6)
        owned = g.uniform(size=n) < 0.8
        t = K.totals(kept, owned)
        assert t["items"] == owned.sum() and t["tiles"] == ((kept > 0) & owned).sum() <= t["items"]
        cls = K.item_order(kept, owned)
        k = kept[owned]
        assert ((cls == 0) == (k == 0)).all() and (cls <= K.KEY_NB).all()
        o = np.argsort(k, kind="stable")
        assert (np.diff(cls[o]) >= 0).all()                 # a denser tile is never in a lower class

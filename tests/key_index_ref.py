"""A numpy restatement of the key index's totals (nr_free_vis.hip, k_key_index):
per cached tile the distinct winners of its in-frame pixels, of which the first
KI_RT -- ranked by their first pixel in the tile's p = ly * TW + lx order -- are
staged; a pixel whose winner is not staged is a direct pixel.

The winners come from the oracle (the id colours of tests/visible_ref.py), the
cached tiles from tests/key_cache_ref.py: every cached tile is indexed, also one
whose kept pairs win nothing inside it (its count is 0)."""
import numpy as np

import key_cache_ref as K
import scenes
import visible_plan_ref as P
import visible_ref as V

TW, TH = V.TW, V.TH
KI_RT = 280                                      # staged winners per tile (nr_free.h)
SLOT_BYTES = TH * TW * 2 + KI_RT * 4 + 8         # u16 per pixel, the staged winners' ids, {count, direct pixels}


def winner_ids(xy, z, size, depth=(True, True)):
    """H x W: the 1-based number of every pixel's winner on the oracle's frame, 0 without one."""
    n = len(xy)
    assert n < 2 ** 24
    col = np.zeros((n, 4))
    col[:, 0] = (np.arange(n) + 1) * 2.0 ** -24
    col[:, 3] = 1.0
    ctx = scenes.OracleFactory().context(size[0], size[1], False)
    ctx.set_color(0.0, 0.0, 0.0, 0.0)
    V.set_depth(ctx, depth)
    ctx.draw_triangles(xy, col, z=z, gouraud=False)
    return np.rint(ctx.get_buffer_numpy()[..., 0] * 2.0 ** 24).astype(np.int64)


def tile_index(ids, size, rt=KI_RT):
    """Per tile (row-major over the frame's tiles): the distinct winners of its
    in-frame pixels, and its direct pixels when the rt winners with the earliest
    first pixel are staged."""
    tx, ty = P.tiles_of(size)
    pad = np.zeros((ty * TH, tx * TW), dtype=np.int64)
    pad[:size[1], :size[0]] = ids
    tiles = pad.reshape(ty, TH, tx, TW).transpose(0, 2, 1, 3).reshape(tx * ty, TH * TW)
    distinct = np.zeros(tx * ty, dtype=np.int64)
    direct = np.zeros(tx * ty, dtype=np.int64)
    for t, px in enumerate(tiles):
        w, first, count = np.unique(px[px > 0], return_index=True, return_counts=True)
        distinct[t] = len(w)
        direct[t] = count[np.argsort(first, kind="stable")[rt:]].sum()
    return distinct, direct


def totals(ids, size, cached_tiles, shard=None, rt=KI_RT):
    """{"tiles", "staged", "direct", "bytes"} of the key index of a generation
    with `cached_tiles` cached tiles, over the winner image `ids`."""
    owned = P.owned_tiles(size, shard)
    distinct, direct = tile_index(ids, size, rt)
    return {"tiles": int(cached_tiles), "staged": int(np.minimum(distinct, rt)[owned].sum()),
            "direct": int(direct[owned].sum()), "bytes": int(cached_tiles) * SLOT_BYTES}


def scene_totals(xy, z, size, shard=None, depth=(True, True)):
    """The key index's totals of one scene, and (distinct, direct) per tile."""
    ids = winner_ids(xy, z, size, depth)
    cached = K.scene_totals(xy, z, size, shard, depth)[0]["tiles"]
    return totals(ids, size, cached, shard), tile_index(ids, size)

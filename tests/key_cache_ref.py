"""A numpy restatement of the key cache's totals (nr_free_bin.hip, k_key_plan):
one key item per owned tile, a cached slot of TH * TW keys for every owned tile
with a kept pair.

The kept counts are the visible list's (tests/visible_plan_ref.py: the oracle's
winners' pairs, padded to a pair per slice in a tile the schedule had split), so
everything here comes from the CPU alone.  A tile is cached when it keeps a
pair, whether or not a kept triangle wins a pixel inside it: the binning's tile
rectangle is wider than the triangle, so a kept pair may cover nothing of its
tile, and the tile's cached ids are then all zero -- allowed, it shades as the
raster would have."""
import numpy as np

import visible_plan_ref as P
import visible_ref as V

TW, TH = V.TW, V.TH
KEY_BYTES = TH * TW * 8      # one cached tile
KEY_NB = 16                  # density classes of the cached items


def totals(kept, owned):
    """{"tiles", "items", "bytes"} of the key cache over the kept counts."""
    kept = np.where(owned, np.asarray(kept, dtype=np.int64), 0)
    tiles = int((kept > 0).sum())
    return {"tiles": tiles, "items": int(np.asarray(owned).sum()), "bytes": tiles * KEY_BYTES}


def item_order(kept, owned):
    """Class of every owned tile in the item list's order (largest first):
    KEY_NB equal bins of [1, the largest kept count] in f32 as the kernel forms
    them, 0 for an owned tile without a kept pair (those come last)."""
    kept = np.where(owned, np.asarray(kept, dtype=np.int64), 0)
    top = int(kept.max()) if kept.size else 0
    scale = np.float32(KEY_NB) / np.float32(top + 1)
    cls = 1 + np.minimum((kept.astype(np.float32) * scale).astype(np.int64), KEY_NB - 1)
    return np.where(kept > 0, cls, 0)[np.asarray(owned, dtype=bool)]


def scene_totals(xy, z, size, shard=None, depth=(True, True), split_at=0, dslice=0):
    """The key cache's totals of one scene, and the scene's plans
    (visible_plan_ref.scene_plans)."""
    s = P.scene_plans(xy, z, size, shard, split_at, dslice, None, None, depth)
    return totals(s["kept"], s["owned"]), s


def winner_tiles(xy, z, size, shard=None, depth=(True, True)):
    """bool per tile: some pixel of the tile has a winner on the oracle's frame."""
    import scenes
    n = len(xy)
    col = np.zeros((n, 4))
    col[:, 0] = (np.arange(n) + 1) * 2.0 ** -24
    col[:, 3] = 1.0
    ctx = scenes.OracleFactory().context(size[0], size[1], False)
    ctx.set_color(0.0, 0.0, 0.0, 0.0)
    V.set_depth(ctx, depth)
    ctx.draw_triangles(xy, col, z=z, gouraud=False)
    won = ctx.get_buffer_numpy()[..., 0] > 0
    tx, ty = P.tiles_of(size)
    pad = np.zeros((ty * TH, tx * TW), dtype=bool)
    pad[:size[1], :size[0]] = won
    t = pad.reshape(ty, TH, tx, TW).any(axis=(1, 3)).reshape(-1)
    return t & P.owned_tiles(size, shard)

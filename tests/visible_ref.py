"""CPU helpers of the visible-list tests (tests/test_visible_list_ref.py,
tests/test_visible_list_gpu.py): which triangles of a batch win a pixel of the
oracle's frame, and the (tile, triangle) pairs the binning gives a batch.

Winners come from the oracle itself: the batch drawn with flat colours that
carry the triangle's number (red = (t + 1) * 2^-24, exact in f64 and under the
identity colour transform) over a frame cleared to 0, so the red channel of the
frame names every pixel's winner.  Visibility depends on positions, depths and
the depth state only, so the winners of the id-coloured batch are those of the
batch with its own colours."""
import numpy as np

import scenes

TW, TH = 64, 32            # the rasters' screen tiles (nr_tri.h)
_ID = 2.0 ** -24


def set_depth(ctx, depth, zclear=0xFFFFFFFF):
    ctx.set_depth_state(*depth)
    ctx.clear_depth(zclear)


def winners(xy, z, size, depth=(True, True), zclear=0xFFFFFFFF, shard=None):
    """Sorted indices of the triangles that win at least one pixel when the
    batch is drawn under `depth` over a frame whose depth is cleared to
    `zclear`; shard (nshards, shard): a pixel of the tile rows that rank owns
    (a rank rasterises, and so marks, only those)."""
    n = len(xy)
    assert n < 2 ** 24
    col = np.zeros((n, 4))
    col[:, 0] = (np.arange(n) + 1) * _ID
    col[:, 3] = 1.0
    ctx = scenes.OracleFactory().context(size[0], size[1], False)
    ctx.set_color(0.0, 0.0, 0.0, 0.0)
    set_depth(ctx, depth, zclear)
    ctx.draw_triangles(xy, col, z=z, gouraud=False)
    ids = np.rint(ctx.get_buffer_numpy()[..., 0] / _ID).astype(np.int64)
    if shard is not None:
        ids = ids[(np.arange(size[1]) // TH) % shard[0] == shard[1]]
    w = np.unique(ids)
    return w[w > 0] - 1


def tile_pairs(xy, size, shard=None):
    """(tile, triangle) pairs per triangle under the identity transform: the
    binning's tile rectangle (nr_tri.h tri_tiles: rows [ceil(ymin), ceil(ymax)),
    columns [floor(xmin) - 2, ceil(xmax) + 2], clamped to the frame; nothing for
    a degenerate or off-screen triangle), counted over the tile rows the shard
    (nshards, shard) owns."""
    W, H = size
    p = np.asarray(xy, dtype=np.float64).reshape(-1, 3, 2)
    x, y = p[..., 0], p[..., 1]
    assert np.isfinite(p).all() and np.abs(p).max() < 1e7
    den = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
    r0 = np.clip(np.ceil(y.min(1)), 0, H).astype(np.int64)
    r1 = np.clip(np.ceil(y.max(1)), 0, H).astype(np.int64)
    xmn, xmx = x.min(1), x.max(1)
    hit = (den != 0) & (r0 < r1) & ~((np.ceil(xmx) + 2 < 0) | (np.floor(xmn) - 2 > W - 1))
    c0 = np.clip(np.floor(xmn) - 2, 0, W - 1).astype(np.int64)
    c1 = np.clip(np.ceil(xmx) + 2, 0, W - 1).astype(np.int64)
    cols = c1 // TW - c0 // TW + 1
    ty0, ty1 = r0 // TH, (np.maximum(r1, 1) - 1) // TH
    tiles_y = (H + TH - 1) // TH
    owned = np.ones(tiles_y, dtype=np.int64)
    if shard is not None:
        owned = (np.arange(tiles_y) % shard[0] == shard[1]).astype(np.int64)
    cum = np.concatenate([[0], np.cumsum(owned)])
    rows = cum[np.minimum(ty1, tiles_y - 1) + 1] - cum[np.minimum(ty0, tiles_y - 1)]
    return np.where(hit, cols * rows, 0)

"""A numpy restatement of the key records' totals (nr_tri_free.hip,
key_records_step; the sizes of csrc/nr_key_records.h): the record store of a
generation holds one 128-byte Gouraud shading record per distinct winner of
every cached tile the context owns -- tests/key_index_ref.py's tile_index(...)[0]
summed over those tiles, not capped at KI_RT -- and is built only when it is no
larger than the context's f64 framebuffer."""
import numpy as np

import key_cache_ref as K
import key_index_ref as I
import visible_plan_ref as P

REC_BYTES = 16 * 8                               # a Gouraud record (nr_tri_shade.h RecLen)


def records(ids, size, shard=None):
    """Distinct winners summed over the owned tiles of the winner image `ids`
    (a tile without a winner adds none, cached or not)."""
    distinct, _ = I.tile_index(ids, size)
    return int(distinct[P.owned_tiles(size, shard)].sum())


def cap_bytes(size, alpha=False):
    """The f64 framebuffer of a context: W * H * ipp doubles."""
    return size[0] * size[1] * (4 if alpha else 3) * 8


def fits(n_records, size, alpha=False):
    return n_records * REC_BYTES <= cap_bytes(size, alpha)


def totals(ids, size, cached_tiles, shard=None, alpha=False):
    """{"slots", "records", "bytes"} of the record store of a generation with
    `cached_tiles` cached tiles over the winner image `ids`, or None when the
    store would exceed the cap (it is not built)."""
    n = records(ids, size, shard)
    if not fits(n, size, alpha):
        return None
    return {"slots": int(cached_tiles), "records": n, "bytes": n * REC_BYTES}


def scene_totals(xy, z, size, shard=None, depth=(True, True), alpha=False):
    ids = I.winner_ids(xy, z, size, depth)
    cached = K.scene_totals(xy, z, size, shard, depth)[0]["tiles"]
    return totals(ids, size, cached, shard, alpha)


def pixel_triangles(size):
    """One opaque Gouraud triangle around every pixel centre of a size[0] x
    size[1] frame, each covering that pixel alone: as many winners as pixels,
    so 128 bytes of records per pixel against the framebuffer's 24 or 32."""
    w, h = size
    x, y = [a.ravel().astype(np.float64) for a in np.meshgrid(np.arange(w), np.arange(h))]
    xy = np.stack([x - 0.3, y - 0.3, x + 0.5, y - 0.3, x - 0.3, y + 0.5], axis=1)
    n = w * h
    z = np.repeat(np.linspace(0.2, 0.8, n)[:, None], 3, axis=1)
    k = np.arange(n * 3, dtype=np.float64).reshape(n, 3)
    col = np.stack([(k * 37 % 101) / 101.0, (k * 53 % 103) / 103.0, (k * 71 % 107) / 107.0, np.ones((n, 3))], axis=2)
    return np.ascontiguousarray(xy), np.ascontiguousarray(z), np.ascontiguousarray(col.reshape(n, 12))

"""A numpy restatement of the visible plan (nr_free_bin.hip, k_vis_plan): the
work items of a pruned pair list, planned from the tiles' kept counts.

The kept counts come from the CPU alone: the binning's tile rectangle rule
(tests/visible_ref.py) gives every tile's pairs, the oracle's winners say which
triangles are kept (a kept triangle keeps its pair in every tile it touches),
and the pruning's padding rule keeps at least one pair per slice of a tile the
schedule had split.  From them: the split limits, every tile's items, the
totals (pairs, items, split slices, dense tiles) and the items' size classes.

The constants restate the library's (nr_free.h, nr_free_bin.hip)."""
import numpy as np

import visible_ref as V

TW, TH = V.TW, V.TH
SLICE, SLICE_MIN, SLICE_TARGET = 1024, 64, 256
SPLIT_AT, DSLICE = 1024, 1024            # a binning's default split limits
VIS_SPLIT_AT, VIS_DSLICE = 1024, 1024    # the visible plan's
HEAVY_PAIRS = 256                        # a dense tile
PLAN_ONE, PLAN_SPLIT = 10, 3
PLAN_NB = 1 + PLAN_ONE + PLAN_SPLIT


def tiles_of(size):
    return (size[0] + TW - 1) // TW, (size[1] + TH - 1) // TH


def owned_tiles(size, shard=None):
    """bool per tile (row-major): the tile rows rank `shard[1]` of `shard[0]` owns."""
    tx, ty = tiles_of(size)
    rows = np.ones(ty, dtype=bool) if shard is None else (np.arange(ty) % shard[0] == shard[1])
    return np.repeat(rows, tx)


def tile_counts(xy, size, shard=None, subset=None):
    """Pairs per tile (row-major) of the triangles `subset` (all when None):
    V.tile_pairs' rectangle rule, accumulated per tile over the owned rows."""
    W, H = size
    p = np.asarray(xy, dtype=np.float64).reshape(-1, 3, 2)
    if subset is not None:
        p = p[np.asarray(subset, dtype=np.int64)]
    tx, ty = tiles_of(size)
    if len(p) == 0:
        return np.zeros(tx * ty, dtype=np.int64)
    x, y = p[..., 0], p[..., 1]
    den = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
    r0 = np.clip(np.ceil(y.min(1)), 0, H).astype(np.int64)
    r1 = np.clip(np.ceil(y.max(1)), 0, H).astype(np.int64)
    xmn, xmx = x.min(1), x.max(1)
    hit = (den != 0) & (r0 < r1) & ~((np.ceil(xmx) + 2 < 0) | (np.floor(xmn) - 2 > W - 1))
    c0 = np.clip(np.floor(xmn) - 2, 0, W - 1).astype(np.int64)[hit] // TW
    c1 = np.clip(np.ceil(xmx) + 2, 0, W - 1).astype(np.int64)[hit] // TW
    t0, t1 = r0[hit] // TH, (np.maximum(r1[hit], 1) - 1) // TH
    d = np.zeros((ty + 1, tx + 1), dtype=np.int64)   # a difference array over the tile rectangles
    np.add.at(d, (t0, c0), 1)
    np.add.at(d, (t0, c1 + 1), -1)
    np.add.at(d, (t1 + 1, c0), -1)
    np.add.at(d, (t1 + 1, c1 + 1), 1)
    cnt = d.cumsum(0).cumsum(1)[:ty, :tx].reshape(-1)
    return np.where(owned_tiles(size, shard), cnt, 0)


def limits(total, split_at, dslice):
    """(lim, dsl) of a plan over `total` pairs: a tile of more than lim pairs
    is split into slices of about dsl."""
    s = SLICE_MIN
    while s < SLICE and s * SLICE_TARGET < total:
        s *= 2
    lim = min(s, split_at)
    return lim, max(SLICE_MIN, min(lim, dslice))


def items_of(cnt, owned, lim, dsl):
    """Work items per tile: none for a tile of another rank, one up to lim
    pairs (an empty tile too), else ceil(c / dsl)."""
    cnt = np.asarray(cnt, dtype=np.int64)
    return np.where(owned, np.where(cnt > lim, (cnt + dsl - 1) // dsl, 1), 0)


def kept_counts(full, won, ni_full):
    """The pruned list's counts: the winners' pairs, and in a tile the
    schedule split at least a pair per slice (padded with losers: such a tile
    holds more pairs than slices)."""
    return np.where(ni_full > 1, np.maximum(won, np.minimum(ni_full, full)), won)


def size_classes(cnt, lim, dsl, top):
    """Size class per tile (k_vis_plan lays the items out largest class
    first): 0 empty, 1..PLAN_ONE equal bins of [1, top] in f32 as the kernel
    forms them, the PLAN_SPLIT highest by slice count (2-3, 4-7, >= 8)."""
    cnt = np.asarray(cnt, dtype=np.int64)
    ni = (cnt + dsl - 1) // dsl
    split = PLAN_NB - np.where(ni >= 8, 1, np.where(ni >= 4, 2, 3))
    scale = np.float32(PLAN_ONE) / np.float32(top + 1)
    one = 1 + np.minimum((cnt.astype(np.float32) * scale).astype(np.int64), PLAN_ONE - 1)
    return np.where(cnt > lim, split, np.where(cnt == 0, 0, one))


def plan(cnt, owned, lim, dsl):
    cnt = np.where(owned, np.asarray(cnt, dtype=np.int64), 0)
    ni = items_of(cnt, owned, lim, dsl)
    one = cnt[owned & (cnt <= lim)]
    top = max(int(one.max()) if len(one) else 0, 1)
    return {"pairs": int(cnt.sum()), "items": int(ni.sum()), "split": int(ni[ni > 1].sum()),
            "heavy": int((cnt >= HEAVY_PAIRS).sum()), "ni": ni, "lim": lim, "dsl": dsl, "top": top,
            "classes": size_classes(cnt, lim, dsl, top)}


def totals(p):
    return {k: p[k] for k in ("pairs", "items", "split", "heavy")}


def full_plan(full, owned, split_at=0, dslice=0):
    """A binning's plan of the full counts (split limits 0: the defaults)."""
    lim, dsl = limits(int(np.asarray(full).sum()), split_at or SPLIT_AT, dslice or DSLICE)
    return plan(full, owned, lim, dsl)


def visible_plans(kept, owned, full_total, split_at=0, dslice=0, sched_split_at=0, sched_dslice=0):
    """(preferred, fallback): the visible plan under its own limits
    (SetSplitLimits' when given, else VIS_SPLIT_AT / VIS_DSLICE) and under the
    limits the schedule was binned under, which the kernel takes when the
    preferred plan's items or key slots have no room -- both with the slice
    length of the schedule's full total."""
    lim, dsl = limits(full_total, split_at or VIS_SPLIT_AT, dslice or VIS_DSLICE)
    lim_s, dsl_s = limits(full_total, sched_split_at or SPLIT_AT, sched_dslice or DSLICE)
    return plan(kept, owned, lim, dsl), plan(kept, owned, lim_s, dsl_s)


def scene_plans(xy, z, size, shard=None, split_at=0, dslice=0, sched_split_at=None, sched_dslice=None,
                depth=(True, True)):
    """Everything the tests need of one scene: the full plan, the kept counts
    and the two visible plans.  sched_*: the limits the schedule was binned
    under when they differ from the visible plan's override."""
    sa = split_at if sched_split_at is None else sched_split_at
    sd = dslice if sched_dslice is None else sched_dslice
    owned = owned_tiles(size, shard)
    full = tile_counts(xy, size, shard)
    won = tile_counts(xy, size, shard, V.winners(xy, z, size, depth, shard=shard))
    fp = full_plan(full, owned, sa, sd)
    kept = kept_counts(full, won, fp["ni"])
    pref, fall = visible_plans(kept, owned, int(full.sum()), split_at, dslice, sa, sd)
    return {"full": fp, "kept": kept, "won": won, "pref": pref, "fall": fall, "owned": owned}

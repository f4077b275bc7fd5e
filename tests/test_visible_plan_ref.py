"""The numpy restatement of the visible plan (tests/visible_plan_ref.py) on its
own: its per-tile counts against the per-triangle pair rule of
tests/visible_ref.py, the properties the device plan relies on (under the
schedule's limits no tile has more items than in the full plan, so the fall-back
always fits), the size classes, and that the scenes of the GPU test
(tests/test_visible_replan_gpu.py) contain the cases it claims."""
import numpy as np
import pytest

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
def test_tile_counts_agree_with_the_pair_rule(oracle, mesh, shard):
    xy, z, _ = _mesh(mesh)
    s = P.scene_plans(xy, z, (W, H), shard)
    per_tri = V.tile_pairs(xy, (W, H), shard)
    assert P.tile_counts(xy, (W, H), shard).sum() == per_tri.sum() == s["full"]["pairs"]
    w = V.winners(xy, z, (W, H), shard=shard)
    assert s["won"].sum() == per_tri[w].sum()
    assert (s["won"] <= s["kept"]).all() and (s["kept"] <= P.tile_counts(xy, (W, H), shard)).all()
    assert (s["kept"][~s["owned"]] == 0).all()
    # the padding: a tile the schedule split keeps a pair per slice, and at most that many losers
    split = s["full"]["ni"] > 1
    assert (s["kept"][split] >= s["full"]["ni"][split]).all()
    assert s["kept"].sum() - s["won"].sum() <= s["full"]["split"]
    # under the schedule's limits no tile has more items than it had: the fall-back always fits
    assert (s["fall"]["ni"] <= s["full"]["ni"]).all()
    assert s["fall"]["items"] <= s["full"]["items"] and s["fall"]["split"] <= s["full"]["split"]
    assert s["pref"]["pairs"] == s["fall"]["pairs"] == int(s["kept"].sum())


def test_big_sphere_holds_both_kinds_of_formerly_split_tiles(oracle):
    xy, z, _ = _mesh(BIG)
    s = P.scene_plans(xy, z, (W, H))
    was, now = s["full"]["ni"] > 1, s["pref"]["ni"]
    assert (was & (now == 1)).any() and (was & (now > 1)).any()
    assert (s["pref"]["lim"], s["pref"]["dsl"]) == (P.VIS_SPLIT_AT, P.VIS_DSLICE)   # the visible plan's own limits apply
    assert (s["fall"]["lim"], s["fall"]["dsl"]) == (P.SPLIT_AT, P.DSLICE)
    assert s["pref"]["split"] <= s["full"]["split"]                                   # and fit the schedule's slots
    late = P.scene_plans(xy, z, (W, H), None, 64, 64, 0, 0)    # limits of 64 asked of a schedule binned at the defaults
    assert late["pref"]["split"] > 2 * late["full"]["split"] and late["fall"]["split"] <= late["full"]["split"]


def test_small_batches_keep_the_schedules_slice_length(oracle):
    xy, z, _ = _mesh(SMALL)
    s = P.scene_plans(xy, z, (W, H))
    assert s["full"]["lim"] < P.VIS_SPLIT_AT and s["pref"]["lim"] == s["full"]["lim"] == s["fall"]["lim"]


def test_random_counts_fall_back_within_the_full_plan():
    g = scenes.rng(3)
    for _ in range(50):
        n = int(g.integers(1, 400))
        full = g.integers(0, 5000, n) * (g.uniform(size=n) < 0.7)
        kept = (full * g.uniform(0, 1, n)).astype(np.int64)
        owned = g.uniform(size=n) < 0.8
        sa, sd = int(g.choice([0, 64, 256, 1024])), int(g.choice([0, 64, 128, 1024]))
        fp = P.full_plan(np.where(owned, full, 0), owned, sa, sd)
        kept = P.kept_counts(np.where(owned, full, 0), np.where(owned, kept, 0), fp["ni"])
        pref, fall = P.visible_plans(kept, owned, fp["pairs"], 0, 0, sa, sd)
        assert (fall["ni"] <= fp["ni"]).all()
        assert pref["lim"] <= max(fall["lim"], P.VIS_SPLIT_AT) and pref["dsl"] >= P.SLICE_MIN
        for p in (pref, fall):
            assert p["items"] == int(owned.sum()) + int((p["ni"][p["ni"] > 1] - 1).sum())
            assert p["items"] <= n + p["pairs"] // P.SLICE_MIN + 1   # the room the items are given


def test_size_classes():
    cnt = np.array([0, 1, 19, 20, 100, 195, 196, 300, 512, 513, 1100, 2047, 2049, 4096])
    lim, dsl, top = 512, 512, 300
    c = P.size_classes(cnt, lim, dsl, top)
    assert c[0] == 0 and c[1] == 1
    assert (np.diff(c) >= 0).all()                                   # longer items never in a lower class
    assert c[list(cnt).index(300)] == P.PLAN_ONE                     # the largest one-slice count fills the top bin
    assert list(c[-5:]) == [P.PLAN_NB - 3, P.PLAN_NB - 3, P.PLAN_NB - 2, P.PLAN_NB - 2, P.PLAN_NB - 1]   # 2, 3, 4, 5, 8 slices
    # bins of [1, top] spread what bins of [1, lim] leave in the lowest classes
    kept = np.arange(1, 201)
    assert np.unique(P.size_classes(kept, 1024, 1024, 200)).size == P.PLAN_ONE
    assert np.unique(P.size_classes(kept, 1024, 1024, 1024)).size <= 2

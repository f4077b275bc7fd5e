"""The visible plan (the pruned pair list's own work items, planned on the
device from the tiles' kept counts: k_vis_plan) against the CPU: every frame bit
for bit with the oracle (f64 framebuffer, u32 depth; the frame output in one RGB
and one YUV420P case), and GetVisiblePlanTotals equal to the numpy restatement
of the plan (tests/visible_plan_ref.py), which derives the kept counts from the
oracle's winners and the pruning's padding rule.

Frames, meshes, the oracle cache and the counting context are those of
tests/test_visible_list_gpu.py.  With a readback after each frame, frame 0 bins
cold, frame 1 bins warm, frame 2 marks the winners, frame 3 prunes, plans the
kept counts and is the first rasterised under the visible plan.  Only a
schedule with split tiles is planned again (one without keeps its items).

The plan kernel checks its totals against the real capacities.  Items always
have room (an item per tile and per SLICE_MIN kept pairs); key slots are
allocated for the schedule's split slices T, at most 1.25 T asked for and a
regrow to at most 1.5 x the need, so a preferred plan of <= T slices must be
taken, one of > 2 max(T, 1) slices must fall back to the schedule's limits, and
between the two either plan is accepted -- each exactly."""
import functools

import numpy as np
import pytest

import scenes
import test_visible_list_gpu as L
import textured_ref as T
import visible_plan_ref as P
import visible_ref as V

pytestmark = pytest.mark.gpu

W, H = L.W, L.H
SMALL, BIG = L.SMALL, L.BIG
Frame, Run = L.Frame, L.Run
ZW, NZ, ZT = L.ZW, L.NZ, L.ZT


@functools.lru_cache(maxsize=None)
def _plans(mesh, size=(W, H), shard=None, split=(0, 0), sched=None, depth=ZW):
    xy, z, _ = L._mesh(mesh)
    sa, sd = (None, None) if sched is None else sched
    return P.scene_plans(xy, z, size, shard, split[0], split[1], sa, sd, depth)


def check_plan(run, mesh, size=(W, H), split=(0, 0), sched=None, depth=ZW):
    """GetScheduleTotals and GetVisiblePlanTotals against the numpy plans;
    returns the plans and which one the device took."""
    s = _plans(mesh, size, run.shard, split, sched, depth)
    full, pref, fall = P.totals(s["full"]), P.totals(s["pref"]), P.totals(s["fall"])
    assert run.ctx.schedule_totals() == full, (run.ctx.schedule_totals(), full)
    got = run.ctx.visible_plan_totals()
    print(f"full {full} visible {got} (preferred {pref}, fall-back {fall})")
    assert run.ctx.visible_pair_count() == pref["pairs"] == fall["pairs"]
    assert fall["items"] <= full["items"] and fall["split"] <= full["split"]
    if pref["split"] <= full["split"]:
        assert got == pref, (got, pref)
    elif pref["split"] > 2 * max(full["split"], 1):
        assert got == fall, (got, fall)
    else:
        assert got in (pref, fall), (got, pref, fall)
    return s, ("pref" if got == pref else "fall")


def repeat(run, fr, n):
    for _ in range(n):
        run.draw(fr)
    return run.ctx.replanned_batch_count()


@pytest.mark.parametrize("mesh", [SMALL, BIG])
@pytest.mark.parametrize("shard", [None, (2, 0), (2, 1), (8, 3)])
def test_repeat_frames_replan(gpu, oracle, shard, mesh):
    run = Run(shard)
    got = []
    for _ in range(8):
        run.draw(Frame(mesh))
        got.append(run.ctx.replanned_batch_count())
    assert run.pruned == [0, 0, 0, 1, 2, 3, 4, 5], run.pruned   # (as without the visible plan)
    assert run.reused == [0, 0, 1, 2, 3, 4, 5, 6], run.reused
    assert got == run.pruned, got                               # the first pruned frame already runs the plan
    s, _ = check_plan(run, mesh)
    if mesh == BIG and shard is None:
        # the coverage the reference guarantees: a tile the schedule split that is one item now, one that stays split
        was, now = s["full"]["ni"] > 1, s["pref"]["ni"]
        assert (was & (now == 1)).any() and (was & (now > 1)).any(), (was.sum(), now[was])
        assert P.totals(s["pref"])["split"] <= P.totals(s["full"])["split"]   # (so the preferred plan is the one taken)
    assert run.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("size", [(64, 32), (128, 64)])
def test_hidden_split_tile_is_one_short_item(gpu, oracle, size):
    mesh = ("hidden",) + size
    run = Run(size=size)
    assert repeat(run, Frame(mesh, size=size), 6) == 3
    s, which = check_plan(run, mesh, size)
    assert s["full"]["ni"][0] > 2 and s[which]["ni"][0] == 1, (s["full"]["ni"], s[which]["ni"])
    assert s["kept"][0] == s["full"]["ni"][0]   # two winners, padded to a pair per former slice
    assert run.ctx.visible_plan_totals()["split"] == 0
    assert run.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("split", [(64, 64), (256, 128)])
def test_split_limits_many_split_tiles(gpu, oracle, split):
    """SetSplitLimits before the first draw: the schedule and the visible plan
    share the limits, and many tiles stay split (the slices' merges)."""
    run = Run()
    run.ctx.set_split_limits(*split)
    assert repeat(run, Frame(BIG), 6) == 3
    s, which = check_plan(run, BIG, split=split)
    assert (s[which]["ni"] > 1).sum() >= 8, s[which]["ni"]
    assert run.ctx.warm_failure_count() == 0


def test_preferred_limits_without_room_fall_back_on_the_device(gpu, oracle):
    """The schedule binned under the default limits (few key slots), the
    visible plan asked for slices of 64: far more slots than there are, so the
    kernel plans under the schedule's limits -- and the frames stay exact."""
    run = Run()
    repeat(run, Frame(BIG), 3)
    run.ctx.set_split_limits(64, 64)
    assert repeat(run, Frame(BIG), 3) == 3
    s, which = check_plan(run, BIG, split=(64, 64), sched=(0, 0))
    assert P.totals(s["pref"])["split"] > 2 * max(P.totals(s["full"])["split"], 1)   # (the reference's guarantee)
    assert which == "fall"
    assert run.ctx.warm_failure_count() == 0


def test_depth_modes_in_turn(gpu, oracle):
    """The visible plan serves the capturing mode only; the other modes run
    the schedule's items over the full list, frame by frame in turn."""
    run = Run()
    assert repeat(run, Frame(SMALL), 4) == 1
    for k, depth in enumerate([NZ, ZW, ZT, ZW, NZ, ZT, ZW]):
        run.draw(Frame(SMALL, depth=depth))
    assert run.ctx.replanned_batch_count() == 1 + 3 == run.pruned[-1], run.pruned
    run.draw(Frame(SMALL, pre="other"))                 # LESS + write over a depth an earlier draw wrote
    run.draw(Frame(SMALL, zclear=0x80000000))           # and over a clear to another value
    run.draw(Frame(SMALL, pre="other"))
    assert run.ctx.replanned_batch_count() == run.pruned[-1] > 4, run.pruned
    check_plan(run, SMALL)
    assert run.ctx.warm_failure_count() == 0


def test_no_test_mode_plans_its_own_winners(gpu, oracle):
    run = Run()
    assert repeat(run, Frame(SMALL, depth=NZ), 5) == 2
    check_plan(run, SMALL, depth=NZ)


def test_flat_buffer(gpu, oracle):
    mesh = ("flat",) + SMALL
    run = Run()
    assert repeat(run, Frame(mesh), 6) == 3
    check_plan(run, mesh)


def test_textured_buffer(gpu, oracle):
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    w, h, bg = 200, 140, (0.25, 0.25, 0.25, 0.25)
    b = T.soup(w, h, 1600, 11, T.texture_rgb())   # (dense enough for split tiles: only such a schedule is planned again)
    want = T.expected_payload(w, h, False, bg, "zw", 0xFFFFFFFF, [b])
    buf, tex = R.TriangleBuffer(b["xy"], uv=b["uv"], z=b["z"]), gpu.texture(b["tex"])
    ctx = gpu.context(w, h, False)
    ctx.set_warm_binning(1)
    ctx.set_color_transform(*b["ct"])
    for k in range(6):
        ctx.set_color(*bg)
        V.set_depth(ctx, ZW)
        ctx.draw_triangle_buffer(buf, tex)
        got = ctx.get_buffer_numpy()
        assert scenes.bits_equal(got, want[0]), (k, scenes.first_mismatch(got, want[0]))
        assert np.array_equal(ctx.get_depth_buffer(), want[1]), k
    assert ctx.schedule_totals()["split"] > 0
    assert ctx.replanned_batch_count() == ctx.pruned_batch_count() == 3
    tot = ctx.visible_plan_totals()
    assert tot["pairs"] == ctx.visible_pair_count() and 0 < tot["items"] <= ctx.schedule_totals()["items"], tot


def test_rgba_context(gpu, oracle):
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    xy, z, c = L._mesh(SMALL)
    buf = R.TriangleBuffer(xy, c, z=z, gouraud=True)
    outs = []
    for fac in (gpu, scenes.OracleFactory()):
        ctx = fac.context(W, H, True)
        if fac is gpu:
            ctx.set_warm_binning(1)
        for k in range(5 if fac is gpu else 1):
            ctx.set_color(*L.NONUNI)
            V.set_depth(ctx, ZW)
            if fac is gpu:
                ctx.draw_triangle_buffer(buf)
            else:
                ctx.draw_triangles(xy, c, z=z)
            outs.append((ctx.get_buffer_numpy(), ctx.get_depth_buffer()))
        if fac is gpu:
            assert ctx.replanned_batch_count() == 2
    for k, (f, d) in enumerate(outs[:-1]):
        assert scenes.bits_equal(f, outs[-1][0]), (k, scenes.first_mismatch(f, outs[-1][0]))
        assert np.array_equal(d, outs[-1][1]), k


EMPTIED, UNSPLIT, ESIZE = ("emptied", 150), ("emptied", 40), (128, 64)


def _emptied_mesh(name=EMPTIED):
    """A 128 x 64 frame (2 x 2 tiles): a soup of name[1] triangles inside tile
    (0, 0) -- 150 split the tile (more than SLICE_MIN pairs), 40 do not -- and
    in tile (1, 1) three slivers that span a pixel row between two pixel
    columns: a pair each, no pixel, so no winner, and pruning empties the tile."""
    if name not in L._MESH:
        n = name[1]
        g = scenes.rng(7)
        c = np.stack([g.uniform(12, 48, n), g.uniform(10, 22, n)], axis=1)
        soup = (c[:, None, :] + g.uniform(-8, 8, size=(n, 3, 2))).reshape(n, 6)
        k = np.arange(3)[:, None] * np.array([7.0, 3.0])
        sl = (np.array([[90.2, 40.2], [90.4, 40.2], [90.3, 41.3]])[None] + k[:, None, :]).reshape(3, 6)
        col = g.uniform(0, 1, size=(n + 3, 3, 4))
        col[..., 3] = 1.0
        L._MESH[name] = (np.ascontiguousarray(np.concatenate([soup, sl])), g.uniform(0, 1, size=(n + 3, 3)),
                         col.reshape(n + 3, 12))
    return L._MESH[name]


def test_a_schedule_without_split_tiles_keeps_its_items(gpu, oracle):
    """The plan is taken only where the schedule has split tiles (the slices
    and merges it removes are the measured gain): a schedule without any is
    pruned and rasterised under its own items, exactly."""
    _emptied_mesh(UNSPLIT)
    assert _plans(UNSPLIT, ESIZE)["full"]["split"] == 0
    run = Run(size=ESIZE)
    assert repeat(run, Frame(UNSPLIT, size=ESIZE), 6) == 0
    assert run.pruned == [0, 0, 0, 1, 2, 3], run.pruned
    assert run.ctx.schedule_totals()["split"] == 0 and run.ctx.visible_plan_totals() is None
    assert run.ctx.visible_pair_count() == _plans(UNSPLIT, ESIZE)["pref"]["pairs"]


@pytest.mark.parametrize("fmt", ["rgb", "yuv420p"])
def test_pending_uniform_clear_and_frame_output(gpu, oracle, fmt):
    """A uniform colour clear stays pending on the tiles without a kept pair
    (the fast clear) -- the never covered ones and the one pruning emptied,
    now an empty item -- and the raster writes the frame output itself."""
    xy, _, _ = _emptied_mesh()
    s = _plans(EMPTIED, ESIZE)
    full = P.tile_counts(xy, ESIZE)
    assert list(full > 0) == [True, False, False, True] and list(s["kept"] > 0) == [True, False, False, False], (full, s["kept"])
    assert s["full"]["split"] > 0   # (so the schedule is planned again)
    run = Run(size=ESIZE)
    fr = Frame(EMPTIED, clear=L.UNI, size=ESIZE)
    repeat(run, fr, 4)
    check_plan(run, EMPTIED, ESIZE)
    run.ctx.set_frame_format(fmt)
    run.ctx.gather_frame_u8()
    run.draw(fr)
    run.ctx.gather_frame_u8()
    assert run.ctx.replanned_batch_count() == 2 == run.pruned[-1], run.pruned
    out, u8 = run.ctx.get_frame_u8(), L._want(fr)["u8"]
    assert np.array_equal(out, scenes.yuv420p(u8) if fmt == "yuv420p" else u8), fmt


@pytest.mark.parametrize("mesh", [SMALL, BIG])
def test_unread_frames(gpu, oracle, mesh):
    """12 frames without a readback: the host prunes, plans and takes the
    plan's totals whenever it first sees them, and waits for nothing."""
    run = Run()
    for _ in range(12):
        run.draw(Frame(mesh), read=False)
    run.check(Frame(mesh), " (after 12 unread frames)")
    p, r = run.ctx.pruned_batch_count(), run.ctx.replanned_batch_count()
    print(f"re-planned batches among 12 unread frames: {r} (pruned {p})")
    assert 0 <= r <= p
    assert repeat(run, Frame(mesh), 2) == r + 2
    check_plan(run, mesh)
    assert run.ctx.warm_failure_count() == 0


def test_switch_and_invalidation(gpu, oracle):
    run = Run()
    A = Frame(SMALL)
    assert repeat(run, A, 5) == 2
    run.ctx.set_visible_replan(2)           # off: the pruned list in place, under the schedule's items
    assert repeat(run, A, 2) == 2 and run.pruned[-1] == 4, run.pruned
    run.ctx.set_visible_replan(0)
    assert repeat(run, A, 2) == 4 and run.pruned[-1] == 6, run.pruned
    check_plan(run, SMALL)
    # a list pruned with the switch off is planned when it comes on
    run2 = Run()
    run2.ctx.set_visible_replan(2)
    assert repeat(run2, A, 5) == 0 and run2.pruned[-1] == 2 and run2.ctx.visible_plan_totals() is None
    run2.ctx.set_visible_replan(0)
    assert repeat(run2, A, 2) == 2 and run2.pruned[-1] == 4
    check_plan(run2, SMALL)
    # a transform change past 2 px: a new schedule, marked, pruned and planned afresh
    moved = Frame(SMALL, move=(7.0, 5.0))
    r0 = run.ctx.replanned_batch_count()
    run.draw(moved)
    assert run.ctx.visible_plan_totals() is None and run.ctx.replanned_batch_count() == r0
    assert repeat(run, moved, 4) > r0
    # a resize: another key
    small = Frame(SMALL, size=(320, 208))
    run.draw(small)
    assert run.ctx.visible_plan_totals() is None
    r0 = run.ctx.replanned_batch_count()
    assert repeat(run, small, 4) > r0
    check_plan(run, SMALL, (320, 208))
    # another batch taking the list's binning set: exact, re-planned wherever pruned
    r0, p0 = run.ctx.replanned_batch_count(), run.pruned[-1]
    repeat(run, Frame(SMALL, size=(320, 208), pre="other"), 4)
    assert run.ctx.replanned_batch_count() - r0 == run.pruned[-1] - p0 > 0, run.pruned
    assert run.ctx.warm_failure_count() == 0

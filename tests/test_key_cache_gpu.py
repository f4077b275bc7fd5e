"""The key cache (an unchanged TriangleBuffer draw shaded from the final
visibility keys that one capture frame stored: k_keys, no raster) against the
CPU oracle: every frame bit for bit on the f64 framebuffer and the u32 depth,
the frame output in one RGB and one YUV420P case.

Frames, meshes, the oracle cache and the counting context are those of
tests/test_visible_list_gpu.py.  With a readback after each frame the stages
follow from the host code: frame 0 bins cold, frame 1 bins warm, frame 2 marks
the winners, frame 3 prunes (and plans the key items), frame 4 -- the host has
seen the items' totals and allocated the slots -- is the capture frame, frame 5
has seen the capture frame complete and is the first shaded from the cache.
GetKeyCachedBatchCount moves on cached frames only, and a cached batch counts
as the pruned (reused, warm) batch it replaces.

GetKeyCacheTotals is checked against tests/key_cache_ref.py, which derives the
kept counts from the oracle's winners."""
import functools

import numpy as np
import pytest

import bilinear_ref as B
import key_cache_ref as K
import scenes
import test_visible_list_gpu as L
import textured_ref as T
import visible_ref as V

pytestmark = pytest.mark.gpu

W, H = L.W, L.H
SMALL, BIG = L.SMALL, L.BIG
NONUNI, UNI = L.NONUNI, L.UNI
ZW, NZ, ZT = L.ZW, L.NZ, L.ZT
CACHED_AT = 5   # the first cached frame of a generation read back frame by frame


class Frame(L.Frame):
    """L.Frame with a colour transform (opaque: its alpha factor stays 1)."""

    def __init__(self, mesh, ct=(1.0, 1.0, 1.0, 1.0), **kw):
        super().__init__(mesh, **kw)
        self.ct = ct

    def key(self):
        return super().key() + (self.ct,)

    def issue(self, ctx, draw):
        def with_ct(t):
            t.set_color_transform(*self.ct)
            draw(t)
            t.set_color_transform(1.0, 1.0, 1.0, 1.0)
        super().issue(ctx, with_ct)


class Run(L.Run):
    def __init__(self, shard=None, size=(W, H)):
        super().__init__(shard, size)
        self.cached = []

    def draw(self, fr, read=True):
        super().draw(fr, read)
        if read:
            self.cached.append(self.ctx.key_cached_batch_count())

    def repeat(self, fr, n):
        for _ in range(n):
            self.draw(fr)
        return self.ctx.key_cached_batch_count()


@functools.lru_cache(maxsize=None)
def _totals(mesh, size=(W, H), shard=None, depth=ZW):
    xy, z, _ = L._mesh(mesh)
    return K.scene_totals(xy, z, size, shard, depth)[0]


def check_totals(run, mesh, size=(W, H), depth=ZW):
    want, got = _totals(mesh, size, run.shard, depth), run.ctx.key_cache_totals()
    print(f"key cache {got}")
    assert got == want, (got, want)
    return got


@pytest.mark.parametrize("mesh", [SMALL, BIG])
@pytest.mark.parametrize("shard", [None, (2, 0), (2, 1), (8, 3)])
def test_stage_sequence(gpu, oracle, shard, mesh):
    run = Run(shard)
    run.repeat(Frame(mesh), 8)
    assert run.cached == [0, 0, 0, 0, 0, 1, 2, 3], run.cached    # cold, warm, marking, pruned, capture, then cached
    assert run.pruned == [0, 0, 0, 1, 2, 3, 4, 5], run.pruned    # (as without the key cache)
    assert run.reused == [0, 0, 1, 2, 3, 4, 5, 6], run.reused
    assert run.warm == [0, 1, 2, 3, 4, 5, 6, 7], run.warm
    t = check_totals(run, mesh)
    assert 0 < t["tiles"] < t["items"]
    assert run.ctx.warm_failure_count() == 0


def test_a_shard_change_starts_a_new_generation(gpu, oracle):
    run = Run((2, 0))
    assert run.repeat(Frame(SMALL), 7) == 2
    check_totals(run, SMALL)
    run.ctx.set_shard(2, 1)
    run.shard = (2, 1)
    c0 = run.ctx.key_cached_batch_count()
    run.draw(Frame(SMALL))
    assert run.ctx.key_cache_totals() is None and run.ctx.key_cached_batch_count() == c0
    assert run.repeat(Frame(SMALL), 6) > c0
    check_totals(run, SMALL)
    assert run.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("depth", [ZW, NZ])
@pytest.mark.parametrize("mesh", [SMALL, ("flat",) + SMALL])
def test_flat_and_gouraud_buffers(gpu, oracle, mesh, depth):
    run = Run()
    assert run.repeat(Frame(mesh, depth=depth), 7) == 2
    assert run.cached == [0, 0, 0, 0, 0, 1, 2], run.cached
    check_totals(run, mesh, depth=depth)
    assert run.ctx.warm_failure_count() == 0


def test_live_colour_state(gpu, oracle):
    """Clear colour and colour transform change between cached frames: each is
    exact and still cached (nothing colour-side is in the cache)."""
    run = Run()
    assert run.repeat(Frame(SMALL), 6) == 1
    frames = [Frame(SMALL, clear=UNI), Frame(SMALL, ct=(0.5, 0.25, 0.75, 1.0)), Frame(SMALL, clear=(0.9, 0.1, 0.4, 0.3)),
              Frame(SMALL, ct=(0.3, 1.0, 0.6, 1.0), clear=UNI), Frame(SMALL)]
    for k, fr in enumerate(frames):
        run.draw(fr)
        assert run.cached[-1] == 2 + k, run.cached
    assert not scenes.bits_equal(L._want(frames[0])["f64"], L._want(frames[1])["f64"])
    assert run.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("fmt", ["rgb", "yuv420p"])
def test_frame_output_of_a_cached_frame(gpu, oracle, fmt):
    """The output format changes between cached frames; under a uniform clear
    the raster -- here k_keys -- writes the frame output itself."""
    run = Run()
    fr = Frame(SMALL, clear=UNI)
    assert run.repeat(fr, 6) == 1
    for f in (fmt, "rgb" if fmt == "yuv420p" else "yuv420p", fmt):
        run.ctx.set_frame_format(f)
        run.ctx.gather_frame_u8()
        run.draw(fr)
        run.ctx.gather_frame_u8()
        out, u8 = run.ctx.get_frame_u8(), L._want(fr)["u8"]
        assert np.array_equal(out, scenes.yuv420p(u8) if f == "yuv420p" else u8), f
    assert run.cached[-3:] == [2, 3, 4], run.cached


@pytest.mark.parametrize("mode", ["zw", "nz"])
def test_textured_buffer_toggles_filter_and_texture(gpu, oracle, mode):
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    b = B.soup_batches("opaque", False)[0]
    texs = [T.texture_rgb(), T.texture_rgb(seed=8, w=11, h=7)]
    gtex = [gpu.texture(t) for t in texs]
    buf = R.TriangleBuffer(b["xy"], uv=b["uv"], z=b["z"])
    ctx = gpu.context(B.W, B.H, False)
    ctx.set_warm_binning(1)
    ctx.set_transform(*b["m"])
    ctx.set_color_transform(*b["ct"])
    plan = [(0, 0)] * 6 + [(1, 0), (0, 1), (1, 1), (0, 0)]   # (filter, texture) per frame: toggled on the cached frames
    wants, cached = {}, []
    for k, (filt, ti) in enumerate(plan):
        if (filt, ti) not in wants:
            wants[(filt, ti)] = B.expected_payload(B.W, B.H, False, B.BG, mode, B.FAR, [dict(b, tex=texs[ti])], filt=filt)
        ctx.set_color(*B.BG)
        T._set_depth_mode(ctx, mode)
        ctx.clear_depth(B.FAR)
        ctx.set_triangle_texture_filter(filt)
        ctx.draw_triangle_buffer(buf, gtex[ti])
        got, want = (ctx.get_buffer_numpy(), ctx.get_depth_buffer()), wants[(filt, ti)]
        assert scenes.bits_equal(got[0], want[0]), (k, filt, ti, scenes.first_mismatch(got[0], want[0]))
        if want[1] is not None:
            assert np.array_equal(got[1], want[1]), (k, "depth")
        cached.append(ctx.key_cached_batch_count())
    assert not scenes.bits_equal(wants[(1, 0)][0], wants[(0, 0)][0])
    assert cached == [0, 0, 0, 0, 0, 1, 2, 3, 4, 5], cached
    assert ctx.warm_failure_count() == 0
    t = ctx.key_cache_totals()
    assert t is not None and 0 < t["tiles"] <= t["items"] and t["bytes"] == t["tiles"] * K.KEY_BYTES, t


def test_ineligible_draws_are_not_cached(gpu, oracle):
    """LESS without write, a depth clear to another value and a depth an
    earlier draw has written: exact, never from the cache (whose keys assume a
    pending clear to 0xFFFFFFFF); the next eligible frame is cached again."""
    run = Run()
    assert run.repeat(Frame(SMALL), 6) == 1
    c = 1
    for fr in (Frame(SMALL, depth=ZT), Frame(SMALL, zclear=0x80000000), Frame(SMALL, depth=NZ)):
        assert run.repeat(fr, 2) == c, (fr.key(), run.cached)
        c = run.repeat(Frame(SMALL), 1)
        assert c == run.cached[-3] + 1, run.cached
    # a draw from host arrays first: it leaves depth written and takes a binning set in rotation, so the
    # static buffer bins warm again now and then -- never cached; eligible frames are cached once its list is in place
    assert run.repeat(Frame(SMALL, pre="other"), 4) == c, run.cached
    assert run.repeat(Frame(SMALL), 3) > c, run.cached
    assert run.ctx.warm_failure_count() == 0


def test_no_capture_without_the_capture_condition(gpu, oracle):
    run = Run()
    assert run.repeat(Frame(SMALL), 4) == 0           # pruned; the key items are planned
    assert run.repeat(Frame(SMALL, zclear=0x80000000), 3) == 0   # pruned frames, none may capture
    assert run.pruned[-1] == 4, run.pruned
    assert run.repeat(Frame(SMALL), 1) == 0           # the capture frame
    assert run.repeat(Frame(SMALL), 2) == 2, run.cached
    check_totals(run, SMALL)


@pytest.mark.parametrize("size", [(64, 32), (128, 64)])
def test_hidden_split_tile(gpu, oracle, size):
    """A split tile: the slice that finishes last merges, captures and shades."""
    mesh = ("hidden",) + size
    run = Run(size=size)
    assert run.repeat(Frame(mesh, size=size), 8) == 3
    assert run.ctx.schedule_totals()["split"] > 2
    check_totals(run, mesh, size)
    assert run.ctx.warm_failure_count() == 0


def test_split_tiles_that_stay_split(gpu, oracle):
    """Split limits of 64: many tiles are still split under the visible plan on
    the capture frame; the key items have no slices."""
    run = Run()
    run.ctx.set_split_limits(64, 64)
    assert run.repeat(Frame(BIG), 7) == 2
    assert run.ctx.visible_plan_totals()["split"] >= 8
    xy, z, _ = L._mesh(BIG)
    want = K.scene_totals(xy, z, (W, H), None, ZW, 64, 64)[0]
    assert run.ctx.key_cache_totals() == want, (run.ctx.key_cache_totals(), want)
    assert run.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("size", [(70, 45), (1, 58)])
def test_frame_edges(gpu, oracle, size):
    mesh = ("soup",) + size
    run = Run(size=size)
    assert run.repeat(Frame(mesh, size=size), 8) == 3
    assert run.cached == [0, 0, 0, 0, 0, 1, 2, 3], run.cached
    check_totals(run, mesh, size)
    assert run.ctx.warm_failure_count() == 0


def test_what_ends_the_generation(gpu, oracle):
    run = Run()
    A = Frame(SMALL)
    assert run.repeat(A, 6) == 1
    # a transform change within 2 px: binned loose, not cached; back under the schedule's transform: cached again
    c = run.repeat(Frame(SMALL, move=(0.4, 0.3)), 1)
    assert c == 1 and run.ctx.loose_batch_count() == 1
    assert run.repeat(A, 3) > c, run.cached
    # a transform change past 2 px: a new schedule
    moved = Frame(SMALL, move=(7.0, 5.0))
    c = run.ctx.key_cached_batch_count()
    run.draw(moved)
    assert run.ctx.key_cache_totals() is None and run.ctx.key_cached_batch_count() == c
    assert run.repeat(moved, 4) == c and run.repeat(moved, 2) > c, run.cached
    # a resize: another key
    small = Frame(SMALL, size=(320, 208))
    c = run.ctx.key_cached_batch_count()
    run.draw(small)
    assert run.ctx.key_cache_totals() is None
    assert run.repeat(small, 4) == c and run.repeat(small, 2) > c, run.cached
    check_totals(run, SMALL, (320, 208))
    run.draw(A)   # (back to the tests' frame size)
    # a second buffer of the same size under the same transform: its own keys
    run.repeat(A, 6)
    del run.bufs[SMALL]
    c = run.ctx.key_cached_batch_count()
    assert run.repeat(Frame("changed"), 5) == c and run.repeat(Frame("changed"), 2) > c, run.cached
    check_totals(run, "changed")
    # another TriangleBuffer's batch in between takes the schedule: every frame exact, the generation starts over
    c = run.ctx.key_cached_batch_count()
    for _ in range(2):
        run.draw(Frame("other"))
        run.draw(Frame("changed"))
    assert run.ctx.key_cached_batch_count() == c, run.cached
    assert run.ctx.warm_failure_count() == 0


def test_switches(gpu, oracle):
    run = Run()
    A = Frame(SMALL)
    assert run.repeat(A, 6) == 1
    run.ctx.set_key_cache(2)                       # off: the visible list; the cached keys are kept
    assert run.repeat(A, 2) == 1 and run.pruned[-1] == run.pruned[-3] + 2, (run.cached, run.pruned)
    check_totals(run, SMALL)
    run.ctx.set_key_cache(0)
    assert run.repeat(A, 2) == 3, run.cached
    run.ctx.set_visible_pruning(2)                 # no visible list in use, so no cache either
    assert run.repeat(A, 2) == 3, run.cached
    run.ctx.set_visible_pruning(0)
    assert run.repeat(A, 2) == 5, run.cached
    run.ctx.set_list_reuse(2)                      # every warm batch bins
    assert run.repeat(A, 2) == 5, run.cached
    run.ctx.set_list_reuse(0)
    assert run.repeat(A, 2) >= 6, run.cached
    run.ctx.set_warm_binning(2)                    # cold batches; the generation's lists are gone
    assert run.repeat(A, 2) == run.cached[-3], run.cached
    run.ctx.set_warm_binning(1)
    c = run.ctx.key_cached_batch_count()
    assert run.repeat(A, 8) > c, run.cached
    # the switch off from the start: nothing is planned or captured until it comes on
    run2 = Run()
    run2.ctx.set_key_cache(2)
    assert run2.repeat(A, 7) == 0 and run2.ctx.key_cache_totals() is None and run2.pruned[-1] == 4
    run2.ctx.set_key_cache(0)
    assert run2.repeat(A, 2) == 0 and run2.repeat(A, 2) == 2, run2.cached
    assert run.ctx.warm_failure_count() == 0 and run2.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_fault_on_a_frame_that_would_have_been_cached(gpu, oracle, mode):
    """A fault injected at frame 7: that frame bins (not reused, pruned or
    cached), falls back exactly and is reported once; then the buffer bins cold
    (1, 3: banned) or gets a new schedule, cached afresh (2, 4)."""
    from libnativecpurenderer_amd import _lib
    run = Run()
    _lib.clear_error()
    for k in range(16):
        if k == 7:
            run.ctx.set_warm_fault_injection(mode)
        run.draw(Frame(SMALL))
    c = run.cached
    assert c[:8] == [0, 0, 0, 0, 0, 1, 2, 2], c
    assert run.ctx.warm_failure_count() == 1
    assert "warm binning" in _lib.last_error(), _lib.last_error()
    if mode in (2, 4):
        assert c[-1] > c[7], c
    else:
        assert c[-1] == c[7] and run.ctx.key_cache_totals() is None, c


@pytest.mark.parametrize("mesh", [SMALL, BIG])
def test_unread_frames(gpu, oracle, mesh):
    """12 frames without a readback: the host takes each stage when it first
    sees the one before complete, by a query, and waits for nothing -- so how
    many of the 12 were cached depends on how far it ran ahead (printed)."""
    run = Run()
    for _ in range(12):
        run.draw(Frame(mesh), read=False)
    run.check(Frame(mesh), " (after 12 unread frames)")
    c = run.ctx.key_cached_batch_count()
    print(f"cached batches among 12 unread frames: {c} (pruned {run.ctx.pruned_batch_count()})")
    assert 0 <= c <= 7   # (frame 5 is the first that can be)
    assert run.repeat(Frame(mesh), 4) >= c + 1, run.cached
    check_totals(run, mesh)
    assert run.ctx.warm_failure_count() == 0

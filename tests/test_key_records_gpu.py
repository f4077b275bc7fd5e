"""The key records (an indexed Gouraud TriangleBuffer draw shaded by k_keys_rec
from the generation's record store, which k_key_records fills once) against
the CPU oracle: every frame bit for bit on the f64 framebuffer and the u32
depth, the frame output in one RGB and one YUV420P case.

Frames, meshes, the oracle cache and the counting contexts are those of
tests/test_key_index_gpu.py, test_key_cache_gpu.py, test_visible_list_gpu.py and
test_deferred_stores_gpu.py.  The stages follow from the host code
(nr_tri_free.hip): with a readback after each frame, frame 4 is the capture
frame -- the index, the slots' distinct counts and the scan of the record
offsets are enqueued right behind it, before the event that frame 5 polls --
so frame 5, the first cached and indexed one, sees the scan's total, sizes the
store and enqueues k_key_records, and still runs k_keys_idx itself; frame 6 is
the first shaded from the records.  RECORDS_AT = 6 = the first indexed frame
+ 1.  GetKeyRecordBatchCount moves on record frames only, and a record batch
counts as the indexed (cached, pruned, reused, warm) batch it is.

GetKeyRecordTotals is checked against tests/key_records_ref.py.  By that
reference (tests/test_key_records_ref.py) SMALL's store fits under the cap,
BIG's only as a shard's: unsharded BIG is the natural over-the-cap scene, and
stays on k_keys_idx.

NR_KEYS_WIDE is read once per process, so the 512-thread instances are reached
by test_the_wide_instances, which runs a choice of these cases in a child
process with NR_KEYS_WIDE=1."""
import os
import subprocess
import sys

import numpy as np
import pytest

import key_records_ref as KR
import scenes
import test_deferred_stores_gpu as D
import test_key_cache_gpu as C
import test_key_index_gpu as I
import test_visible_list_gpu as L

pytestmark = pytest.mark.gpu

W, H = L.W, L.H
SMALL, BIG = L.SMALL, L.BIG
NONUNI, UNI = L.NONUNI, L.UNI
ZW, NZ, ZT = L.ZW, L.NZ, L.ZT
Frame = I.Frame
RECORDS_AT = C.CACHED_AT + 1
OVER = (64, 32)


class Run(D.Run):
    """D.Run (deferral mode, frame output) that also keeps the record batch
    count after each checked frame; by default nothing defers."""

    def __init__(self, shard=None, size=(W, H), mode=2, fmt="rgb", gather=False):
        super().__init__(shard, size, mode=mode, fmt=fmt, gather=gather)
        self.recs = []

    def draw(self, fr, read=True):
        super().draw(fr, read)
        if read:
            self.recs.append(self.ctx.key_record_batch_count())

    def repeat(self, fr, n):
        """-> (cached, indexed, record) batch counts after n more checked frames."""
        return super().repeat(fr, n) + (self.recs[-1],)


def _want_totals(mesh, size=(W, H), shard=None, depth=ZW):
    return KR.totals(I._scene(mesh, size, depth), size, C._totals(mesh, size, shard, depth)["tiles"], shard)


def check_totals(run, mesh, size=(W, H), depth=ZW):
    want, got = _want_totals(mesh, size, run.shard, depth), run.ctx.key_record_totals()
    print(f"key records {got}")
    assert got == want, (got, want)
    return got


def started(fr, **kw):
    """A Run whose last frame (frame 6) was the first shaded from the records."""
    run = Run(**kw)
    assert run.repeat(fr, RECORDS_AT + 1) == (2, 2, 1), (run.cached, run.indexed, run.recs)
    return run


@pytest.mark.parametrize("mesh", [SMALL, BIG])
@pytest.mark.parametrize("shard", [None, (2, 1), (8, 3)])
def test_stage_sequence(gpu, oracle, shard, mesh):
    run = Run(shard)
    run.repeat(Frame(mesh), 9)
    assert run.cached == [0, 0, 0, 0, 0, 1, 2, 3, 4], run.cached
    assert run.indexed == run.cached, run.indexed
    t = check_totals(run, mesh)
    if mesh == BIG and shard is None:            # over the cap (test_key_records_ref): no store, k_keys_idx
        assert t is None and run.recs == [0] * 9, run.recs
    else:
        assert t["records"] > 0
        assert run.recs == [0] * RECORDS_AT + [1, 2, 3], run.recs
        assert (t["records"] > run.ctx.key_index_totals()["staged"]) == (mesh == BIG)   # records past KI_RT
    I.check_totals(run, mesh)
    assert run.ctx.warm_failure_count() == 0


def _winners(n):
    tile, win = I._dense_tile()
    assert len(win) >= n
    name = ("winners", n)
    xy, z, c = L._mesh(BIG)
    L._MESH[name] = tuple(np.ascontiguousarray(a[win[:n]]) for a in (xy, z, c))
    return name


@pytest.mark.parametrize("n", [279, 280, 281, 560, 561])
def test_record_boundary(gpu, oracle, n):
    """Exactly n winners in one tile (as test_key_index_gpu's boundary case):
    with 560 and 561 the directly loaded records run two, then a third, per
    thread of the 256-thread workgroup."""
    name = _winners(n)
    run = started(Frame(name))
    t = check_totals(run, name)
    assert t["records"] >= n
    assert (run.ctx.key_index_totals()["direct"] > 0) == (n > 280)
    assert run.repeat(Frame(name), 2) == (4, 4, 3)
    assert run.ctx.warm_failure_count() == 0


def test_the_densest_tile(gpu, oracle):
    """Every winner of BIG's densest tile (1715 by the reference): the direct
    loads run several rounds per thread."""
    tile, win = I._dense_tile()
    name = _winners(len(win))
    run = started(Frame(name))
    assert check_totals(run, name)["records"] >= len(win) > 4 * 280


def _column():
    """Eight triangles down a one-pixel-wide frame, four pixels each: few enough
    winners for the ten records that a (1, 58) context's cap allows."""
    name = ("column",)
    if name not in L._MESH:
        y0 = 7.0 * np.arange(8)
        xy = np.stack([np.full(8, -2.0), y0 - 0.5, np.full(8, 3.0), y0 - 0.5, np.full(8, -2.0), y0 + 6.5], axis=1)
        z = np.repeat(np.linspace(0.3, 0.7, 8)[:, None], 3, axis=1)
        c = scenes.rng(7).uniform(0, 1, size=(8, 3, 4))
        c[..., 3] = 1.0
        L._MESH[name] = (np.ascontiguousarray(xy), np.ascontiguousarray(z), np.ascontiguousarray(c.reshape(8, 12)))
    return name


@pytest.mark.parametrize("deferred", [False, True])
def test_a_one_pixel_wide_frame(gpu, oracle, deferred):
    """(1, 58) with a store that fits: the narrowest tile the record path shades."""
    size, mesh = (1, 58), _column()
    want = _want_totals(mesh, size)
    assert want is not None and 0 < want["records"] <= 10, want
    if deferred:
        fr = Frame(mesh, clear=UNI, size=size)
        run = pending(fr, size=size)
        run.check(fr)
    else:
        run = started(Frame(mesh, size=size), size=size)
    check_totals(run, mesh, size)
    assert run.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("size", [(64, 32), (65, 33), (1, 58)])
def test_frame_edges(gpu, oracle, size):
    """(1, 58): a 1392-byte framebuffer, ten records -- by the reference the
    soup's store is over the cap there, and the frames stay on k_keys_idx
    (test_a_one_pixel_wide_frame has a mesh whose store fits)."""
    mesh = ("soup",) + size
    if _want_totals(mesh, size) is None:
        assert size == (1, 58)
        run = Run(size=size)
        assert run.repeat(Frame(mesh, size=size), RECORDS_AT + 2) == (3, 3, 0), (run.indexed, run.recs)
    else:
        run = started(Frame(mesh, size=size), size=size)
    check_totals(run, mesh, size)
    assert run.ctx.warm_failure_count() == 0


def test_rgba_context(gpu, oracle):
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    xy, z, c = L._mesh(SMALL)
    fr = Frame(SMALL, clear=(0.3, 0.1, 0.2, 0.6))
    ora = scenes.OracleFactory().context(W, H, True)
    fr.issue(ora, lambda t: t.draw_triangles(xy, c, z=z))
    want = (ora.get_buffer_numpy(), ora.get_depth_buffer())
    ctx = R.RenderContext(W, H, True)
    ctx.set_warm_binning(1)
    buf = R.TriangleBuffer(xy, c, z=z, gouraud=True)
    for k in range(8):
        fr.issue(ctx, lambda t: t.draw_triangle_buffer(buf))
        g = ctx.get_buffer_numpy()
        assert scenes.bits_equal(g, want[0]), (k, scenes.first_mismatch(g, want[0]))
        assert np.array_equal(ctx.get_depth_buffer(), want[1]), k
    assert ctx.key_indexed_batch_count() == 3 and ctx.key_record_batch_count() == 2
    assert ctx.key_record_totals() == _want_totals(SMALL)


@pytest.mark.parametrize("shard", [None, (2, 1)])
def test_no_test_depth_mode(gpu, oracle, shard):
    run = started(Frame(BIG if shard else SMALL, depth=NZ), shard=shard)
    check_totals(run, BIG if shard else SMALL, depth=NZ)
    assert run.ctx.warm_failure_count() == 0


def test_live_colour_state(gpu, oracle):
    """Clear colour and colour transform change between record frames: each is
    exact and still shaded from the records (which hold neither)."""
    run = started(Frame(SMALL))
    frames = [Frame(SMALL, clear=UNI), Frame(SMALL, ct=(0.5, 0.25, 0.75, 1.0)), Frame(SMALL, clear=(0.9, 0.1, 0.4, 0.3)),
              Frame(SMALL, ct=(0.3, 1.0, 0.6, 1.0), clear=UNI), Frame(SMALL)]
    for k, fr in enumerate(frames):
        run.draw(fr)
        assert run.recs[-1] == 2 + k, run.recs
    assert run.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("fmt,shard,mesh", [("rgb", None, SMALL), ("yuv420p", None, 561), ("rgb", (2, 1), BIG)])
def test_frame_output_of_a_record_frame(gpu, oracle, fmt, shard, mesh):
    """Not deferred (KO_ALL) under a uniform clear: k_keys_rec writes the frame
    output itself, staged and directly loaded pixels (561: that many winners
    in one tile; BIG as a shard's)."""
    fr = Frame(_winners(mesh) if mesh == 561 else mesh, clear=UNI)
    run = started(fr, shard=shard)
    # (a shard's planar output is not compared: D.Run.check_frame_output; its RGB rows are)
    for f in (fmt, fmt, fmt) if shard else (fmt, "rgb" if fmt == "yuv420p" else "yuv420p", fmt):
        run.fmt = f
        run.ctx.set_frame_format(f)
        run.ctx.gather_frame_u8()
        run.draw(fr)
        run.check_frame_output(fr)
    assert run.recs[-3:] == [2, 3, 4], run.recs
    assert run.counts()[:2] == (0, 0), run.counts()


# ---- deferred record frames (KO_FRAME), and the roads out of the pending state ------------

def pending(fr, shard=None, size=(W, H), fmt="rgb", halves=2):
    """D.pending one stage later: frames 5 and 6 deferred and were read back,
    frame 7 -- shaded from the records -- is pending, its frame output checked."""
    run = Run(shard, size, mode=1, fmt=fmt, gather=True)
    assert run.repeat(fr, RECORDS_AT + 1) == (2, 2, 1), (run.cached, run.indexed, run.recs)
    assert run.counts() == (2, 2 * halves, 0, 8), run.counts()
    run.draw(fr, read=False)
    assert run.counts() == (3, 2 * halves, 0, 8), run.counts()
    assert run.ctx.key_record_batch_count() == 2
    run.check_frame_output(fr)
    return run


F = D.F


@pytest.mark.parametrize("fmt", ["rgb", "yuv420p"])
def test_readback_of_a_deferred_record_frame(gpu, oracle, fmt):
    run = pending(F, fmt=fmt)
    run.check(F)
    assert run.counts() == (3, 6, 0, 16), run.counts()
    run.draw(F)
    assert run.counts() == (4, 8, 0, 32), run.counts()
    assert run.recs[-1] == 3


@pytest.mark.parametrize("first", ["depth", "colour"])
def test_one_half_then_the_other(gpu, oracle, first):
    run = pending(F)
    want = D.want_of(F)
    for half in (first, "colour" if first == "depth" else "depth"):
        if half == "depth":
            assert np.array_equal(run.ctx.get_depth_buffer(), want[1])
        else:
            assert scenes.bits_equal(run.ctx.get_buffer_numpy(), want[0])
    assert run.counts() == (3, 6, 0, 16), run.counts()


@pytest.mark.parametrize("depth", [ZW, ZT])
def test_a_second_batch(gpu, oracle, depth):
    run = pending(F)
    if depth == ZT:
        run.ctx.set_force_ordered_raster(True)
    D._second_batch(depth)(run.ctx)
    run.ctx.set_force_ordered_raster(False)
    assert run.counts() == (3, 5, 0, 16), run.counts()
    run.check_buffers(D.want_after(F, "batch " + ("zt" if depth == ZT else "zw"), D._second_batch(depth)), F, "batch")


@pytest.mark.parametrize("recorded", [False, True])
def test_a_rectangle(gpu, oracle, recorded):
    run = pending(F)
    if recorded:
        run.ctx.begin_commands()
    run.ctx.draw_rect(*D.RECT)
    if recorded:
        assert run.counts() == (3, 4, 0, 8), run.counts()   # (queued: nothing has used the buffer yet)
        run.ctx.end_commands()
    assert run.counts() == (3, 5, 0, 16), run.counts()
    run.check_buffers(D.want_after(F, "rect", lambda t: t.draw_rect(*D.RECT)), F, "rectangle")
    assert run.counts() == (3, 6, 0, 16), run.counts()


def test_set_pixel_and_apply_pixel(gpu, oracle):
    run = pending(F)
    D._pixels(run.ctx)
    assert run.counts() == (3, 5, 0, 16), run.counts()
    run.check_buffers(D.want_after(F, "pixels", D._pixels), F, "pixels")


def test_a_texture_from_the_frame(gpu, oracle):
    """The deferred record frame as a texture, drawn into a second context."""
    def through(fac, ctx):
        tex = ctx.as_texure()
        c2 = fac.context(200, 120, False)
        c2.set_color(0.0, 0.0, 0.0, 0.0)
        c2.draw_texture(tex, 10, 5, 170, 100)
        return c2.get_buffer_numpy()
    run = pending(F)
    got = through(gpu, run.ctx)
    assert run.counts() == (3, 5, 0, 16), run.counts()
    xy, z, c = L._mesh(F.mesh)
    ora = scenes.OracleFactory().context(W, H, False)
    F.issue(ora, lambda t: t.draw_triangles(xy, c, z=z))
    want = through(scenes.OracleFactory(), ora)
    assert scenes.bits_equal(got, want), scenes.first_mismatch(got, want)
    run.check(F)
    assert run.counts() == (3, 6, 0, 16), run.counts()


@pytest.mark.parametrize("which", ["colour", "depth"])
def test_a_clear_then_a_draw(gpu, oracle, which):
    def ops(ctx):
        if which == "colour":
            ctx.set_color(0.4, 0.4, 0.4, 0.4)
        else:
            ctx.clear_depth(0xFFFFFFFF)
        D._second_batch(ZW)(ctx)
    run = pending(F)
    ops(run.ctx)
    assert run.counts() == (3, 5, 0, 16), run.counts()     # (the other half alone)
    run.check_buffers(D.want_after(F, which + " clear, batch", ops), F, "clear then batch")


def test_the_next_frame_supersedes(gpu, oracle):
    run = pending(F)
    other = Frame(SMALL, clear=(0.7, 0.7, 0.7, 0.7), ct=(0.5, 0.25, 0.75, 1.0))
    for fr in (other, F, other):
        run.draw(fr, read=False)
    assert run.counts() == (6, 4, 3, 8), run.counts()
    run.check_frame_output(other)
    run.check(other)
    assert run.ctx.key_record_batch_count() == 5


def test_a_resize_drops_the_pending_values(gpu, oracle):
    run = pending(F)
    small = Frame(SMALL, clear=UNI, size=(320, 208))
    run.draw(small)
    assert run.ctx.key_record_totals() is None
    run.draw(F)
    assert run.counts()[:2] == (3, 4), run.counts()
    assert run.repeat(F, RECORDS_AT)[2] == 3               # frame 6 of the new generation: from its own store
    check_totals(run, SMALL)


def test_the_buffer_destroyed_with_a_pending_record_frame(gpu, oracle):
    run = pending(F)
    del run.bufs[F.mesh]               # DestroyTriangleBuffer resolves: the values come from its arrays
    assert run.counts() == (3, 5, 0, 16), run.counts()
    run.check(F)
    changed = Frame("changed", clear=UNI)
    assert run.repeat(changed, RECORDS_AT + 3)[2] > 2      # another buffer: a generation and a store of its own
    check_totals(run, "changed")


def test_a_second_context_draws_the_buffer_in_between(gpu, oracle):
    a = pending(F)
    b = Run()
    b.bufs = a.bufs
    assert b.repeat(F, RECORDS_AT + 1) == (2, 2, 1)
    a.check(F)
    assert a.counts() == (3, 6, 0, 16), a.counts()
    check_totals(a, SMALL)
    check_totals(b, SMALL)


@pytest.mark.parametrize("switch", ["key_records", "key_index", "key_cache", "warm_binning", "fragments"])
def test_a_switch_between_the_deferred_frame_and_the_read(gpu, oracle, switch):
    run = pending(F)
    if switch == "key_records":
        run.ctx.set_key_records(2)
    elif switch == "key_index":
        run.ctx.set_key_index(2)
    elif switch == "key_cache":
        run.ctx.set_key_cache(2)
    elif switch == "warm_binning":
        run.ctx.set_warm_binning(2)
    else:
        run.ctx.set_fragment_counting(True)
    run.check(F)
    assert run.counts() == (3, 6, 0, 16), run.counts()
    run.draw(F, read=False)
    run.draw(F)
    run.draw(F)
    assert run.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("shard", [(2, 1), (8, 3)])
def test_deferred_shards_with_direct_records(gpu, oracle, shard):
    fr = Frame(BIG, clear=UNI)
    run = pending(fr, shard=shard)
    assert run.ctx.key_index_totals()["direct"] > 0
    run.check(fr)
    run.draw(fr, read=False)
    run.draw(fr, read=False)
    run.check_frame_output(fr)
    run.check(fr)
    assert run.ctx.key_record_batch_count() == 4


def test_deferred_no_test_depth_mode(gpu, oracle):
    fr = Frame(SMALL, clear=UNI, depth=NZ)
    run = pending(fr, halves=1)
    run.check(fr)
    assert run.counts() == (3, 3, 0, 16), run.counts()


@pytest.mark.parametrize("size", [(64, 32), (65, 33)])
def test_deferred_frame_edges(gpu, oracle, size):
    """(The third edge size, (1, 58), has no store: test_frame_edges.)"""
    mesh = ("soup",) + size
    fr = Frame(mesh, clear=UNI, size=size)
    run = pending(fr, size=size)
    run.check(fr)


# ---- lifetime and invalidation ----------------------------------------------------------

def test_a_transform_change_starts_a_new_generation(gpu, oracle):
    run = started(Frame(SMALL))
    run.draw(Frame(SMALL, move=(0.4, 0.3)))                # loose: binned under the schedule, the generation stays
    assert run.recs[-1] == 1, run.recs
    run.repeat(Frame(SMALL), 3)
    assert run.recs[-1] > 1, run.recs                      # ... and its records are used again
    moved = Frame(SMALL, move=(40.0, 30.0))                # another binning key: a new generation
    run.draw(moved)
    r0 = run.recs[-1]
    assert run.ctx.key_record_totals() is None
    run.repeat(moved, RECORDS_AT + 2)
    assert run.recs[-1] > r0, run.recs                     # which built its own records under its transform ...
    assert run.ctx.key_record_totals() is not None
    run.draw(Frame(SMALL))                                 # ... and the first transform's frame is exact again


def test_resize_and_back(gpu, oracle):
    run = started(Frame(SMALL))
    small = Frame(SMALL, size=(320, 208))
    run.draw(small)
    assert run.ctx.key_record_totals() is None and run.recs[-1] == 1
    assert run.repeat(small, RECORDS_AT - 1)[2] == 1 and run.repeat(small, 1)[2] == 2, run.recs
    check_totals(run, SMALL, (320, 208))
    assert run.repeat(Frame(SMALL), RECORDS_AT)[2] == 2 and run.repeat(Frame(SMALL), 1)[2] == 3, run.recs
    check_totals(run, SMALL)
    assert run.ctx.warm_failure_count() == 0


def test_a_shard_change_starts_a_new_generation(gpu, oracle):
    run = started(Frame(BIG), shard=(2, 0))
    check_totals(run, BIG)
    run.ctx.set_shard(2, 1)
    run.shard = (2, 1)
    run.draw(Frame(BIG))
    assert run.ctx.key_record_totals() is None and run.recs[-1] == 1
    assert run.repeat(Frame(BIG), RECORDS_AT)[2] == 2, run.recs
    check_totals(run, BIG)
    assert run.ctx.warm_failure_count() == 0


def test_a_second_context_on_the_same_buffer(gpu, oracle):
    a, b = Run(), Run()
    b.bufs = a.bufs
    for _ in range(8):
        a.draw(Frame(SMALL))
        b.draw(Frame(SMALL))
    assert a.recs == b.recs == [0] * RECORDS_AT + [1, 2], (a.recs, b.recs)
    check_totals(a, SMALL)
    check_totals(b, SMALL)


def test_switches(gpu, oracle):
    A = Frame(_winners(561))
    run = started(A)
    run.ctx.set_key_records(2)                     # off: k_keys_idx; the store is kept
    assert run.repeat(A, 2) == (4, 4, 1), (run.indexed, run.recs)
    assert run.ctx.key_record_totals() is not None
    run.ctx.set_key_records(0)                     # resumes at once
    assert run.repeat(A, 2) == (6, 6, 3), (run.indexed, run.recs)
    run.ctx.set_key_index(2)                       # k_keys: neither indexed nor from the records
    assert run.repeat(A, 2) == (8, 6, 3), (run.indexed, run.recs)
    run.ctx.set_key_index(0)
    assert run.repeat(A, 2) == (10, 8, 5), (run.indexed, run.recs)
    # the switch off from the start: the store is built all the same, one indexed frame later
    run2 = Run()
    run2.ctx.set_key_records(2)
    assert run2.repeat(A, RECORDS_AT + 1) == (2, 2, 0)
    assert run2.ctx.key_record_totals() == run.ctx.key_record_totals()
    run2.ctx.set_key_records(0)
    assert run2.repeat(A, 2) == (4, 4, 2), (run2.indexed, run2.recs)
    # the index off while the generation is young: the store is built by the first indexed frame after
    run3 = Run()
    run3.ctx.set_key_index(2)
    assert run3.repeat(A, RECORDS_AT + 1) == (2, 0, 0)
    assert run3.ctx.key_record_totals() is None
    run3.ctx.set_key_index(0)
    assert run3.repeat(A, 2) == (4, 2, 1), (run3.indexed, run3.recs)
    assert run.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("mesh", [("flat",) + SMALL])
def test_a_flat_buffer_never_reaches_the_records(gpu, oracle, mesh):
    run = Run()
    assert run.repeat(Frame(mesh), 8) == (3, 0, 0)
    assert run.ctx.key_record_totals() is None
    assert run.ctx.warm_failure_count() == 0


def test_a_textured_buffer_never_reaches_the_records(gpu, oracle):
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    import bilinear_ref as B
    import textured_ref as T
    b = B.soup_batches("opaque", False)[0]
    tex = T.texture_rgb()
    gtex = gpu.texture(tex)
    buf = R.TriangleBuffer(b["xy"], uv=b["uv"], z=b["z"])
    ctx = gpu.context(B.W, B.H, False)
    ctx.set_warm_binning(1)
    ctx.set_transform(*b["m"])
    ctx.set_color_transform(*b["ct"])
    want = B.expected_payload(B.W, B.H, False, B.BG, "zw", B.FAR, [dict(b, tex=tex)], filt=0)
    for k in range(8):
        ctx.set_color(*B.BG)
        T._set_depth_mode(ctx, "zw")
        ctx.clear_depth(B.FAR)
        ctx.set_triangle_texture_filter(0)
        ctx.draw_triangle_buffer(buf, gtex)
        got = (ctx.get_buffer_numpy(), ctx.get_depth_buffer())
        assert scenes.bits_equal(got[0], want[0]), (k, scenes.first_mismatch(got[0], want[0]))
        assert np.array_equal(got[1], want[1]), (k, "depth")
    assert ctx.key_cached_batch_count() == 3 and ctx.key_record_batch_count() == 0
    assert ctx.key_record_totals() is None


def test_a_store_over_the_cap_is_not_built(gpu, oracle):
    """One triangle per pixel of a 64 x 32 frame: 2048 records, 256 KB against a
    48 KB framebuffer (test_key_records_ref).  The generation stays on
    k_keys_idx, every frame exact; SetKeyRecords changes nothing."""
    name = ("pixels",) + OVER
    L._MESH[name] = KR.pixel_triangles(OVER)
    from libnativecpurenderer_amd import _lib
    fr = Frame(name, size=OVER)
    run = Run(size=OVER)
    _lib.clear_error()                             # (the error string is the process's: an earlier test's may stand)
    assert run.repeat(fr, 9) == (4, 4, 0), (run.cached, run.indexed, run.recs)
    assert run.ctx.key_record_totals() is None
    assert run.ctx.key_index_totals()["direct"] > 0
    assert _lib.last_error() == ""                 # nothing latched: over the cap is no error
    assert run.ctx.warm_failure_count() == 0


# ---- the 512-thread instances -----------------------------------------------------------

WIDE_CASES = ("test_stage_sequence or test_record_boundary or test_the_densest_tile or test_frame_edges "
              "or test_readback_of_a_deferred_record_frame or test_deferred_shards_with_direct_records "
              "or test_frame_output_of_a_record_frame or test_deferred_frame_edges or test_a_one_pixel_wide_frame")


def test_the_wide_instances(gpu):
    """NR_KEYS_WIDE=1: every batch shaded from the key cache runs its 512-thread
    instance.  The variable is read once per process: a child runs the cases."""
    env = dict(os.environ, NR_KEYS_WIDE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k", WIDE_CASES],
                       env=env, capture_output=True, text=True, timeout=120, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]

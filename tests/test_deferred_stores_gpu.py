"""Deferred stores (a cached Gouraud TriangleBuffer draw that writes the frame
output itself leaves the cached tiles' f64 framebuffer values and depths
pending -- k_keys_idx' frame-only instance -- until something uses the buffers:
the resolve kernel) against the CPU oracle: the frame output of the deferred
frame, and the f64 framebuffer and the u32 depth after every road out of the
pending state, bit for bit.

Frames, meshes, the oracle cache and the counting context are those of
tests/test_key_index_gpu.py and tests/test_key_cache_gpu.py: with a readback
after each frame, frame 5 is the first cached and indexed one.  Every case but
the automatic-mode ones sets SetDeferredStores(1) and gathers the frame output
once at the start, so under a uniform clear every cached frame defers --
frame 5 too, whose readback resolves it.

The counts (GetDeferredStoreCounts: deferred batches, resolve launches, records
superseded with their values never needed, the rule's threshold) are written
down from the host code, not from a run:
  * a deferred LESS + write frame read back colour first, then depth, launches
    two resolves (one per half); a no-test frame has no depth half: one;
  * something that needs both halves at once (a batch: frame_params; the
    buffer destroyed) launches one;
  * the first use of a record that had deferred doubles the threshold (2, 4,
    ...), in every mode;
  * a record ends superseded when the next frame's clears have overwritten
    both halves before anything used either."""
import functools

import numpy as np
import pytest

import scenes
import test_key_index_gpu as I
import test_visible_list_gpu as L

pytestmark = pytest.mark.gpu

W, H = L.W, L.H
SMALL, BIG = L.SMALL, L.BIG
NONUNI, UNI = L.NONUNI, L.UNI
ZW, NZ, ZT = L.ZW, L.NZ, L.ZT
Frame = I.Frame
RECT = (37.0, 21.0, 140.0, 90.0, 0.5, 0.25, 0.75, 0.5)


class Run(I.Run):
    """I.Run with the deferral mode set and the frame output on."""

    def __init__(self, shard=None, size=(W, H), mode=1, fmt="rgb", gather=True):
        super().__init__(shard, size)
        self.fmt = fmt
        self.ctx.set_deferred_stores(mode)
        self.ctx.set_frame_format(fmt)
        if gather:
            self.ctx.gather_frame_u8()

    def counts(self):
        c = self.ctx.deferred_store_counts()
        return c["deferred"], c["resolves"], c["superseded"], c["threshold"]

    def rows(self, fr):
        from libnativecpurenderer_amd import sharding
        return slice(None) if self.shard is None else sharding.owned_rows(fr.size[1], *self.shard)

    def check_frame_output(self, fr):
        """The frame output of the frame just drawn (it resolves nothing)."""
        before = self.counts()
        self.ctx.gather_frame_u8()
        out, u8 = self.ctx.get_frame_u8(), L._want(fr)["u8"]
        if self.fmt == "yuv420p":
            assert self.shard is None
            assert np.array_equal(out, scenes.yuv420p(u8)), "yuv420p frame output"
        else:
            rows = self.rows(fr)
            assert np.array_equal(out[rows], u8[rows]), "u8 frame output"
        assert self.counts() == before, (before, self.counts())

    def check_buffers(self, want, fr, what=""):
        rows = self.rows(fr)
        g = self.ctx.get_buffer_numpy()[rows]
        assert scenes.bits_equal(g, want[0][rows]), f"{what}: {scenes.first_mismatch(g, want[0][rows])}"
        assert np.array_equal(self.ctx.get_depth_buffer()[rows], want[1][rows]), f"{what}: depth"


def pending(fr, shard=None, size=(W, H), fmt="rgb", halves=2):
    """A Run with one deferred frame of `fr` pending, its frame output checked.
    halves: resolve launches a colour-then-depth readback costs (2; 1 without a
    depth test).  Frame 5, the first cached one, deferred and was read back."""
    run = Run(shard, size, fmt=fmt)
    assert run.repeat(fr, 6) == (1, 1), (run.cached, run.indexed)
    assert run.counts() == (1, halves, 0, 4), run.counts()
    run.draw(fr, read=False)
    assert run.counts() == (2, halves, 0, 4), run.counts()
    run.check_frame_output(fr)
    return run


_AFTER = {}


def want_after(fr, name, ops):
    """The oracle's (f64, depth) after frame `fr` and then ops(ctx)."""
    key = (fr.key(), name)
    if key not in _AFTER:
        xy, z, c = L._mesh(fr.mesh)
        ctx = scenes.OracleFactory().context(*fr.size, False)
        fr.issue(ctx, lambda t: t.draw_triangles(xy, c, z=z))
        ops(ctx)
        _AFTER[key] = (ctx.get_buffer_numpy(), ctx.get_depth_buffer())
    return _AFTER[key]


def want_of(fr):
    return L._want(fr)["f64"], L._want(fr)["depth"]


F = Frame(SMALL, clear=UNI)


# ---- roads out of the pending state -------------------------------------------------

@pytest.mark.parametrize("fmt", ["rgb", "yuv420p"])
def test_readback_of_both_buffers(gpu, oracle, fmt):
    run = pending(F, fmt=fmt)
    run.check(F)
    assert run.counts() == (2, 4, 0, 8), run.counts()
    run.check(F)                       # (nothing is pending any more)
    assert run.counts() == (2, 4, 0, 8), run.counts()
    run.draw(F)                        # and the next frame defers and resolves again
    assert run.counts() == (3, 6, 0, 16), run.counts()


def test_depth_first_then_colour(gpu, oracle):
    run = pending(F)
    want = want_of(F)
    assert np.array_equal(run.ctx.get_depth_buffer(), want[1])
    assert run.counts() == (2, 3, 0, 8), run.counts()
    assert scenes.bits_equal(run.ctx.get_buffer_numpy(), want[0])
    assert run.counts() == (2, 4, 0, 8), run.counts()
    run.check(F)


def test_colour_first_then_depth(gpu, oracle):
    run = pending(F)
    want = want_of(F)
    assert scenes.bits_equal(run.ctx.get_buffer_numpy(), want[0])
    assert run.counts() == (2, 3, 0, 8), run.counts()
    assert np.array_equal(run.ctx.get_depth_buffer(), want[1])
    assert run.counts() == (2, 4, 0, 8), run.counts()


def _second_batch(depth):
    def ops(ctx):
        xy, z, c = L._mesh("other")
        ctx.set_depth_state(*depth)
        ctx.draw_triangles(xy, c, z=z)
    return ops


def test_a_second_batch_from_host_arrays(gpu, oracle):
    run = pending(F)
    _second_batch(ZW)(run.ctx)
    assert run.counts() == (2, 3, 0, 8), run.counts()      # (both halves, one launch)
    run.check_buffers(want_after(F, "batch zw", _second_batch(ZW)), F, "second batch")
    assert run.counts() == (2, 3, 0, 8), run.counts()


def test_the_ordered_raster_tests_against_the_deferred_depth(gpu, oracle):
    """LESS without write: the ordered raster, whose every fragment is tested
    against the depths the deferred frame left pending."""
    run = pending(F)
    run.ctx.set_force_ordered_raster(True)
    _second_batch(ZT)(run.ctx)
    run.ctx.set_force_ordered_raster(False)
    assert run.ctx.last_raster_path() == "ordered"
    assert run.counts() == (2, 3, 0, 8), run.counts()
    run.check_buffers(want_after(F, "batch zt", _second_batch(ZT)), F, "ordered batch")


@pytest.mark.parametrize("recorded", [False, True])
def test_a_rectangle(gpu, oracle, recorded):
    run = pending(F)
    if recorded:
        run.ctx.begin_commands()
    run.ctx.draw_rect(*RECT)
    if recorded:
        assert run.counts() == (2, 2, 0, 4), run.counts()   # (queued: nothing has used the buffer yet)
        run.ctx.end_commands()
    assert run.counts() == (2, 3, 0, 8), run.counts()
    run.check_buffers(want_after(F, "rect", lambda t: t.draw_rect(*RECT)), F, "rectangle")
    assert run.counts() == (2, 4, 0, 8), run.counts()


def _pixels(ctx):
    ctx.set_pixel(5, 7, 0.25, 0.5, 0.75, 1.0)
    ctx.apply_pixel(300, 200, 0.9, 0.1, 0.3, 0.5)
    ctx.apply_pixel(301, 200, 0.2, 0.8, 0.4, 0.25)


def test_set_pixel_and_apply_pixel(gpu, oracle):
    run = pending(F)
    _pixels(run.ctx)
    assert run.counts() == (2, 3, 0, 8), run.counts()
    run.check_buffers(want_after(F, "pixels", _pixels), F, "pixels")


def test_a_texture_from_the_frame(gpu, oracle):
    """The frame as a texture, drawn into a second context."""
    def through(fac, ctx):
        tex = ctx.as_texure()
        c2 = fac.context(200, 120, False)
        c2.set_color(0.0, 0.0, 0.0, 0.0)
        c2.draw_texture(tex, 10, 5, 170, 100)
        return c2.get_buffer_numpy()
    run = pending(F)
    got = through(gpu, run.ctx)
    assert run.counts() == (2, 3, 0, 8), run.counts()
    xy, z, c = L._mesh(F.mesh)
    ora = scenes.OracleFactory().context(W, H, False)
    F.issue(ora, lambda t: t.draw_triangles(xy, c, z=z))
    want = through(scenes.OracleFactory(), ora)
    assert scenes.bits_equal(got, want), scenes.first_mismatch(got, want)
    run.check(F)
    assert run.counts() == (2, 4, 0, 8), run.counts()


def test_a_colour_clear_then_a_draw_against_the_deferred_depth(gpu, oracle):
    def ops(ctx):
        ctx.set_color(0.4, 0.4, 0.4, 0.4)
        _second_batch(ZW)(ctx)
    run = pending(F)
    ops(run.ctx)
    assert run.counts() == (2, 3, 0, 8), run.counts()      # (the depth half alone; the colour half was superseded)
    run.check_buffers(want_after(F, "colour clear, batch", ops), F, "colour clear then batch")
    assert run.counts() == (2, 3, 0, 8), run.counts()


def test_a_depth_clear_then_a_draw(gpu, oracle):
    def ops(ctx):
        ctx.clear_depth(0xFFFFFFFF)
        _second_batch(ZW)(ctx)
    run = pending(F)
    ops(run.ctx)
    assert run.counts() == (2, 3, 0, 8), run.counts()      # (the colour half alone)
    run.check_buffers(want_after(F, "depth clear, batch", ops), F, "depth clear then batch")
    assert run.counts() == (2, 3, 0, 8), run.counts()


def test_the_next_frame_supersedes(gpu, oracle):
    run = pending(F)
    run.draw(F, read=False)
    assert run.counts() == (3, 2, 1, 4), run.counts()      # no resolve: both halves overwritten by the clears
    run.check_frame_output(F)
    run.check(F)
    assert run.counts() == (3, 4, 1, 8), run.counts()


def test_four_deferred_frames_unread_then_a_read(gpu, oracle):
    run = pending(F)
    other = Frame(SMALL, clear=(0.7, 0.7, 0.7, 0.7), ct=(0.5, 0.25, 0.75, 1.0))
    for fr in (other, F, other):
        run.draw(fr, read=False)
    assert run.counts() == (5, 2, 3, 4), run.counts()
    run.check_frame_output(other)
    run.check(other)                   # (the last frame's state, not an earlier one's)
    assert run.counts() == (5, 4, 3, 8), run.counts()


def test_a_resize_drops_the_pending_values(gpu, oracle):
    run = pending(F)
    small = Frame(SMALL, clear=UNI, size=(320, 208))
    run.draw(small)                    # (a new generation: cold)
    assert run.counts() == (2, 2, 0, 4), run.counts()
    run.draw(F)                        # (and another: its frame 0)
    assert run.counts() == (2, 2, 0, 4), run.counts()
    assert run.repeat(F, 5)[1] == 3                        # its frame 5, the first indexed one of the new generation ...
    assert run.counts() == (3, 4, 0, 8), run.counts()      # ... deferred, and was read back


def test_the_buffer_destroyed_then_a_readback(gpu, oracle):
    run = pending(F)
    del run.bufs[F.mesh]               # DestroyTriangleBuffer: the pending values are formed from its arrays
    assert run.counts() == (2, 3, 0, 8), run.counts()
    run.check(F)
    assert run.counts() == (2, 3, 0, 8), run.counts()


def test_the_buffer_destroyed_and_made_again(gpu, oracle):
    """Another buffer of the same size right after the destroy (it may well
    get the same memory): the pending frame is the first buffer's."""
    run = pending(F)
    del run.bufs[F.mesh]
    changed = Frame("changed", clear=UNI)
    run.buffer("changed")
    run.check(F)
    run.draw(changed)
    run.draw(F)
    assert run.counts()[0] == 2, run.counts()


def test_a_second_context_draws_the_buffer_in_between(gpu, oracle):
    a = pending(F)
    b = Run()
    b.bufs = a.bufs
    b.draw(F)
    b.draw(Frame(SMALL))
    assert a.counts() == (2, 2, 0, 4), a.counts()
    a.check(F)
    assert a.counts() == (2, 4, 0, 8), a.counts()
    assert b.counts() == (0, 0, 0, 2), b.counts()


@pytest.mark.parametrize("switch", ["key_index", "key_cache", "warm_binning", "fragments"])
def test_a_switch_between_the_deferred_frame_and_the_read(gpu, oracle, switch):
    run = pending(F)
    if switch == "key_index":
        run.ctx.set_key_index(2)
    elif switch == "key_cache":
        run.ctx.set_key_cache(2)
    elif switch == "warm_binning":
        run.ctx.set_warm_binning(2)
    else:
        run.ctx.set_fragment_counting(True)
    run.check(F)
    assert run.counts() == (2, 4, 0, 8), run.counts()
    run.draw(F, read=False)            # pending again unless the switch keeps the draw off k_keys_idx
    run.draw(F)
    run.draw(F)
    assert run.ctx.warm_failure_count() == 0


# ---- variants -------------------------------------------------------------------------

@pytest.mark.parametrize("shard", [(2, 1), (8, 3)])
def test_shards(gpu, oracle, shard):
    run = pending(F, shard=shard)
    run.check(F)
    assert run.counts() == (2, 4, 0, 8), run.counts()
    run.draw(F, read=False)
    run.draw(F, read=False)
    run.check_frame_output(F)
    run.check(F)
    assert run.counts() == (4, 6, 1, 16), run.counts()


def test_rgba_context(gpu, oracle):
    """Four doubles per pixel, a non-zero uniform clear."""
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    xy, z, c = L._mesh(SMALL)
    fr = Frame(SMALL, clear=(0.6, 0.6, 0.6, 0.6))
    ora = scenes.OracleFactory().context(W, H, True)
    fr.issue(ora, lambda t: t.draw_triangles(xy, c, z=z))
    want = (ora.get_buffer_numpy(), ora.get_depth_buffer(), ora.get_buffer_as_uint8_numpy())
    ctx = R.RenderContext(W, H, True)
    ctx.set_warm_binning(1)
    ctx.set_deferred_stores(1)
    ctx.gather_frame_u8()
    buf = R.TriangleBuffer(xy, c, z=z, gouraud=True)
    for k in range(8):
        fr.issue(ctx, lambda t: t.draw_triangle_buffer(buf))
        if k == 6:
            continue                   # (unread: superseded by frame 7)
        ctx.gather_frame_u8()
        if k >= 5:
            assert np.array_equal(ctx.get_frame_u8(), want[2]), k
        g = ctx.get_buffer_numpy()
        assert scenes.bits_equal(g, want[0]), (k, scenes.first_mismatch(g, want[0]))
        assert np.array_equal(ctx.get_depth_buffer(), want[1]), k
    assert ctx.key_indexed_batch_count() == 3
    c = ctx.deferred_store_counts()
    assert (c["deferred"], c["resolves"], c["superseded"], c["threshold"]) == (3, 4, 1, 8), c


def test_a_colour_transform(gpu, oracle):
    fr = Frame(SMALL, clear=UNI, ct=(0.5, 0.25, 0.75, 1.0))
    run = pending(fr)
    run.check(fr)
    assert run.counts() == (2, 4, 0, 8), run.counts()


@pytest.mark.parametrize("fmt", ["rgb", "yuv420p"])
def test_no_test_depth_mode(gpu, oracle, fmt):
    """No depth test: a record has a colour half alone."""
    fr = Frame(BIG, clear=UNI, depth=NZ)
    run = pending(fr, fmt=fmt, halves=1)
    run.check(fr)
    assert run.counts() == (2, 2, 0, 8), run.counts()
    run.draw(fr, read=False)
    run.draw(fr, read=False)
    assert run.counts() == (4, 2, 1, 8), run.counts()
    run.check(fr)
    assert run.counts() == (4, 3, 1, 16), run.counts()


# ---- edges ----------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(64, 32), (65, 33), (1, 58)])
def test_frame_edges(gpu, oracle, size):
    mesh = ("soup",) + size
    fr = Frame(mesh, clear=UNI, size=size)
    run = pending(fr, size=size)
    run.check(fr)
    assert run.counts() == (2, 4, 0, 8), run.counts()


@pytest.mark.parametrize("fmt", ["rgb", "yuv420p"])
def test_direct_pixels(gpu, oracle, fmt):
    """BIG: dense tiles with more than KI_RT winners, so some pixels load
    their record directly, their id from the slot's key."""
    fr = Frame(BIG, clear=UNI)
    run = pending(fr, fmt=fmt)
    assert run.ctx.key_index_totals()["direct"] > 0
    run.check(fr)
    assert run.counts() == (2, 4, 0, 8), run.counts()


def test_staged_record_boundary(gpu, oracle):
    """The 281-winner tile of the key-index tests: one winner past KI_RT."""
    n = 281
    tile, win = I._dense_tile()
    name = ("winners", n)
    xy, z, c = L._mesh(BIG)
    L._MESH[name] = tuple(np.ascontiguousarray(a[win[:n]]) for a in (xy, z, c))
    fr = Frame(name, clear=UNI)
    run = pending(fr)
    assert run.ctx.key_index_totals()["direct"] > 0
    run.check(fr)
    assert run.counts() == (2, 4, 0, 8), run.counts()


# ---- never deferred -------------------------------------------------------------------

def _never(run, fr):
    run.repeat(fr, 6)
    for _ in range(4):
        run.draw(fr, read=False)
    run.check(fr)
    return run.counts()


def test_no_frame_output_requested(gpu, oracle):
    run = Run(gather=False)
    assert _never(run, F) == (0, 0, 3, 2), run.counts()
    assert run.indexed[-1] == 1 and run.ctx.key_indexed_batch_count() == 5


def test_a_non_uniform_clear(gpu, oracle):
    run = Run()
    assert _never(run, Frame(SMALL, clear=NONUNI)) == (0, 0, 3, 2), run.counts()
    assert run.ctx.key_indexed_batch_count() == 5


def test_a_flat_buffer_runs_k_keys(gpu, oracle):
    run = Run()
    assert _never(run, Frame(("flat",) + SMALL, clear=UNI)) == (0, 0, 0, 2), run.counts()   # (no record at all)
    assert run.ctx.key_cached_batch_count() == 5 and run.ctx.key_indexed_batch_count() == 0


def test_mode_off(gpu, oracle):
    run = Run(mode=2)
    assert _never(run, F) == (0, 0, 3, 2), run.counts()
    assert run.ctx.key_indexed_batch_count() == 5


# ---- automatic mode -------------------------------------------------------------------

def test_automatic_mode(gpu, oracle):
    """Frames read back never defer (every record is needed: the run stays 0).
    Unread, cleared frames: the first stores (the record before it was read),
    the second stores (a run of 1), the third cached frame on defers (a run of
    2, the threshold).  One read of a deferred frame: two resolves, threshold 4,
    and the next deferral comes only after four superseded records."""
    run = Run(mode=0)
    assert run.repeat(F, 8) == (3, 3)
    assert run.counts() == (0, 0, 0, 2), run.counts()
    want = [(0, 0, 0, 2), (0, 0, 1, 2), (1, 0, 2, 2), (2, 0, 3, 2)]
    for k, w in enumerate(want):
        run.draw(F, read=False)
        assert run.counts() == w, (k, run.counts())
    run.check_frame_output(F)
    run.check(F)
    assert run.counts() == (2, 2, 3, 4), run.counts()
    want = [(2, 2, 3, 4), (2, 2, 4, 4), (2, 2, 5, 4), (2, 2, 6, 4), (3, 2, 7, 4), (4, 2, 8, 4)]
    for k, w in enumerate(want):
        run.draw(F, read=False)
        assert run.counts() == w, (k, run.counts())
    run.check_frame_output(F)
    run.check(F)
    assert run.counts() == (4, 4, 8, 8), run.counts()
    assert run.ctx.warm_failure_count() == 0

"""The key index (a cached Gouraud TriangleBuffer draw shaded by k_keys_idx from
the per-tile winner index that k_key_index builds right after the key cache's
capture frame) against the CPU oracle: every frame bit for bit on the f64
framebuffer and the u32 depth, the frame output in one RGB and one YUV420P case.

Frames, meshes, the oracle cache and the counting context are those of
tests/test_visible_list_gpu.py and tests/test_key_cache_gpu.py.  The index adds
no stage: with a readback after each frame, frame 4 is the capture frame (the
index is enqueued right behind it) and frame 5 the first cached -- and, for a
Gouraud buffer, the first indexed -- one.  GetKeyIndexedBatchCount moves on
indexed frames only, and an indexed batch counts as the cached (pruned, reused,
warm) batch it is.

GetKeyIndexTotals is checked against tests/key_index_ref.py, which numbers each
tile's winners from the oracle's frame the way k_key_index does (by their first
pixel), so the staged winners and the directly loaded pixels are both exact.
tests/test_key_index_ref.py asserts what makes these cases reach both paths:
SMALL stays under KI_RT winners in every tile, BIG exceeds it in most."""
import functools

import numpy as np
import pytest

import bilinear_ref as B
import key_index_ref as I
import scenes
import test_key_cache_gpu as C
import test_visible_list_gpu as L
import textured_ref as T

pytestmark = pytest.mark.gpu

W, H = L.W, L.H
SMALL, BIG = L.SMALL, L.BIG
NONUNI, UNI = L.NONUNI, L.UNI
ZW, NZ, ZT = L.ZW, L.NZ, L.ZT
Frame = C.Frame


class Run(C.Run):
    def __init__(self, shard=None, size=(W, H)):
        super().__init__(shard, size)
        self.indexed = []

    def draw(self, fr, read=True):
        super().draw(fr, read)
        if read:
            self.indexed.append(self.ctx.key_indexed_batch_count())

    def repeat(self, fr, n):
        """-> (cached, indexed) batch counts after n more checked frames."""
        super().repeat(fr, n)
        return self.cached[-1], self.indexed[-1]


@functools.lru_cache(maxsize=None)
def _scene(mesh, size=(W, H), depth=ZW):
    """The winner image of a mesh's frame on the CPU."""
    xy, z, _ = L._mesh(mesh)
    return I.winner_ids(xy, z, size, depth)


def _want_totals(mesh, size=(W, H), shard=None, depth=ZW):
    return I.totals(_scene(mesh, size, depth), size, C._totals(mesh, size, shard, depth)["tiles"], shard)


def check_totals(run, mesh, size=(W, H), depth=ZW):
    want, got = _want_totals(mesh, size, run.shard, depth), run.ctx.key_index_totals()
    print(f"key index {got}")
    assert got == want, (got, want)
    return got


@pytest.mark.parametrize("mesh", [SMALL, BIG])
@pytest.mark.parametrize("shard", [None, (2, 1), (8, 3)])
def test_stage_sequence(gpu, oracle, shard, mesh):
    run = Run(shard)
    run.repeat(Frame(mesh), 8)
    assert run.cached == [0, 0, 0, 0, 0, 1, 2, 3], run.cached
    assert run.indexed == run.cached, run.indexed
    t = check_totals(run, mesh)
    assert t["tiles"] > 0 and t["staged"] > 0
    assert (t["direct"] > 0) == (mesh == BIG), t
    assert run.ctx.warm_failure_count() == 0


@functools.lru_cache(maxsize=None)
def _dense_tile():
    """The densest tile of BIG and its winners (0-based triangle numbers)."""
    ids = _scene(BIG)
    distinct, _ = I.tile_index(ids, (W, H))
    t = int(np.argmax(distinct))
    tx = (W + I.TW - 1) // I.TW
    y0, x0 = (t // tx) * I.TH, (t % tx) * I.TW
    w = np.unique(ids[y0:y0 + I.TH, x0:x0 + I.TW])
    return t, w[w > 0] - 1


@pytest.mark.parametrize("n", [279, 280, 281, 560])
def test_staged_record_boundary(gpu, oracle, n):
    """Exactly n winners in one tile: a winner stays one when other triangles
    are removed, so n of a dense tile's winners leave that tile n distinct."""
    tile, win = _dense_tile()
    assert len(win) >= 560
    name = ("winners", n)
    xy, z, c = L._mesh(BIG)
    L._MESH[name] = tuple(np.ascontiguousarray(a[win[:n]]) for a in (xy, z, c))
    distinct, direct = I.tile_index(_scene(name), (W, H))
    assert distinct[tile] == n == distinct.max()
    run = Run()
    assert run.repeat(Frame(name), 6) == (1, 1)
    t = check_totals(run, name)
    assert t["staged"] == np.minimum(distinct, I.KI_RT).sum()   # (that tile's count capped at KI_RT)
    assert (t["staged"] < distinct.sum()) == (n > I.KI_RT)
    assert (t["direct"] > 0) == (n > I.KI_RT), t
    assert run.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("size", [(64, 32), (65, 33), (1, 58)])
def test_frame_edges(gpu, oracle, size):
    mesh = ("soup",) + size
    run = Run(size=size)
    assert run.repeat(Frame(mesh, size=size), 7) == (2, 2)
    check_totals(run, mesh, size)
    assert run.ctx.warm_failure_count() == 0


def test_rgba_context(gpu, oracle):
    """A context with an alpha channel (four doubles per pixel)."""
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    xy, z, c = L._mesh(SMALL)
    fr = Frame(SMALL, clear=(0.3, 0.1, 0.2, 0.6))
    ora = scenes.OracleFactory().context(W, H, True)
    fr.issue(ora, lambda t: t.draw_triangles(xy, c, z=z))
    want = (ora.get_buffer_numpy(), ora.get_depth_buffer())
    ctx = R.RenderContext(W, H, True)
    ctx.set_warm_binning(1)
    buf = R.TriangleBuffer(xy, c, z=z, gouraud=True)
    for k in range(7):
        fr.issue(ctx, lambda t: t.draw_triangle_buffer(buf))
        g = ctx.get_buffer_numpy()
        assert scenes.bits_equal(g, want[0]), (k, scenes.first_mismatch(g, want[0]))
        assert np.array_equal(ctx.get_depth_buffer(), want[1]), k
    assert ctx.key_cached_batch_count() == 2 and ctx.key_indexed_batch_count() == 2
    assert ctx.key_index_totals() == _want_totals(SMALL)


def test_live_colour_state(gpu, oracle):
    """Clear colour and colour transform change between indexed frames: each
    is exact and still indexed (nothing colour-side is in the index)."""
    run = Run()
    assert run.repeat(Frame(SMALL), 6) == (1, 1)
    frames = [Frame(SMALL, clear=UNI), Frame(SMALL, ct=(0.5, 0.25, 0.75, 1.0)), Frame(SMALL, clear=(0.9, 0.1, 0.4, 0.3)),
              Frame(SMALL, ct=(0.3, 1.0, 0.6, 1.0), clear=UNI), Frame(SMALL)]
    for k, fr in enumerate(frames):
        run.draw(fr)
        assert run.cached[-1] == run.indexed[-1] == 2 + k, (run.cached, run.indexed)
    assert run.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("mesh", [SMALL, BIG])
@pytest.mark.parametrize("fmt", ["rgb", "yuv420p"])
def test_frame_output_of_an_indexed_frame(gpu, oracle, fmt, mesh):
    """The output format changes between indexed frames; under a uniform clear
    k_keys_idx writes the frame output itself (staged and direct pixels)."""
    run = Run()
    fr = Frame(mesh, clear=UNI)
    assert run.repeat(fr, 6) == (1, 1)
    for f in (fmt, "rgb" if fmt == "yuv420p" else "yuv420p", fmt):
        run.ctx.set_frame_format(f)
        run.ctx.gather_frame_u8()
        run.draw(fr)
        run.ctx.gather_frame_u8()
        out, u8 = run.ctx.get_frame_u8(), L._want(fr)["u8"]
        assert np.array_equal(out, scenes.yuv420p(u8) if f == "yuv420p" else u8), f
    assert run.indexed[-3:] == [2, 3, 4], run.indexed


def test_switches(gpu, oracle):
    run = Run()
    A = Frame(BIG)
    assert run.repeat(A, 6) == (1, 1)
    run.ctx.set_key_index(2)                       # off: k_keys; the index is kept
    assert run.repeat(A, 2) == (3, 1), (run.cached, run.indexed)
    check_totals(run, BIG)
    run.ctx.set_key_index(0)                       # resumes at once
    assert run.repeat(A, 2) == (5, 3), (run.cached, run.indexed)
    run.ctx.set_key_cache(2)                       # the visible list: neither cached nor indexed
    assert run.repeat(A, 2) == (5, 3), (run.cached, run.indexed)
    run.ctx.set_key_cache(0)
    assert run.repeat(A, 2) == (7, 5), (run.cached, run.indexed)
    # the switch off from the start: the index is built with the capture frame all the same
    run2 = Run()
    run2.ctx.set_key_index(2)
    assert run2.repeat(A, 7) == (2, 0)
    check_totals(run2, BIG)
    run2.ctx.set_key_index(0)
    assert run2.repeat(A, 2) == (4, 2), (run2.cached, run2.indexed)
    assert run.ctx.warm_failure_count() == 0 and run2.ctx.warm_failure_count() == 0


def test_ineligible_draws_between_indexed_frames(gpu, oracle):
    """LESS without write and a depth clear to another value: exact, from
    neither the cache nor the index; the next eligible frame is indexed again."""
    run = Run()
    assert run.repeat(Frame(SMALL), 6) == (1, 1)
    c = 1
    for fr in (Frame(SMALL, depth=ZT), Frame(SMALL, zclear=0x80000000)):
        assert run.repeat(fr, 2) == (c, c), (fr.key(), run.cached, run.indexed)
        c += 1
        assert run.repeat(Frame(SMALL), 1) == (c, c), (run.cached, run.indexed)
    assert run.ctx.warm_failure_count() == 0


def test_resize_and_back(gpu, oracle):
    """A resize starts a new generation: its index comes back with its cache,
    at the generation's sixth frame."""
    run = Run()
    assert run.repeat(Frame(SMALL), 6) == (1, 1)
    small = Frame(SMALL, size=(320, 208))
    run.draw(small)
    assert run.ctx.key_index_totals() is None and run.indexed[-1] == 1
    assert run.repeat(small, 4) == (1, 1) and run.repeat(small, 1) == (2, 2), (run.cached, run.indexed)
    check_totals(run, SMALL, (320, 208))
    assert run.repeat(Frame(SMALL), 5) == (2, 2) and run.repeat(Frame(SMALL), 1) == (3, 3), (run.cached, run.indexed)
    check_totals(run, SMALL)
    assert run.ctx.warm_failure_count() == 0


def test_a_shard_change_starts_a_new_generation(gpu, oracle):
    run = Run((2, 0))
    assert run.repeat(Frame(BIG), 7) == (2, 2)
    check_totals(run, BIG)
    run.ctx.set_shard(2, 1)
    run.shard = (2, 1)
    run.draw(Frame(BIG))
    assert run.ctx.key_index_totals() is None and run.indexed[-1] == 2
    assert run.repeat(Frame(BIG), 6) == (4, 4), (run.cached, run.indexed)
    check_totals(run, BIG)
    assert run.ctx.warm_failure_count() == 0


def test_a_second_context_on_the_same_buffer(gpu, oracle):
    """Each context has its own schedule, cache and index of the shared buffer."""
    a, b = Run(), Run()
    b.bufs = a.bufs
    for _ in range(7):
        a.draw(Frame(BIG))
        b.draw(Frame(BIG))
    assert a.indexed == b.indexed == [0, 0, 0, 0, 0, 1, 2], (a.indexed, b.indexed)
    assert a.buffer(BIG) is b.buffer(BIG)
    check_totals(a, BIG)
    check_totals(b, BIG)


def test_no_test_depth_mode(gpu, oracle):
    """No depth test (the highest covering id wins): k_keys_idx' ZMODE 0."""
    run = Run()
    assert run.repeat(Frame(BIG, depth=NZ), 7) == (2, 2)
    check_totals(run, BIG, depth=NZ)
    assert run.ctx.warm_failure_count() == 0


def test_a_flat_buffer_is_cached_but_never_indexed(gpu, oracle):
    run = Run()
    assert run.repeat(Frame(("flat",) + SMALL), 7) == (2, 0)
    assert run.ctx.key_index_totals() is not None   # (the index is the keys': built, not used)
    assert run.ctx.warm_failure_count() == 0


def test_a_textured_buffer_is_cached_but_never_indexed(gpu, oracle):
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    b = B.soup_batches("opaque", False)[0]
    tex = T.texture_rgb()
    gtex = gpu.texture(tex)
    buf = R.TriangleBuffer(b["xy"], uv=b["uv"], z=b["z"])
    ctx = gpu.context(B.W, B.H, False)
    ctx.set_warm_binning(1)
    ctx.set_transform(*b["m"])
    ctx.set_color_transform(*b["ct"])
    want = B.expected_payload(B.W, B.H, False, B.BG, "zw", B.FAR, [dict(b, tex=tex)], filt=0)
    for k in range(7):
        ctx.set_color(*B.BG)
        T._set_depth_mode(ctx, "zw")
        ctx.clear_depth(B.FAR)
        ctx.set_triangle_texture_filter(0)
        ctx.draw_triangle_buffer(buf, gtex)
        got = (ctx.get_buffer_numpy(), ctx.get_depth_buffer())
        assert scenes.bits_equal(got[0], want[0]), (k, scenes.first_mismatch(got[0], want[0]))
        assert np.array_equal(got[1], want[1]), (k, "depth")
    assert ctx.key_cached_batch_count() == 2 and ctx.key_indexed_batch_count() == 0
    assert ctx.warm_failure_count() == 0

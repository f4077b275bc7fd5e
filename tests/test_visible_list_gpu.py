"""The visible list (a reused TriangleBuffer draw rasterised from its kept
pair list without the triangles that won no pixel on the schedule's marking
frame) against the CPU oracle: every frame bit for bit on the f64 framebuffer
and the u32 depth, the frame output in one RGB and one YUV420P case.

What is checked beside exact frames: which batches are rasterised from the
visible list (GetPrunedBatchCount), how many pairs it keeps
(GetVisiblePairCount, against the oracle's winners: tests/visible_ref.py), that
only an eligible frame marks (LESS + write over a pending depth clear to
0xFFFFFFFF, or no depth test), that only draws of the capturing depth mode use
the list, that a split tile keeps a pair per slice, that a list whose binning
failed is never pruned, and that whatever ends the schedule generation ends the
list.

The counts follow from the host code, with a readback after each frame (so
the host has seen the marking frame complete by the next draw): frame 0 bins
cold, frame 1 bins warm (the list), frame 2 reuses it and marks the winners,
frame 3 prunes and is the first rasterised from the visible list.

Every frame clears colour and depth before its draws, so a frame depends only
on its own description: the oracle renders each distinct frame once (_ORACLE)
and the tests share the result."""
import functools

import numpy as np
import pytest

import scenes
import textured_ref as T
import visible_ref as V

pytestmark = pytest.mark.gpu

W, H = 640, 400
SMALL, BIG = (60, 200), (250, 700)   # sphere_mesh rows x cols
NONUNI, UNI = (0.1, 0.2, 0.3, 0.1), (0.2, 0.2, 0.2, 0.2)
ZW, NZ, ZT = (True, True), (False, False), (True, False)   # LESS + write, no test, LESS without write

_MESH = {}
_ORACLE = {}


def _hidden_split(size):
    """400 slivers inside tile 0 (far), then two triangles that cover the
    whole frame (near): the tile is dense enough to be split, and only the two
    covering triangles win a pixel."""
    i = np.arange(400)
    x0, y0 = 5.0 + (i % 40), 3.0 + (i // 40) * 2.5
    sl = np.stack([x0, y0, x0 + 8.0, y0 + 0.7, x0 + 1.0, y0 + 2.2], axis=1)
    w, h = size
    a, b, c, d = (-10.0, -10.0), (w + 10.0, -10.0), (w + 10.0, h + 10.0), (-10.0, h + 10.0)
    cover = np.array([a + b + c, a + c + d])
    xy = np.concatenate([sl, cover])
    z = np.concatenate([np.full((400, 3), 0.9), np.full((2, 3), 0.1)])
    col = scenes.rng(11).uniform(0, 1, size=(402, 3, 4))
    col[..., 3] = 1.0
    return np.ascontiguousarray(xy), z, col.reshape(402, 12)


def _mesh(name):
    """Triangle arrays (xy, z, colours) by name: a sphere mesh (rows, cols),
    ("flat", rows, cols) the same with one colour per triangle, "other" (a
    second opaque soup), "changed" (as many triangles as SMALL, other content),
    ("soup", w, h) a small soup over a w x h frame, ("hidden", w, h)."""
    if name not in _MESH:
        if name == "other":
            _MESH[name] = scenes.triangle_soup(3000, W, H, 12, seed=3, gouraud=True)
        elif name == "changed":
            xy, z, c = scenes.sphere_mesh(W, H, *SMALL)
            _MESH[name] = (np.ascontiguousarray(xy[::-1] * 0.8 + 20.0), np.ascontiguousarray(z[::-1]),
                           np.ascontiguousarray(c[::-1]))
        elif name[0] == "flat":
            xy, z, c = scenes.sphere_mesh(W, H, *name[1:])
            _MESH[name] = (xy, z, np.ascontiguousarray(c[:, :4]))
        elif name[0] == "soup":
            _MESH[name] = scenes.triangle_soup(300, name[1], name[2], 9, seed=5, gouraud=True)
        elif name[0] == "hidden":
            _MESH[name] = _hidden_split(name[1:])
        else:
            _MESH[name] = scenes.sphere_mesh(W, H, *name)
    return _MESH[name]


class Frame:
    """One frame: clear colour, depth state, depth clear to `zclear`, then --
    with `pre` -- that mesh from host arrays under LESS + write (so the depth
    is no pending clear any more), then one draw of `mesh` under a
    translation.  size: the context is resized to it first when it differs."""

    def __init__(self, mesh, clear=NONUNI, depth=ZW, move=(0.0, 0.0), size=(W, H), zclear=0xFFFFFFFF, pre=None):
        self.mesh, self.clear, self.depth, self.move, self.size = mesh, clear, depth, move, size
        self.zclear, self.pre = zclear, pre

    def key(self):
        return (self.mesh, self.clear, self.depth, self.move, self.size, self.zclear, self.pre)

    def issue(self, ctx, draw):
        if (ctx.width, ctx.height) != self.size:
            ctx.resize(*self.size)
        ctx.set_color(*self.clear)
        V.set_depth(ctx, self.depth, self.zclear)
        if self.pre is not None:
            xy, z, c = _mesh(self.pre)
            ctx.set_depth_state(*ZW)
            ctx.draw_triangles(xy, c, z=z)
            ctx.set_depth_state(*self.depth)
        ctx.save_state()
        if self.move != (0.0, 0.0):
            ctx.translate(*self.move)
        draw(ctx)
        ctx.restore_state()


def _want(fr):
    if fr.key() not in _ORACLE:
        xy, z, c = _mesh(fr.mesh)
        ctx = scenes.OracleFactory().context(*fr.size, False)
        fr.issue(ctx, lambda t: t.draw_triangles(xy, c, z=z))
        _ORACLE[fr.key()] = {"f64": ctx.get_buffer_numpy(), "depth": ctx.get_depth_buffer(),
                             "u8": ctx.get_buffer_as_uint8_numpy()}
    return _ORACLE[fr.key()]


@functools.lru_cache(maxsize=None)
def _winner_pairs(mesh, size, shard):
    """(pairs of the whole batch, pairs of its LESS + write winners) on the
    CPU, in the tile rows the shard owns."""
    xy, z, _ = _mesh(mesh)
    pairs = V.tile_pairs(xy, size, shard)
    return int(pairs.sum()), int(pairs[V.winners(xy, z, size, shard=shard)].sum())


class Run:
    """A GPU context drawing Frames; its TriangleBuffers are made once per
    mesh name.  draw() checks the frame against the oracle unless read=False,
    and keeps the counts after each checked frame."""

    def __init__(self, shard=None, size=(W, H)):
        from libnativecpurenderer_amd import libNativeCPURendererPybind as R
        self.R = R
        self.ctx = R.RenderContext(size[0], size[1], False)
        self.ctx.set_warm_binning(1)
        self.shard = shard
        if shard is not None:
            self.ctx.set_shard(*shard)
        self.bufs = {}
        self.k = 0
        self.pruned, self.reused, self.warm = [], [], []

    def buffer(self, name):
        if name not in self.bufs:
            xy, z, c = _mesh(name)
            self.bufs[name] = self.R.TriangleBuffer(xy, c, z=z, gouraud=c.shape[1] == 12)
        return self.bufs[name]

    def check(self, fr, what=""):
        from libnativecpurenderer_amd import sharding
        want = _want(fr)
        rows = slice(None) if self.shard is None else sharding.owned_rows(fr.size[1], *self.shard)
        g = self.ctx.get_buffer_numpy()[rows]
        assert scenes.bits_equal(g, want["f64"][rows]), f"frame {self.k}{what}: {scenes.first_mismatch(g, want['f64'][rows])}"
        assert np.array_equal(self.ctx.get_depth_buffer()[rows], want["depth"][rows]), f"frame {self.k}{what} depth"

    def draw(self, fr, read=True):
        buf = self.buffer(fr.mesh)
        fr.issue(self.ctx, lambda t: t.draw_triangle_buffer(buf))
        if read:
            self.check(fr)
            self.pruned.append(self.ctx.pruned_batch_count())
            self.reused.append(self.ctx.reused_batch_count())
            self.warm.append(self.ctx.warm_batch_count())
        self.k += 1

    def visible_within(self, mesh, size=(W, H)):
        """GetVisiblePairCount against the CPU: the winners' pairs, plus at
        most one padding pair per slice of a split tile."""
        tot = self.ctx.schedule_totals()
        pairs, wp = _winner_pairs(mesh, size, self.shard)
        vis = self.ctx.visible_pair_count()
        print(f"visible pairs {vis} of {tot['pairs']} (winners' pairs {wp}, split slices {tot['split']})")
        assert tot["pairs"] == pairs, (tot, pairs)
        assert wp <= vis <= wp + tot["split"], (vis, wp, tot)
        return vis, tot


@pytest.mark.parametrize("mesh", [SMALL, BIG])
@pytest.mark.parametrize("shard", [None, (2, 0), (2, 1), (8, 3)])
def test_repeat_frames_prune(gpu, oracle, shard, mesh):
    run = Run(shard)
    for _ in range(8):
        run.draw(Frame(mesh))
    assert run.pruned == [0, 0, 0, 1, 2, 3, 4, 5], run.pruned   # cold, warm binning, marking frame, then pruned
    assert run.reused == [0, 0, 1, 2, 3, 4, 5, 6], run.reused   # (as without the visible list)
    assert run.warm == [0, 1, 2, 3, 4, 5, 6, 7], run.warm
    vis, tot = run.visible_within(mesh)
    pairs, wp = _winner_pairs(mesh, (W, H), shard)
    assert wp <= 0.75 * pairs   # (the bound holds of the oracle's winners: two-faced spheres)
    assert 0 < vis <= 0.75 * tot["pairs"], (vis, tot)
    assert run.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("mesh", [SMALL, BIG])
def test_unread_frames(gpu, oracle, mesh):
    """12 frames with no readback between them: the host prunes when it first
    sees the marking frame complete, by a query, and waits for nothing -- so
    how many of the 12 were pruned depends on how far it ran ahead (printed).
    After the readback the marking frame is certainly complete."""
    run = Run()
    for _ in range(12):
        run.draw(Frame(mesh), read=False)
    run.check(Frame(mesh), " (after 12 unread frames)")
    p = run.ctx.pruned_batch_count()
    print(f"pruned batches among 12 unread frames: {p}")
    assert 0 <= p <= 9   # (frame 3 is the first that can be)
    for _ in range(2):
        run.draw(Frame(mesh))
    assert run.pruned == [p + 1, p + 2], (p, run.pruned)
    run.visible_within(mesh)
    assert run.ctx.warm_failure_count() == 0


def test_depth_states_in_turn(gpu, oracle):
    """The list captured under LESS + write serves LESS + write draws only --
    also over a depth another draw has written, or one cleared to another
    value; draws in the other modes use the full list."""
    run = Run()
    seq = [(ZW, 4, [0, 0, 0, 1]), (NZ, 2, [1, 1]), (ZT, 2, [1, 1]), (ZW, 2, [2, 3])]
    for depth, n, want in seq:
        k = len(run.pruned)
        for _ in range(n):
            run.draw(Frame(SMALL, depth=depth))
        assert run.pruned[k:] == want, (depth, run.pruned)
    assert run.reused[-1] == len(run.reused) - 2, run.reused   # every frame from the third on reused a list
    # a depth cleared to another value: the list (captured over 0xFFFFFFFF) still serves
    for _ in range(2):
        run.draw(Frame(SMALL, zclear=0x80000000))
    assert run.pruned[-2:] == [4, 5], run.pruned
    # another batch first (host arrays: it takes a binning set in rotation, so the static
    # buffer bins warm again now and then): exact, and pruned wherever its list is in place
    r0, p0 = run.reused[-1], run.pruned[-1]
    for _ in range(4):
        run.draw(Frame(SMALL, pre="other"))
    assert run.pruned[-1] - p0 == run.reused[-1] - r0 > 0, (run.pruned, run.reused)
    assert run.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("how", ["zclear", "pre", "less_nowrite"])
def test_no_marking_frame_without_the_capture_condition(gpu, oracle, how):
    """LESS + write marks only over a pending depth clear to 0xFFFFFFFF, and
    LESS without write never: such frames reuse the full list."""
    fr = {"zclear": Frame(SMALL, zclear=0x80000000), "pre": Frame(SMALL, pre="other"),
          "less_nowrite": Frame(SMALL, depth=ZT)}[how]
    run = Run()
    for _ in range(6):
        run.draw(fr)
    assert run.pruned[-1] == 0 and run.ctx.visible_pair_count() == 0, run.pruned
    assert run.reused[-1] > 0, run.reused
    for _ in range(5):   # eligible frames: marked and pruned within them
        run.draw(Frame(SMALL))
    assert run.pruned[-1] > 0, (run.pruned, run.reused)
    run.visible_within(SMALL)
    assert run.ctx.warm_failure_count() == 0


def test_no_test_mode_captures_for_itself(gpu, oracle):
    """A list captured with the depth test off (the highest covering index
    wins) serves that mode; LESS + write draws use the full list."""
    run = Run()
    for _ in range(5):
        run.draw(Frame(SMALL, depth=NZ))
    assert run.pruned == [0, 0, 0, 1, 2], run.pruned
    for _ in range(2):
        run.draw(Frame(SMALL, depth=ZW))
    assert run.pruned[-2:] == [2, 2], run.pruned
    run.draw(Frame(SMALL, depth=NZ))
    assert run.pruned[-1] == 3, run.pruned


@pytest.mark.parametrize("size", [(64, 32), (128, 64)])
def test_hidden_split_tile(gpu, oracle, size):
    """A split tile whose slivers are all hidden behind two covering
    triangles keeps fewer winners than it has slices: it is padded to a pair
    per slice."""
    mesh = ("hidden",) + size
    run = Run(size=size)
    for _ in range(6):
        run.draw(Frame(mesh, size=size))
    assert run.pruned == [0, 0, 0, 1, 2, 3], run.pruned
    vis, tot = run.visible_within(mesh, size)
    assert tot["split"] > 2, tot                    # the tile is split into more slices than it has winners
    assert len(V.winners(*_mesh(mesh)[:2], size)) == 2
    assert vis >= tot["split"], (vis, tot)
    assert run.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("size", [(70, 40), (1, 58)])
def test_edge_shapes(gpu, oracle, size):
    mesh = ("soup",) + size
    run = Run(size=size)
    for _ in range(6):
        run.draw(Frame(mesh, size=size))
    assert run.pruned == [0, 0, 0, 1, 2, 3], run.pruned
    run.visible_within(mesh, size)
    assert run.ctx.warm_failure_count() == 0


def test_flat_buffer(gpu, oracle):
    mesh = ("flat",) + SMALL
    run = Run()
    for _ in range(6):
        run.draw(Frame(mesh))
    assert run.pruned == [0, 0, 0, 1, 2, 3], run.pruned
    run.visible_within(mesh)


def test_textured_buffer(gpu, oracle):
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    w, h, bg = 200, 140, (0.25, 0.25, 0.25, 0.25)
    b = T.soup(w, h, 240, 11, T.texture_rgb())
    want = T.expected_payload(w, h, False, bg, "zw", 0xFFFFFFFF, [b])
    buf, tex = R.TriangleBuffer(b["xy"], uv=b["uv"], z=b["z"]), gpu.texture(b["tex"])
    ctx = gpu.context(w, h, False)
    ctx.set_warm_binning(1)
    ctx.set_color_transform(*b["ct"])
    pruned = []
    for k in range(6):
        ctx.set_color(*bg)
        V.set_depth(ctx, ZW)
        ctx.draw_triangle_buffer(buf, tex)
        got = ctx.get_buffer_numpy()
        assert scenes.bits_equal(got, want[0]), (k, scenes.first_mismatch(got, want[0]))
        assert np.array_equal(ctx.get_depth_buffer(), want[1]), k
        pruned.append(ctx.pruned_batch_count())
    assert pruned == [0, 0, 0, 1, 2, 3], pruned
    assert 0 < ctx.visible_pair_count() < ctx.schedule_totals()["pairs"]


@pytest.mark.parametrize("fmt", ["rgb", "yuv420p"])
def test_frame_output_of_a_pruned_frame(gpu, oracle, fmt):
    run = Run()
    fr = Frame(SMALL, clear=UNI)   # (a uniform clear: the raster writes the frame output itself)
    for _ in range(4):
        run.draw(fr)
    run.ctx.set_frame_format(fmt)
    run.ctx.gather_frame_u8()
    run.draw(fr)
    run.ctx.gather_frame_u8()
    assert run.pruned[-2:] == [1, 2], run.pruned
    out, u8 = run.ctx.get_frame_u8(), _want(fr)["u8"]
    assert np.array_equal(out, scenes.yuv420p(u8) if fmt == "yuv420p" else u8), fmt


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_fault_after_pruning_began(gpu, oracle, mode):
    """A fault injected at frame 5: that frame bins (neither reused nor
    pruned), falls back exactly and is reported once; then the buffer bins
    cold (1, 3: banned), or gets a new schedule, marked and pruned afresh (2, 4)."""
    from libnativecpurenderer_amd import _lib
    run = Run()
    _lib.clear_error()
    for k in range(11):
        if k == 5:
            run.ctx.set_warm_fault_injection(mode)
        run.draw(Frame(SMALL))
    p = run.pruned
    assert p[:6] == [0, 0, 0, 1, 2, 2], p
    assert run.ctx.warm_failure_count() == 1
    assert "warm binning" in _lib.last_error(), _lib.last_error()
    if mode in (2, 4):
        assert p[-1] > p[5], p
    else:
        assert p[-1] == p[5] and run.ctx.visible_pair_count() == 0, p


@pytest.mark.parametrize("read", [True, False])
@pytest.mark.parametrize("mesh", [SMALL, BIG])
def test_failed_list_is_never_pruned(gpu, oracle, mesh, read):
    """Fault 3 on the binning frame itself (frame 1), the frames after it
    read back one by one or not at all: whether the host sees the failure
    before or after it sees the marking frame complete, the list is not
    pruned; every frame read is exact and the failure is counted once."""
    run = Run()
    run.draw(Frame(mesh))
    run.ctx.set_warm_fault_injection(3)
    for _ in range(6):
        run.draw(Frame(mesh), read=read)
    run.check(Frame(mesh), " (after the failed list's frames)")
    assert run.ctx.pruned_batch_count() == 0
    assert run.ctx.visible_pair_count() == 0
    assert run.ctx.warm_failure_count() == 1


def test_moving_resized_and_second_buffer(gpu, oracle):
    run = Run()
    A = Frame(SMALL)

    def repeats(n):
        for _ in range(n):
            run.draw(A)

    repeats(5)
    assert run.pruned[-1] == 2, run.pruned
    run.draw(Frame(SMALL, move=(0.4, 0.3)))   # loose: binned, not pruned; the list stays
    assert run.ctx.loose_batch_count() == 1 and run.pruned[-1] == 2, run.pruned
    vis = run.ctx.visible_pair_count()
    repeats(3)   # back under the schedule's transform: at most one warm binning, then pruned again
    assert run.pruned[-1] >= 4, run.pruned
    assert run.ctx.visible_pair_count() == vis   # (the same list: nothing marked again)
    run.draw(Frame(SMALL, size=(320, 208)))   # a resize: another key, a new schedule
    assert run.ctx.visible_pair_count() == 0
    p0 = run.pruned[-1]
    repeats(5)
    assert run.pruned[-1] > p0, run.pruned
    run.visible_within(SMALL)
    # a second buffer of the same size under the same transform: its own winners
    del run.bufs[SMALL]
    p0 = run.pruned[-1]
    for _ in range(5):
        run.draw(Frame("changed"))
    assert run.pruned[-1] > p0, run.pruned
    run.visible_within("changed")
    assert run.ctx.warm_failure_count() == 0


def test_switches(gpu, oracle):
    run = Run()
    for _ in range(5):
        run.draw(Frame(SMALL))
    assert run.pruned[-1] == 2, run.pruned
    run.ctx.set_visible_pruning(2)
    for _ in range(2):
        run.draw(Frame(SMALL))
    assert run.pruned[-2:] == [2, 2] and run.reused[-1] == run.reused[-3] + 2, (run.pruned, run.reused)
    run.ctx.set_visible_pruning(0)
    for _ in range(2):
        run.draw(Frame(SMALL))
    assert run.pruned[-2:] == [3, 4], run.pruned
    run.ctx.set_list_reuse(2)   # no reuse, so no pruning either
    for _ in range(2):
        run.draw(Frame(SMALL))
    assert run.pruned[-2:] == [4, 4] and run.reused[-1] == run.reused[-3], (run.pruned, run.reused)
    assert run.ctx.warm_failure_count() == 0

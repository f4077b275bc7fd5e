"""List reuse (a TriangleBuffer drawn again under the binning key of its last
warm binning is rasterised from the pair list that binning left in place: no
binning at all) against the CPU oracle, every frame bit for bit on the f64
framebuffer and the u32 depth.

What is checked beside exact frames: which batches reuse (GetReusedBatchCount),
that whatever writes the kept list's binning set, or changes what a binning
would give, ends the reuse (another buffer, a moved transform, an ordered batch,
host arrays, a resize), that a list whose binning failed falls back on every
reuse and is reported once, and that SetListReuse(2) restores a warm binning
per frame.

The counts asserted here follow from the host code: frame 0 of a context bins
cold and is validated at the next call (the schedule), frame 1 bins warm into
it (the list), frames 2.. reuse it -- frames - 2 reused batches, frames - 1 warm
ones.

Every frame clears colour and depth before its one draw, so a frame depends
only on its own description: the oracle renders each distinct frame once
(_ORACLE) and the tests share the result."""
import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

W, H = 640, 400
SMALL, BIG = (60, 200), (250, 700)   # sphere_mesh rows x cols: bins beside the raster (gate) / inline
NONUNI, UNI = (0.1, 0.2, 0.3, 0.1), (0.2, 0.2, 0.2, 0.2)

_MESH = {}
_ORACLE = {}


def _mesh(name):
    """Triangle arrays (xy, z, colours) by name: a sphere mesh (rows, cols),
    "other" (a second opaque buffer), "blend" (a translucent soup: ordered)."""
    if name not in _MESH:
        if name == "other":
            _MESH[name] = scenes.triangle_soup(3000, W, H, 12, seed=3, gouraud=True)
        elif name == "blend":
            _MESH[name] = scenes.triangle_soup(1500, W, H, 20, seed=4, alpha=(0.2, 0.8))
        elif name == "changed":   # as many triangles as SMALL, other content
            xy, z, c = scenes.sphere_mesh(W, H, *SMALL)
            _MESH[name] = (np.ascontiguousarray(xy[::-1] * 0.8 + 20.0), np.ascontiguousarray(z[::-1]),
                           np.ascontiguousarray(c[::-1]))
        else:
            _MESH[name] = scenes.sphere_mesh(W, H, *name)
    return _MESH[name]


class Frame:
    """One frame: clear colour, depth state, clear depth, one draw of `mesh`
    under a translation.  how: "buffer" (GPU: a TriangleBuffer) or "host"
    (DrawTriangles from host arrays).  size: the context is resized to it
    first when it differs."""

    def __init__(self, mesh, clear=NONUNI, depth=(True, True), move=(0.0, 0.0), how="buffer", size=(W, H)):
        self.mesh, self.clear, self.depth, self.move, self.how, self.size = mesh, clear, depth, move, how, size

    def key(self):
        return (self.mesh, self.clear, self.depth, self.move, self.size)

    def issue(self, ctx, draw):
        if (ctx.width, ctx.height) != self.size:
            ctx.resize(*self.size)
        ctx.set_color(*self.clear)
        ctx.set_depth_state(*self.depth)
        ctx.clear_depth()
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


class Run:
    """A GPU context drawing Frames; its TriangleBuffers are made once per
    mesh name.  draw() checks the frame against the oracle unless read=False."""

    def __init__(self, shard=None):
        from libnativecpurenderer_amd import libNativeCPURendererPybind as R
        self.R = R
        self.ctx = R.RenderContext(W, H, False)
        self.ctx.set_warm_binning(1)
        self.shard = shard
        if shard is not None:
            self.ctx.set_shard(*shard)
        self.bufs = {}
        self.k = 0
        self.reused, self.warm = [], []   # the counts after each frame

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
        xy, z, c = _mesh(fr.mesh)
        if fr.how == "host":
            fr.issue(self.ctx, lambda t: t.draw_triangles(xy, c, z=z))
        else:
            buf = self.buffer(fr.mesh)
            fr.issue(self.ctx, lambda t: t.draw_triangle_buffer(buf))
        if read:
            self.check(fr)
            self.reused.append(self.ctx.reused_batch_count())
            self.warm.append(self.ctx.warm_batch_count())
        self.k += 1


@pytest.mark.parametrize("mesh", [SMALL, BIG])
@pytest.mark.parametrize("shard", [None, (2, 0), (2, 1), (8, 3)])
def test_repeat_frames_reuse_the_list(gpu, oracle, shard, mesh):
    run = Run(shard)
    for _ in range(8):
        run.draw(Frame(mesh))
    assert run.reused == [0, 0, 1, 2, 3, 4, 5, 6], run.reused   # cold, warm binning, then reuse
    assert run.warm == [0, 1, 2, 3, 4, 5, 6, 7], run.warm
    assert run.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("mesh", [SMALL, BIG])
def test_same_key_other_state_reuses(gpu, oracle, mesh):
    """Clear colour, depth state and the frame output format are no part of
    the binning key: frames that differ only in them reuse the list."""
    run = Run()
    frames = [Frame(mesh), Frame(mesh), Frame(mesh, clear=UNI), Frame(mesh, clear=NONUNI),
              Frame(mesh, depth=(False, False)), Frame(mesh, depth=(True, True)), Frame(mesh, clear=UNI, depth=(False, True))]
    for fr in frames:
        run.draw(fr)
    # frame output (the raster also writes the u8 frame of a uniformly cleared frame): RGB, then YUV420P
    fr = Frame(mesh, clear=UNI)
    for fmt in ("rgb", "yuv420p", "rgb"):
        run.ctx.set_frame_format(fmt)
        run.ctx.gather_frame_u8()
        run.draw(fr)
        run.ctx.gather_frame_u8()
        out, u8 = run.ctx.get_frame_u8(), _want(fr)["u8"]
        assert np.array_equal(out, scenes.yuv420p(u8) if fmt == "yuv420p" else u8), fmt
    n = len(frames) + 3
    assert run.reused == [0, 0] + list(range(1, n - 1)), run.reused
    assert run.ctx.warm_failure_count() == 0


def test_other_batches_end_the_reuse(gpu, oracle):
    """Between exact repeats of buffer A: another buffer, A moved beyond 2 px
    (cold, a new schedule), A moved by less (loose) and back, blended (ordered)
    batches, DrawTriangles from host arrays, a resize and back.  The ordered
    and the host-array batches leave A's schedule in place and come three in a
    row, so one of them takes the binning set of A's list whichever it is: the
    next A must bin again.  Every frame is exact."""
    run = Run()
    A = Frame(SMALL)

    def repeats(n=3):
        for _ in range(n):
            run.draw(A)

    repeats()
    assert run.reused[-1] == 1, run.reused
    run.draw(Frame("other"))
    repeats()
    run.draw(Frame(SMALL, move=(9.0, 5.0)))
    repeats()
    run.draw(Frame(SMALL, move=(0.4, 0.3)))
    assert run.ctx.loose_batch_count() == 1
    r0 = run.reused[-1]
    repeats(2)
    assert run.reused[-1] > r0, run.reused   # back under the schedule's own transform
    for _ in range(3):
        run.draw(Frame("blend", depth=(True, False)))
        assert run.ctx.last_raster_path() == "ordered"
    r0 = run.reused[-1]
    repeats()
    assert run.reused[-3:] == [r0, r0 + 1, r0 + 2], run.reused   # one warm binning, then reuse again
    for _ in range(3):
        run.draw(Frame(SMALL, how="host"))
    r0 = run.reused[-1]
    repeats()
    assert run.reused[-3:] == [r0, r0 + 1, r0 + 2], run.reused
    run.draw(Frame(SMALL, size=(320, 208)))
    r0 = run.reused[-1]
    repeats()
    assert run.reused[-1] > r0, run.reused
    run.ctx.resize(320, 208)   # (nothing drawn at the other size: the key never changed)
    r0 = run.reused[-1]
    repeats(2)
    assert run.reused[-2:] == [r0, r0 + 1], run.reused   # the resized context bins once more
    assert run.ctx.warm_failure_count() == 0


@pytest.mark.parametrize("mode,mesh", [(1, SMALL), (2, SMALL), (3, SMALL), (1, BIG), (3, BIG)])
def test_fault_on_a_frame_that_would_have_reused(gpu, oracle, mode, mesh):
    """A fault injected at frame 4 of 8 (1 ranges overflow, 2 token withheld,
    3 pairs dropped): that frame bins instead of reusing, falls back exactly
    and is reported once; then the buffer bins cold (1, 3: banned) or warm and
    reused again after a cold binning (2)."""
    from libnativecpurenderer_amd import _lib
    run = Run()
    _lib.clear_error()
    for k in range(8):
        if k == 4:
            run.ctx.set_warm_fault_injection(mode)
        run.draw(Frame(mesh))
    r, w = run.reused, run.warm
    assert r[:5] == [0, 0, 1, 2, 2], r   # frame 4 binned
    assert w[4] == w[3] + 1, w           # as a warm batch
    assert run.ctx.warm_failure_count() == 1
    assert "warm binning" in _lib.last_error(), _lib.last_error()
    if mode == 2:
        assert r[7] > r[4], r   # cold, warm binning, reuse
    else:
        assert r[7] == r[4] and w[7] == w[4], (r, w)


def test_delayed_binning_then_four_frames(gpu, oracle):
    """Fault 4: the binning beside the raster lands after the raster's token
    wait gave up.  The frame and the four after it are exact, one failure."""
    run = Run()
    for k in range(9):
        if k == 4:
            run.ctx.set_warm_fault_injection(4)
        run.draw(Frame(SMALL))
    assert run.reused[4] == run.reused[3], run.reused
    assert run.ctx.warm_failure_count() == 1


@pytest.mark.parametrize("mesh", [SMALL, BIG])
def test_reuse_before_the_host_has_seen_the_failure(gpu, oracle, mesh):
    """Fault 3 at frame 4, then two more frames enqueued with no readback or
    flush in between: whether or not the host has seen the failure by then, a
    reused failed list falls back like its binning frame did -- the frame read
    back at the end is exact, and the failure is counted once."""
    run = Run()
    for k in range(4):
        run.draw(Frame(mesh))
    run.ctx.set_warm_fault_injection(3)
    for k in range(3):
        run.draw(Frame(mesh), read=False)
    run.check(Frame(mesh), " (after three unread frames)")
    assert run.ctx.warm_failure_count() == 1


def test_switch_off_bins_every_frame(gpu, oracle):
    """SetListReuse(2): a warm binning per frame, the cursors running on from
    epoch to epoch on each binning set."""
    run = Run()
    run.ctx.set_list_reuse(2)
    for _ in range(8):
        run.draw(Frame(SMALL))
    assert run.reused[-1] == 0, run.reused
    assert run.warm[-1] >= 5, run.warm
    run.ctx.set_list_reuse(0)   # and on again: the last binning's list is the one reused
    for _ in range(2):
        run.draw(Frame(SMALL))
    assert run.reused[-2:] == [1, 2], run.reused
    assert run.ctx.warm_failure_count() == 0


def test_new_buffer_of_the_same_size_is_not_reused(gpu, oracle):
    """Buffer identity is the uid, not the address or the size: A destroyed, a
    buffer of as many triangles and other content drawn under the same
    transform bins cold."""
    run = Run()
    for _ in range(4):
        run.draw(Frame(SMALL))
    r0, w0 = run.reused[-1], run.warm[-1]
    assert r0 == 2
    del run.bufs[SMALL]
    assert len(_mesh("changed")[0]) == len(_mesh(SMALL)[0])
    run.draw(Frame("changed"))
    assert (run.reused[-1], run.warm[-1]) == (r0, w0), (run.reused, run.warm)
    assert run.ctx.warm_failure_count() == 0

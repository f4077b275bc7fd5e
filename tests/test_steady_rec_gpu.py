"""The steady record kernel (k_keys_rec: one load round for the record copy,
KR_RT staged records at a padded LDS stride, the index ring of the pixel pass,
empty items cleared a wave each in 16-byte words, a workgroup per work unit)
against the CPU oracle, bit for bit on all four outputs: the f64 framebuffer,
the u32 depth, and the frame output as RGB and as YUV420P planes.

Helpers, stages and counts are those of tests/test_key_records_gpu.py: read
back frame by frame, frame RECORDS_AT (6) is the first shaded from the records,
and a deferred run (SetDeferredStores(1)) has frame 7 pending.  Every case
asserts that GetKeyRecordBatchCount rose (and the deferred count where the case
defers), so none passes without reaching the kernel.  The kernel writes the
frame output itself only over a pending uniform clear, so every frame here
clears to UNI.

Meshes are one-pixel triangles (tests/key_records_ref.py pixel_triangles) on
the first n pixels of one tile: n winners in that tile exactly
(GetKeyRecordTotals says so), every other owned tile an empty item.

Winner counts: 1, 31, 32, 33, 63, 64, 65 are the copy's unit counts on either
side of 256 and 512 (a record is eight units); 247, 248, 249 lie around KR_RT
(the staged count, nr_free.h), 280 and 281 around the index's KI_RT.

Frame shapes: 128x64, 128x32, 320x32, 384x32 and 384x64 are whole tiles with
rows whose byte addresses are 16-byte aligned in both formats (the 16-byte
stores); 144x64 is aligned as RGB (432-byte rows) and not as YUV420P (72-byte
chroma rows); 130x66 and 66x34 are misaligned with edge tiles; 65x33 is odd
(no YUV420P output exists for it: SetFrameFormat wants even sizes).  Their
empty runs are 3, 1, 4, 5, 11, 5, 8, 3 and 3 items: below, at and above a
256-thread workgroup's four (a 512-thread one's eight), with remainders.

Shards: (2, 1) owns tile row 1 of a 384x96 frame.  (8, 3) owns tile row 3,
which no frame of 96 rows has: that case is 192x128, fewer pixels than 384x96.
A shard's planes are compared on its owned rows.

NR_KEYS_WIDE is read once per process: test_the_wide_instances runs this file
again in a child process with NR_KEYS_WIDE=1 (the 512-thread instances)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import key_records_ref as KR
import scenes
import test_key_records_gpu as G
import test_visible_list_gpu as L

pytestmark = pytest.mark.gpu

UNI = L.UNI
Frame = G.Frame
RECORDS_AT = G.RECORDS_AT
TW, TH = 64, 32

_ORACLE = {}


def pixels(n, tile=(0, 0)):
    """n one-pixel triangles on the first n pixels (row by row) of tile (tx, ty)."""
    name = ("pixels", n) + tile
    if name not in L._MESH:
        xy, z, c = KR.pixel_triangles((TW, TH))
        xy = xy[:n].copy()
        xy[:, 0::2] += TW * tile[0]
        xy[:, 1::2] += TH * tile[1]
        L._MESH[name] = (np.ascontiguousarray(xy), np.ascontiguousarray(z[:n]), np.ascontiguousarray(c[:n]))
    return name


def _want(fr, alpha):
    if not alpha:
        return L._want(fr)
    if fr.key() not in _ORACLE:
        xy, z, c = L._mesh(fr.mesh)
        ctx = scenes.OracleFactory().context(*fr.size, True)
        fr.issue(ctx, lambda t: t.draw_triangles(xy, c, z=z))
        _ORACLE[fr.key()] = {"f64": ctx.get_buffer_numpy(), "depth": ctx.get_depth_buffer(),
                             "u8": ctx.get_buffer_as_uint8_numpy()}
    return _ORACLE[fr.key()]


class Run(G.Run):
    """G.Run, optionally on a context with an alpha channel, whose frame output
    is compared in either format (a shard's on its owned rows)."""

    def __init__(self, shard=None, size=(128, 64), mode=2, fmt="rgb", gather=False, alpha=False):
        super().__init__(shard, size, mode=mode, fmt=fmt, gather=gather)
        self.alpha = alpha
        if alpha:
            self.ctx = self.R.RenderContext(size[0], size[1], True)
            self.ctx.set_warm_binning(1)
            if shard is not None:
                self.ctx.set_shard(*shard)
            self.ctx.set_deferred_stores(mode)
            self.ctx.set_frame_format(fmt)
            if gather:
                self.ctx.gather_frame_u8()

    def check(self, fr, what=""):
        want, rows = _want(fr, self.alpha), self.rows(fr)
        g = self.ctx.get_buffer_numpy()[rows]
        assert scenes.bits_equal(g, want["f64"][rows]), f"frame {self.k}{what}: {scenes.first_mismatch(g, want['f64'][rows])}"
        assert np.array_equal(self.ctx.get_depth_buffer()[rows], want["depth"][rows]), f"frame {self.k}{what} depth"

    def check_frame_output(self, fr):
        before = self.counts()
        self.ctx.gather_frame_u8()
        out, u8, rows = self.ctx.get_frame_u8(), _want(fr, self.alpha)["u8"], self.rows(fr)
        if self.fmt == "yuv420p":
            w, h = fr.size
            crows = rows if isinstance(rows, slice) else rows[::2] // 2
            want, at = scenes.yuv420p(u8), 0
            for name, ph, pw, r in (("Y", h, w, rows), ("U", h // 2, w // 2, crows), ("V", h // 2, w // 2, crows)):
                got_p = out[at:at + ph * pw].reshape(ph, pw)[r]
                want_p = want[at:at + ph * pw].reshape(ph, pw)[r]
                assert np.array_equal(got_p, want_p), f"yuv420p {name} plane: {np.argwhere(got_p != want_p)[:4]}"
                at += ph * pw
        else:
            assert np.array_equal(out[rows], u8[rows]), f"u8 frame output: {np.argwhere(out[rows] != u8[rows])[:4]}"
        assert self.counts() == before, (before, self.counts())


def formats(size):
    return ("rgb", "yuv420p") if size[0] % 2 == 0 and size[1] % 2 == 0 else ("rgb",)


def exact(fr, size, deferred, shard=None, alpha=False):
    """Frames of `fr` shaded by k_keys_rec, every output compared: not deferred
    (the KO_ALL instance writes all four), or deferred (the KO_FRAME instance
    writes the frame output; the f64 values and the depths after the resolve)."""
    if not deferred:
        run = Run(shard, size, alpha=alpha)
        assert run.repeat(fr, RECORDS_AT + 1) == (2, 2, 1), (run.cached, run.indexed, run.recs)
        for k, fmt in enumerate(formats(size)):
            run.fmt = fmt
            run.ctx.set_frame_format(fmt)
            run.ctx.gather_frame_u8()
            run.draw(fr)
            run.check_frame_output(fr)
            assert run.recs[-1] == 2 + k, run.recs
        assert run.counts()[0] == 0, run.counts()
        assert run.ctx.warm_failure_count() == 0
        return run
    for fmt in formats(size):
        run = Run(shard, size, mode=1, fmt=fmt, gather=True, alpha=alpha)
        assert run.repeat(fr, RECORDS_AT + 1) == (2, 2, 1), (run.cached, run.indexed, run.recs)
        assert run.counts()[0] == 2, run.counts()
        run.draw(fr, read=False)
        assert run.counts()[0] == 3 and run.ctx.key_record_batch_count() == 2, run.counts()
        run.check_frame_output(fr)
        run.check(fr)
        assert run.ctx.warm_failure_count() == 0
    return run


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 247, 248, 249, 280, 281])
def test_winner_counts_in_one_tile(gpu, oracle, n, deferred):
    size = (128, 64)
    run = exact(Frame(pixels(n), clear=UNI, size=size), size, deferred)
    t = run.ctx.key_record_totals()
    # (a triangle at the tile's right edge is also binned into the next tile, which it wins no pixel of: that
    # tile is then a cached slot without a record)
    assert t["slots"] in (1, 2) and t["records"] == n, t


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("size", [(128, 64), (144, 64), (130, 66), (66, 34), (65, 33), (384, 32), (128, 32), (320, 32),
                                  (384, 64)])
def test_frame_shapes(gpu, oracle, size, deferred):
    run = exact(Frame(pixels(40), clear=UNI, size=size), size, deferred)
    tiles = ((size[0] + TW - 1) // TW) * ((size[1] + TH - 1) // TH)
    t = run.ctx.key_cache_totals()
    assert t["tiles"] == 1 and t["items"] == tiles, t


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("alpha", [False, True])
def test_contexts(gpu, oracle, alpha, deferred):
    size = (192, 64)
    exact(Frame(pixels(70, (1, 1)), clear=UNI, size=size), size, deferred, alpha=alpha)


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("shard,size,tile", [((2, 1), (384, 96), (2, 1)), ((8, 3), (192, 128), (1, 3))])
def test_shards(gpu, oracle, shard, size, tile, deferred):
    run = exact(Frame(pixels(40, tile), clear=UNI, size=size), size, deferred, shard=shard)
    t = run.ctx.key_cache_totals()
    # (the mesh's first column is also binned into the tile on its left: a cached slot without a record)
    assert t["tiles"] in (1, 2) and t["items"] == (size[0] + TW - 1) // TW, t


def test_a_frame_without_empty_items(gpu, oracle):
    """One tile, cached: the list has no empty item."""
    size = (64, 32)
    run = exact(Frame(pixels(40), clear=UNI, size=size), size, True)
    t = run.ctx.key_cache_totals()
    assert t["tiles"] == 1 and t["items"] == 1, t


def test_the_wide_instances(gpu):
    """NR_KEYS_WIDE=1: the 512-thread instances (eight empty items per unit).
    The variable is read once per process: a child runs the file."""
    if os.environ.get("NR_KEYS_WIDE") == "1":
        return
    env = dict(os.environ, NR_KEYS_WIDE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.abspath(__file__)],
                       env=env, capture_output=True, text=True, timeout=240,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]

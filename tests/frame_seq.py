"""Sequences of frames as plain data: one vocabulary for what a TriangleBuffer
drawn again and again can meet between its draws, one interpreter (run) that
executes a sequence on a factory (scenes.GpuFactory or scenes.OracleFactory),
and the hypothesis strategies that generate sequences (tests/test_frame_seq.py
checks what they generate, tests/test_seq_fuzz_gpu.py runs them on the GPU
against the oracle).  The single-frame counterpart is tests/frame_ops.py, whose
helpers this file uses.

A repeat draw of a TriangleBuffer takes a shortcut that depends on host state
earlier frames left behind (the warm schedule, its kept pair list, the visible
list, the visible plan, the key cache), so here the context -- its
framebuffer, depth, transform and every knob -- lives for the whole sequence,
and nothing is cleared unless an operation says so.

A sequence is (W, H, alpha, knobs, buffers, frames).

knobs       dict, GPU only, applied to every context when it is created: warm
            (set_warm_binning), reuse (set_list_reuse), prune
            (set_visible_pruning), coop (set_coop_raster), split
            (set_split_limits arguments or None), paircap
            (set_pair_capacity_override), ordered (set_force_ordered_raster),
            replan (set_visible_replan, 0 | 2), keys (set_key_cache, 0 | 2).
buffers     TriangleBuffers made before the first frame, over the W x H frame:
            ("flat" | "gouraud" | "blend", n, seed, spread)  colour soups (frame_ops.colour_soup), blend: translucent
            ("patch", n, seed, spread)   a Gouraud soup over the left 55 % of the frame: the tiles right of it keep no pair
            ("tex", n, seed, spread)     one (u, v) per triangle (frame_ops.textured_soup, "const"); texture per draw
            ("hidden", seed)             400 slivers inside tile 0 behind two covering triangles
            ("sphere", rows, cols)       scenes.sphere_mesh
frames      [(ops, read)]: after a frame with read=True, and after the last
            frame, every context's f64 buffer, u32 depth and u8 image (or,
            with a frame format and no shard, the frame output) are recorded.

Operations (OPS).  The oracle runs the same call unless another lowering is
stated:

("clear", rgba)         set_color; a uniform colour (r == g == b == a) stays a pending clear in the library, which
                        the next order-free batch consumes on chip with the per-tile fast clear; any other is written
("cleardepth", value) ("depthstate", test, write) ("ct", rgba)
("buf", i, move, tex)   buffer i under MOVES[move], applied inside save / restore; tex "rgb" | "rgba" for a
                        textured buffer (an RGBA texture takes the ordered raster), else None
                        -> draw_triangles of the same arrays; textured: flat colours textured_ref.flat_colours
("host", i, tex)        the same arrays through draw_triangles / draw_textured_triangles
("soup", seed)          150 translucent triangles from host arrays
("rect", c, g) ("circle", c, g) ("tex", name, g)   primitives: they write colour, never depth
("resize", w, h)
("shard", None | (n, k))  GPU: set_shard; then on both sides set_color(BG) and clear_depth(), because the rows a
                        shard does not own hold no history.  Records of a sharded context are compared on
                        sharding.owned_rows only, and its frame output is not gathered.
("fmt", None | "rgb" | "yuv420p")   GPU: set_frame_format and gather_frame_u8 at every frame's end
                        -> the u8 image / scenes.yuv420p of it.  None changes nothing in the library, which
                        cannot switch its frame output off once a gather has switched it on: the interpreter
                        only stops gathering and records the u8 image again
("warm", m) ("reuse", m) ("prune", m) ("coop", m) ("split", v) ("paircap", v) ("ordered", v) ("replan", m) ("keys", m)
("begin",) ("end",)
                        GPU only: the knobs flipped mid-sequence, command recording -> nothing
("fragcount", on)       set_fragment_counting; while on (and unsharded) the count after each frame is recorded
                        -> the sum of last_fragment_count() over the triangle draws since
("recreate", i, seed)   buffer i destroyed and made again with other content of as many triangles
("ctx", c)              the operations that follow go to context c (0 | 1; the second one is made, like the
                        first, at its first use): the same buffers, a schedule each

No fault injection: every sequence ends with warm_failure_count() == 0 and no
latched error ("failures", "error" of the GPU run).
"""
from __future__ import annotations

import math
import random

import numpy as np
from hypothesis import HealthCheck, given, settings, strategies as st

import frame_ops as F
import scenes
import textured_ref as T
import visible_ref as V

BG = (0.25, 0.5, 0.75, 1.0)
FULL = 0xFFFFFFFF
MOVES = {"none": None, "sub": ("t", 0.4, 0.3), "edge": ("t", 2.0, -2.0), "over": ("t", 2.0000001, 0.0),
         "far": ("t", 9.0, 5.0), "scale": ("s", 1.001)}
KNOBS_DEFAULT = dict(warm=1, reuse=0, prune=0, coop=0, split=None, paircap=0, ordered=False, replan=0, keys=0)
KNOB_OPS = ("warm", "reuse", "prune", "coop", "split", "paircap", "ordered", "replan", "keys")
TEXTURES = {"rgb": (F.NOMINAL_UV[0], F.NOMINAL_UV[1], 3, "f64", 5, None),
            "rgba": (F.NOMINAL_UV[0], F.NOMINAL_UV[1], 4, "u8", 6, None)}
ALL_OPS = ("clear", "cleardepth", "depthstate", "ct", "buf", "host", "soup", "rect", "circle", "tex", "resize", "shard",
           "fmt") + KNOB_OPS + ("begin", "end", "fragcount", "recreate", "ctx")
BUFFER_KINDS = ("flat", "gouraud", "blend", "tex", "hidden", "patch")
ARRAYS = ("frame", "f64", "depth", "u8")
COUNTERS = ("warm", "loose", "reused", "pruned", "replanned", "cached")
KEY_TILE_BYTES = V.TW * V.TH * 8              # a cached tile: a key of 8 bytes per pixel of the rasters' tile


# ---------------------------------------------------------------------------
# inputs from the specs
# ---------------------------------------------------------------------------
def hidden_soup(W, H, seed):
    """400 slivers inside tile 0 (far), then two triangles that cover the whole
    frame (near): the tile is dense enough to be split, and only the two
    covering triangles win a pixel."""
    i = np.arange(400)
    x0, y0 = 5.0 + (i % 40) + seed % 3, 3.0 + (i // 40) * 2.5
    sl = np.stack([x0, y0, x0 + 8.0, y0 + 0.7, x0 + 1.0, y0 + 2.2], axis=1)
    a, b, c, d = (-10.0, -10.0), (W + 10.0, -10.0), (W + 10.0, H + 10.0), (-10.0, H + 10.0)
    xy = np.concatenate([sl, np.array([a + b + c, a + c + d])])
    z = np.concatenate([np.full((400, 3), 0.9), np.full((2, 3), 0.1)])
    col = scenes.rng(seed).uniform(0, 1, size=(402, 3, 4))
    col[..., 3] = 1.0
    return np.ascontiguousarray(xy), z, col.reshape(402, 12)


_ARRAYS = {}


def buffer_arrays(spec, W, H):
    """(xy, z, colours | uv) of a buffer spec over a W x H frame; made once and
    never written."""
    key = (spec, W, H)
    if key not in _ARRAYS:
        kind = spec[0]
        if kind == "hidden":
            a = hidden_soup(W, H, spec[1])
        elif kind == "sphere":
            a = scenes.sphere_mesh(W, H, spec[1], spec[2])
        elif kind == "tex":
            a = F.textured_soup(spec[1], W, H, spec[2], spec[3], "const", F.NOMINAL_UV)
        elif kind == "patch":                 # (of the 4 tile columns at 200 x 140, the right one or two keep no pair)
            a = F.colour_soup(spec[1], 0.55 * W, H, spec[2], spec[3], True, False)
        else:
            a = F.colour_soup(spec[1], W, H, spec[2], spec[3], kind != "flat", kind == "blend")
        _ARRAYS[key] = a
    return _ARRAYS[key]


def triangle_count(spec):
    return {"hidden": 402, "sphere": 2 * spec[1] * spec[-1]}.get(spec[0], spec[1])


def recreated(spec, seed):
    """The spec of as many triangles and other content."""
    return ("hidden", seed) if spec[0] == "hidden" else (spec[0], spec[1], seed, spec[3])


# ---------------------------------------------------------------------------
# the interpreter
# ---------------------------------------------------------------------------
def owned_tile_count(W, H, shard):
    """Tiles of a W x H frame in the tile rows rank shard[1] of shard[0] owns."""
    tx, ty = (W + V.TW - 1) // V.TW, (H + V.TH - 1) // V.TH
    return tx * (ty if shard is None else len(range(shard[1], ty, shard[0])))


def check_key_totals(t, c, made_for):
    """What holds of key_cache_totals() without a reference: a key item per
    tile the context's shard owns, a cached slot for some of them.  For none
    only where a shard may own no tile with a kept pair: it owns no tile at
    all (1 x 58 is two tiles), or the frame is not of the size `made_for` its
    buffers were made to cover (64 x 32 resized to 200 x 140: the tile rows
    of rank 1 of 3 lie below every triangle)."""
    size = (c.ctx.width, c.ctx.height)
    items = owned_tile_count(size[0], size[1], c.shard)
    some = items > 0 and (c.shard is None or size == made_for)
    assert t["items"] == items and some <= t["tiles"] <= items, (t, items, c.shard)
    assert t["bytes"] == t["tiles"] * KEY_TILE_BYTES, t


class _Context:
    def __init__(self, ctx):
        self.ctx = ctx
        self.shard = None
        self.fmt = None
        self.depth = (True, True)
        self.counting = False
        self.frags = 0
        self.uniform = False                  # a uniform colour clear that nothing has drawn over yet
        self.written = False                  # any other colour clear (written at once) that nothing has drawn over yet
        self.pruned_at = -1                   # GPU: the last frame with a pruned batch


class _Run:
    def __init__(self, fac, seq):
        self.fac = fac
        self.gpu = fac.name != "oracle"
        self.W, self.H, self.alpha, self.knobs, self.specs, self.frames = seq
        self.specs = list(self.specs)
        self.ctxs = {}
        self.draws = []                       # GPU: one entry per triangle batch
        if self.gpu:
            from libnativecpurenderer_amd import _lib, libNativeCPURendererPybind as R
            self.R, self._lib = R, _lib

    # ---- contexts, resources ------------------------------------------------
    def set_knob(self, ctx, name, v):
        if name == "split":
            ctx.set_split_limits(*(v or (0, 0)))
        else:
            {"warm": ctx.set_warm_binning, "reuse": ctx.set_list_reuse, "prune": ctx.set_visible_pruning,
             "coop": ctx.set_coop_raster, "paircap": ctx.set_pair_capacity_override,
             "ordered": ctx.set_force_ordered_raster, "replan": ctx.set_visible_replan,
             "keys": ctx.set_key_cache}[name](v)

    def context(self, c):
        if c not in self.ctxs:
            ctx = self.fac.context(self.W, self.H, self.alpha)
            if self.gpu:
                for name in KNOB_OPS:
                    self.set_knob(ctx, name, self.knobs[name])
            ctx.set_color(*BG)
            ctx.set_depth_state(True, True)
            ctx.clear_depth()
            self.ctxs[c] = _Context(ctx)
        return self.ctxs[c]

    def make_buffer(self, i):
        spec = self.specs[i]
        xy, z, a = arrays = buffer_arrays(spec, self.W, self.H)
        gbuf = None
        if self.gpu:
            self.bufs[i] = None               # (the old buffer is destroyed first)
            gbuf = (self.R.TriangleBuffer(xy, uv=a, z=z) if spec[0] == "tex" else
                    self.R.TriangleBuffer(xy, a, z=z, gouraud=a.shape[1] == 12))
        self.bufs[i] = (spec, arrays, gbuf)

    def make_resources(self):
        self.texs = {name: self.fac.texture(F.texture_array(spec)) for name, spec in TEXTURES.items()}
        if not self.gpu:
            self.texels = {name: F.oracle_texels(t) for name, t in self.texs.items()}
        self.bufs = [None] * len(self.specs)
        for i in range(len(self.specs)):
            self.make_buffer(i)

    # ---- triangle batches -----------------------------------------------------
    def _counts(self, ctx):
        return (ctx.warm_batch_count(), ctx.loose_batch_count(), ctx.reused_batch_count(), ctx.pruned_batch_count(),
                ctx.replanned_batch_count(), ctx.key_cached_batch_count())

    def batch(self, what, i, draw):
        """Runs draw() and notes what became of the batch: GPU "ordered" |
        "pruned" | "reused" | "loose" | "warm" | "cold"; a batch shaded from the
        key cache is a pruned batch too, here as in the library's counters
        ("pruned" with cached=True), and so is one under the visible plan
        (replanned=True)."""
        c = self.cur
        before = self._counts(c.ctx) if self.gpu else None
        uniform, written, c.uniform, c.written = c.uniform, c.written, False, False
        draw()
        if self.gpu:
            d = [a - b for a, b in zip(self._counts(c.ctx), before)]
            how = ("ordered" if c.ctx.last_raster_path() == "ordered" else
                   "pruned" if d[3] else "reused" if d[2] else "loose" if d[1] else "warm" if d[0] else "cold")
            if how == "pruned":
                c.pruned_at = self.k
            self.draws.append(dict(frame=self.k, ctx=self.cid, op=what, buf=i, how=how, depth=c.depth, shard=c.shard,
                                   counting=c.counting, fmt=c.fmt, uniform=uniform, written=written, replanned=bool(d[4]), cached=bool(d[5])))
        elif c.counting:
            c.frags += c.ctx.last_fragment_count()

    def draw(self, what, i, move, tex):
        spec, (xy, z, a), gbuf = self.bufs[i]
        ctx = self.cur.ctx
        if spec[0] != "tex":
            call = ((lambda: ctx.draw_triangle_buffer(gbuf)) if self.gpu and what == "buf" else
                    (lambda: ctx.draw_triangles(xy, a, z=z, gouraud=a.shape[1] == 12)))
        elif not self.gpu:
            flat = T.flat_colours(self.texels[tex], a[:, :2])
            call = lambda: ctx.draw_triangles(xy, flat, z=z, gouraud=False)   # noqa: E731
        elif what == "buf":
            call = lambda: ctx.draw_triangle_buffer(gbuf, self.texs[tex])   # noqa: E731
        else:
            call = lambda: ctx.draw_textured_triangles(self.texs[tex], xy, a, z=z)   # noqa: E731
        m = MOVES[move]
        ctx.save_state()
        if m and m[0] == "t":
            ctx.translate(m[1], m[2])
        elif m:
            ctx.scale(m[1], m[1])
        self.batch(what, i, call)
        ctx.restore_state()

    # ---- one operation --------------------------------------------------------
    def op(self, op):
        k = op[0]
        if k == "ctx":
            self.cid, self.cur = op[1], self.context(op[1])
            return
        c = self.cur
        ctx = c.ctx
        if k in ("rect", "circle", "tex", "resize", "shard"):
            c.uniform = c.written = False
        if k == "clear":
            ctx.set_color(*op[1])
            c.uniform = len(set(op[1])) == 1
            c.written = not c.uniform
        elif k == "cleardepth":
            ctx.clear_depth(op[1])
        elif k == "depthstate":
            ctx.set_depth_state(op[1], op[2])
            c.depth = (bool(op[1]), bool(op[2]))
        elif k == "ct":
            ctx.set_color_transform(*op[1])
        elif k == "buf":
            self.draw("buf", op[1], op[2], op[3])
        elif k == "host":
            self.draw("host", op[1], "none", op[2])
        elif k == "soup":
            xy, z, col = F.colour_soup(150, self.W, self.H, op[1], 20.0, True, True)
            self.batch("soup", None, lambda: ctx.draw_triangles(xy, col, z=z, gouraud=True))
        elif k == "rect":
            g = op[2]
            ctx.draw_rect(g[0], g[1], g[2], g[3], *op[1])
        elif k == "circle":
            g = op[2]
            ctx.draw_circle(g[0], g[1], g[2], *op[1])
        elif k == "tex":
            g = op[2]
            ctx.draw_texture(self.texs[op[1]], g[0], g[1], g[2], g[3])
        elif k == "resize":
            assert c.fmt != "yuv420p" or (op[1] % 2 == 0 and op[2] % 2 == 0), "YUV420P needs even sizes"
            ctx.resize(op[1], op[2])
        elif k == "shard":
            c.shard = op[1]
            if self.gpu:
                ctx.set_shard(*(op[1] or (1, 0)))
            ctx.set_color(*BG)
            ctx.clear_depth()
            if c.counting:
                self.op(("fragcount", True))
        elif k == "fmt":
            assert op[1] != "yuv420p" or (ctx.width % 2 == 0 and ctx.height % 2 == 0), "YUV420P needs even sizes"
            c.fmt = op[1]
            if self.gpu and op[1]:
                ctx.set_frame_format(op[1])
                if c.shard is None:
                    ctx.gather_frame_u8()     # (from now on the raster writes the frame output too)
        elif k in KNOB_OPS:
            if self.gpu:
                self.set_knob(ctx, k, op[1])
        elif k in ("begin", "end"):
            if self.gpu:
                (ctx.begin_commands if k == "begin" else ctx.end_commands)()
        elif k == "fragcount":
            c.counting, c.frags = bool(op[1]), 0
            if self.gpu:
                ctx.set_fragment_counting(bool(op[1]))
        elif k == "recreate":
            self.specs[op[1]] = recreated(self.specs[op[1]], op[2])
            self.make_buffer(op[1])
        else:
            raise ValueError(f"unknown operation {op!r}")

    # ---- a frame's end ---------------------------------------------------------
    def end_frame(self, read, out):
        for cid, c in sorted(self.ctxs.items()):
            ctx = c.ctx
            output = c.fmt is not None and c.shard is None
            if output and self.gpu:
                ctx.gather_frame_u8()
            if c.counting and c.shard is None:
                out["frags"].append((self.k, cid, ctx.get_fragment_count() if self.gpu else c.frags))
            if not read:
                continue
            rec = dict(k=self.k, ctx=cid, shard=c.shard, f64=ctx.get_buffer_numpy(), depth=ctx.get_depth_buffer())
            if not output:
                rec["u8"] = ctx.get_buffer_as_uint8_numpy()
            elif self.gpu:
                rec["frame"] = ctx.get_frame_u8()
            else:
                u8 = ctx.get_buffer_as_uint8_numpy()
                rec["frame"] = u8 if c.fmt == "rgb" else scenes.yuv420p(u8)
            out["records"].append(rec)
        if self.gpu:
            cs = [c.ctx for _, c in sorted(self.ctxs.items())]
            n = dict(zip(COUNTERS, (sum(v) for v in zip(*[self._counts(x) for x in cs]))))
            n["path"] = self.cur.ctx.last_raster_path()
            if read:                          # (these wait for the device: only where the frame is read anyway)
                n["visible"] = self.cur.ctx.visible_pair_count()
                n["totals"] = self.cur.ctx.schedule_totals()
                n["failures"] = sum(x.warm_failure_count() for x in cs)
                n["keytotals"] = self.cur.ctx.key_cache_totals()
                n["vplan"] = self.cur.ctx.visible_plan_totals()
                # (the exact totals: tests/key_cache_ref.py.  A shard change leaves the schedule of the shard before
                # in place until a batch bins under the new one: only after a frame with a pruned batch are the
                # totals those of the context's shard and size.)
                if n["keytotals"] and self.cur.pruned_at == self.k:
                    check_key_totals(n["keytotals"], self.cur, (self.W, self.H))
            out["counters"].append(n)

    def run(self):
        out = dict(records=[], frags=[], counters=[], draws=self.draws, failures=0, error="")
        if self.gpu:
            self._lib.clear_error()
        self.make_resources()
        self.k = 0
        self.op(("ctx", 0))
        for self.k, (ops, read) in enumerate(self.frames):
            for op in ops:
                self.op(op)
            self.end_frame(read or self.k == len(self.frames) - 1, out)
        if self.gpu:
            out["failures"] = sum(c.ctx.warm_failure_count() for c in self.ctxs.values())
            out["error"] = self._lib.last_error()
        return out


def run(fac, seq):
    """Executes `seq` on `fac`: dict records [dict k (the frame's number), ctx,
    shard, f64, depth, u8 | frame], frags [(frame, ctx, count)], and on the GPU counters
    (per frame: warm, loose, reused, pruned, replanned, cached summed over the
    contexts, path; only after a recorded frame also visible, totals, failures,
    keytotals, vplan of the current context: visible_pair_count,
    warm_failure_count, key_cache_totals and visible_plan_totals wait for the
    device, and an unread frame is there so that the host runs ahead of it),
    draws (per triangle batch: frame, ctx, op, buf, how, depth, shard, counting,
    fmt, uniform: drawn over a pending uniform colour clear, written: over any
    other colour clear, replanned, cached),
    failures, error."""
    return _Run(fac, seq).run()


def mismatches(got, want):
    """[(frame, context, what, scenes.first_mismatch)] over the records and
    fragment counts of two runs; a sharded record on its owned rows."""
    from libnativecpurenderer_amd import sharding
    bad = []
    if [(r["k"], r["ctx"]) for r in got["records"]] != [(r["k"], r["ctx"]) for r in want["records"]]:
        return [(None, None, "records", "not the same frames recorded")]
    for g, w in zip(got["records"], want["records"]):
        rows = slice(None) if w["shard"] is None else sharding.owned_rows(w["f64"].shape[0], *w["shard"])
        cut = lambda r: dict({k: (r[k] if k == "frame" else r[k][rows]) for k in ARRAYS if k in r}, probes=[])   # noqa: E731
        bad += [(w["k"], w["ctx"], what, how) for what, how in F.mismatches(cut(g), cut(w))]
    if got["frags"] != want["frags"]:
        bad.append((None, None, "fragment counts", f"{got['frags']} != {want['frags']}"))
    return bad


# ---------------------------------------------------------------------------
# what a sequence holds (for the generator's own test and the GPU test's Reached)
# ---------------------------------------------------------------------------
def frame_buffers(ops):
    """The buffers a frame draws with "buf", per context switch ignored."""
    return [op[1] for op in ops if op[0] == "buf"]


def clears(ops):
    """Does the frame clear colour or depth (a shard change and a resize do)?"""
    return any(op[0] in ("clear", "cleardepth", "shard", "resize") for op in ops)


def _longest(flags):
    best = run_ = 0
    for f in flags:
        run_ = run_ + 1 if f else 0
        best = max(best, run_)
    return best


def quiet_runs(frames):
    """[(first frame, length)] of the maximal runs of read frames with the same
    operations: six of them reach the key cache (cold, warm, marking, pruned,
    capture, cached)."""
    runs, k = [], 0
    while k < len(frames):
        j = k + 1
        if frames[k][1]:
            while j < len(frames) and frames[j] == frames[k]:
                j += 1
            runs.append((k, j - k))
        k = j
    return runs


def describe(seq):
    """dict: ops (the operation kinds used), kinds (of the buffers drawn with
    "buf"), moves (MOVES names drawn on a buffer that "buf" had drawn at least
    twice before: after a repeat), unclear (longest run of frames without a
    colour or depth clear), two (a frame draws two different buffers), shard_mid
    (a shard change after frame 0), unread (longest run of read=False frames
    that follows a repeat), clears ("uniform" / "other": the colour clears of
    frames after a repeat)."""
    W, H, alpha, knobs, specs, frames = seq
    specs = list(specs)
    ops_used, kinds, moves = set(), set(), set()
    seen = {}
    unread, repeated = [], False
    clear_kinds = set()
    for ops, read in frames:
        for op in ops:
            ops_used.add(op[0])
            if op[0] == "clear" and repeated:
                clear_kinds.add("uniform" if len(set(op[1])) == 1 else "other")
            if op[0] == "buf":
                kinds.add(specs[op[1]][0])
                if seen.get(op[1], 0) >= 2:
                    moves.add(op[2])
                seen[op[1]] = seen.get(op[1], 0) + 1
            elif op[0] == "recreate":
                specs[op[1]] = recreated(specs[op[1]], op[2])
                seen[op[1]] = 0
        unread.append(repeated and not read)
        repeated = repeated or any(v >= 2 for v in seen.values())
    return dict(ops=ops_used, kinds=kinds, moves=moves, clears=clear_kinds,
                unclear=_longest([not clears(ops) for ops, _ in frames]),
                two=any(len(set(frame_buffers(ops))) >= 2 for ops, _ in frames),
                shard_mid=any(op[0] == "shard" for ops, _ in frames[1:] for op in ops),
                unread=_longest(unread))


# ---------------------------------------------------------------------------
# strategies
# ---------------------------------------------------------------------------
# hypothesis draws two seeds and the pixel format; the sequence follows from
# them (random.Random), so its distribution is the one written below.  A
# sequence is runs of unchanged repeats of one frame template (clears, then the
# template's buffer draws with its other batches between them), at least five
# frames long more often than not -- cold, warm, marking frame, pruned,
# pruned -- and seven or more in a third of the small sequences and every large
# one (capture, cached), with one or two disturbances between two runs; what a disturbance switches
# off (a knob, an ordered colour transform, fragment counting) is mostly
# switched back on a frame or two later.
SIZES = [(200, 140)] * 7 + [(64, 32)] * 2 + [(1, 58)]     # 4 x 5 tiles with partial right and bottom tiles; one tile; one column
DEPTHS = [(True, True)] * 4 + [(False, False)] * 3 + [(True, False), (False, True)]
SHARDS = [(2, 0), (2, 1), (2, 1), (3, 1), (8, 3)]
_DISTURB = (["move"] * 5 + ["depth"] * 5 + ["colour"] * 4 + ["zval"] * 3 + ["noclear"] * 5 + ["ct"] * 2 + ["shard"] * 2 + ["resize"] * 2 +
            ["fmt"] * 2 + ["knob"] * 12 + ["fragcount"] + ["recreate"] + ["ctx"] * 3 + ["batch"] * 5 + ["template"] * 2 +
            ["unread"] * 3)
_DISTURB_LARGE = ["move"] * 2 + ["depth", "depth", "zval", "colour", "noclear", "resize", "resize", "unread"]
_OFF = {"warm": (2, 1), "reuse": (2, 0), "prune": (2, 0), "paircap": (50, 0), "ordered": (True, False), "replan": (2, 0),
        "keys": (2, 0)}   # (off, on)


class _Gen:
    def __init__(self, r, W, H, large=False, long=False):
        self.r, self.W, self.H, self.large, self.long = r, W, H, large, long
        self.cur = 0
        self.S = {c: dict(depth=(True, True), shard=None, fmt=None, size=(W, H)) for c in (0, 1)}
        self.cc = self.cd = True
        self.zval = FULL
        self.colour = self.clear_colour(r.random() < 0.5)
        self.extras = []
        self.coop = None
        # a large sequence holds, whatever else is drawn: a loose move, and a depth-mode switch or a resize and back
        self.must = r.sample(["loose", r.choice(["depth", "resize"])], 2) if large else []
        self.pending = []                     # (frame, context, op): what is switched back later

    def seed(self):
        return self.r.randrange(2**31 - 1)

    def col(self):
        return [round(self.r.random(), 3) for _ in range(4)]

    def clear_colour(self, uniform):
        """(a uniform clear stays pending in the library, any other is written)"""
        return [round(self.r.random(), 3)] * 4 if uniform else self.col()

    def g4(self):
        return [round(self.r.uniform(-20.0, 160.0), 1) for _ in range(4)]

    def buffers(self):
        r = self.r
        specs = []
        for k in range(r.choice([1, 2, 2, 3])):
            kind = (r.choice(["flat", "gouraud", "gouraud", "tex", "hidden", "patch"]) if k == 0 else
                    r.choice(["blend", "blend", "blend", "tex", "tex", "flat", "gouraud"]))
            if kind == "hidden" and (self.W < 64 or any(s[0] == "hidden" for s in specs)):
                kind = "gouraud"
            if kind == "hidden":
                specs.append(("hidden", self.seed()))
                continue
            n = r.choice([200, 300, 500, 900, 1600, 3000])
            # (the oracle's cost: the bounding boxes of a buffer cover about 250 000 pixels at the most)
            spread = min(r.choice([3.0, 6.0, 12.0, 25.0]), round(math.sqrt(250000 / n) / 2, 1))
            specs.append((kind, n, self.seed(), spread))
        self.specs = specs
        return specs

    def texref(self, i, first=False):
        """(the template's first draw is mostly opaque: an RGBA texture takes the ordered raster)"""
        if self.specs[i][0] != "tex":
            return None
        return "rgba" if self.r.random() < (0.1 if first else 0.6) else "rgb"

    def other_batch(self):
        r = self.r
        kind = r.choice(["host", "soup", "rect", "circle", "tex", "prims", "prims"])
        if kind == "host":
            i = r.randrange(len(self.specs))
            return [("host", i, self.texref(i))]
        if kind == "soup":
            return [("soup", self.seed())]
        prims = []
        for _ in range(1 if kind != "prims" else 3):
            p = kind if kind != "prims" else r.choice(["rect", "circle", "tex"])
            g = self.g4()
            prims.append(("tex", r.choice(["rgb", "rgba"]), g) if p == "tex" else
                         ("circle", self.col(), [g[0], g[1], abs(g[2]) % 50]) if p == "circle" else ("rect", self.col(), g))
        return [("begin",)] + prims + [("end",)] if kind == "prims" or r.random() < 0.3 else prims

    def later(self, k, op, p=0.8, after=(1, 1, 2, 3)):
        if self.r.random() < p:
            self.pending.append((k + self.r.choice(after), self.cur, op))

    def disturb(self, k, name):
        """The operations of one disturbance before frame k's clears; what it
        changes of the template stays."""
        r, s = self.r, self.S[self.cur]
        if name == "loose":
            self.move = (0, "sub")
        elif name == "move":
            self.move = (r.randrange(len(self.draws)), r.choice(["sub", "sub", "edge", "edge", "over", "over", "far", "scale"]))
        elif name == "depth":
            # (mostly between the two modes that capture a visible list, each for itself)
            other = {(True, True): (False, False), (False, False): (True, True)}.get(s["depth"])
            s["depth"] = other if other and r.random() < 0.6 else r.choice([d for d in DEPTHS if d != s["depth"]])
            return [("depthstate",) + s["depth"]]
        elif name == "colour":               # uniform <-> non-uniform, or (a tile nothing is drawn in shows it) another uniform one
            uniform = len(set(self.colour)) == 1
            self.colour, self.cc = self.clear_colour(not uniform or r.random() < 0.4), True
        elif name == "zval":                 # (mostly back to 0xFFFFFFFF later: the depth clear the shortcuts capture over)
            self.zval, self.cd = r.choice(F.DEPTH_VALUES), True
            if self.zval != FULL:
                self.later(k, ("_clears",), p=0.7, after=(1, 2, 3))
        elif name == "noclear":
            if self.cc and self.cd:
                self.cc, self.cd = r.choice([(False, False), (False, False), (True, False)])
                self.later(k, ("_clears",), p=0.7, after=(1, 2, 3))
            else:
                self.cc = self.cd = True
        elif name == "ct":
            a = r.choice([1.0, 1.0, 0.5])
            if a != 1.0:
                self.later(k, ("ct", [1.0, 1.0, 1.0, 1.0]))
            return [("ct", [round(r.uniform(0.5, 1.0), 3) for _ in range(3)] + [a])]
        elif name == "shard":
            s["shard"] = r.choice(SHARDS) if s["shard"] is None else r.choice([None, None, (2, 1)])
            return [("shard", s["shard"])]
        elif name == "resize":
            first = (self.W, self.H)
            pool = [(320, 208), first] if self.large else [(200, 140), (64, 32), (1, 58), first]
            sizes = [z for z in pool if z != s["size"] and (z[0] % 2 == 0 or s["fmt"] != "yuv420p")]
            s["size"] = first if first in sizes and r.random() < 0.7 else r.choice(sizes)   # (mostly back)
            if self.large and s["size"] != first:
                self.later(k, ("resize",) + first, p=1.0, after=(1, 2))
            return [("resize",) + s["size"]]
        elif name == "fmt":
            even = s["size"][0] % 2 == 0 and s["size"][1] % 2 == 0
            s["fmt"] = r.choice([f for f in (None, "rgb", "yuv420p") if f != s["fmt"] and (even or f != "yuv420p")])
            return [("fmt", s["fmt"])]
        elif name == "knob":
            knob = r.choice(KNOB_OPS + ("keys", "keys", "replan"))
            if knob in _OFF:
                self.later(k, (knob, _OFF[knob][1]), p=0.9)
                return [(knob, _OFF[knob][0])]
            if knob == "coop":                # (never the value the last flip left)
                self.coop = r.choice([m for m in (0, 1, 2) if m != self.coop])
                return [("coop", self.coop)]
            return [("split", r.choice([None, (64, 64)]))]
        elif name == "fragcount":
            self.later(k, ("fragcount", False), p=1.0, after=(1, 2, 2))
            return [("fragcount", True)]
        elif name == "recreate":
            return [("recreate", r.choice(self.draws)[0], self.seed())]
        elif name == "ctx":
            self.cur = 1 - self.cur
            self.later(k, ("ctx", 1 - self.cur), p=0.7, after=(1, 2, 7, 8))
            return [("ctx", self.cur)]
        elif name == "batch":
            if self.extras and r.random() < 0.5:
                self.extras = []
            elif r.random() < 0.3:
                self.extras = self.other_batch()
            else:
                self.once = self.other_batch()
        elif name == "template":
            i = r.randrange(len(self.specs))
            how = r.choice(["add", "add", "drop", "swap"])
            if how == "add" or len(self.draws) == 1:
                self.draws.insert(r.randrange(len(self.draws) + 1), (i, self.texref(i)))
            elif how == "drop":
                self.draws.pop(r.randrange(len(self.draws)))
            else:
                self.draws.reverse()
        return []

    def frames(self, n):
        r = self.r
        self.draws = [(0, self.texref(0, True))]
        pre = []
        if not self.large:                    # how the sequence starts
            if r.random() < 0.45:
                pre += self.disturb(0, "depth")
            if r.random() < 0.2:
                pre += self.disturb(0, "shard")
            # (tiles without a kept pair: the rasters write their share of a frame output themselves under a pending
            # uniform colour clear, so a patch mostly starts with both)
            patch = self.specs[0][0] == "patch"
            if patch and r.random() < 0.7:
                self.colour = self.clear_colour(True)
            if r.random() < (0.7 if patch else 0.2):
                pre += self.disturb(0, "fmt")
            if len(self.specs) > 1 and r.random() < 0.6:
                self.draws.append((1, self.texref(1)))
        # (the key cache: six unchanged read frames reach it -- cold, warm, marking, pruned, capture, cached; frame 0
        # differs from the ones after it by what `pre` holds)
        if self.large:
            quiet = r.choice([6, 7])
        elif self.long:
            quiet = r.choice([7, 8]) + bool(pre)
        else:
            quiet = r.choice([4, 5, 5, 6]) if r.random() < 0.85 else 0
            if self.specs[0][0] == "patch":   # (its empty tiles are there for the cached frames)
                quiet = max(quiet, 6)
        unread = 0
        opening = quiet
        # (a long sequence now and then goes on in the second context at once: room to be cached there too)
        first = "ctx" if self.long and r.random() < 0.3 else None
        out = []
        for k in range(n):
            self.move, self.once = None, []
            # (a patch after its opening run: a uniform clear mostly to another colour than the frame before, which is
            # what shows in a tile without a kept pair; the colour is live state and ends no shortcut)
            patch = not self.large and self.specs[0][0] == "patch"
            if patch and k >= opening and len(set(self.colour)) == 1 and r.random() < 0.5:
                self.colour = self.clear_colour(True)
            due = [p for p in self.pending if p[0] <= k and p[1] == self.cur]
            for p in sorted(due, key=lambda p: p[2][0] == "ctx"):   # (the context switch last)
                self.pending.remove(p)
                if p[2][0] == "_clears":      # (not an operation: the template clears colour and depth again, to 0xFFFFFFFF)
                    self.cc, self.cd, self.zval = True, True, FULL
                    continue
                pre.append(p[2])
                if p[2][0] == "ctx":
                    self.cur = p[2][1]
                elif p[2][0] == "resize":
                    self.S[self.cur]["size"] = p[2][1:]
            read = True
            if unread:
                unread -= 1
                read = False
            elif quiet:
                quiet -= 1
            else:
                kinds = _DISTURB_LARGE if self.large else _DISTURB
                name = self.must.pop(0) if self.must else first or r.choice(kinds)
                if name == "unread":
                    unread = r.choice([2, 3]) if self.large else r.choice([3, 4, 5])
                    read = False
                else:
                    pre += self.disturb(k, name)
                    if r.random() < 0.35:     # (now and then two at once)
                        pre += self.disturb(k, r.choice([d for d in kinds if d not in (name, "unread", "ctx")]))
                    quiet = (r.choice([1, 2]) if self.must else r.choice([0, 1, 2, 6, 7, 7, 8]) if self.long else
                             r.choice([0, 0, 1, 1, 2, 5, 6]))
                    if name == "ctx" and (first or r.random() < 0.6):   # (long enough in the other context to be cached there)
                        quiet = max(quiet, 6)
                    first = None
            ops = pre
            if self.cc:
                ops.append(("clear", self.colour))
            if self.cd:
                ops.append(("cleardepth", self.zval))
            for j, (i, tex) in enumerate(self.draws):
                ops.append(("buf", i, self.move[1] if self.move and self.move[0] == j else "none", tex))
                if j == 0:
                    ops += self.extras + self.once
            out.append((ops, read))
            pre = []
        return out


def make_small_seq(seed, salt, alpha):
    r = random.Random(f"seq/{seed}/{salt}/{alpha}")
    W, H = r.choice(SIZES)
    long = r.random() < 1 / 3                 # long enough to be cached, disturbed and cached again
    g = _Gen(r, W, H, long=long)
    specs = g.buffers()
    knobs = dict(KNOBS_DEFAULT, warm=r.choice([0, 1, 1]), coop=r.choice([0, 0, 1, 2]))
    if r.random() < (0.8 if specs[0][0] == "hidden" else 0.15):
        knobs["split"] = (64, 64)
    return (W, H, alpha, knobs, specs, g.frames(r.randint(18, 24) if long else r.randint(10, 16)))


def make_large_seq(seed, salt, alpha):
    r = random.Random(f"large/{seed}/{salt}/{alpha}")
    g = _Gen(r, 640, 400, large=True)
    g.specs = [("sphere", 250, 700)]
    return (640, 400, alpha, dict(KNOBS_DEFAULT), g.specs, g.frames(r.randint(12, 14)))


_seed = st.integers(0, 2**31 - 1)


def small_seqs():
    """200 x 140, 64 x 32 or 1 x 58; 10-16 frames, a third of them 18-24 with an
    opening run of 7-8 unchanged frames; 1-3 buffers of 200-3000 triangles."""
    return st.builds(make_small_seq, _seed, _seed, st.booleans())


def large_seqs():
    """640 x 400, one buffer of 350 000 triangles (the inline warm binning);
    12-14 frames, the first 6-7 unchanged (the visible plan -- the schedule has
    split tiles -- and the key cache), then clears, depth modes, moves, resize
    and back, unread frames."""
    return st.builds(make_large_seq, _seed, _seed, st.booleans())


SMALL_EXAMPLES = 64
LARGE_EXAMPLES = 3


def for_each_sequence(kind, visit):
    """Calls visit(seq) for the examples of the "small" or "large" sequences:
    one inner @given function with fixed settings and derandomize=True, so that
    every caller (the generator's own CPU test and the GPU test) draws exactly
    the same examples."""
    strategy, n = {"small": (small_seqs(), SMALL_EXAMPLES), "large": (large_seqs(), LARGE_EXAMPLES)}[kind]

    @settings(max_examples=n, deadline=None, derandomize=True, database=None,
              suppress_health_check=list(HealthCheck))
    @given(strategy)
    def examples(seq):
        visit(seq)

    examples()

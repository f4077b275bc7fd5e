"""Edge-parameter differential fuzz of the reference primitives: cases as plain
data, one interpreter (run), seeded generators per family, and small Python
restatements of the host-side decisions (tests/test_prim_fuzz.py checks on the
CPU that the cases reach what they claim; tests/test_prim_fuzz_gpu.py runs them
on the HIP library against the oracle, bit for bit, on every submission path).

A case is a dict of plain data:

  name      "<family>-<seed>"
  ctx       (W, H, alpha)
  textures  [(w, h, "u8" | "f64", channels, seed)]; f64 texels are U(-0.5, 1.5)
  aux       None or (W, H, alpha, ops): a second context drawn by `ops` before
            the first operation; its *shared* texture (as_texture_shared) is
            texture len(textures)
  ops       list of tuples, see Runner.step.  A texture argument is an index
            into the table: the textures above, the aux texture, then every
            texture made by "resample" / "snapshot" in the order they are made
  empty     indices of the draw operations that are meant to draw nothing (they
            pin a quirk: a bounding box that truncates to nothing, an early
            return) and are not counted as coverage
  tile, K   ("list" family) the command-list tile (tx, ty) the case aims at and
            the number of its commands that must hit it

run(case, fac) drives any factory of tests/scenes.py (OracleFactory,
GpuFactory, GpuRecordingFactory, GpuPackedFactory(False / True)) and returns
the f64 buffer, the u8 buffer, every get_color probe, every boolean returned by
set_pixel / apply_pixel / restore_state, the f64 contents of every texture made
by resample / as_texure, and the command-list length at every "list_len"
operation.  The packed front end queues set_pixel / apply_pixel /
restore_state and has no result to hand back: those entries are None there and
mismatches() skips them (their effect is still compared through the buffers).

Generators are seeded numpy PCG64 (scenes.rng), not hypothesis: hypothesis
examples differ between processes here (mixed-frame fuzz).

Shapes.  Frames are at most 129x70: widths from {1, 2, 63, 64, 65, 129},
heights from {1, 4, 15, 16, 17, 33, 70}, RGB and RGBA.  Textures are 1x5, 5x1,
2x2, 2x9, 9x2, 3x3 and 16x12, u8 and f64, RGB and RGBA: the smallest sizes that
cross a 64x16 command-list tile, a 64x4 k_prim block and the sampler's w-2
clamp.

Left out on purpose:
  * a shared texture of the destination context drawn into itself: the library
    samples a snapshot, the reference reads while it writes, and the oracle
    cannot stand in for either;
  * non-finite colour arguments, and any case whose oracle buffer holds a NaN
    or an infinity (NaN sign and payload differ between x86 and the GPU, and
    the comparison is bit for bit) -- so no gradient under a transform whose
    inverse is not finite;
  * non-finite geometry is in: it never reaches a colour.
"""
from __future__ import annotations

import ctypes
import hashlib
import math

import numpy as np

import scenes

LONG_MIN, LONG_MAX = -(1 << 63), (1 << 63) - 1
WIDTHS = (1, 2, 63, 64, 65, 129)
HEIGHTS = (1, 4, 15, 16, 17, 33, 70)
TEX_SHAPES = ((1, 5), (5, 1), (2, 2), (2, 9), (9, 2), (3, 3), (16, 12))   # (w, h)
IDENT = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
CL_W, CL_H = 64, 16          # k_cmd_list tile
SENTINEL = 0.3141592653589793

STATE_OPS = {"save", "restore", "set_transform", "apply_transform", "scale", "translate", "rotate",
             "set_ct", "apply_ct"}
DRAW_OPS = {"draw_rect", "draw_texture", "draw_split", "draw_line", "draw_circle", "draw_vgrd",
            "draw_mut_grd", "fill_color"}
QUEUED_OPS = DRAW_OPS | {"set_pixel", "apply_pixel"}


def up(v):
    return math.nextafter(v, math.inf)


def down(v):
    return math.nextafter(v, -math.inf)


# ---------------------------------------------------------------------------
# the interpreter
# ---------------------------------------------------------------------------
def texture_array(spec):
    w, h, dtype, ch, seed = spec
    g = scenes.rng(seed)
    if dtype == "u8":
        return g.integers(0, 256, size=(h, w, ch), dtype=np.uint8)
    return g.uniform(-0.5, 1.5, size=(h, w, ch))


def texture_contents(tex):
    if hasattr(tex, "get_buffer_numpy"):
        return tex.get_buffer_numpy()
    out = np.empty((tex.height, tex.width, 4 if tex.enableAlpha else 3), dtype=np.float64)
    tex.lib.OracleGetTextureBuffer(tex._ptr, out.ctypes.data_as(ctypes.c_void_p))
    return out


class Runner:
    """One context of one factory executing operations one at a time."""

    def __init__(self, case, fac, texs=None):
        W, H, alpha = case["ctx"]
        self.fac = fac
        self.aux = None
        if texs is None:
            texs = [fac.texture(texture_array(s)) for s in case["textures"]]
            if case.get("aux"):
                aw, ah, aalpha, aops = case["aux"]
                self.aux = Runner({"ctx": (aw, ah, aalpha)}, fac, texs=[])
                for op in aops:
                    self.aux.step(op)
                texs.append(self.aux.ctx.as_texture_shared())
        self.texs = texs
        self.ctx = fac.context(W, H, alpha)
        self.probes, self.bools, self.made, self.list_len = [], [], [], []

    def step(self, op):
        c, k, a = self.ctx, op[0], op[1:]
        if k == "set_color": c.set_color(*a)
        elif k == "fill_color": c.fill_color(*a)
        elif k == "save": c.save_state()
        elif k == "restore": self.bools.append(c.restore_state())
        elif k == "set_transform": c.set_transform(*a)
        elif k == "apply_transform": c.apply_transform(*a)
        elif k == "scale": c.scale(*a)
        elif k == "translate": c.translate(*a)
        elif k == "rotate": c.rotate(*a)
        elif k == "set_ct": c.set_color_transform(*a)
        elif k == "apply_ct": c.apply_color_transform(*a)
        elif k == "draw_rect": c.draw_rect(*a)
        elif k == "draw_texture": c.draw_texture(self.texs[a[0]], *a[1:])
        elif k == "draw_split": c.draw_splitted_texture(self.texs[a[0]], *a[1:])
        elif k == "draw_line": c.draw_line(*a)
        elif k == "draw_circle": c.draw_circle(*a)
        elif k == "draw_vgrd": c.draw_vertical_grd(*a)
        elif k == "draw_mut_grd": c.draw_vertical_mut_grd(a[0], a[1], a[2], a[3], [(p, tuple(s)) for p, s in a[4]])
        elif k == "set_pixel": self.bools.append(c.set_pixel(*a))
        elif k == "apply_pixel": self.bools.append(c.apply_pixel(*a))
        elif k == "get_color": self.probes.append(c.get_color(*a))
        elif k == "resample":
            t = self.texs[a[0]].resample(a[1], a[2])
            self.texs.append(t)
            self.made.append(texture_contents(t))
        elif k == "snapshot":
            t = c.as_texure()
            self.texs.append(t)
            self.made.append(texture_contents(t))
        elif k == "list_len":
            # (a packed front end submits what it holds before it answers)
            rec = hasattr(c, "is_recording") and c.is_recording()
            self.list_len.append(int(c.command_list_length()) if rec else None)
        else:
            raise ValueError(f"unknown operation {op!r}")

    def finish(self):
        c = self.ctx
        return {"f64": c.get_buffer_numpy(), "u8": c.get_buffer_as_uint8_numpy(),
                "probes": np.array(self.probes, dtype=np.float64).reshape(-1, 4),
                "bools": [None if b is None else bool(b) for b in self.bools],
                "made": self.made, "list_len": self.list_len}


def run(case, fac, upto=None):
    r = Runner(case, fac)
    for op in case["ops"][:upto]:
        r.step(op)
    return r.finish()


def mismatches(got, want):
    """Names of the returned items that differ (bit for bit) between a library
    run and an oracle run."""
    bad = []
    for k in ("f64", "u8", "probes"):
        if not scenes.bits_equal(got[k], want[k]):
            bad.append(f"{k}: {scenes.first_mismatch(got[k], want[k])}")
    if len(got["bools"]) != len(want["bools"]):
        bad.append("bools: length")
    else:
        for i, (g, w) in enumerate(zip(got["bools"], want["bools"])):
            if g is not None and g != w:
                bad.append(f"bools[{i}]: {g} vs {w}")
    if len(got["made"]) != len(want["made"]):
        bad.append("made: length")
    else:
        for i, (g, w) in enumerate(zip(got["made"], want["made"])):
            if not scenes.bits_equal(g, w):
                bad.append(f"made[{i}]: {scenes.first_mismatch(g, w)}")
    return bad


def trace(case, fac):
    """Runs the case on `fac` (the oracle) and, beside it, every draw operation
    alone: a second context gets the state operations only, and before each draw
    it is cleared to SENTINEL, takes the draw, and is read back.  Returns the
    run's outputs and one record per draw operation: its index, the operation,
    the transform it ran under and the mask (H, W) of the pixels it changed."""
    main = Runner(case, fac)
    alone = Runner(case, fac, texs=main.texs)
    s = SENTINEL
    sent = np.float64(s).view(np.uint64)
    recs = []
    for i, op in enumerate(case["ops"]):
        if op[0] in STATE_OPS:
            alone.step(op)
            alone.bools.clear()
        elif op[0] in DRAW_OPS:
            alone.ctx.set_color(s, s, s, s)
            alone.step(op)
            buf = alone.ctx.get_buffer_numpy()
            recs.append({"i": i, "op": op, "m": tuple(alone.ctx.get_transform()),
                         "mask": (buf.view(np.uint64) != sent).any(axis=2)})
        main.step(op)
    return main.finish(), recs


def describe(case, i, fac):
    """"op 17: ('draw_line', ...) under m = (...)" for a failure message."""
    r = Runner(case, fac)
    for op in case["ops"][:i]:
        if op[0] in STATE_OPS:
            r.step(op)
    return f"op {i}: {case['ops'][i]!r} under m = {tuple(r.ctx.get_transform())!r}"


def digest(case):
    return hashlib.sha256(repr(sorted(case.items())).encode()).hexdigest()


# ---------------------------------------------------------------------------
# Python restatements of the host-side decisions (libNativeCPURenderer.cpp
# lines as cited in nr_prims.hip); Python floats are the same IEEE doubles and
# each expression keeps the source's order
# ---------------------------------------------------------------------------
def py_f2i64(v):
    """(i64)v of x86-64 (cvttsd2si): (value, took the out-of-range arm)."""
    if not (v >= -9223372036854775808.0 and v < 9223372036854775808.0):
        return LONG_MIN, True
    return int(v), False


def py_xform(m, x, y):
    return m[0] * x + m[2] * y + m[4], m[1] * x + m[3] * y + m[5]


def _dmin(a, b):
    return b if b < a else a


def _dmax(a, b):
    return b if a < b else a


def py_get_boarder(m, x, y, w, h, W, H):
    """cpp:693-718 -> (l, r, t, b, some corner took the LONG_MIN arm)."""
    ltx, lty = py_xform(m, x, y)
    rtx, rty = py_xform(m, x + w, y)
    lbx, lby = py_xform(m, x, y + h)
    rbx, rby = py_xform(m, x + w, y + h)
    vals = [py_f2i64(_dmin(_dmin(ltx, rtx), _dmin(lbx, rbx))), py_f2i64(_dmax(_dmax(ltx, rtx), _dmax(lbx, rbx))),
            py_f2i64(_dmin(_dmin(lty, rty), _dmin(lby, rby))), py_f2i64(_dmax(_dmax(lty, rty), _dmax(lby, rby)))]
    lim = (W, W, H, H)
    out = [max(0, min(lim[k], vals[k][0])) for k in range(4)]
    return out[0], out[1], out[2], out[3], any(v[1] for v in vals)


def py_fast_range(x, w, limit):
    """cpp:741-742 as nr_prims.hip fast_range -> (lo, hi, arms reached)."""
    arms = set()
    lim = x + w
    s, low = py_f2i64(x)
    if low:
        arms.add("long_min")
    if not (float(s) < lim):
        return 0, 0, arms
    if not (lim < 9.0e15):
        e = LONG_MAX
        arms.add("long_max")
    else:
        e = math.ceil(lim)
        while float(e - 1) >= lim:
            e -= 1
            arms.add("ceil_down")
        while float(e) < lim:
            e += 1
            arms.add("ceil_up")
    return max(s, 0), min(e, limit), arms


def py_is_no_transform(m):
    return m[0] - 1 + m[1] + m[2] + m[3] - 1 + m[4] + m[5] < 1e-5


def _ffloor(v):
    return v if math.isinf(v) else float(math.floor(v))


def _fceil(v):
    return v if math.isinf(v) else float(math.ceil(v))


def py_line_box(m, x1, y1, x2, y2, width, W, H):
    """DrawLine's host-side scan range (nr_prims.hip DrawLine): None when the
    call returns early, else (kind, i0, i1, j0, j1) with kind "cull", "singular"
    (det == 0 or not finite) or "nonfinite" (a transformed corner is)."""
    if width <= 0:
        return None
    dx, dy = x2 - x1, y2 - y1
    ln = math.sqrt(dx * dx + dy * dy)
    if ln == 0:
        return None
    ux, uy = dx / ln, dy / ln
    vx, vy = -uy, ux
    hw = width / 2
    pts = [(x1 - vx * hw, y1 - vy * hw), (x1 + vx * hw, y1 + vy * hw),
           (x2 + vx * hw, y2 + vy * hw), (x2 - vx * hw, y2 - vy * hw)]
    det = m[0] * m[3] - m[1] * m[2]
    if not (det != 0) or not math.isfinite(det):
        return ("singular", 0, W, 0, H)
    mnx = mny = math.inf
    mxx = mxy = -math.inf
    for px, py in pts:
        sx, sy = py_xform(m, px, py)
        if not math.isfinite(sx) or not math.isfinite(sy):
            return ("nonfinite", 0, W, 0, H)
        mnx, mxx = min(mnx, sx), max(mxx, sx)
        mny, mxy = min(mny, sy), max(mxy, sy)
    mag = max(max(abs(mnx), abs(mxx)), max(abs(mny), abs(mxy)))
    margin = 2.0 + mag * 1e-9
    fx0, fx1 = _ffloor(mnx - margin), _fceil(mxx + margin) + 1
    fy0, fy1 = _ffloor(mny - margin), _fceil(mxy + margin) + 1
    return ("cull", int(max(0.0, min(float(W), fx0))), int(max(0.0, min(float(W), fx1))),
            int(max(0.0, min(float(H), fy0))), int(max(0.0, min(float(H), fy1))))


def py_ranges(op, m, W, H):
    """Pixel ranges (i0, i1, j0, j1) of the commands the operation queues on a
    recording context, in order (an empty range queues nothing), and the arms of
    the bound computations it took."""
    k, a = op[0], op[1:]
    arms, out = set(), []

    def border(x, y, w, h):
        l, r, t, b, low = py_get_boarder(m, x, y, w, h, W, H)
        if low:
            arms.add("f2i64_long_min")
        out.append((l, r, t, b))

    if k in ("draw_rect", "draw_vgrd"):
        if a[2] > 0 and a[3] > 0:
            border(a[0], a[1], a[2], a[3])
    elif k == "draw_mut_grd":
        x, y, w, h, steps = a
        for (p, _), (q, _) in zip(steps, steps[1:]):
            if w > 0 and h * (q - p) > 0:
                border(x, y + h * p, w, h * (q - p))
    elif k == "draw_circle":
        if a[2] > 0:
            border(a[0] - a[2], a[1] - a[2], 2 * a[2], 2 * a[2])
    elif k == "draw_texture":
        _, x, y, w, h = a
        if w != 0 and h != 0:
            if py_is_no_transform(m):
                i0, i1, a0 = py_fast_range(x, w, W)
                j0, j1, a1 = py_fast_range(y, h, H)
                arms |= {"fast"} | a0 | a1
                out.append((i0, i1, j0, j1))
            else:
                arms.add("inverse")
                border(x, y, w, h)
    elif k == "draw_split":
        if a[3] != 0 and a[4] != 0:
            border(a[1], a[2], a[3], a[4])
    elif k == "draw_line":
        box = py_line_box(m, a[0], a[1], a[2], a[3], a[4], W, H)
        if box:
            arms.add("line_" + box[0])
            out.append(box[1:])
    elif k == "fill_color":
        out.append((0, W, 0, H))
    elif k == "apply_pixel":
        if 0 <= a[0] < W and 0 <= a[1] < H:
            out.append((a[0], a[0] + 1, a[1], a[1] + 1))
    elif k == "set_pixel":
        x, y = a[0], a[1]
        if 0 <= x < W and 0 <= y < H:
            out.append((0, W, y, min(y + 2, H)) if x + 1 == W else (x, x + 2, y, y + 1))
    return [r for r in out if r[1] > r[0] and r[3] > r[2]], arms


def hits_tile(r, tx, ty):
    """k_cmd_list's test of a command's range against tile (tx, ty)."""
    x0, y0 = tx * CL_W, ty * CL_H
    return not (r[0] >= x0 + CL_W or r[1] <= x0 or r[2] >= y0 + CL_H or r[3] <= y0)


# ---------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------
def _col(g, alpha=None):
    a = float(g.choice([1.0, g.uniform(0.2, 0.9)])) if alpha is None else alpha
    return tuple(float(v) for v in g.uniform(0, 1, 3)) + (a,)


def _case(family, seed, ctx, textures, ops, empty=(), aux=None, **extra):
    d = {"name": f"{family}-{seed}", "ctx": ctx, "textures": list(textures), "aux": aux,
         "ops": list(ops), "empty": tuple(sorted(empty))}
    d.update(extra)
    return d


class _Ops(list):
    """An operation list that remembers which draws are meant to be empty."""

    def __init__(self):
        super().__init__()
        self.empty = []

    def add(self, *op, empty=False):
        if empty:
            self.empty.append(len(self))
        self.append(tuple(op))


def gen_bounds(seed):
    """Quad edges on integers, on pixel centres and one ulp either side; sums
    that round; coordinates at 2^53, 9.0e15, 9.3e18 and 1e300; quads that hold
    the whole screen or miss it by a pixel; zero and negative sizes."""
    g = scenes.rng(1000 + seed)
    W, H = WIDTHS[seed % 6], HEIGHTS[(2 * seed + 1) % 7]
    texs = [(3, 3, "u8", 4, 11 + seed), (16, 12, "f64", 3, 12 + seed)]
    o = _Ops()
    o.add("set_color", 0.125, 0.125, 0.125, 0.125)
    # (a frame 1 or 2 pixels wide or high takes a quad that starts one pixel before it,
    # so that the half-pixel and one-ulp shifts below still leave pixel 0 inside)
    x0, y0 = float(W // 4 - (W <= 2)), float(H // 4 - (H <= 2))
    w0, h0 = float(max(2, W // 2)), float(max(2, H // 2))

    def quads(x, y, w, h, k):
        """One quad through every bounded primitive (k picks the kind)."""
        kind = k % 4
        if kind == 0: o.add("draw_rect", x, y, w, h, *_col(g))
        elif kind == 1: o.add("draw_texture", k % 2, x, y, w, h)
        elif kind == 2: o.add("draw_split", (k // 4) % 2, x, y, w, h, 0.1, 0.9, 0.2, 1.0)
        else: o.add("draw_vgrd", x, y, w, h, *_col(g), *_col(g))

    for rnd, m in enumerate((IDENT, (1.0, 0.0, 0.0, 1.0, 0.25, 0.5))):   # fast path, then inverse path
        o.add("set_transform", *m)
        k = rnd
        for dx in (0.0, 0.5):
            for x, y in ((x0 + dx, y0 + dx), (down(x0 + dx), up(y0 + dx)), (up(x0 + dx), down(y0 + dx))):
                for w, h in ((w0, h0), (down(w0), up(h0))):
                    quads(x, y, w, h, k)
                    k += 1
        quads(x0 + 0.1, y0 + 0.7, w0 + 0.2, h0 + 0.1, k)          # x + w rounds
        quads(-5.0, -5.0, W + 10.0, H + 10.0, k + 1)              # holds the whole screen
        quads(-3.5, -2.5, W + 7.0, H + 5.0, k + 2)
        quads(-3.5, -2.5, W + 7.0, H + 5.0, k + 3)
        quads(-3.5, -2.5, W + 7.0, H + 5.0, k + 4)
        # one pixel off each side: the truncated box is empty
        for j, (x, y, w, h) in enumerate(((-2.5, 0.0, 1.0, float(H)), (W + 1.0, 0.0, 3.0, float(H)),
                                          (0.0, -2.5, float(W), 1.0), (0.0, H + 1.0, float(W), 3.0))):
            kind = j + rnd
            if kind % 2 == 0: o.add("draw_rect", x, y, w, h, *_col(g), empty=True)
            else: o.add("draw_texture", 0, x, y, w, h, empty=True)
    o.add("set_transform", *IDENT)
    big = float(2 ** 53)
    o.add("draw_rect", -big, -big, 2 * big, 2 * big, *_col(g))
    o.add("draw_texture", 1, -1.0, -1.0, big + 5, big + 5)                      # lim = 2^53 + 4 (> 9.0e15: LONG_MAX)
    o.add("draw_texture", 0, -1.0e15, -1.0e15, 1.0e16 + 1.0, 1.0e16 + 1.0)       # lim >= 9.0e15: LONG_MAX
    o.add("draw_texture", 1, -1.0e15, -2.0, up(1.0e16) - 2.0e15, 8.9e15)         # around 9.0e15 from both sides
    o.add("draw_texture", 0, -9.3e18, -9.3e18, 1.9e19, 1.9e19)                   # start below LONG_MIN
    o.add("draw_rect", -9.3e18, -9.3e18, 9.3e18 + 4096, 9.3e18 + 4096, *_col(g))  # corner below LONG_MIN
    o.add("draw_rect", -1e300, -1e300, 2e300, 2e300, *_col(g), empty=True)        # both corners -> LONG_MIN: empty box
    o.add("draw_texture", 1, -1e300, -1e300, 2e300, 2e300)                        # fast path: the whole screen
    o.add("set_transform", 1.0, 0.0, 0.0, 1.0, 0.25, 0.5)
    o.add("draw_split", 0, -9.3e18, -9.3e18, 9.3e18 + 4096, 9.3e18 + 4096, 0.0, 1.0, 0.0, 1.0)
    o.add("draw_texture", 1, -1e300, -1e300, 2e300, 2e300, empty=True)
    o.add("draw_circle", 0.0, 0.0, 1e300, *_col(g), empty=True)
    for m in (IDENT, (1.0, 0.0, 0.0, 1.0, 0.25, 0.5)):                            # zero and negative sizes
        o.add("set_transform", *m)
        o.add("draw_rect", x0, y0, 0.0, h0, *_col(g), empty=True)
        o.add("draw_rect", x0, y0, w0, -3.0, *_col(g), empty=True)
        o.add("draw_texture", 0, x0, y0, 0.0, h0, empty=True)
        o.add("draw_texture", 1, x0 + w0, y0 + h0, -w0, -h0, empty=True)
        o.add("draw_split", 0, x0 + w0, y0, -w0, h0, 0.0, 1.0, 0.0, 1.0, empty=True)
        o.add("draw_vgrd", x0, y0, -1.0, h0, *_col(g), *_col(g), empty=True)
        o.add("draw_circle", x0, y0, 0.0, *_col(g), empty=True)
    return _case("bounds", seed, (W, H, seed % 2 == 1), texs, o, o.empty)


def threshold_matrices():
    """Matrices whose signed sum (cpp:551-553) lies within 1e-6 of 1e-5, on both sides."""
    out = []
    for d in (1e-6, -1e-6, 1e-7, -1e-7):
        out.append((1.0, 0.0, 0.0, 1.0, 1e-5 + d, 0.0))
        out.append((1.0, 0.0, 0.0, 1.0, 0.0, 1e-5 + d))
    out.append((1.0, 0.0, 0.0, 1.0, up(1e-5), 0.0))
    out.append((1.0, 0.0, 0.0, 1.0, down(1e-5), 0.0))
    out.append((1.0, 0.0, 0.0, 1.0, 1e-5, 0.0))
    out.append((1.0, 5e-6, 5e-6 + 1e-7, 1.0, 0.0, 0.0))
    out.append((1.0, 5e-6, 5e-6 - 1e-7, 1.0, 0.0, 0.0))
    return out


def gen_fastpath(seed):
    """DrawTexture around IsNoTransform's threshold, under pure rotations and
    under large negative translations (fast path: the transform is ignored), and
    the same matrices with DrawSplittedTexture and DrawRect, which honour it."""
    g = scenes.rng(2000 + seed)
    W, H = (63, 64, 65, 129, 64, 65)[seed % 6], (33, 70, 17, 33, 16, 70)[seed % 6]
    texs = [(16, 12, "u8", 4, 21 + seed), (3, 3, "f64", 3, 22 + seed), (2, 9, "u8", 3, 23 + seed)]
    o = _Ops()
    o.add("set_color", 0.25, 0.25, 0.25, 0.25)
    mats = threshold_matrices()
    for ang in (0.3, -0.2, 0.05, math.pi / 2):
        c, s = math.cos(ang), math.sin(ang)
        mats.append((c, s, -s, c, 0.0, 0.0))                       # pure rotation: the sum is 2c - 2 < 0
        mats.append((c, s, -s, c, W / 2, 0.0))                     # ... about a point: the sum is positive
    for tx, ty in ((-1000.0, -1000.0), (-1e9, 3.0), (-W * 1.0, -H * 1.0)):
        mats.append((1.0, 0.0, 0.0, 1.0, tx, ty))                  # large negative translation
    mats.append((2.0, 0.0, 0.0, 0.5, -W / 2, -10.0))               # a scale that the fast path ignores
    for k, m in enumerate(mats):
        o.add("set_transform", *m)
        x, y = float(g.uniform(0, W / 3)), float(g.uniform(0, H / 3))
        w, h = float(g.uniform(W / 4, W / 2)), float(g.uniform(H / 4, H / 2))
        o.add("draw_texture", k % 3, x, y, w, h)
        # the same screen quad in user space, for the draws that honour the transform
        det = m[0] * m[3] - m[1] * m[2]
        ux = (m[3] * (x - m[4]) - m[2] * (y - m[5])) / det
        uy = (-m[1] * (x - m[4]) + m[0] * (y - m[5])) / det
        uw, uh = w / math.hypot(m[0], m[1]), h / math.hypot(m[2], m[3])
        o.add("draw_split", (k + 1) % 3, ux, uy, uw, uh, 0.0, 1.0, 0.0, 1.0)
        o.add("draw_rect", ux + uw / 4, uy + uh / 4, uw / 2, uh / 2, *_col(g))
    return _case("fastpath", seed, (W, H, seed % 2 == 0), texs, o, o.empty)


def gen_texel(seed):
    """Every small texture at scales that put u, v exactly on texel boundaries
    (fast and inverse path), and split ranges that are reversed, empty or reach
    outside [0, 1]; f64 texels outside [0, 1]; textures 1 texel wide or high."""
    W, H = (63, 64, 65, 129)[seed % 4], (33, 70)[seed % 2]
    texs = [(tw, th, ("u8", "f64")[(seed + k) % 2], (3, 4)[(seed // 2 + k) % 2], 31 + 7 * seed + k)
            for k, (tw, th) in enumerate(TEX_SHAPES)]
    o = _Ops()
    o.add("set_color", 0.0, 0.0, 0.0, 0.0)
    for k, (tw, th) in enumerate(TEX_SHAPES):
        o.add("set_transform", *IDENT)
        o.add("draw_texture", k, 1.0 + k, 1.0, tw * 2.0, th * 2.0)             # u = (i - x) / 2
        o.add("draw_texture", k, 20.0 + k, 2.0, float(tw), float(th))          # u = i - x
        o.add("draw_texture", k, 2.5 + k, 0.5, tw * 4.0, th * 2.0)             # u on quarter texels
        o.add("set_transform", 1.0, 0.0, 0.0, 1.0, 0.5, 0.25)                  # inverse path, ix = i - 0.5
        o.add("draw_texture", k, 0.5 + k, 10.75, tw * 2.0, th * 2.0)
        o.add("draw_split", k, 30.5, 0.75, tw * 2.0, th * 2.0, 0.0, 1.0, 0.0, 1.0)
        o.add("draw_split", k, 3.5 + k, 5.75, 24.0, 16.0, 0.9, 0.1, 1.0, 0.0)   # reversed
        o.add("draw_split", k, 8.5, 3.75 + k, 16.0, 12.0, 0.5, 0.5, 0.25, 0.25)  # empty range
        o.add("draw_split", k, 12.5, 1.75, 20.0, 18.0, -0.5, 1.5, -0.25, 1.25)  # reaches outside [0, 1]
        o.add("draw_split", k, 1.5, 2.75, 9.0, 7.0, 2.0, 3.0, -2.0, -1.0)       # wholly outside
        o.add("draw_split", k, 40.5, 4.75, 2.0 * tw, 2.0 * th, 0.0, 0.5, 0.5, 1.0)
    return _case("texel", seed, (W, H, seed % 2 == 1), texs, o, o.empty)


def edge_matrices(W, H):
    """(name, matrix) of the transforms the `transform` and `line` families
    draw under; each maps user points near the origin to the screen centre."""
    cx, cy = float(W // 2), float(H // 2)
    out = [("reflect_x", (-1.0, 0.0, 0.0, 1.0, cx, cy)), ("reflect_y", (1.0, 0.0, 0.0, -1.0, cx, cy)),
           ("swap", (0.0, 1.0, 1.0, 0.0, cx, cy)), ("aniso", (1e-6, 0.0, 0.0, 1e6, cx, cy)),
           ("aniso_t", (1e6, 0.0, 0.0, 1e-6, cx, cy)), ("neg_det_small", (1.0, 1.0, 1.0, 1.0 - 1e-9, cx, cy))]
    for eps in (1e-3, 1e-6, 1e-9, 1e-12):
        out.append((f"shear_{eps:g}", (1.0, 1.0, 1.0, 1.0 + eps, cx, cy)))
    out.append(("singular", (1.0, 1.0, 1.0, 1.0, cx, cy)))
    out.append(("zero", (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)))
    out.append(("subnormal_det", (1e-160, 0.0, 0.0, 1e-160, cx, cy)))
    return out


def _user_extent(name, m):
    """Half-sizes (ex, ey) of a user-space quad about the origin that lands on
    about 10 screen pixels around the centre under matrix `name`."""
    if name.startswith("aniso"):
        return 10.0 / m[0], 10.0 / m[3]
    if name.startswith("shear") or name == "neg_det_small":
        d = abs(m[0] * m[3] - m[1] * m[2])
        return 5.0 / d, 5.0 / d          # the band |(i - cx) - (j - cy)| <= ~5 of the near-singular map
    if name == "subnormal_det":
        return 1e161, 1e161
    if name in ("singular", "zero"):
        return 1e10, 1e10                # inv_det = 1e9: every pixel maps within 1e12 of the origin
    return 10.0, 6.0


def gen_transform(seed):
    """Every primitive under reflections, strong anisotropy, shears from
    det 1e-3 down to a subnormal determinant and det == 0; a deep save /
    restore stack and a restore on an empty stack."""
    g = scenes.rng(4000 + seed)
    W, H = (63, 64, 65, 129, 65, 64)[seed % 6], (33, 70, 17, 33, 70, 16)[seed % 6]
    texs = [(3, 3, "u8", 4, 41 + seed), (2, 2, "f64", 3, 42 + seed)]
    o = _Ops()
    o.add("set_color", 0.5, 0.5, 0.5, 0.5)
    o.add("restore")                                               # empty stack: false
    for name, m in edge_matrices(W, H):
        o.add("set_transform", *m)
        ex, ey = _user_extent(name, m)
        finite_inv = name != "subnormal_det"
        point = name == "zero"          # every corner maps to pixel (0, 0): GetBoarder's box is empty
        o.add("draw_rect", -ex, -ey, 2 * ex, 2 * ey, *_col(g), empty=point)
        o.add("draw_texture", 0, -ex, -ey, 2 * ex, 2 * ey)         # (the zero matrix sums to -2: the fast path)
        o.add("draw_split", 1, -ex / 2, -ey / 2, ex, ey, 0.0, 1.0, 0.0, 1.0, empty=point)
        o.add("draw_circle", 0.0, 0.0, max(ex, ey), *_col(g), empty=point)
        if finite_inv:                                             # (a NaN inverse makes a gradient NaN)
            o.add("draw_vgrd", -ex, -ey, 2 * ex, 2 * ey, *_col(g), *_col(g), empty=point)
        o.add("draw_line", -ex, 0.0, ex, 0.0, ey / 2, *_col(g), empty=not finite_inv)
    o.add("set_transform", *IDENT)
    for k in range(20):                                            # deeper than any stack's first allocation
        o.add("save")
        o.add("apply_transform", 1.0, 0.01 * (k % 3), -0.01, 1.0, 1.0, 0.5)
        o.add("apply_ct", 0.97, 1.0, 0.98, 1.0)
        if k % 4 == 0:
            o.add("draw_rect", float(k), 1.0, W / 3, H / 3, *_col(g))
            o.add("rotate", 0.05)
            o.add("draw_texture", 0, W / 4, H / 8, W / 3, H / 2)
    for k in range(22):                                            # two more than were saved
        o.add("restore")
        if k % 5 == 0:
            o.add("draw_circle", W / 2 - k, H / 2, 4.5, *_col(g))
    return _case("transform", seed, (W, H, seed % 2 == 1), texs, o, o.empty)


def gen_line(seed):
    """Lines under the edge matrices, partly and wholly off screen, widths from
    1e-3 to 1e6, a length that underflows, axis-aligned lines (horizontal
    polygon edges), endpoints at 1e12, and both full-scan fallbacks."""
    g = scenes.rng(5000 + seed)
    W, H = (63, 64, 65, 129, 129, 2)[seed % 6], (33, 70, 17, 33, 15, 70)[seed % 6]
    o = _Ops()
    o.add("set_color", 0.75, 0.75, 0.75, 0.75)
    for name, m in edge_matrices(W, H):
        o.add("set_transform", *m)
        ex, ey = _user_extent(name, m)
        nan_inv = name == "subnormal_det"
        o.add("draw_line", -ex, 0.0, ex, 0.0, ey / 2, *_col(g, 1.0), empty=nan_inv)
        o.add("draw_line", -ex / 2, -ey / 2, ex / 2, ey / 2, ey / 4, *_col(g), empty=nan_inv)
        o.add("draw_line", 0.0, -ey, 0.0, ey, ex / 3, *_col(g), empty=nan_inv)
    o.add("set_transform", *IDENT)
    r = min(W, H)
    o.add("draw_line", 0.0, 0.0, r - 1.0, r - 1.0, 1e-3, *_col(g, 1.0))            # through the pixel centres (i, i)
    o.add("draw_line", 0.0, H // 2 * 1.0, W * 1.0, H // 2 * 1.0, 1e-3, *_col(g))   # horizontal, on a pixel row
    o.add("draw_line", W // 2 * 1.0, -3.0, W // 2 * 1.0, H + 3.0, 1.0, *_col(g))   # vertical: horizontal end edges
    o.add("draw_line", 0.0, 1.0, W - 1.0, 1.0, 2.0, *_col(g))                      # edges exactly on rows 0 and 2
    o.add("draw_line", -20.0, -10.0, W / 2, H / 2, 3.0, *_col(g))                  # partly off screen
    o.add("draw_line", W / 2, H / 2, W + 50.0, H + 9.0, 2.5, *_col(g))
    o.add("draw_line", -30.0, -5.0, -3.0, -40.0, 2.0, *_col(g), empty=True)        # wholly off screen
    o.add("draw_line", W + 5.0, 0.0, W + 9.0, H * 1.0, 3.0, *_col(g), empty=True)
    for wd in (1e-3, 0.1, 1.0, 30.0, 1e3, 1e6):
        o.add("draw_line", 0.0, 0.0, W - 1.0, (W - 1.0) * (H > 1), wd, *_col(g))
    o.add("draw_line", 5.0, 5.0, 5.0 + 1e-170, 5.0, 3.0, *_col(g), empty=True)     # dx * dx underflows: len == 0
    o.add("draw_line", 1.0, 1.0, 1.0, 1.0, 3.0, *_col(g), empty=True)
    o.add("draw_line", 1.0, 1.0, 9.0, 3.0, 0.0, *_col(g), empty=True)              # width <= 0
    o.add("draw_line", 1.0, 1.0, 9.0, 3.0, -2.0, *_col(g), empty=True)
    o.add("draw_line", -1e12, -1e12, 1e12, 1e12, 3.0, *_col(g))                    # endpoints at 1e12
    o.add("draw_line", -1e12, H / 2, 1e12, H / 2 + 1.0, 2.0, *_col(g))
    o.add("set_transform", 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)                           # singular: the full scan
    o.add("draw_line", -1.0, -1.0, 1.0, 1.0, 2.0, *_col(g))
    o.add("set_transform", 2.0, 4.0, 1.0, 2.0, 3.0, 1.0)                           # det == 0 with a translation
    o.add("draw_line", -1e10, -1e10, 1e10, 1e10, 1e10, *_col(g))
    o.add("set_transform", 1e160, 0.0, 0.0, 1e-160, 0.0, 0.0)                      # finite det, a corner overflows
    o.add("draw_line", -1e150, -1e150, 1e150, 1e150, 1e150, *_col(g))
    o.add("set_transform", 1e200, 0.0, 0.0, 1e200, 0.0, 0.0)                       # det overflows
    o.add("draw_line", -1e-100 * W, -1e-100 * H, 1e-100 * W, 1e-100 * H, 1e-100, *_col(g))
    return _case("line", seed, (W, H, seed % 2 == 0), [], o, o.empty)


def gen_circle_grad(seed):
    """Circles below half a pixel, dist == radius, huge radii, the
    subnormal-determinant circle; gradients of tiny height, repeated stops."""
    g = scenes.rng(6000 + seed)
    W, H = (63, 64, 65, 129, 64, 65)[seed % 6], (33, 70, 17, 33, 15, 16)[seed % 6]
    o = _Ops()
    o.add("set_color", 1.0, 1.0, 1.0, 1.0)
    cx, cy = float(W // 2), float(H // 2)
    # radius < 1/2: the truncated box [l, r) never holds a covered pixel
    o.add("draw_circle", cx, cy, 0.3, *_col(g), empty=True)
    o.add("draw_circle", cx + 0.2, cy - 0.4, 0.45, *_col(g), empty=True)
    o.add("draw_circle", 0.1, 0.1, 0.4, *_col(g), empty=True)
    o.add("save")
    o.add("scale", 3.0, 3.0)                                   # ... but under a scale it is 1.2 pixels
    o.add("draw_circle", cx / 3, cy / 3, 0.4, *_col(g))
    o.add("draw_circle", 2.1, 1.9, 0.49, *_col(g))
    o.add("restore")
    for rad in (1.0, 2.0, 5.0, 13.0):                          # centre on a pixel, integer radius: dist == radius
        o.add("draw_circle", cx, cy, rad, *_col(g))
    o.add("draw_circle", 5.0, 5.0, 5.0, *_col(g))              # (2, 1), (1, 2): 3-4-5
    o.add("draw_circle", cx + 0.5, cy + 0.5, 2.5, *_col(g))
    for rad in (1e4, 1e10, 1e18):                              # huge
        o.add("draw_circle", cx, cy, rad, *_col(g))
    o.add("draw_circle", cx, cy, 1e19, *_col(g), empty=True)   # x + r beyond i64: LONG_MIN, an empty box
    o.add("draw_circle", cx, cy, 1e300, *_col(g), empty=True)
    o.add("set_transform", 1e-160, 0.0, 0.0, 1e-160, cx, cy)   # subnormal det: inf/NaN inverse, NaN > r is false
    o.add("draw_circle", 0.0, 0.0, 1e161, *_col(g))
    o.add("draw_circle", 1e160, -1e160, 4e160, *_col(g))
    o.add("set_transform", *IDENT)
    # gradients
    o.add("draw_vgrd", 1.0, cy, W - 2.0, 1e-9, *_col(g), *_col(g), empty=True)    # h < 1: an empty box
    o.add("draw_vgrd", 1.0, cy - 0.5, W - 2.0, 0.75, *_col(g), *_col(g), empty=True)
    o.add("draw_vgrd", 0.0, 0.0, W * 1.0, 1.0, *_col(g), *_col(g))                 # one row: t = 0
    o.add("draw_vgrd", 0.0, down(1.0), W * 1.0, 2.0, *_col(g), *_col(g))
    o.add("save")
    o.add("scale", 1.0, 1e9)                                   # tiny user-space height, rows 2..H-2 on screen
    o.add("draw_vgrd", 1.0, 2e-9, W - 2.0, (H - 4.0) * 1e-9 if H > 6 else 3e-9, *_col(g), *_col(g))
    o.add("restore")
    o.add("set_transform", 1.0, 0.0, 0.0, 1e300, 0.0, 0.0)
    o.add("draw_vgrd", 0.0, 2e-300, W / 2, (H - 3.0) * 1e-300, *_col(g), *_col(g))
    o.add("set_transform", 1.0, 0.0, 0.0, 1e-300, 0.0, 1.0)    # user heights around 1e300
    o.add("draw_vgrd", W / 4, 0.0, W / 2, 1e301, *_col(g), *_col(g))
    o.add("set_transform", *IDENT)
    c = [_col(g) for _ in range(5)]
    o.add("draw_mut_grd", 0.0, 1.0, W * 1.0, H - 1.0,
          ((0.0, c[0]), (0.5, c[1]), (0.5, c[2]), (0.5, c[3]), (1.0, c[4])))       # repeated stops: zero-height bands
    o.add("draw_mut_grd", W / 4, 0.0, W / 2, H * 1.0, ((0.0, c[1]), (0.0, c[2]), (1.0, c[3]), (1.0, c[0])))
    o.add("draw_mut_grd", 0.0, 0.0, W * 1.0, H * 1.0, ((0.0, c[4]), (1.0, c[0]), (0.25, c[2])))   # a stop that goes back
    return _case("circle_grad", seed, (W, H, seed % 2 == 1), [], o, o.empty)


def gen_blend(seed):
    """Source alpha and colour transforms whose product is exactly 1, one ulp
    off, 0, negative or above 1; zero and negative colour transforms; a
    fill_color after each."""
    g = scenes.rng(7000 + seed)
    W, H = WIDTHS[(seed + 2) % 6], HEIGHTS[(3 * seed + 2) % 7]
    alpha = seed % 2 == 0
    texs = [(3, 3, "f64", 4, 71 + seed), (2, 2, "u8", 4, 72 + seed)]
    o = _Ops()
    o.add("set_color", 0.2, 0.4, 0.6, 0.8)
    pairs = [(0.5, 2.0), (0.25, 4.0), (up(0.5), 2.0), (down(0.5), 2.0), (1.0, up(1.0)), (1.0, down(1.0)),
             (0.0, 1.0), (0.7, 0.0), (-0.5, 1.0), (0.5, -1.0), (1.5, 1.0), (0.75, 2.0), (1.0, 1.0),
             (3.0, 1.0 / 3.0), (0.1, 10.0), (-1.0, -1.0)]
    cts = [(1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (-1.0, -0.5, 2.0), (0.5, 1.0, 0.0)]
    for k, (a, ct3) in enumerate(pairs):
        ct = cts[(k + seed) % 4]
        o.add("set_ct", ct[0], ct[1], ct[2], ct3)
        noop = (a * ct3 == 0) and not alpha            # RGB, alpha 0: dst * 1 + src * 0
        rgb = tuple(float(v) for v in g.uniform(0, 1, 3))
        kind = (k + seed) % 4
        if kind == 0: o.add("draw_rect", -1.0, -1.0, W / 2 + 2, H + 2.0, *rgb, a, empty=noop)
        elif kind == 1: o.add("draw_circle", W / 2, H / 2, W + H + 0.0, *rgb, a, empty=noop)
        elif kind == 2: o.add("draw_vgrd", 0.0, 0.0, W * 1.0, H * 1.0, *rgb, a, *rgb[::-1], a, empty=noop)
        else: o.add("draw_line", -1.0, H / 2 - 0.5, W + 1.0, H / 2 - 0.5, H + 4.0, *rgb, a, empty=noop)
        o.add("apply_pixel", W - 1, H - 1, *rgb, a)
        o.add("apply_pixel", 0, 0, *rgb[::-1], a)
        fa = (1.0, 0.5, a, 0.0)[k % 4]
        o.add("fill_color", *_col(g, fa), empty=(fa * ct3 == 0 and not alpha))
    for k, ct3 in enumerate((1.0, 2.0, -1.0, 0.0, up(1.0))):   # texel alpha through the colour transform
        o.add("set_ct", 1.0, -1.0, 0.0, ct3)
        o.add("draw_texture", k % 2, 0.0, 0.0, W * 1.0, H * 1.0, empty=(ct3 == 0 and not alpha))
        o.add("fill_color", 0.3, 0.3, 0.3, 0.5, empty=(ct3 == 0 and not alpha))
    return _case("blend", seed, (W, H, alpha), texs, o, o.empty)


def gen_pixels(seed):
    """set_pixel / apply_pixel at the corners, at W-1 on every row, at the last
    pixel and out of range; set_color uniform and non-uniform; get_color at
    negative, fractional and past-the-end coordinates.  One seed per frame shape
    and alpha."""
    g = scenes.rng(8000 + seed)
    W, H = WIDTHS[seed % 6], HEIGHTS[(seed // 6) % 7]
    alpha = seed >= 42
    o = _Ops()
    o.add("set_color", 0.1, 0.2, 0.3, 0.9)                     # non-uniform: the SetPixel overrun on RGB
    probes = [(0.0, 0.0), (-3.5, -0.25), (W - 1.0, H - 1.0), (W - 0.5, H - 0.5), (W * 1.0, H * 1.0),
              (W + 7.0, -2.0), (0.999, H / 2), (W / 2, 0.5), (1e300, 1e300), (-1e300, 1e18), (1.0, 1.0)]
    for p in probes:
        o.add("get_color", *p)
    corners = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    for x, y in corners:
        o.add("set_pixel", x, y, *_col(g))
    for y in range(H):
        o.add("set_pixel", W - 1, y, *_col(g))                 # the overrun wraps into the next row
        if y % 3 == 0:
            o.add("apply_pixel", W - 1, y, *_col(g))
    o.add("set_ct", 0.5, 1.0, 2.0, 0.5)
    for x, y in corners + [(W // 2, H // 2)]:
        o.add("apply_pixel", x, y, *_col(g))
    outside = [(-1, 0), (0, -1), (W, 0), (0, H), (W, H), (-1, -1), (1 << 40, 0), (0, -(1 << 62)), (W - 1, H)]
    for x, y in outside:
        o.add("set_pixel", x, y, *_col(g))
        o.add("apply_pixel", x, y, *_col(g))
    for p in probes[:6]:
        o.add("get_color", *p)
    o.add("set_color", 0.375, 0.375, 0.375, 0.375)             # uniform: a pending clear
    o.add("set_pixel", W - 1, H - 1, *_col(g))                 # the last pixel: no store past the end
    o.add("set_pixel", W - 1, 0, *_col(g))
    o.add("apply_pixel", 0, H - 1, *_col(g))
    o.add("get_color", W - 1.0, H - 1.0)
    o.add("set_color", 0.9, 0.8, 0.7, 0.6)                     # non-uniform over queued pixels
    o.add("set_pixel", 0, 0, *_col(g))
    for p in probes[:5]:
        o.add("get_color", *p)
    o.add("set_color", 0.5, 0.5, 0.5, 0.25)                    # three equal, alpha differs: non-uniform
    return _case("pixels", seed, (W, H, alpha), [], o, o.empty)


def _small_draw(g, o, x0, x1, y0, y1):
    """One small draw with its pixel range inside [x0, x1) x [y0, y1) (identity transform)."""
    kind = int(g.integers(0, 5))
    x, y = int(g.integers(x0, max(x0 + 1, x1 - 3))), int(g.integers(y0, max(y0 + 1, y1 - 3)))
    if kind == 0 and x + 3 <= x1 and y + 3 <= y1: o.add("draw_rect", x + 0.0, y + 0.0, 2.5, 1.5, *_col(g))
    elif kind == 1 and x + 4 <= x1 and y + 4 <= y1: o.add("draw_circle", x + 1.5, y + 1.5, 1.5, *_col(g))
    elif kind == 2 and x + 2 <= x1: o.add("set_pixel", x, y, *_col(g))
    elif kind == 3 and x + 3 <= x1 and y + 3 <= y1: o.add("draw_vgrd", x + 0.0, y + 0.0, 2.0, 2.0, *_col(g), *_col(g))
    else: o.add("apply_pixel", x, y, *_col(g))


LIST_SEEDS = 11


def gen_list(seed):
    """Aimed at k_cmd_list: 255..513 commands on one tile, a tile first hit in
    the second round of 256, a pending clear with untouched tiles, calls that
    drop or flush the queue in mid-list, a snapshot and another context's shared
    texture drawn in mid-list, frames narrower than a tile and 64 / 65 wide."""
    g = scenes.rng(9000 + seed)
    o = _Ops()
    texs, aux, extra = [(3, 3, "u8", 4, 91 + seed)], None, {}
    if seed < 5:
        K = (255, 256, 257, 512, 513)[seed]
        W, H, alpha = 129, 33, seed % 2 == 0
        o.add("set_color", 0.1, 0.3, 0.5, 0.7)
        for _ in range(K):
            _small_draw(g, o, 64, 128, 16, 32)                 # tile (1, 1)
        o.add("list_len", K)
        extra = {"tile": (1, 1), "K": K}
    elif seed == 5:
        W, H, alpha = 129, 33, True
        o.add("set_color", 0.1, 0.3, 0.5, 0.7)
        for _ in range(256):
            _small_draw(g, o, 0, 128, 0, 32)                   # all miss tile (2, 2) = pixel (128, 32)
        o.add("draw_rect", 120.0, 30.0, 9.5, 3.5, *_col(g))
        o.add("list_len", 257)
        extra = {"tile": (2, 2), "K": 1}
    elif seed == 6:
        W, H, alpha = 129, 70, False
        o.add("set_color", 0.5, 0.5, 0.5, 0.5)                 # uniform: pending until the list runs
        for _ in range(40):
            _small_draw(g, o, 0, 64, 0, 16)                    # tile (0, 0) only
        o.add("draw_rect", 70.0, 40.0, 30.0, 5.0, *_col(g))
        o.add("list_len", 41)
        extra = {"tile": (2, 4), "K": 0}
    elif seed == 7:
        W, H, alpha = 65, 33, True
        aux = (9, 7, True, [("set_color", 0.2, 0.2, 0.2, 0.2), ("draw_rect", 1.0, 1.0, 5.0, 4.0, 0.9, 0.1, 0.4, 1.0),
                            ("draw_circle", 6.0, 4.0, 2.5, 0.1, 0.8, 0.3, 0.5)])
        o.add("set_color", 0.25, 0.25, 0.25, 0.25)
        for _ in range(30):
            _small_draw(g, o, 0, 65, 0, 33)
        o.add("list_len", 30)
        o.add("set_color", 0.1, 0.2, 0.3, 0.4)                 # non-uniform: drops the queue
        o.add("list_len", 0)
        for _ in range(20):
            _small_draw(g, o, 0, 65, 0, 33)
        o.add("list_len", 20)
        o.add("get_color", 3.0, 4.0)                           # flushes
        o.add("list_len", 0)
        for _ in range(10):
            _small_draw(g, o, 0, 65, 0, 33)
        o.add("snapshot")                                      # texture 2 (after the aux texture 1)
        o.add("draw_texture", 2, 5.0, 3.0, 40.0, 20.0)
        for _ in range(10):
            _small_draw(g, o, 0, 65, 0, 33)
        o.add("list_len", 11)
        o.add("draw_texture", 1, 2.0, 2.0, 27.0, 21.0)         # another context's shared texture: runs at once
        o.add("list_len", 0)
        for _ in range(5):
            _small_draw(g, o, 0, 65, 0, 33)
        o.add("draw_split", 1, 30.0, 10.0, 18.0, 14.0, 0.0, 1.0, 0.0, 1.0)
        o.add("fill_color", 0.3, 0.6, 0.9, 0.25)
        o.add("list_len", 1)
    else:
        W, H = ((2, 17), (64, 16), (65, 17))[seed - 8]
        alpha = seed % 2 == 0
        o.add("set_color", 0.6, 0.6, 0.6, 0.6)
        for _ in range(40):
            _small_draw(g, o, 0, W, 0, H)
        o.add("draw_texture", 0, 0.0, 0.0, W * 1.0, H * 1.0)
        o.add("fill_color", 0.2, 0.1, 0.9, 0.5)
        o.add("list_len", 42)
    return _case("list", seed, (W, H, alpha), texs, o, o.empty, aux=aux, **extra)


def gen_resample(seed):
    """Every small texture resampled to 1x1, 3x7, 7x3 and twice its size; each
    result is read back (run's "made") and drawn."""
    W, H = 65, 33
    dtype, ch = ("u8", "f64")[seed % 2], (3, 4)[seed // 2 % 2]
    texs = [(tw, th, dtype, ch, 101 + 7 * seed + k) for k, (tw, th) in enumerate(TEX_SHAPES)]
    o = _Ops()
    o.add("set_color", 0.0, 0.0, 0.0, 0.0)
    t = len(texs)
    for k, (tw, th) in enumerate(TEX_SHAPES):
        for j, (rw, rh) in enumerate(((1, 1), (3, 7), (7, 3), (2 * tw, 2 * th))):
            o.add("resample", k, rw, rh)
            if j % 2:
                o.add("set_transform", 1.0, 0.0, 0.0, 1.0, 0.5, 0.5)
            o.add("draw_texture", t, 1.0 + 8 * k + j, 1.0 + 7 * j, rw * 2.0, rh * 2.0)
            o.add("set_transform", *IDENT)
            t += 1
    o.add("resample", t - 1, 5, 4)                             # a resampled texture resampled again
    o.add("draw_split", t, 40.0, 20.0, 20.0, 12.0, 0.0, 1.0, 0.0, 1.0)
    # (f64)x / W * tw decides the texel: with the textures above and any target below 400 it never does
    # (x / W * tw truncates like the exact quotient), but 1 / 49 * 49 < 1 -- a 49-wide source to 49 columns
    # takes texel 0 at x = 1; likewise rows at 49
    o.add("resample", len(texs) - 1, 49, 3)                    # texture t + 1: 16x12 -> 49x3
    o.add("resample", t + 1, 49, 3)                            # t + 2
    o.add("resample", t + 1, 3, 49)                            # t + 3: 3 wide, 49 high
    o.add("resample", t + 3, 3, 49)                            # t + 4
    o.add("draw_texture", t + 2, 2.0, 28.0, 49.0, 3.0)
    o.add("draw_texture", t + 4, 60.0, 1.0, 3.0, 30.0)
    return _case("resample", seed, (W, H, seed % 2 == 1), texs, o, o.empty)


FAMILIES = {
    "bounds": (gen_bounds, 6), "fastpath": (gen_fastpath, 6), "texel": (gen_texel, 4),
    "transform": (gen_transform, 6), "line": (gen_line, 6), "circle_grad": (gen_circle_grad, 6),
    "blend": (gen_blend, 6), "pixels": (gen_pixels, 84), "list": (gen_list, LIST_SEEDS),
    "resample": (gen_resample, 4),
}


def cases(family):
    gen, n = FAMILIES[family]
    return [gen(seed) for seed in range(n)]


def all_cases():
    return [c for f in FAMILIES for c in cases(f)]


def case_ids():
    return [(f, s) for f, (_, n) in FAMILIES.items() for s in range(n)]


def golden_lines(case, out):
    """"<case>/<output> <sha256>" of one case's oracle outputs (tests/golden/prim_fuzz.sha256)."""
    items = [("f64", out["f64"]), ("u8", out["u8"]), ("probes", out["probes"]),
             ("bools", np.array([bool(b) for b in out["bools"]], dtype=np.uint8))]
    items += [(f"made{i}", m) for i, m in enumerate(out["made"])]
    return [f"{case['name']}/{k} {hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()}" for k, v in items]

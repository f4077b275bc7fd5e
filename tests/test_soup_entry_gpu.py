"""The six soup entry points (DrawTriangles, DrawTexturedTriangles,
DrawTexturedTrianglesPerspective and their Device forms) share one staging
helper and one rule for whose memory a batch reads (nrtri::Batch::callerOwned).

Equivalence: the same soup through the host form and through the device form
with aligned and misaligned arrays, with and without z, on both rasters, gives
the expected frame and depth bit for bit.

Lifetime: a device batch that still reads an array of the caller's is sized in
the call, so once the caller has synchronised it may rewrite its tensors; a
misaligned batch without z and q is fully staged, may be deferred, and its
overflow re-run reads the staging only.

96 x 40 is 2 x 2 tiles of 64 x 32 with a partial tile each way; every triangle
crosses x = 64, so it lies in at least two tiles.  With 5 triangles 3n is odd
(the staging pads z), with 6 it is not."""
import functools

import numpy as np
import pytest

import mesh_ref as MR
import persp_ref as P
import scenes
import textured_ref as T

pytestmark = pytest.mark.gpu

W, H = 96, 40
BG, CLEAR, CT = P.BG, P.CLEAR, P.CT
KINDS = ("flat", "gouraud", "tex", "persp")
RECT = (30.0, 10.0, 50.0, 25.0, 0.9, 0.1, 0.1, 0.5)


@functools.lru_cache(maxsize=None)
def _soup(n):
    g = scenes.rng(71 + n)
    tex = T.texture_rgb()
    xy = np.empty((n, 3, 2))
    xy[:, 0, 0], xy[:, 1, 0], xy[:, 2, 0] = g.uniform(4, 56, n), g.uniform(72, 93, n), g.uniform(4, 93, n)
    xy[:, 0, 1], xy[:, 1, 1], xy[:, 2, 1] = g.uniform(1, 12, n), g.uniform(14, 26, n), g.uniform(28, 39, n)
    e1, e2 = xy[:, 1] - xy[:, 0], xy[:, 2] - xy[:, 0]
    assert (np.abs(e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]) > 100).all()
    assert (xy[..., 0].min(axis=1) < 60).all() and (xy[..., 0].max(axis=1) > 68).all()   # crosses x = 64
    assert (xy[..., 1].max(axis=1) > 33).any()                                           # and some y = 32
    uv = np.empty((n, 3, 2))
    uv[..., 0], uv[..., 1] = g.uniform(-3, tex.shape[1] + 3, (n, 3)), g.uniform(-3, tex.shape[0] + 3, (n, 3))
    rgba = g.uniform(0, 1, (n, 3, 4))
    rgba[..., 3] = 1.0
    b = dict(xy=xy.reshape(n, 6), uv=uv.reshape(n, 6), z=g.uniform(0.05, 0.99, (n, 3)), q=g.uniform(0.2, 5.0, (n, 3)),
             gouraud=rgba.reshape(n, 12), flat=np.ascontiguousarray(rgba[:, 0]), tex=tex, ct=CT, m=T.IDENT)
    for a in b.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return b


def _batch(n, has_z):
    b = _soup(n)
    return b if has_z else dict(b, z=None)


@functools.lru_cache(maxsize=None)
def _expected(kind, n, has_z):
    b = _batch(n, has_z)
    if kind == "tex":
        want = T.expected_payload(W, H, False, BG, "zw", CLEAR, [b])
    elif kind == "persp":
        want = P.expected_payload(W, H, False, BG, "zw", CLEAR, [b])
    else:
        octx = scenes.OracleFactory().context(W, H, False)
        MR.begin_frame(octx, "zw", b["m"], b["ct"], bg=BG, clear=CLEAR)
        octx.draw_triangles(b["xy"], b[kind], z=b["z"], gouraud=kind == "gouraud")
        want = MR.read_frame(octx, "zw")
    assert (want[1] != CLEAR).mean() > 0.25     # the soup covers a good part of the frame
    for a in want:
        a.setflags(write=False)
    return want


def _plus_rect(want, b):
    """`want` with RECT drawn over it by the oracle (the depth is not touched)."""
    octx = scenes.OracleFactory().context(W, H, False)
    for y in range(H):
        for x in range(W):
            octx.set_pixel(x, y, *want[0][y, x], 1.0)
    octx.set_transform(*b["m"])
    octx.set_color_transform(*b["ct"])
    octx.draw_rect(*RECT)
    out = octx.get_buffer_numpy()
    assert not scenes.bits_equal(out, want[0])
    return out, want[1]


def _same(got, want, what):
    assert scenes.bits_equal(got[0], want[0]), (what, scenes.first_mismatch(got[0], want[0]))
    assert np.array_equal(got[1], want[1]), (what, "depth", scenes.first_mismatch(got[1], want[1]))


def _attr(kind):
    return "uv" if kind in ("tex", "persp") else kind


def _tensors(b, kind, dev, off):
    """The batch's arrays as device tensors, `off` doubles past a 16-byte boundary (off: {name: 0 | 1})."""
    import torch
    out = {}
    for k in ("xy", _attr(kind), "z", "q"):
        if b[k] is None or (k == "q" and kind != "persp"):
            out[k] = None
            continue
        flat = torch.from_numpy(np.array(b[k], dtype=np.float64).ravel())
        t = torch.zeros(flat.numel() + 2, dtype=torch.float64, device=dev)[off[k]:off[k] + flat.numel()]
        t.copy_(flat)
        assert t.data_ptr() % 16 == 8 * off[k]
        out[k] = t
    torch.cuda.synchronize(dev)
    return out


def _draw_host(ctx, tex, b, kind):
    if kind in ("tex", "persp"):
        ctx.draw_textured_triangles(tex, b["xy"], b["uv"], z=b["z"], q=b["q"] if kind == "persp" else None)
    else:
        ctx.draw_triangles(b["xy"], b[kind], z=b["z"], gouraud=kind == "gouraud")


def _draw_device(ctx, tex, b, kind, t):
    n = b["xy"].shape[0]
    if kind in ("tex", "persp"):
        ctx.draw_textured_triangles_device(tex, t["xy"], t["uv"], n, z=t["z"], q=t["q"])
    else:
        ctx.draw_triangles_device(t["xy"], t[kind], n, z=t["z"], gouraud=kind == "gouraud")


def _ctx(gpu, b, force=False):
    ctx = gpu.context(W, H, False)
    ctx.set_force_ordered_raster(force)
    MR.begin_frame(ctx, "zw", b["m"], b["ct"], bg=BG, clear=CLEAR)
    return ctx


@pytest.mark.parametrize("has_z", [True, False])
@pytest.mark.parametrize("n", [5, 6])
@pytest.mark.parametrize("kind", KINDS)
def test_entry_points_agree(gpu, kind, n, has_z):
    import torch
    b, want = _batch(n, has_z), _expected(kind, n, has_z)
    dev = torch.device("cuda", gpu.context(8, 8, False).device)
    tex = gpu.texture(b["tex"])
    for force in (False, True):
        path = "ordered" if force else "order-free"
        ctx = _ctx(gpu, b, force)
        _draw_host(ctx, tex, b, kind)
        assert ctx.last_raster_path() == path
        _same(MR.read_frame(ctx, "zw"), want, f"{kind} n={n} z={has_z} host {path}")
        for off in (0, 1):
            t = _tensors(b, kind, dev, dict.fromkeys(("xy", _attr(kind), "z", "q"), off))
            ctx = _ctx(gpu, b, force)
            _draw_device(ctx, tex, b, kind, t)
            assert ctx.last_raster_path() == path
            _same(MR.read_frame(ctx, "zw"), want, f"{kind} n={n} z={has_z} device +{off} {path}")


# (kind, xy / uv offset, with z): aligned arrays are all the caller's; misaligned xy / uv are re-staged and z
# (and q) stay the caller's; the converse -- misaligned, no z, no q -- is fully staged and may be deferred
LIFETIMES = [("tex", 0, True), ("tex", 1, True), ("persp", 0, True), ("persp", 1, True), ("persp", 1, False),
             ("tex", 1, False)]


@pytest.mark.parametrize("n", [5, 6])
@pytest.mark.parametrize("kind,off,has_z", LIFETIMES)
def test_overflowing_device_batch_never_rereads_caller_arrays(gpu, kind, off, has_z, n):
    import torch
    b = _batch(n, has_z)
    want = _plus_rect(_expected(kind, n, has_z), b)
    dev = torch.device("cuda", gpu.context(8, 8, False).device)
    t = _tensors(b, kind, dev, {"xy": off, "uv": off, "z": 0, "q": 0})
    tex = gpu.texture(b["tex"])                # (alive to the end: destroying a texture settles every context)
    ctx = _ctx(gpu, b)
    ctx.set_pair_capacity_override(n - 1)      # every triangle lies in at least two tiles: the pair list overflows
    _draw_device(ctx, tex, b, kind, t)
    assert ctx.last_raster_path() == "order-free"
    torch.cuda.synchronize(dev)
    for k, a in t.items():                     # the caller reuses its tensors
        if a is not None:
            a.fill_(float("nan") if k == "xy" else 0.0)
    torch.cuda.synchronize(dev)
    ctx.draw_rect(*RECT)
    _same(MR.read_frame(ctx, "zw"), want, f"{kind} +{off} z={has_z} n={n}")

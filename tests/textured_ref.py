"""Expected frames of textured triangle batches, derived from the CPU oracle.

The oracle has no textured draw, so the expected frame of a textured batch is
built from what it does have -- DrawTriangles (coverage, barycentrics, depth,
Gouraud interpolation) and ApplyPixel -- plus the nearest sampler restated in
numpy (sample).  Two derivations:

expected_payload   opaque batches (RGB texture, colourTransform[3] == 1), any
    depth mode, any number of batches: the same triangles are drawn on the
    oracle as Gouraud batches whose vertex colours are (u_k, v_k, t, 1), t the
    triangle's running index, on an RGBA context with colour transform
    (1, 1, 1, 1) over a background whose channel 2 is -1.  With alpha exactly
    1 ApplyPixel stores the interpolated values unchanged, so channels 0 and 1
    are the winning fragment's u and v by the very expression the feature
    specifies (a0 + (a1-a0)*w1 + (a2-a0)*w2), channel 2 is the winner's index
    (t + 0*w1 + 0*w2 is exact) and the oracle's depth buffer is the expected
    depth.  The expected colour is sample(tex, u, v) * ct with alpha 1;
    uncovered pixels keep the background.

expected_loop      any batch (RGBA texture, ct[3] != 1 included): triangle by
    triangle in submission order.  A scratch oracle context (depth cleared to
    0xFFFFFFFF, test and write on) draws the triangle alone with payload
    (u, v, 1, 1): its coverage, u, v and quantised depth zq (scenes keep
    z <= 0.99, so every covered pixel passes there).  numpy applies zq < D
    where the mode tests depth, the oracle's exported ApplyPixel blends the
    texel into the main oracle context at each passing pixel, and numpy
    updates D where the mode writes.

Depth modes: "zw" test + write, "zt" test without write, "nz" no test.
A batch is a dict: xy (n, 6), uv (n, 6), z (n, 3) or None, tex (h, w, 3|4) f64,
ct (4,), m (6,) the context transform.
"""
import numpy as np

import scenes

MODES = ("zw", "zt", "nz")
IDENT = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def sample(tex, u, v):
    """The reference's nearest sampler (clamps in its order: x < 0 -> 0,
    x >= w-1 -> w-2, then y; texel ((i64)y, (i64)x)); a NaN coordinate is 0.
    Returns (..., 4): alpha 1 for a texture without alpha."""
    h, w, c = tex.shape
    with np.errstate(invalid="ignore"):
        x = np.where(np.isnan(u), 0.0, u)
        x = np.where(x < 0, 0.0, x)
        x = np.where(x >= w - 1, float(w - 2), x)
        y = np.where(np.isnan(v), 0.0, v)
        y = np.where(y < 0, 0.0, y)
        y = np.where(y >= h - 1, float(h - 2), y)
    xi, yi = x.astype(np.int64), y.astype(np.int64)
    t = tex[yi, xi]
    if c == 3:
        t = np.concatenate([t, np.ones(t.shape[:-1] + (1,))], axis=-1)
    return t, yi * w + xi


def _set_depth_mode(ctx, mode):
    if mode == "zw":
        ctx.set_depth_state(True, True)
    elif mode == "zt":
        ctx.set_depth_state(True, False)
    else:
        ctx.set_depth_state(False, False)


def _payload(uv, t0):
    n = uv.shape[0]
    p = np.empty((n, 3, 4))
    p[:, :, 0:2] = uv.reshape(n, 3, 2)
    p[:, :, 2] = (t0 + np.arange(n, dtype=np.float64))[:, None]
    p[:, :, 3] = 1.0
    return p.reshape(n, 12)


def expected_payload(W, H, alpha, bg, mode, clear_depth, batches, info=None):
    """(framebuffer (H, W, 3|4) f64, depth (H, W) u32 or None) after the opaque
    `batches` over a frame cleared to `bg` / `clear_depth`.  info (a dict)
    receives covered (bool mask) and texels (distinct texel ids hit)."""
    ora = scenes.OracleFactory()
    ctx = ora.context(W, H, True)
    ctx.set_color(0.0, 0.0, -1.0, 0.0)
    _set_depth_mode(ctx, mode)
    if mode != "nz":
        ctx.clear_depth(clear_depth)
    starts, t0 = [], 0
    for b in batches:
        assert b["tex"].shape[2] == 3 and b["ct"][3] == 1, "payload derivation: opaque batches only"
        ctx.set_transform(*b["m"])
        ctx.draw_triangles(b["xy"], _payload(b["uv"], t0), z=b["z"], gouraud=True)
        starts.append(t0)
        t0 += b["xy"].shape[0]
    pay = ctx.get_buffer_numpy()
    depth = ctx.get_depth_buffer() if mode != "nz" else None
    back = ora.context(W, H, alpha)   # the background as the oracle's SetColor leaves it
    back.set_color(*bg)
    fb = back.get_buffer_numpy()
    idx = pay[..., 2]
    covered = idx >= 0
    texels = set()
    for k, b in enumerate(batches):
        end = starts[k] + b["xy"].shape[0]
        sel = covered & (idx >= starts[k]) & (idx < end)
        if not sel.any():
            continue
        t, tid = sample(b["tex"], pay[..., 0][sel], pay[..., 1][sel])
        ct = np.asarray(b["ct"], dtype=np.float64)
        fb[sel, 0] = t[:, 0] * ct[0]
        fb[sel, 1] = t[:, 1] * ct[1]
        fb[sel, 2] = t[:, 2] * ct[2]
        if alpha:
            fb[sel, 3] = t[:, 3] * ct[3]
        texels |= {(k, int(i)) for i in np.unique(tid)}
    if info is not None:
        info["covered"] = covered
        info["texels"] = texels
    return fb, depth


def expected_loop(W, H, alpha, bg, mode, clear_depth, batches, info=None):
    """The same by the per-triangle derivation (any batch).  info receives
    covered, texels, zpass / zfail (fragment counts of the depth test)."""
    ora = scenes.OracleFactory()
    main = ora.context(W, H, alpha)
    main.set_color(*bg)
    scratch = ora.context(W, H, True)
    scratch.set_depth_state(True, True)
    D = np.full((H, W), clear_depth, dtype=np.uint32)
    covered = np.zeros((H, W), dtype=bool)
    texels = set()
    zpass = zfail = 0
    lib, mp = main.lib, main._ptr
    for k, b in enumerate(batches):
        n = b["xy"].shape[0]
        assert b["z"] is None or np.nanmax(b["z"]) <= 0.99
        main.set_color_transform(*b["ct"])
        scratch.set_transform(*b["m"])
        pay = _payload(b["uv"], 0)
        pay[:, 2::4] = 1.0
        for t in range(n):
            scratch.set_color(0.0, 0.0, -1.0, 0.0)
            scratch.clear_depth(0xFFFFFFFF)
            scratch.draw_triangles(b["xy"][t:t + 1], pay[t:t + 1],
                                   z=None if b["z"] is None else b["z"][t:t + 1], gouraud=True)
            p = scratch.get_buffer_numpy()
            cov = p[..., 2] == 1.0
            if not cov.any():
                continue
            zq = scratch.get_depth_buffer() if b["z"] is not None else np.zeros((H, W), dtype=np.uint32)
            ok = cov & (zq < D) if mode != "nz" else cov
            zpass += int(ok.sum())
            zfail += int((cov & ~ok).sum())
            ys, xs = np.nonzero(ok)
            if ys.size == 0:
                continue
            tx, tid = sample(b["tex"], p[ys, xs, 0], p[ys, xs, 1])
            for y, x, c in zip(ys.tolist(), xs.tolist(), tx.tolist()):
                lib.ApplyPixel(mp, x, y, c[0], c[1], c[2], c[3])
            if mode == "zw":
                D[ok] = zq[ok]
            covered |= ok
            texels |= {(k, int(i)) for i in np.unique(tid)}
    if info is not None:
        info.update(covered=covered, texels=texels, zpass=zpass, zfail=zfail)
    return main.get_buffer_numpy(), (D if mode != "nz" else None)


def flat_colours(tex, uv):
    """rgba (n, 4) of a batch whose three vertices share one (u, v) per
    triangle: the texel every fragment of the triangle samples."""
    t, _ = sample(tex, uv[:, 0], uv[:, 1])
    return np.ascontiguousarray(t)


def expected_flat(W, H, alpha, bg, mode, clear_depth, batches):
    """Constant-UV batches as the oracle's own flat DrawTriangles."""
    ora = scenes.OracleFactory()
    ctx = ora.context(W, H, alpha)
    ctx.set_color(*bg)
    _set_depth_mode(ctx, mode)
    if mode != "nz":
        ctx.clear_depth(clear_depth)
    for b in batches:
        ctx.set_transform(*b["m"])
        ctx.set_color_transform(*b["ct"])
        ctx.draw_triangles(b["xy"], flat_colours(b["tex"], b["uv"]), z=b["z"], gouraud=False)
    return ctx.get_buffer_numpy(), (ctx.get_depth_buffer() if mode != "nz" else None)


def draw_gpu(ctx, fac, mode, clear_depth, bg, batches, textures=None):
    """The batches through the library (ctx: a fresh GPU context)."""
    ctx.set_color(*bg)
    _set_depth_mode(ctx, mode)
    if mode != "nz":
        ctx.clear_depth(clear_depth)
    for k, b in enumerate(batches):
        tex = textures[k] if textures else fac.texture(b["tex"])
        ctx.set_transform(*b["m"])
        ctx.set_color_transform(*b["ct"])
        ctx.draw_textured_triangles(tex, b["xy"], b["uv"], z=b["z"])
    return ctx.get_buffer_numpy(), (ctx.get_depth_buffer() if mode != "nz" else None)


# ---- scenes -------------------------------------------------------------
def texture_rgb(seed=5, w=37, h=23):
    return scenes.rng(seed).uniform(0, 1, size=(h, w, 3))


def texture_rgba(seed=6, w=16, h=9):
    return scenes.rng(seed).uniform(0, 1, size=(h, w, 4))


XFORM = (0.9 * np.cos(0.2), 0.9 * np.sin(0.2), -0.9 * np.sin(0.2), 0.9 * np.cos(0.2), 14.0, -9.0)


def soup(W, H, n, seed, tex, spread=40.0, m=IDENT, ct=(0.9, 0.8, 0.7, 1.0), zrange=(0.05, 0.99), const_uv=False):
    """n triangles as tests/test_depth_edges_gpu.py::_scene places them
    (centroid uniform over the frame, vertices within +-spread), depths in
    zrange, UVs uniform in [-3, w+3] x [-3, h+3] (all four clamps fire)."""
    g = np.random.default_rng(seed)
    c = np.stack([g.uniform(0, W, n), g.uniform(0, H, n)], axis=1)
    xy = (c[:, None, :] + g.uniform(-spread, spread, size=(n, 3, 2))).reshape(n, 6)
    z = g.uniform(zrange[0], zrange[1], size=(n, 3))
    h, w, _ = tex.shape
    uv = np.empty((n, 3, 2))
    uv[..., 0] = g.uniform(-3, w + 3, size=(n, 3))
    uv[..., 1] = g.uniform(-3, h + 3, size=(n, 3))
    if const_uv:
        uv[:, 1:, :] = uv[:, :1, :]
    return dict(xy=xy, uv=uv.reshape(n, 6), z=z, tex=tex, ct=tuple(ct), m=tuple(m))

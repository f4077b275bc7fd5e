"""Expected frames of bilinear-filtered textured batches (DESIGN.md §3
"Bilinear texture filtering"), derived from the CPU oracle as textured_ref and
persp_ref derive the nearest ones.

sample_bilinear is the filter restated in numpy, elementwise and in the literal
order: the coordinate clamps of the reference's sampler (NaN -> 0 first, the
project's rule), the truncation, the four texels and, per channel,

    c0*(1 - fu)*(1 - fv) + c1*fu*(1 - fv) + c2*(1 - fu)*fv + c3*fu*fv

with every numpy operation one rounded f64 operation, products and sum left to
right.  Alpha of a texture without alpha is the literal 1.

A batch is persp_ref's dict; q is optional (absent: an affine batch -- q of
ones gives the affine (u, v) bit for bit, tests/test_persp_gpu.py).  The two
derivations are persp_ref's with the sampler exchanged: its payload and
oracle-pass helpers are reused, `filt` picks the sampler (0: textured_ref's
nearest one, so that one code path yields both frames of a scene).
"""
import numpy as np

import persp_ref as P
import scenes
import textured_ref as T


def footprint(u, n):
    """(i, f) of coordinate array u on an axis of n texels, the literal form:
    NaN -> 0; x < 0 -> 0; x >= n-1 -> n-2; i = (i64)x; f = x - i."""
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        x = np.where(np.isnan(u), 0.0, u)
        x = np.where(x < 0, 0.0, x)
        x = np.where(x >= n - 1, float(n - 2), x)
    i = x.astype(np.int64)
    return i, x - i


def footprint_kernel(u, n):
    """The form the kernels use (nr_tri.h tex_bilinear), which needs n-2 and
    the constant 1 only: x' = fmax(x, 0) (NaN -> 0), i = (int)fmin(x', n-2),
    f = x' - i, and f >= 1 -> 0."""
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        xc = np.fmax(u, 0.0)
        i = np.fmin(xc, float(n - 2)).astype(np.int64)
        d = xc - i
        return i, np.where(d < 1.0, d, 0.0)


def sample_bilinear(tex, u, v, footprint=footprint):
    """(..., 4) filtered texels at (u, v) (arrays of one shape)."""
    h, w, c = tex.shape
    ix, fu = footprint(u, w)
    iy, fv = footprint(v, h)
    c0, c1, c2, c3 = tex[iy, ix], tex[iy, ix + 1], tex[iy + 1, ix], tex[iy + 1, ix + 1]
    fu, fv = fu[..., None], fv[..., None]
    t = c0 * (1 - fu) * (1 - fv) + c1 * fu * (1 - fv) + c2 * (1 - fu) * fv + c3 * fu * fv
    if c == 3:
        t = np.concatenate([t, np.ones(t.shape[:-1] + (1,))], axis=-1)
    return t


def _sample(tex, u, v, filt):
    return sample_bilinear(tex, u, v) if filt else T.sample(tex, u, v)[0]


def expected_payload(W, H, alpha, bg, mode, clear_depth, batches, info=None, filt=1):
    """(framebuffer, depth or None) after the opaque `batches` (persp_ref's
    two oracle passes: the winner's U, V, Q, then its index).  info receives
    covered, and per covered pixel u, v (the sampled coordinate) and batch."""
    for b in batches:
        assert b["tex"].shape[2] == 3 and b["ct"][3] == 1, "payload derivation: opaque batches only"
    pay, depth = P._oracle_pass(W, H, mode, clear_depth, batches, False)
    idx = P._oracle_pass(W, H, mode, clear_depth, batches, True)[0][..., 0]
    back = scenes.OracleFactory().context(W, H, alpha)
    back.set_color(*bg)
    fb = back.get_buffer_numpy()
    covered = idx >= 0
    us, vs = np.full((H, W), np.nan), np.full((H, W), np.nan)
    which = np.full((H, W), -1, dtype=np.int64)
    t0 = 0
    for k, b in enumerate(batches):
        end = t0 + b["xy"].shape[0]
        sel = covered & (idx >= t0) & (idx < end)
        t0 = end
        if not sel.any():
            continue
        u, v = P.persp_uv(pay[..., 0][sel], pay[..., 1][sel], pay[..., 2][sel])
        t = _sample(b["tex"], u, v, filt)
        ct = np.asarray(b["ct"], dtype=np.float64)
        fb[sel, 0] = t[:, 0] * ct[0]
        fb[sel, 1] = t[:, 1] * ct[1]
        fb[sel, 2] = t[:, 2] * ct[2]
        if alpha:
            fb[sel, 3] = t[:, 3] * ct[3]
        us[sel], vs[sel], which[sel] = u, v, k
    if info is not None:
        info.update(covered=covered, u=us, v=vs, batch=which)
    return fb, depth


def expected_loop(W, H, alpha, bg, mode, clear_depth, batches, info=None, filt=1):
    """The same by the per-triangle derivation (any batch)."""
    ora = scenes.OracleFactory()
    main = ora.context(W, H, alpha)
    main.set_color(*bg)
    scratch = ora.context(W, H, True)
    scratch.set_depth_state(True, True)
    D = np.full((H, W), clear_depth, dtype=np.uint32)
    covered = np.zeros((H, W), dtype=bool)
    lib, mp = main.lib, main._ptr
    for b in batches:
        n = b["xy"].shape[0]
        assert b["z"] is None or n == 0 or np.nanmax(b["z"]) <= 0.99
        main.set_color_transform(*b["ct"])
        scratch.set_transform(*b["m"])
        pay = P._payload(b)
        for t in range(n):
            scratch.set_color(0.0, 0.0, 0.0, 0.0)
            scratch.clear_depth(0xFFFFFFFF)
            scratch.draw_triangles(b["xy"][t:t + 1], pay[t:t + 1],
                                   z=None if b["z"] is None else b["z"][t:t + 1], gouraud=True)
            p = scratch.get_buffer_numpy()
            cov = p[..., 3] == 1.0
            if not cov.any():
                continue
            zq = scratch.get_depth_buffer() if b["z"] is not None else np.zeros((H, W), dtype=np.uint32)
            ok = cov & (zq < D) if mode != "nz" else cov
            ys, xs = np.nonzero(ok)
            if ys.size == 0:
                continue
            u, v = P.persp_uv(p[ys, xs, 0], p[ys, xs, 1], p[ys, xs, 2])
            tx = _sample(b["tex"], u, v, filt)
            for y, x, c in zip(ys.tolist(), xs.tolist(), tx.tolist()):
                lib.ApplyPixel(mp, x, y, c[0], c[1], c[2], c[3])
            if mode == "zw":
                D[ok] = zq[ok]
            covered |= ok
    if info is not None:
        info.update(covered=covered)
    return main.get_buffer_numpy(), (D if mode != "nz" else None)


def draw_gpu(ctx, fac, mode, clear_depth, bg, batches, textures=None, filt=1):
    """The batches through the library with the context's filter set to
    `filt`: draw_textured_triangles, with q= where the batch has one."""
    ctx.set_triangle_texture_filter(filt)
    ctx.set_color(*bg)
    T._set_depth_mode(ctx, mode)
    if mode != "nz":
        ctx.clear_depth(clear_depth)
    for k, b in enumerate(batches):
        tex = textures[k] if textures else fac.texture(b["tex"])
        ctx.set_transform(*b["m"])
        ctx.set_color_transform(*b["ct"])
        ctx.draw_textured_triangles(tex, b["xy"], b["uv"], z=b["z"], q=b.get("q"))
    return ctx.get_buffer_numpy(), (ctx.get_depth_buffer() if mode != "nz" else None)


# ---- the scenes the GPU tests draw (tests/test_bilinear_ref.py checks that
# they discriminate) -------------------------------------------------------------
W, H = P.W, P.H
BG, CLEAR, FAR, CT, CT_BLEND, KINDS = P.BG, P.CLEAR, P.FAR, P.CT, P.CT_BLEND, P.KINDS


def soup_batches(kind, persp):
    """persp_ref's two-batch soup scene; affine: the same batches without q."""
    bs = P.soup_batches(kind)
    return bs if persp else [{k: v for k, v in b.items() if k != "q"} for b in bs]


def integer_uv_batches():
    """The opaque scene with every corner's (u, v) an integer inside the clamp
    range and one (u, v) per triangle: every fragment's coordinate is that
    integer exactly (u + 0*w1 + 0*w2), where the filter returns the texel."""
    out = []
    for k, b in enumerate(soup_batches("opaque", False)):
        h, w, _ = b["tex"].shape
        n = b["xy"].shape[0]
        g = scenes.rng(70 + k)
        uv = np.empty((n, 3, 2))
        uv[:, :, 0] = g.integers(0, w - 1, size=(n, 1)).astype(np.float64)
        uv[:, :, 1] = g.integers(0, h - 1, size=(n, 1)).astype(np.float64)
        out.append(dict(b, uv=uv.reshape(n, 6)))
    return out


def tiny_texture_batch(alpha):
    """A 2x2 texture (the smallest: ix = iy = 0 always) under UVs spanning [-1, 2]."""
    tex = scenes.rng(33).uniform(0, 1, size=(2, 2, 4 if alpha else 3))
    b = T.soup(W, H, 60, 34, tex, spread=45.0, m=T.XFORM, ct=CT_BLEND if alpha else CT)
    b["uv"] = scenes.rng(35).uniform(-1.0, 2.0, size=b["uv"].shape)
    return b


def odd_uv_batch(persp):
    """NaN, +-inf and huge coordinates on some corners (and, perspective, a
    degenerate q: 0, negative, inf, NaN) -- every value gives a defined colour."""
    b = P.soup(W, H, 60, 41, T.texture_rgb(), spread=40.0, ct=CT)
    g = scenes.rng(6)
    odd_uv = [np.nan, np.inf, -np.inf, 1e300, -1e300, 1e19, -0.5, 2.0 ** 31, 2.0 ** 63]
    uv = b["uv"].copy()
    for t in range(0, 60, 2):
        for c in g.choice(6, size=1 + t // 2 % 3, replace=False):
            uv[t, c] = odd_uv[int(g.integers(len(odd_uv)))]
    for k, val in enumerate(odd_uv):
        uv[2 * k + 1] = val
    b["uv"] = uv
    if not persp:
        del b["q"]
        return b
    odd_q = [0.0, -1.0, np.inf, -np.inf, np.nan, 1e300, 1e-300]
    q = b["q"].copy()
    for t in range(1, 60, 4):
        q[t, int(g.integers(3))] = odd_q[int(g.integers(len(odd_q)))]
    for k, val in enumerate(odd_q):
        q[20 + 2 * k] = val
    b["q"] = q
    return b

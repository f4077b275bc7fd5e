"""Expected frames of textured batches under a wrap state (DESIGN.md §3 "Wrap
addressing", SetTriangleTextureWrap), derived from the CPU oracle as
bilinear_ref and modulate_ref derive the clamped ones.

fold is the rule restated in numpy, elementwise and in the literal order; per
axis of n texels, mode 0 clamp (bilinear_ref.footprint), 1 repeat, 2 mirror:

    P = n (repeat) or 2n (mirror);  k = floor(x / P);  t = x - k * P
    !(t >= 0) -> 0;  t >= P -> 0;  i0 = (i64)t;  f = t - i0;  i1 = i0 + 1, P -> 0
    c(j) = j (repeat);  j < n ? j : 2n - 1 - j (mirror)

fold_kernel is the form of nr_tri.h wrap_fold: the clamp axis by
bilinear_ref.footprint_kernel, a wrapped axis as the base index and a signed
step to the +1 neighbour.  tests/test_wrap_ref.py proves the two equal.

A batch is persp_ref's dict: q optional (absent: an affine batch), rgba (n, 12)
optional (present: a modulated batch, modulate_ref's).  The two derivations are
bilinear_ref's / modulate_ref's with the sampler exchanged: their payload and
oracle-pass helpers are reused.
"""
import math

import numpy as np

import bilinear_ref as BL
import modulate_ref as M
import persp_ref as P
import scenes
import textured_ref as T

CLAMP, REPEAT, MIRROR = 0, 1, 2


def fold(x, n, mode):
    """(j0, j1, f) of coordinate array x on an axis of n texels: the literal form."""
    x = np.asarray(x, dtype=np.float64)
    if mode == CLAMP:
        i, f = BL.footprint(x, n)
        return i, i + 1, f
    Pd = float(n if mode == REPEAT else 2 * n)
    with np.errstate(all="ignore"):
        k = np.floor(x / Pd)
        t = x - k * Pd
        t = np.where(t >= 0.0, t, 0.0)
        t = np.where(t >= Pd, 0.0, t)
    i0 = t.astype(np.int64)
    f = t - i0
    i1 = i0 + 1
    i1 = np.where(i1 == int(Pd), 0, i1)
    if mode == MIRROR:
        i0 = np.where(i0 < n, i0, 2 * n - 1 - i0)
        i1 = np.where(i1 < n, i1, 2 * n - 1 - i1)
    return i0, i1, f


def period_kernel(p):
    """(f64)p as the kernels form it (nr_tri.h wrap_period), by integer operations:
    the exponent from the leading bit, the rest shifted into the mantissa."""
    p = int(p)
    assert 2 <= p < 2 ** 30
    e = p.bit_length() - 1
    bits = ((1023 + e) << 52) | ((p << (52 - e)) & 0x000FFFFFFFFFFFFF)
    return float(np.array([bits], dtype=np.uint64).view(np.float64)[0])


def fold_kernel(x, n, mode):
    """The kernels' form (nr_tri.h wrap_fold): (c0, c0 + d, f) in 32-bit indices."""
    x = np.asarray(x, dtype=np.float64)
    if mode == CLAMP:
        i, f = BL.footprint_kernel(x, n)
        return i, i + 1, f
    Pd = period_kernel(n if mode == REPEAT else 2 * n)
    with np.errstate(all="ignore"):
        k = np.floor(x / Pd)
        t = x - k * Pd
        t = np.where(~(t >= 0.0), 0.0, t)
        t = np.where(t >= Pd, 0.0, t)
    i0 = t.astype(np.int32)
    f = t - i0.astype(np.float64)
    i1 = i0 + np.int32(1)
    if mode == MIRROR:
        i1 = np.where(i1 == 2 * n, 0, i1)
        c0 = np.where(i0 < n, i0, 2 * n - 1 - i0)
        d = np.where(i1 < n, i1, 2 * n - 1 - i1) - c0
    else:
        i1 = np.where(i1 == n, 0, i1)
        c0 = i0
        d = i1 - i0
    return c0.astype(np.int64), (c0 + d).astype(np.int64), f


def fold_scalar(x, n, mode):
    """One coordinate in plain Python floats and ints: the transcription fold is checked against."""
    x = float(x)
    if mode == CLAMP:
        if x != x:
            x = 0.0
        if x < 0:
            x = 0.0
        if x >= n - 1:
            x = float(n - 2)
        i = int(x)
        return i, i + 1, x - i
    Pd = float(n) if mode == REPEAT else float(2 * n)
    q = x / Pd
    k = float(math.floor(q)) if math.isfinite(q) and q != 0 else q   # (floor keeps a zero's sign, and inf, NaN)
    t = x - k * Pd
    if not (t >= 0.0):
        t = 0.0
    if t >= Pd:
        t = 0.0
    i0 = int(t)
    f = t - float(i0)
    i1 = i0 + 1
    if i1 == int(Pd):
        i1 = 0
    if mode == MIRROR:
        c = lambda j: j if j < n else 2 * n - 1 - j
        return c(i0), c(i1), f
    return i0, i1, f


def sample(tex, u, v, filt, wrap, fold=fold):
    """(..., 4) texels at (u, v) under the filter (0 nearest, 1 bilinear) and the
    wrap state (mode of u, mode of v).  Alpha of a texture without alpha: the literal 1."""
    h, w, c = tex.shape
    i0, i1, fu = fold(u, w, wrap[0])
    j0, j1, fv = fold(v, h, wrap[1])
    if filt:
        c0, c1, c2, c3 = tex[j0, i0], tex[j0, i1], tex[j1, i0], tex[j1, i1]
        fu, fv = fu[..., None], fv[..., None]
        t = c0 * (1 - fu) * (1 - fv) + c1 * fu * (1 - fv) + c2 * (1 - fu) * fv + c3 * fu * fv
    else:
        t = tex[j0, i0]
    if c == 3:
        t = np.concatenate([t, np.ones(t.shape[:-1] + (1,))], axis=-1)
    return t


def outside(x, n):
    """Where a sampled coordinate lies outside [0, n-1): where a wrapped axis can differ from the clamped one."""
    with np.errstate(invalid="ignore"):
        return ~((x >= 0) & (x < n - 1))


def _wrap_of(wrap, k):
    """The wrap state of batch k: `wrap` is one state for the scene, or a list with one per batch."""
    return wrap[k] if isinstance(wrap, list) else wrap


def _modulated(batches):
    mod = ["rgba" in b for b in batches]
    assert all(mod) or not any(mod), "a scene is modulated or it is not"
    return bool(batches) and mod[0]


def expected_payload(W, H, alpha, bg, mode, clear_depth, batches, info=None, filt=0, wrap=(0, 0)):
    """(framebuffer, depth or None) after the opaque `batches` (bilinear_ref's /
    modulate_ref's oracle passes).  info receives covered, and per covered pixel
    u, v (the sampled coordinate) and batch."""
    mod = _modulated(batches)
    for b in batches:
        assert M.is_opaque(b) if mod else (b["tex"].shape[2] == 3 and b["ct"][3] == 1), "opaque batches only"
    pay, depth = P._oracle_pass(W, H, mode, clear_depth, batches, False)
    col = M._colour_pass(W, H, mode, clear_depth, batches) if mod else None
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
        t = sample(b["tex"], u, v, filt, _wrap_of(wrap, k))
        ct = np.asarray(b["ct"], dtype=np.float64)
        if mod:
            g = col[sel]
            for c in range(3):
                fb[sel, c] = t[:, c] * g[:, c] * ct[c]
            if alpha:
                fb[sel, 3] = t[:, 3] * 1.0 * ct[3]
        else:
            for c in range(4 if alpha else 3):
                fb[sel, c] = t[:, c] * ct[c]
        us[sel], vs[sel], which[sel] = u, v, k
    if info is not None:
        info.update(covered=covered, u=us, v=vs, batch=which)
    return fb, depth


def expected_loop(W, H, alpha, bg, mode, clear_depth, batches, info=None, filt=0, wrap=(0, 0)):
    """The same by the per-triangle derivation (any batch).  info receives covered
    and frags: per batch the (u, v) of every fragment that was applied."""
    mod = _modulated(batches)
    ora = scenes.OracleFactory()
    main = ora.context(W, H, alpha)
    main.set_color(*bg)
    scratch = ora.context(W, H, True)
    scratch.set_depth_state(True, True)
    D = np.full((H, W), clear_depth, dtype=np.uint32)
    covered = np.zeros((H, W), dtype=bool)
    frags = []
    lib, mp = main.lib, main._ptr

    def alone(b, t, pay):
        scratch.set_color(0.0, 0.0, 0.0, 0.0)
        scratch.clear_depth(0xFFFFFFFF)
        scratch.draw_triangles(b["xy"][t:t + 1], pay[t:t + 1], z=None if b["z"] is None else b["z"][t:t + 1],
                               gouraud=True)
        return scratch.get_buffer_numpy()

    for k, b in enumerate(batches):
        n = b["xy"].shape[0]
        assert b["z"] is None or n == 0 or np.nanmax(b["z"]) <= 0.99
        main.set_color_transform(*b["ct"])
        scratch.set_transform(*b["m"])
        pay = P._payload(b)
        colp, alp = (M._colour_payload(b), M._colour_payload(b, True)) if mod else (None, None)
        fu, fv = [], []
        for t in range(n):
            p = alone(b, t, pay)
            cov = p[..., 3] == 1.0
            if not cov.any():
                continue
            zq = scratch.get_depth_buffer() if b["z"] is not None else np.zeros((H, W), dtype=np.uint32)
            ok = cov & (zq < D) if mode != "nz" else cov
            ys, xs = np.nonzero(ok)
            if ys.size == 0:
                continue
            u, v = P.persp_uv(p[ys, xs, 0], p[ys, xs, 1], p[ys, xs, 2])
            src = sample(b["tex"], u, v, filt, _wrap_of(wrap, k))
            if mod:
                g = alone(b, t, colp)[ys, xs, 0:3]
                ga = alone(b, t, alp)[ys, xs, 0]
                src = np.stack([src[:, 0] * g[:, 0], src[:, 1] * g[:, 1], src[:, 2] * g[:, 2], src[:, 3] * ga], axis=1)
            for y, x, c in zip(ys.tolist(), xs.tolist(), src.tolist()):
                lib.ApplyPixel(mp, x, y, c[0], c[1], c[2], c[3])
            if mode == "zw":
                D[ok] = zq[ok]
            covered |= ok
            fu.append(u)
            fv.append(v)
        frags.append((np.concatenate(fu) if fu else np.zeros(0), np.concatenate(fv) if fv else np.zeros(0)))
    if info is not None:
        info.update(covered=covered, frags=frags)
    return main.get_buffer_numpy(), (D if mode != "nz" else None)


def draw_gpu(ctx, fac, mode, clear_depth, bg, batches, textures=None, filt=0, wrap=(0, 0)):
    """The batches through the library under the filter and the wrap state (set in
    front of each draw, with no readback between the draws: a list of states leaves
    the earlier batches pending under theirs): draw_textured_triangles, with q= where
    the batch has one and colors= where it is modulated."""
    ctx.set_triangle_texture_filter(filt)
    ctx.set_color(*bg)
    T._set_depth_mode(ctx, mode)
    if mode != "nz":
        ctx.clear_depth(clear_depth)
    for k, b in enumerate(batches):
        tex = textures[k] if textures else fac.texture(b["tex"])
        ctx.set_triangle_texture_wrap(*_wrap_of(wrap, k))
        ctx.set_transform(*b["m"])
        ctx.set_color_transform(*b["ct"])
        if "rgba" in b:
            ctx.draw_textured_triangles(tex, b["xy"], b["uv"], z=b["z"], q=P.batch_q(b), colors=b["rgba"])
        else:
            ctx.draw_textured_triangles(tex, b["xy"], b["uv"], z=b["z"], q=b.get("q"))
    return ctx.get_buffer_numpy(), (ctx.get_depth_buffer() if mode != "nz" else None)


# ---- the scenes the GPU tests draw (tests/test_wrap_ref.py checks that they
# discriminate) ------------------------------------------------------------------
W, H = P.W, P.H            # 130 x 97: 3 x 4 tiles, partial right and bottom tiles
BG, CLEAR, FAR, CT, CT_BLEND, KINDS = P.BG, P.CLEAR, P.FAR, P.CT, P.CT_BLEND, P.KINDS
WRAPS = ((1, 1), (2, 2), (1, 0), (0, 2), (2, 1))
FORMS = ("affine", "persp", "mod")


def soup_cases():
    """(kind, form, wrap, filt, mode, alpha) of the soup tests: every wrap state with
    every filter, and every draw form with (1, 1) and (2, 1), each on an opaque scene
    (drawn on the order-free raster and again with the ordered raster forced) and on
    a blended one (ordered); the depth modes and the context's alpha rotate."""
    out = []
    for i, wrap in enumerate(WRAPS):
        for filt in (0, 1):
            j = i + filt
            out.append(("opaque", FORMS[j % 3], wrap, filt, T.MODES[j % 3], bool(filt)))
            out.append((("ct_alpha", "rgba_texture")[j % 2], FORMS[(j + 1) % 3], wrap, filt, T.MODES[(j + 1) % 3],
                        not filt))
    for k, form in enumerate(FORMS):
        for wrap in ((1, 1), (2, 1)):
            out.append(("opaque", form, wrap, 1, "zw", False))
            out.append((("rgba_texture", "ct_alpha")[k % 2], form, wrap, 1, "zw", True))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


def expected(kind, form, wrap, filt, mode, alpha, info=None):
    """The expected frame of a soup case: the payload derivation for an opaque scene, else the loop."""
    fn = expected_payload if kind == "opaque" else expected_loop
    return fn(W, H, alpha, BG, mode, CLEAR, soup_batches(kind, form), info, filt=filt, wrap=wrap)


def texture(w, h, channels=3, seed=90):
    """Small and not a power of two, so that x / P rounds."""
    return scenes.rng(seed + 16 * w + h).uniform(0, 1, size=(h, w, channels))


def tiled_uv(shape3, w, h, seed):
    """(n, 6) UVs uniform over [-2n, 3n) per axis."""
    g = scenes.rng(seed)
    n = shape3[0]
    uv = np.empty((n, 3, 2))
    uv[..., 0] = g.uniform(-2.0 * w, 3.0 * w, size=(n, 3))
    uv[..., 1] = g.uniform(-2.0 * h, 3.0 * h, size=(n, 3))
    return uv.reshape(n, 6)


def soup_batches(kind, form, n=(90, 14)):
    """persp_ref's two-batch soup scene over small tiling textures (5 x 3 and
    7 x 6 RGB; the 6 x 5 RGBA for rgba_texture; the modulated form's second RGB
    texture is the 16 x 16), the UVs redrawn over [-2n, 3n)."""
    bs = P.soup_batches(kind, n)
    if kind == "rgba_texture":
        texs = [texture(6, 5, 4), texture(6, 5, 4)]
    else:
        texs = [texture(5, 3), texture(16, 16) if form == "mod" else texture(7, 6)]
    out = []
    for k, (b, tex) in enumerate(zip(bs, texs)):
        h, w, _ = tex.shape
        b = dict(b, tex=tex, uv=tiled_uv(b["xy"].shape, w, h, 700 + k))
        if form == "affine":
            del b["q"]
        elif form == "mod":
            b = M.with_colours(b, 50 + k)
        out.append(b)
    return out


def inside_batches(form="persp"):
    """The opaque scene with every corner's (u, v) inside [0.2, n - 1.2]: every
    sampled coordinate lies in [0, w-1) x [0, h-1), where the three modes agree (I1).
    (An affine or positive-q perspective coordinate is a convex combination of the
    corners' up to rounding, hence the margin.)"""
    out = []
    for k, b in enumerate(soup_batches("opaque", form)):
        h, w, _ = b["tex"].shape
        g = scenes.rng(720 + k)
        n = b["xy"].shape[0]
        uv = np.empty((n, 3, 2))
        uv[..., 0] = g.uniform(0.2, w - 1.2, size=(n, 3))
        uv[..., 1] = g.uniform(0.2, h - 1.2, size=(n, 3))
        out.append(dict(b, uv=uv.reshape(n, 6)))
    return out


def tiny_texture_batch(alpha=False):
    """bilinear_ref's 2 x 2 scene with the UVs over [-4, 6): the smallest texture, where the repeat step
    -(n-1) and the mirror's -1 coincide."""
    b = BL.tiny_texture_batch(alpha)
    b["uv"] = tiled_uv(b["xy"].shape, 2, 2, 730)
    return b


def dense_batch(n=1000):
    """modulate_ref's dense tile (more distinct winners than the staged records
    hold: pass 3b) as a plain perspective batch over the 5 x 3 texture, UVs over [-2n, 3n)."""
    b = M.dense_batch(n)
    tex = texture(5, 3)
    b = {k: v for k, v in b.items() if k != "rgba"}
    return dict(b, tex=tex, uv=tiled_uv(b["xy"].shape, 5, 3, 740))

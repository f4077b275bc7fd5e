"""Expected frames of modulated textured batches -- texel times interpolated
vertex colour (DESIGN.md §3 "Modulated textured draws") -- derived from the CPU
oracle as persp_ref and bilinear_ref derive the plain textured ones.

A batch is persp_ref's dict (xy, uv, z, q, tex, ct, m; q absent: ones) plus
rgba (n, 12), a colour (r, g, b, A) per corner.  Per covered fragment

    a_k = u_k * q_k, b_k = v_k * q_k;  U, V, Q = I(a), I(b), I(q)
    rq = 1.0 / Q;  u = U * rq;  v = V * rq;  T = the texel at (u, v) by the filter
    G_c = I(c) for c in r, g, b, A;  src_c = T_c * G_c;  ApplyPixel(src)

where I is the expression of a Gouraud channel -- what the oracle's
DrawTriangles stores for a vertex colour drawn with alpha exactly 1.

expected_payload   opaque batches (RGB texture, every A == 1, ct[3] == 1).  Three
    oracle passes over the same triangles and depth state, as Gouraud draws with
    alpha-1 payloads: (a_k, b_k, q_k, 1); (r_k, g_k, b_k, 1); (t, 0, 0, 1) over a
    background of -1.  Then persp_uv, bilinear_ref._sample, the product, * ct.
    The source alpha is 1.0 * (1.0 + 0.0*w1 + 0.0*w2) = 1 for finite barycentrics.

expected_loop      any batch, triangle by triangle on a scratch context, with a
    further pass carrying (A_k, 0, 0, 1); blended by the oracle's ApplyPixel.

uvc / draw_gpu     the batches through the library.

Mesh soups: the colour mesh's clip_soup / expand (mesh_clip_ref, mesh_ref) give
xy, z and the colours; the textured twin of the same mesh gives uv and q
(persp_ref.clip_soup_q / expand_q): both run the same elementwise vertex and
clip arithmetic on the same positions, so triangle for triangle they agree.
"""
import numpy as np

import bilinear_ref as BL
import mesh_clip_ref as MC
import mesh_light_ref as ML
import mesh_ref as MR
import persp_ref as P
import scenes
import textured_ref as T


def batch_rgba(b):
    n = b["xy"].shape[0]
    return np.asarray(b["rgba"], dtype=np.float64).reshape(n, 3, 4)


def uvc(b):
    """(n, 18): per corner (u, v, r, g, b, A), the library's attribute array."""
    n = b["xy"].shape[0]
    uv = np.asarray(b["uv"], dtype=np.float64).reshape(n, 3, 2)
    return np.ascontiguousarray(np.concatenate([uv, batch_rgba(b)], axis=2).reshape(n, 18))


def _colour_payload(b, alpha_pass=False):
    """(n, 12): (r_k, g_k, b_k, 1), or for the alpha pass (A_k, 0, 0, 1)."""
    n = b["xy"].shape[0]
    c = batch_rgba(b)
    p = np.zeros((n, 3, 4))
    if alpha_pass:
        p[:, :, 0] = c[:, :, 3]
    else:
        p[:, :, 0:3] = c[:, :, 0:3]
    p[:, :, 3] = 1.0
    return p.reshape(n, 12)


def _colour_pass(W, H, mode, clear_depth, batches):
    """persp_ref._oracle_pass with the (r, g, b, 1) payload."""
    ctx = scenes.OracleFactory().context(W, H, True)
    ctx.set_color(-1.0, 0.0, 0.0, 0.0)
    T._set_depth_mode(ctx, mode)
    if mode != "nz":
        ctx.clear_depth(clear_depth)
    for b in batches:
        ctx.set_transform(*b["m"])
        ctx.draw_triangles(b["xy"], _colour_payload(b), z=b["z"], gouraud=True)
    return ctx.get_buffer_numpy()


def is_opaque(b):
    return b["tex"].shape[2] == 3 and b["ct"][3] == 1 and bool((batch_rgba(b)[:, :, 3] == 1).all())


def expected_payload(W, H, alpha, bg, mode, clear_depth, batches, info=None, filt=0):
    """(framebuffer, depth or None) after the opaque `batches`.  info receives
    covered, idx (the winner per pixel, -1: none), u, v, G (H, W, 3)."""
    for b in batches:
        assert is_opaque(b), "payload derivation: opaque batches only"
    pay, depth = P._oracle_pass(W, H, mode, clear_depth, batches, False)
    col = _colour_pass(W, H, mode, clear_depth, batches)
    idx = P._oracle_pass(W, H, mode, clear_depth, batches, True)[0][..., 0]
    back = scenes.OracleFactory().context(W, H, alpha)
    back.set_color(*bg)
    fb = back.get_buffer_numpy()
    covered = idx >= 0
    us, vs = np.full((H, W), np.nan), np.full((H, W), np.nan)
    t0 = 0
    for b in batches:
        end = t0 + b["xy"].shape[0]
        sel = covered & (idx >= t0) & (idx < end)
        t0 = end
        if not sel.any():
            continue
        u, v = P.persp_uv(pay[..., 0][sel], pay[..., 1][sel], pay[..., 2][sel])
        t = BL._sample(b["tex"], u, v, filt)
        ct = np.asarray(b["ct"], dtype=np.float64)
        g = col[sel]
        fb[sel, 0] = t[:, 0] * g[:, 0] * ct[0]
        fb[sel, 1] = t[:, 1] * g[:, 1] * ct[1]
        fb[sel, 2] = t[:, 2] * g[:, 2] * ct[2]
        if alpha:
            fb[sel, 3] = t[:, 3] * 1.0 * ct[3]
        us[sel], vs[sel] = u, v
    if info is not None:
        info.update(covered=covered, idx=idx, u=us, v=vs, G=col[..., 0:3])
    return fb, depth


def expected_loop(W, H, alpha, bg, mode, clear_depth, batches, info=None, filt=0):
    """The same by the per-triangle derivation (any batch)."""
    ora = scenes.OracleFactory()
    main = ora.context(W, H, alpha)
    main.set_color(*bg)
    scratch = ora.context(W, H, True)
    scratch.set_depth_state(True, True)
    D = np.full((H, W), clear_depth, dtype=np.uint32)
    covered = np.zeros((H, W), dtype=bool)
    lib, mp = main.lib, main._ptr

    def alone(b, t, pay):
        scratch.set_color(0.0, 0.0, 0.0, 0.0)
        scratch.clear_depth(0xFFFFFFFF)
        scratch.draw_triangles(b["xy"][t:t + 1], pay[t:t + 1], z=None if b["z"] is None else b["z"][t:t + 1],
                               gouraud=True)
        return scratch.get_buffer_numpy()

    for b in batches:
        n = b["xy"].shape[0]
        assert b["z"] is None or n == 0 or np.nanmax(b["z"]) <= 0.99
        main.set_color_transform(*b["ct"])
        scratch.set_transform(*b["m"])
        pay, colp, alp = P._payload(b), _colour_payload(b), _colour_payload(b, True)
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
            g = alone(b, t, colp)[ys, xs, 0:3]
            ga = alone(b, t, alp)[ys, xs, 0]
            u, v = P.persp_uv(p[ys, xs, 0], p[ys, xs, 1], p[ys, xs, 2])
            tx = BL._sample(b["tex"], u, v, filt)
            src = np.stack([tx[:, 0] * g[:, 0], tx[:, 1] * g[:, 1], tx[:, 2] * g[:, 2], tx[:, 3] * ga], axis=1)
            for y, x, c in zip(ys.tolist(), xs.tolist(), src.tolist()):
                lib.ApplyPixel(mp, x, y, c[0], c[1], c[2], c[3])
            if mode == "zw":
                D[ok] = zq[ok]
            covered |= ok
    if info is not None:
        info.update(covered=covered)
    return main.get_buffer_numpy(), (D if mode != "nz" else None)


def expected_gouraud(W, H, alpha, bg, mode, clear_depth, batches):
    """The oracle's own Gouraud DrawTriangles of the batches' colours (identity I2)."""
    ctx = scenes.OracleFactory().context(W, H, alpha)
    ctx.set_color(*bg)
    T._set_depth_mode(ctx, mode)
    if mode != "nz":
        ctx.clear_depth(clear_depth)
    for b in batches:
        ctx.set_transform(*b["m"])
        ctx.set_color_transform(*b["ct"])
        ctx.draw_triangles(b["xy"], batch_rgba(b).reshape(-1, 12), z=b["z"], gouraud=True)
    return ctx.get_buffer_numpy(), (ctx.get_depth_buffer() if mode != "nz" else None)


def draw_gpu(ctx, fac, mode, clear_depth, bg, batches, textures=None, filt=0):
    """The batches through the library: draw_textured_triangles(..., colors=...)."""
    ctx.set_triangle_texture_filter(filt)
    ctx.set_color(*bg)
    T._set_depth_mode(ctx, mode)
    if mode != "nz":
        ctx.clear_depth(clear_depth)
    for k, b in enumerate(batches):
        tex = textures[k] if textures else fac.texture(b["tex"])
        ctx.set_transform(*b["m"])
        ctx.set_color_transform(*b["ct"])
        ctx.draw_textured_triangles(tex, b["xy"], b["uv"], z=b["z"], q=P.batch_q(b), colors=b["rgba"])
    return ctx.get_buffer_numpy(), (ctx.get_depth_buffer() if mode != "nz" else None)


# ---- the scenes the GPU tests draw (tests/test_modulate_ref.py checks their
# own conditions) ----------------------------------------------------------------
W, H = P.W, P.H            # 130 x 97: 3 x 4 tiles, partial right and bottom tiles
W2, H2 = 70, 50            # 2 x 2 tiles, partial both ways
BG, CLEAR, FAR, CT, CT_BLEND = P.BG, P.CLEAR, P.FAR, P.CT, P.CT_BLEND
KINDS = ("opaque", "blended")
TILE_W, TILE_H = 64, 32
GOURAUD_RT = 280           # staged records per tile of a 16-double record: no record of >= 16 doubles stages more


def with_colours(b, seed, alpha=None):
    """b plus rgba: rgb uniform in [0, 1]; A == 1, or uniform in `alpha`."""
    n = b["xy"].shape[0]
    g = scenes.rng(seed)
    c = np.ones((n, 3, 4))
    c[:, :, 0:3] = g.uniform(0.0, 1.0, size=(n, 3, 3))
    if alpha is not None:
        c[:, :, 3] = g.uniform(alpha[0], alpha[1], size=(n, 3))
    return dict(b, rgba=c.reshape(n, 12))


def soup_batches(kind, persp=True, n=(90, 14)):
    """persp_ref's two-batch soup scene (90 slivers and small triangles, 14 large
    ones over them) with corner colours.  blended: RGBA textures, vertex alpha
    in (0.2, 0.9), ct[3] = 0.5.  persp False: q all 1."""
    if kind == "blended":
        t1, t2 = T.texture_rgba(), T.texture_rgba(seed=9, w=12, h=10)
        ct, al = CT_BLEND, (0.2, 0.9)
    else:
        t1, t2 = T.texture_rgb(), T.texture_rgb(seed=8, w=11, h=7)
        ct, al = CT, None
    bs = [P.soup(W, H, n[0], 11, t1, spread=40.0, m=T.XFORM, ct=ct), P.soup(W, H, n[1], 12, t2, spread=70.0, ct=ct)]
    out = []
    for k, b in enumerate(bs):
        b = with_colours(b, 50 + k, al)
        if not persp:
            b["q"] = np.ones_like(b["q"])
        out.append(b)
    return out


def small_batches(kind):
    """The same on the 70 x 50 frame: one batch of 40 triangles."""
    tex = T.texture_rgba() if kind == "blended" else T.texture_rgb()
    b = P.soup(W2, H2, 40, 21, tex, spread=25.0, ct=CT_BLEND if kind == "blended" else CT)
    return [with_colours(b, 60, (0.2, 0.9) if kind == "blended" else None)]


def dense_batch(n=1000):
    """n tiny triangles (vertices within +-1.5 px of a centre) inside the tile
    at columns 64..127, rows 32..63 of the 130 x 97 frame: more distinct winners
    in that tile than any record of 16 doubles or more can stage, so the
    modulated record's smaller table overflows too (shade_tile's pass 3b)."""
    g = scenes.rng(77)
    c = np.stack([g.uniform(66.0, 126.0, n), g.uniform(34.0, 62.0, n)], axis=1)
    xy = (c[:, None, :] + g.uniform(-1.5, 1.5, size=(n, 3, 2))).reshape(n, 6)
    tex = T.texture_rgb()
    h, w, _ = tex.shape
    uv = np.empty((n, 3, 2))
    uv[..., 0] = g.uniform(-3, w + 3, size=(n, 3))
    uv[..., 1] = g.uniform(-3, h + 3, size=(n, 3))
    b = dict(xy=xy, uv=uv.reshape(n, 6), z=g.uniform(0.05, 0.99, size=(n, 3)), tex=tex, ct=CT, m=T.IDENT,
             q=g.uniform(0.2, 5.0, size=(n, 3)))
    return with_colours(b, 78)


def tile_winners(idx, tx, ty):
    """Distinct winners inside tile (tx, ty) of an index pass."""
    t = idx[ty * TILE_H:(ty + 1) * TILE_H, tx * TILE_W:(tx + 1) * TILE_W]
    return int(np.unique(t[t >= 0]).size)


def ones_colours(b):
    return dict(b, rgba=np.ones((b["xy"].shape[0], 12)))


def ones_texture(b):
    h, w, c = b["tex"].shape
    return dict(b, tex=np.ones((h, w, c)))


def clamps_fired(tex, u, v):
    """Which of the sampler's four clamps (u < 0, u >= w-1, v < 0, v >= h-1) some coordinate triggers."""
    h, w, _ = tex.shape
    with np.errstate(invalid="ignore"):
        return bool((u < 0).any()), bool((u >= w - 1).any()), bool((v < 0).any()), bool((v >= h - 1).any())


# ---- the mesh front end ---------------------------------------------------------
# A textured colour mesh is mesh_ref's dict with both colors (nv, 4) and uv (nv, 2), and normals (nv, 3) when lit.
def mesh_twins(mesh, colors=None):
    """(colour mesh, textured mesh) over the positions and indices of `mesh`: the two
    kinds the existing references know, sharing every position-dependent value."""
    base = {k: v for k, v in mesh.items() if k not in ("colors", "uv", "gouraud")}
    return (dict(base, colors=mesh["colors"] if colors is None else colors, gouraud=True), dict(base, uv=mesh["uv"]))


def _interleave(uv, col):
    n = uv.shape[0]
    return np.ascontiguousarray(np.concatenate([uv.reshape(n, 3, 2), col.reshape(n, 3, 4)], axis=2).reshape(n, 18))


def mesh_soup(mesh, M, lit=False, N=None, ambient=None, lights=None, w_near=0.0, cull=0, persp=True):
    """(xy, z, uvc (n_out, 18), q (n_out, 3)) of a draw of a textured colour mesh:
    mesh_light_ref.lit_colors for the colours (lit), then mesh_clip_ref.clip_soup /
    persp_ref.clip_soup_q (the clip stage on) or mesh_ref.expand / persp_ref.expand_q,
    each attribute by the one elementwise expression A_a + (A_b - A_a) * t; q all 1.0
    with the perspective state off."""
    col = ML.lit_colors(mesh, N, ambient, lights) if lit else None
    cm, tm = mesh_twins(mesh, col)
    if w_near > 0 or cull != 0:
        xy, z, c, counts = MC.clip_soup(cm, M, w_near, cull)
        xy2, z2, uv, q, counts2 = P.clip_soup_q(tm, M, w_near, cull, persp)
        assert np.array_equal(counts, counts2)
    else:
        xy, z, c = MR.expand(cm, M)
        xy2, z2, uv, q = P.expand_q(tm, M)
        if not persp:
            q = np.ones_like(q)
    assert scenes.bits_equal(xy, xy2) and scenes.bits_equal(z, z2)
    return xy, z, _interleave(uv, c), q


def mesh_batch(mesh, M, tex, m=MR.XFORM, ct=CT, **kw):
    """The batch such a draw rasterises, for expected_payload / expected_loop."""
    xy, z, a, q = mesh_soup(mesh, M, **kw)
    a = a.reshape(-1, 3, 6)
    n = xy.shape[0]
    return dict(xy=xy, uv=np.ascontiguousarray(a[:, :, 0:2].reshape(n, 6)), rgba=np.ascontiguousarray(a[:, :, 2:6].reshape(n, 12)),
                z=z if n else None, q=q, tex=tex, ct=tuple(ct), m=tuple(m))


MESH_TEX = P.MESH_TEX


def lit_textured_sphere(rows=6, cols=8, alpha=None, seed=3):
    """mesh_light_ref.lit_sphere3d with both vertex colours and (uv_size) texture coordinates."""
    tm = ML.lit_sphere3d(rows, cols, uv_size=MESH_TEX)
    cm = MR.sphere3d(rows, cols, seed=seed, alpha=alpha)
    return dict(tm, colors=cm["colors"], gouraud=True)


def random_textured_color_mesh(nv, n, seed):
    """mesh_light_ref.random_lit_mesh with a uv per vertex running past the texture."""
    m = ML.random_lit_mesh(nv, n, seed)
    g = scenes.rng(seed + 300)
    uv = np.stack([g.uniform(-3, MESH_TEX[0] + 3, nv), g.uniform(-3, MESH_TEX[1] + 3, nv)], axis=1)
    return dict(m, uv=np.ascontiguousarray(uv), gouraud=True)

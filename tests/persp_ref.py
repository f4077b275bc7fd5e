"""Expected frames of perspective-correct textured batches (DESIGN.md §3
"Perspective-correct texture mapping"), derived from the CPU oracle as
textured_ref derives the affine ones.

A batch is textured_ref's dict plus q (n, 3), each corner's 1/w (absent: ones).
Per triangle a_k = u_k * q_k, b_k = v_k * q_k (numpy products, rounded once);
per fragment U, V, Q are a, b, q interpolated by the expression of a Gouraud
channel -- which is what the oracle's DrawTriangles computes for a vertex colour
-- then r = 1.0 / Q, u = U * r, v = V * r in numpy (persp_uv) and
textured_ref.sample picks the texel.

expected_payload   opaque batches.  Pass 1 draws every batch on the oracle as a
    Gouraud batch with vertex payload (a_k, b_k, q_k, 1): with alpha exactly 1
    ApplyPixel stores the interpolated values, so channels 0-2 are the winner's
    U, V, Q.  All four channels are in use, so the winner's index comes from
    pass 2: the same draws with payload (t, 0, 0, 1) over a background whose
    channel 0 is -1.  Both passes see the same positions, depths and depth
    state, hence the same winners.

expected_loop      any batch, triangle by triangle: the scratch context draws the
    triangle alone with payload (a, b, q, 1) over a background of alpha 0;
    covered pixels are those whose alpha became 1.

expand_q / clip_soup_q   the mesh front end's soup with q = 1 / cw restated
    elementwise (a cut vertex: 1 / w_near), on top of mesh_ref / mesh_clip_ref.
"""
import numpy as np

import mesh_clip_ref as MC
import mesh_ref as MR
import scenes
import textured_ref as T


def batch_q(b):
    n = b["xy"].shape[0]
    q = b.get("q")
    return np.ones((n, 3)) if q is None else np.asarray(q, dtype=np.float64).reshape(n, 3)


def persp_uv(U, V, Q):
    """r = 1.0 / Q; (U * r, V * r): one IEEE division, two rounded products."""
    with np.errstate(all="ignore"):
        r = 1.0 / Q
        return U * r, V * r


def _payload(b, index0=None):
    """(n, 12) vertex colours: (a_k, b_k, q_k, 1), or with index0 (t, 0, 0, 1)."""
    n = b["xy"].shape[0]
    p = np.zeros((n, 3, 4))
    if index0 is None:
        uv, q = np.asarray(b["uv"], dtype=np.float64).reshape(n, 3, 2), batch_q(b)
        with np.errstate(all="ignore"):
            p[:, :, 0] = uv[:, :, 0] * q
            p[:, :, 1] = uv[:, :, 1] * q
        p[:, :, 2] = q
    else:
        p[:, :, 0] = (index0 + np.arange(n, dtype=np.float64))[:, None]
    p[:, :, 3] = 1.0
    return p.reshape(n, 12)


def _oracle_pass(W, H, mode, clear_depth, batches, index):
    ctx = scenes.OracleFactory().context(W, H, True)
    ctx.set_color(-1.0, 0.0, 0.0, 0.0)
    T._set_depth_mode(ctx, mode)
    if mode != "nz":
        ctx.clear_depth(clear_depth)
    t0 = 0
    for b in batches:
        ctx.set_transform(*b["m"])
        ctx.draw_triangles(b["xy"], _payload(b, t0 if index else None), z=b["z"], gouraud=True)
        t0 += b["xy"].shape[0]
    return ctx.get_buffer_numpy(), (ctx.get_depth_buffer() if mode != "nz" else None)


def expected_payload(W, H, alpha, bg, mode, clear_depth, batches, info=None):
    """(framebuffer, depth or None) after the opaque `batches`; info receives
    covered, texels, and per covered pixel tid (texel id sampled) and batch."""
    for b in batches:
        assert b["tex"].shape[2] == 3 and b["ct"][3] == 1, "payload derivation: opaque batches only"
    pay, depth = _oracle_pass(W, H, mode, clear_depth, batches, False)
    idx = _oracle_pass(W, H, mode, clear_depth, batches, True)[0][..., 0]
    back = scenes.OracleFactory().context(W, H, alpha)
    back.set_color(*bg)
    fb = back.get_buffer_numpy()
    covered = idx >= 0
    texels = set()
    tids = np.full((H, W), -1, dtype=np.int64)
    t0 = 0
    for k, b in enumerate(batches):
        end = t0 + b["xy"].shape[0]
        sel = covered & (idx >= t0) & (idx < end)
        t0 = end
        if not sel.any():
            continue
        u, v = persp_uv(pay[..., 0][sel], pay[..., 1][sel], pay[..., 2][sel])
        t, tid = T.sample(b["tex"], u, v)
        ct = np.asarray(b["ct"], dtype=np.float64)
        fb[sel, 0] = t[:, 0] * ct[0]
        fb[sel, 1] = t[:, 1] * ct[1]
        fb[sel, 2] = t[:, 2] * ct[2]
        if alpha:
            fb[sel, 3] = t[:, 3] * ct[3]
        tids[sel] = tid
        texels |= {(k, int(i)) for i in np.unique(tid)}
    if info is not None:
        info.update(covered=covered, texels=texels, tids=tids)
    return fb, depth


def expected_loop(W, H, alpha, bg, mode, clear_depth, batches, info=None):
    """The same by the per-triangle derivation (any batch)."""
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
        pay = _payload(b)
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
            zpass += int(ok.sum())
            zfail += int((cov & ~ok).sum())
            ys, xs = np.nonzero(ok)
            if ys.size == 0:
                continue
            u, v = persp_uv(p[ys, xs, 0], p[ys, xs, 1], p[ys, xs, 2])
            tx, tid = T.sample(b["tex"], u, v)
            for y, x, c in zip(ys.tolist(), xs.tolist(), tx.tolist()):
                lib.ApplyPixel(mp, x, y, c[0], c[1], c[2], c[3])
            if mode == "zw":
                D[ok] = zq[ok]
            covered |= ok
            texels |= {(k, int(i)) for i in np.unique(tid)}
    if info is not None:
        info.update(covered=covered, texels=texels, zpass=zpass, zfail=zfail)
    return main.get_buffer_numpy(), (D if mode != "nz" else None)


def draw_gpu(ctx, fac, mode, clear_depth, bg, batches, textures=None):
    """The batches through the library: draw_textured_triangles(..., q=...)."""
    ctx.set_color(*bg)
    T._set_depth_mode(ctx, mode)
    if mode != "nz":
        ctx.clear_depth(clear_depth)
    for k, b in enumerate(batches):
        tex = textures[k] if textures else fac.texture(b["tex"])
        ctx.set_transform(*b["m"])
        ctx.set_color_transform(*b["ct"])
        ctx.draw_textured_triangles(tex, b["xy"], b["uv"], z=b["z"], q=batch_q(b))
    return ctx.get_buffer_numpy(), (ctx.get_depth_buffer() if mode != "nz" else None)


def soup(W, H, n, seed, tex, qrange=(0.2, 5.0), **kw):
    """textured_ref.soup with q uniform in qrange per corner."""
    b = T.soup(W, H, n, seed, tex, **kw)
    b["q"] = np.random.default_rng(seed + 1000).uniform(qrange[0], qrange[1], size=(n, 3))
    return b


def q_spread(q):
    """Largest max / min of q within a triangle (positive finite q)."""
    q = np.asarray(q).reshape(-1, 3)
    ok = np.isfinite(q).all(axis=1) & (q > 0).all(axis=1)
    return float((q[ok].max(axis=1) / q[ok].min(axis=1)).max()) if ok.any() else 0.0


# ---- the mesh front end -------------------------------------------------------
def vertex_q(pos, M):
    """q (nv,) = 1.0 / cw, NaN where not cw > 0."""
    cw = MC.clip_coords(pos, M)[3]
    with np.errstate(all="ignore"):
        return np.where(cw > 0, 1.0 / cw, np.nan)


def expand_q(mesh, M):
    """mesh_ref.expand of a textured mesh plus q (n, 3) gathered like z."""
    xy, z, uv = MR.expand(mesh, M)
    idx = np.asarray(mesh["idx"]).reshape(-1, 3).astype(np.int64)
    return xy, z, uv, np.ascontiguousarray(vertex_q(mesh["pos"], M)[idx])


def clip_soup_q(mesh, M, w_near=0.0, cull=0, persp=True):
    """mesh_clip_ref.clip_soup of a textured mesh plus q (n_out, 3): a corner's
    1 / cw (NaN where not cw > 0), a cut vertex's 1 / w_near; ones with the
    perspective state off.  Returns xy, z, uv, q, counts."""
    info = {}
    xy, z, uv, counts = MC.clip_soup(mesh, M, w_near, cull, info)
    if not persp:
        return xy, z, uv, np.ones((xy.shape[0], 3)), counts
    idx = np.asarray(mesh["idx"]).reshape(-1, 3).astype(np.int64)
    n = idx.shape[0]
    cw = MC.clip_coords(mesh["pos"], M)[3][idx]
    sa, sb = info["sa"], info["sb"]
    aw = np.take_along_axis(cw, sa, axis=1)
    with np.errstate(all="ignore"):
        q = np.where(sa != sb, 1.0 / w_near if w_near > 0 else np.nan, np.where(aw > 0, 1.0 / aw, np.nan))
    halves = np.array([[0, 1, 2], [0, 2, 3]])
    a2 = info["area2"]
    with np.errstate(invalid="ignore"):
        culled = (a2 > 0) if cull == 1 else ((a2 < 0) if cull == 2 else np.zeros((n, 2), dtype=bool))
    keep = info["exists"] & ~culled
    assert np.array_equal(keep.sum(axis=1), counts)
    return xy, z, uv, np.ascontiguousarray(q[:, halves].reshape(n * 2, 3)[keep.reshape(n * 2)]), counts


def mesh_batch(mesh, M, tex, w_near=0.0, cull=0, persp=True, m=MR.XFORM, ct=(0.9, 0.8, 0.7, 1.0)):
    """The batch a draw_mesh of a textured mesh rasterises with the perspective
    state `persp` (the clip stage runs when w_near > 0 or cull != 0)."""
    if w_near > 0 or cull != 0:
        xy, z, uv, q, _ = clip_soup_q(mesh, M, w_near, cull, persp)
    else:
        xy, z, uv, q = expand_q(mesh, M)
        if not persp:
            q = np.ones_like(q)
    return dict(xy=xy, uv=uv, z=z, q=q, tex=tex, ct=tuple(ct), m=tuple(m))


# ---- the per-fragment arithmetic without the oracle ---------------------------
def fragment_uv(xy, uv, q, m, px, py):
    """(u, v, w1, w2) at pixels (px, py) (arrays) of one triangle -- xy (6,),
    uv (6,), q (3,), context transform m -- by the specified expressions, each
    operation a separate rounded numpy operation."""
    xy, uv, q = np.asarray(xy, dtype=np.float64), np.asarray(uv, dtype=np.float64), np.asarray(q, dtype=np.float64)
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    s = MR.xform(m, xy.reshape(1, 6))[0]
    with np.errstate(all="ignore"):
        e1x, e1y, e2x, e2y = s[1, 0] - s[0, 0], s[1, 1] - s[0, 1], s[2, 0] - s[0, 0], s[2, 1] - s[0, 1]
        inv = 1.0 / (e1x * e2y - e2x * e1y)
        dx, dy = px - s[0, 0], py - s[0, 1]
        w1 = (dx * e2y - e2x * dy) * inv
        w2 = (e1x * dy - dx * e1y) * inv
        a = uv[0::2] * q
        b = uv[1::2] * q
        U = a[0] + (a[1] - a[0]) * w1 + (a[2] - a[0]) * w2
        V = b[0] + (b[1] - b[0]) * w1 + (b[2] - b[0]) * w2
        Q = q[0] + (q[1] - q[0]) * w1 + (q[2] - q[0]) * w2
        u, v = persp_uv(U, V, Q)
    return u, v, w1, w2


def affine_share(W, H, mode, clear_depth, batches):
    """Share of the covered pixels of opaque `batches` whose perspective texel
    differs from the texel the affine draw of the same batches samples."""
    info = {}
    expected_payload(W, H, False, BG, mode, clear_depth, batches, info)
    cov = info["covered"]
    # the affine texel ids: textured_ref's payload pass (u, v, index) of the same batches
    ora = scenes.OracleFactory().context(W, H, True)
    ora.set_color(0.0, 0.0, -1.0, 0.0)
    T._set_depth_mode(ora, mode)
    if mode != "nz":
        ora.clear_depth(clear_depth)
    t0, starts = 0, []
    for b in batches:
        ora.set_transform(*b["m"])
        ora.draw_triangles(b["xy"], T._payload(b["uv"], t0), z=b["z"], gouraud=True)
        starts.append(t0)
        t0 += b["xy"].shape[0]
    p = ora.get_buffer_numpy()
    tids = np.full((H, W), -1, dtype=np.int64)
    for k, b in enumerate(batches):
        sel = cov & (p[..., 2] >= starts[k]) & (p[..., 2] < starts[k] + b["xy"].shape[0])
        if sel.any():
            tids[sel] = T.sample(b["tex"], p[..., 0][sel], p[..., 1][sel])[1]
    share = float((tids[cov] != info["tids"][cov]).mean()) if cov.any() else 0.0
    return share, float(cov.mean())


# ---- the scenes the GPU tests draw (tests/test_persp_ref.py checks that they
# discriminate: most covered pixels sample another texel than the affine draw)
W, H = 130, 97             # 3 x 4 tiles, partial right and bottom tiles
BG = (0.25, 0.25, 0.25, 0.25)
CLEAR = 0x90000000         # z in (0.05, 0.99): both outcomes of the LESS test
FAR = 0xFFFFFFFF
CT = (0.9, 0.8, 0.7, 1.0)
CT_BLEND = (0.9, 0.8, 0.7, 0.5)
KINDS = ("opaque", "ct_alpha", "rgba_texture")
NEAR = 0.25
MESH_TEX = (149, 101)      # texels of the mesh scenes' texture (w, h)


def soup_batches(kind, n=(90, 14)):
    """Slivers and small triangles (spread 40) under a rotate + scale transform,
    then large triangles (spread 70) over them; q uniform in [0.2, 5]."""
    if kind == "rgba_texture":
        t1, t2 = T.texture_rgba(), T.texture_rgba(seed=9, w=12, h=10)
    else:
        t1, t2 = T.texture_rgb(), T.texture_rgb(seed=8, w=11, h=7)
    ct = CT_BLEND if kind == "ct_alpha" else CT
    return [soup(W, H, n[0], 11, t1, spread=40.0, m=T.XFORM, ct=ct),
            soup(W, H, n[1], 12, t2, spread=70.0, ct=ct)]


def mesh_texture(alpha=False):
    return scenes.rng(21).uniform(0, 1, size=(MESH_TEX[1], MESH_TEX[0], 4 if alpha else 3))


def mesh_scene():
    """A coarse displaced sphere: its triangles are large enough on the screen
    for 1/cw to vary within them."""
    return MR.sphere3d(rows=4, cols=4, uv_size=MESH_TEX)


def mesh_matrix(name):
    return {"perspective": MR.perspective, "behind_eye": MR.behind_eye, "affine": MR.affine}[name](W, H)


MESH_STATES = ((0.0, 0), (NEAR, 1), (NEAR, 2))   # (near plane, cull mode): the clip stage off, and on
# from inside the sphere every face that shows has area2 > 0: cull 1 leaves a frame without a covered pixel
MESH_EMPTY = (("behind_eye", NEAR, 1),)

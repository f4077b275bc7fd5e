"""The numpy reference of the mesh clip stage (DESIGN.md §3 "Clip stage"):
near-plane clipping against cw = w_near and back-face culling of a mesh's
triangles, restated elementwise in the specified order of operations (every
product, sum and quotient rounded; no `@`, no np.dot), and the oracle frames of
the soup it produces.

clip_soup walks each triangle as the specification does -- Sutherland-Hodgman
from corner 0: emit corner k if inside, then the cut of edge (k, k + 1) if its
ends differ, the cut always formed from the inside end -- with the triangles
side by side in arrays.  tests/test_mesh_clip_ref.py checks it against a scalar
Python-float loop written independently.

A mesh is mesh_ref's dict; matrices are mesh_ref's.
"""
import numpy as np

import mesh_ref as MR
import scenes
import textured_ref as T


def clip_coords(pos, M):
    """(cx, cy, cz, cw), each (nv,): the vertex stage's rows,
    ((M0*px + M1*py) + M2*pz) + M3, before the division."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    M = MR.IDENT16 if M is None else np.asarray(M, dtype=np.float64).reshape(16)
    px, py, pz = pos[:, 0], pos[:, 1], pos[:, 2]

    def row(r):
        return ((M[4 * r] * px + M[4 * r + 1] * py) + M[4 * r + 2] * pz) + M[4 * r + 3]

    return row(0), row(1), row(2), row(3)


def corner_attributes(mesh):
    """Per-corner attributes (n, 3, NA): RGBA for Gouraud, UV for textured,
    NA = 0 for flat -- and the flat colour (n, 4) of i0, or None."""
    idx = np.asarray(mesh["idx"]).reshape(-1, 3).astype(np.int64)
    n = idx.shape[0]
    if "uv" in mesh:
        return np.asarray(mesh["uv"], dtype=np.float64)[idx].reshape(n, 3, 2), None
    col = np.asarray(mesh["colors"], dtype=np.float64)
    if mesh["gouraud"]:
        return col[idx].reshape(n, 3, 4), None
    return np.zeros((n, 3, 0)), col[idx[:, 0]].reshape(n, 4)


def inside_counts(mesh, M, w_near):
    """m (n,): vertices of each triangle with cw >= w_near (False for NaN)."""
    cw = clip_coords(mesh["pos"], M)[3]
    idx = np.asarray(mesh["idx"]).reshape(-1, 3).astype(np.int64)
    with np.errstate(invalid="ignore"):
        return (cw[idx] >= w_near).sum(axis=1)


def area2(xy):
    """(x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0) of a soup (k, 6)."""
    p = np.asarray(xy).reshape(-1, 3, 2)
    with np.errstate(all="ignore"):
        return ((p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1])
                - (p[:, 2, 0] - p[:, 0, 0]) * (p[:, 1, 1] - p[:, 0, 1]))


def clip_soup(mesh, M, w_near=0.0, cull=0, info=None):
    """The soup a mesh draw rasterises under near plane w_near (0: off) and
    cull mode (0 none, 1 drops area2 > 0, 2 drops area2 < 0):
    xy (n_out, 6), z (n_out, 3), attr (n_out, 12 | 4 | 6), counts (n,) = output
    triangles of each source triangle.  Outputs of triangle t precede those of
    t + 1; the halves of a quad are (q0, q1, q2) then (q0, q2, q3).
    info (a dict) receives t (the cut parameters, 1-d) and inside (n,)."""
    idx = np.asarray(mesh["idx"]).reshape(-1, 3).astype(np.int64)
    n = idx.shape[0]
    cx, cy, cz, cw = (c[idx] for c in clip_coords(mesh["pos"], M))   # (n, 3) each
    A, flat = corner_attributes(mesh)
    NA = A.shape[2]
    with np.errstate(invalid="ignore"):
        inside = (cw >= w_near) if w_near > 0 else np.ones((n, 3), dtype=bool)

    # the walk: polygon vertex s of triangle t is (sa, sb) -- corner sa itself
    # when sb == sa, else the cut from sa (inside) towards sb (outside)
    sa = np.zeros((n, 4), dtype=np.int64)
    sb = np.zeros((n, 4), dtype=np.int64)
    fill = np.zeros(n, dtype=np.int64)
    rows = np.arange(n)
    for k in range(3):
        j = (k + 1) % 3
        emit = inside[:, k]
        sa[rows[emit], fill[emit]] = k
        sb[rows[emit], fill[emit]] = k
        fill = fill + emit
        cross = inside[:, k] != inside[:, j]
        a = np.where(inside[:, k], k, j)
        b = np.where(inside[:, k], j, k)
        sa[rows[cross], fill[cross]] = a[cross]
        sb[rows[cross], fill[cross]] = b[cross]
        fill = fill + cross
    assert np.isin(fill, (0, 3, 4)).all()

    def at(c, s):   # (n, 4): component c of corner s[t, slot]
        return np.take_along_axis(c, s, axis=1)

    is_cut = sa != sb
    ax, ay, az, aw = at(cx, sa), at(cy, sa), at(cz, sa), at(cw, sa)
    bx, by, bz, bw = at(cx, sb), at(cy, sb), at(cz, sb), at(cw, sb)
    with np.errstate(all="ignore"):
        t = (aw - w_near) / (aw - bw)
        qx = ax + (bx - ax) * t
        qy = ay + (by - ay) * t
        qz = az + (bz - az) * t
        front = aw > 0
        x = np.where(is_cut, qx / w_near, np.where(front, ax / aw, np.nan))
        y = np.where(is_cut, qy / w_near, np.where(front, ay / aw, np.nan))
        z = np.where(is_cut, qz / w_near, np.where(front, az / aw, np.nan))
        Aa = np.take_along_axis(A, sa[:, :, None], axis=1)   # (n, 4, NA)
        Ab = np.take_along_axis(A, sb[:, :, None], axis=1)
        attr = np.where(is_cut[:, :, None], Aa + (Ab - Aa) * t[:, :, None], Aa)

    halves = np.array([[0, 1, 2], [0, 2, 3]])
    exists = np.stack([fill >= 3, fill == 4], axis=1)                 # (n, 2)
    hx, hy, hz = x[:, halves], y[:, halves], z[:, halves]               # (n, 2, 3)
    xy_all = np.stack([hx, hy], axis=-1).reshape(n, 2, 6)
    a2 = area2(xy_all.reshape(n * 2, 6)).reshape(n, 2)
    with np.errstate(invalid="ignore"):
        culled = (a2 > 0) if cull == 1 else ((a2 < 0) if cull == 2 else np.zeros((n, 2), dtype=bool))
    keep = exists & ~culled
    if flat is not None:
        attr_all = np.broadcast_to(flat[:, None, :], (n, 2, 4))
    else:
        attr_all = attr[:, halves].reshape(n, 2, 3 * NA)
    if info is not None:
        info["t"] = t[is_cut & (np.arange(4)[None, :] < fill[:, None])]
        info["inside"] = inside.sum(axis=1)
        info["exists"] = exists
        info["area2"] = a2
        # the polygons themselves: vertex s < fill[t] of triangle t is (sa, sb) at (x, y, z)
        info.update(sa=sa, sb=sb, fill=fill, x=x, y=y, z=z)
    sel = keep.reshape(n * 2)   # row-major: triangle by triangle, first half first (stable)
    return (np.ascontiguousarray(xy_all.reshape(n * 2, 6)[sel]), np.ascontiguousarray(hz.reshape(n * 2, 3)[sel]),
            np.ascontiguousarray(attr_all.reshape(n * 2, -1)[sel]), keep.sum(axis=1))


# ---- expected frames ----------------------------------------------------------
def oracle_frame(W, H, alpha, mode, draws, m=MR.XFORM, ct=(1.0, 1.0, 1.0, 1.0), before=None, clear=MR.CLEAR):
    """mesh_ref.oracle_frame for clipped draws [(mesh, M, w_near, cull), ...]:
    the oracle's DrawTriangles of each reference soup, in order."""
    ctx = scenes.OracleFactory().context(W, H, alpha)
    MR.begin_frame(ctx, mode, m, ct, clear=clear)
    if before:
        before(ctx)
    for mesh, M, w_near, cull in draws:
        xy, z, attr, _ = clip_soup(mesh, M, w_near, cull)
        if xy.shape[0]:
            ctx.draw_triangles(xy, attr, z=z, gouraud=bool(mesh["gouraud"]))
    return MR.read_frame(ctx, mode)


def textured_batch(mesh, M, tex, w_near, cull, m=MR.XFORM, ct=(0.9, 0.8, 0.7, 1.0)):
    """mesh_ref.textured_batch of the clipped soup (for textured_ref.expected_*)."""
    xy, z, uv, _ = clip_soup(mesh, M, w_near, cull)
    return dict(xy=xy, uv=uv, z=z, tex=tex, ct=tuple(ct), m=tuple(m))

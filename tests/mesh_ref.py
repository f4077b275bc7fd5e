"""The numpy reference of the mesh front end (DESIGN.md §3 "Vertex stage")
and the meshes, matrices and scenes its tests share.

vertex_stage restates the vertex stage with explicit elementwise products and
sums in the specified order (no `@`, no np.dot: BLAS may fuse operations);
expand gathers the transformed vertices and the attributes through the indices
into the triangle-soup layout of draw_triangles.  Expected frames are then the
CPU oracle's DrawTriangles of that soup (oracle_frame), or, for textured
meshes, textured_ref's derivations from it.

A mesh is a dict: pos (nv, 3), idx (n, 3) uint32, and colors (nv, 4) with
gouraud (bool), or uv (nv, 2).
"""
import numpy as np

import scenes
import textured_ref as T

IDENT16 = np.eye(4).reshape(16)


def vertex_stage(pos, M):
    """(x, y, z), each (nv,): c = M (px, py, pz, 1) row by row as
    ((M0*px + M1*py) + M2*pz) + M3, then / cw; NaN where not cw > 0."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    M = IDENT16 if M is None else np.asarray(M, dtype=np.float64).reshape(16)
    px, py, pz = pos[:, 0], pos[:, 1], pos[:, 2]

    def row(r):
        return ((M[4 * r] * px + M[4 * r + 1] * py) + M[4 * r + 2] * pz) + M[4 * r + 3]

    cx, cy, cz, cw = row(0), row(1), row(2), row(3)
    front = cw > 0
    with np.errstate(all="ignore"):
        return (np.where(front, cx / cw, np.nan), np.where(front, cy / cw, np.nan),
                np.where(front, cz / cw, np.nan))


def expand(mesh, M):
    """The soup of `mesh` under M: xy (n, 6), z (n, 3), attr (n, 12) Gouraud /
    (n, 4) flat, the colour of the first index / (n, 6) textured."""
    x, y, z = vertex_stage(mesh["pos"], M)
    idx = np.asarray(mesh["idx"]).reshape(-1, 3).astype(np.int64)
    n = idx.shape[0]
    xy = np.stack([x[idx], y[idx]], axis=-1).reshape(n, 6)
    if "uv" in mesh:
        attr = np.asarray(mesh["uv"], dtype=np.float64)[idx].reshape(n, 6)
    elif mesh["gouraud"]:
        attr = np.asarray(mesh["colors"], dtype=np.float64)[idx].reshape(n, 12)
    else:
        attr = np.asarray(mesh["colors"], dtype=np.float64)[idx[:, 0]].reshape(n, 4)
    return np.ascontiguousarray(xy), np.ascontiguousarray(z[idx]), np.ascontiguousarray(attr)


def xform(m, xy):
    """The context transform on a soup's positions, in nr_xform's order."""
    p = xy.reshape(-1, 3, 2)
    with np.errstate(all="ignore"):
        return np.stack([m[0] * p[..., 0] + m[2] * p[..., 1] + m[4],
                         m[1] * p[..., 0] + m[3] * p[..., 1] + m[5]], axis=-1)


def kept(xy, m=T.IDENT):
    """Triangles the rasters keep: every screen vertex finite and den != 0."""
    s = xform(m, xy)
    with np.errstate(all="ignore"):
        e1, e2 = s[:, 1] - s[:, 0], s[:, 2] - s[:, 0]
        den = e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]
        return np.isfinite(s).all(axis=(1, 2)) & (den != 0)


# ---- meshes ---------------------------------------------------------------
def grid_indices(rows, cols):
    """The triangles of scenes.sphere_mesh's rows x cols quad grid, in its
    order, over vertices numbered i * (cols + 1) + j."""
    i = np.arange(rows)[:, None].repeat(cols, 1).ravel()
    j = np.arange(cols)[None, :].repeat(rows, 0).ravel()
    v = lambda a, b: a * (cols + 1) + b
    t0 = np.stack([v(i, j), v(i + 1, j), v(i + 1, j + 1)], 1)
    t1 = np.stack([v(i, j), v(i + 1, j + 1), v(i, j + 1)], 1)
    return np.stack([t0, t1], 1).reshape(-1, 3).astype(np.uint32)


def sphere_screen_mesh(W, H, rows, cols, R_frac=0.45):
    """scenes.sphere_mesh as an indexed mesh: the same vertex arrays (screen
    x, screen y, depth; colour = normal * 0.5 + 0.5) by the same expressions,
    so that its soup under the identity is sphere_mesh's own."""
    R = R_frac * H
    th = np.linspace(0, np.pi, rows + 1)
    ph = np.linspace(0, 2 * np.pi, cols + 1)
    Tm, Pm = np.meshgrid(th, ph, indexing="ij")
    r = R * (1 + 0.15 * np.sin(5 * Tm) * np.sin(7 * Pm))
    X = r * np.sin(Tm) * np.cos(Pm)
    Y = r * np.cos(Tm)
    Z = r * np.sin(Tm) * np.sin(Pm)
    nx, ny, nz = np.sin(Tm) * np.cos(Pm), np.cos(Tm), np.sin(Tm) * np.sin(Pm)
    pos = np.stack([W / 2 + X, H / 2 - Y, 0.5 + Z / (2.4 * R)], axis=-1).reshape(-1, 3)
    col = np.stack([nx * 0.5 + 0.5, ny * 0.5 + 0.5, nz * 0.5 + 0.5, np.ones_like(nx)], axis=-1).reshape(-1, 4)
    return dict(pos=pos, idx=grid_indices(rows, cols), colors=col, gouraud=True)


def sphere3d(rows=10, cols=16, seed=3, alpha=None, gouraud=True, uv_size=None):
    """A displaced unit sphere around the origin (model space, y up): random
    vertex colours with alpha 1 or uniform in `alpha`; with uv_size = (w, h) a
    textured mesh instead, its UVs running past the texture on every side."""
    th = np.linspace(0, np.pi, rows + 1)
    ph = np.linspace(0, 2 * np.pi, cols + 1)
    Tm, Pm = np.meshgrid(th, ph, indexing="ij")
    r = 1 + 0.15 * np.sin(5 * Tm) * np.sin(7 * Pm)
    pos = np.stack([r * np.sin(Tm) * np.cos(Pm), r * np.cos(Tm), r * np.sin(Tm) * np.sin(Pm)], -1).reshape(-1, 3)
    mesh = dict(pos=np.ascontiguousarray(pos), idx=grid_indices(rows, cols))
    g = scenes.rng(seed)
    if uv_size is not None:
        w, h = uv_size
        u = -3 + (Pm / (2 * np.pi)) * (w + 6)
        v = -3 + (Tm / np.pi) * (h + 6)
        mesh["uv"] = np.ascontiguousarray(np.stack([u, v], -1).reshape(-1, 2))
        return mesh
    col = g.uniform(0, 1, size=(pos.shape[0], 4))
    col[:, 3] = 1.0 if alpha is None else g.uniform(alpha[0], alpha[1], size=pos.shape[0])
    mesh.update(colors=col, gouraud=gouraud)
    return mesh


def random_mesh(nv, n, seed):
    """nv random vertices in [-1, 1]^3 and n random index triples."""
    g = scenes.rng(seed)
    return dict(pos=g.uniform(-1, 1, size=(nv, 3)), idx=g.integers(0, nv, size=(n, 3)).astype(np.uint32),
                colors=g.uniform(0, 1, size=(nv, 4)), gouraud=True)


# ---- matrices (row-major 4x4, viewport included) ----------------------------
def rotation(ax, ay):
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    rx = np.array([[1, 0, 0, 0], [0, cx, -sx, 0], [0, sx, cx, 0], [0, 0, 0, 1.0]])
    ry = np.array([[cy, 0, sy, 0], [0, 1, 0, 0], [-sy, 0, cy, 0], [0, 0, 0, 1.0]])
    return rx @ ry


def perspective(W, H, d=3.0, f=3.2, near=1.8, far=4.2, ax=0.3, ay=0.5, znear=0.05, zfar=0.95):
    """Eye at distance d in front of the origin, looking at it: cw = the
    view-space depth, screen = centre + (H / 2) f (x, -y) / cw, and z = a + b /
    cw runs from znear at cw = near to zfar at cw = far."""
    b = (zfar - znear) / (1 / far - 1 / near)
    a = znear - b / near
    view = rotation(ax, ay)
    view[2, 3] = d
    s = 0.5 * H * f
    proj = np.array([[s, 0, W / 2, 0], [0, -s, H / 2, 0], [0, 0, a, b], [0, 0, 1.0, 0]])
    return np.ascontiguousarray((proj @ view).reshape(16))


def affine(W, H, ax=0.3, ay=0.5, scale=0.42):
    """Orthographic: last row (0, 0, 0, 1), so cw == 1 and nothing is divided."""
    s = scale * H
    vp = np.array([[s, 0, 0, W / 2], [0, -s, 0, H / 2], [0, 0, 0.35, 0.5], [0, 0, 0, 1.0]])
    M = vp @ rotation(ax, ay)
    M[3] = (0.0, 0.0, 0.0, 1.0)
    return np.ascontiguousarray(M.reshape(16))


def behind_eye(W, H):
    """The eye inside the sphere: part of the mesh lies at cw <= 0."""
    return perspective(W, H, d=0.45, f=0.6, near=0.05, far=1.7, ax=0.2, ay=0.4)


def behind_eye_mesh():
    """sphere3d with one vertex moved to cw = 1e-9 under behind_eye: its
    triangles are kept and reach coordinates beyond 1e7."""
    mesh = sphere3d()
    M = behind_eye(130, 97).reshape(4, 4)
    pos = mesh["pos"]
    cw = pos @ M[3, :3] + M[3, 3]
    idx = mesh["idx"].astype(np.int64)
    # a vertex whose triangles lie wholly in front of the eye, the nearest such
    front = np.ones(pos.shape[0], dtype=bool)
    np.logical_and.at(front, idx.ravel(), np.repeat((cw[idx] > 0.05).all(axis=1), 3))
    front &= np.bincount(idx.ravel(), minlength=pos.shape[0]) > 0
    v = np.flatnonzero(front)[np.argmin(cw[front])]
    # along the view axis (row 3 is a unit vector: a rotation's) to cw = 1e-9
    pos[v] += (1e-9 - cw[v]) * M[3, :3]
    return mesh


# ---- expected frames --------------------------------------------------------
XFORM = T.XFORM
BG = (0.25, 0.25, 0.25, 0.25)
CLEAR = 0x90000000         # z in (0.05, 0.95): both outcomes of the LESS test


def begin_frame(ctx, mode, m=XFORM, ct=(1.0, 1.0, 1.0, 1.0), bg=BG, clear=CLEAR):
    ctx.set_color(*bg)
    T._set_depth_mode(ctx, mode)
    if mode != "nz":
        ctx.clear_depth(clear)
    ctx.set_transform(*m)
    ctx.set_color_transform(*ct)


def read_frame(ctx, mode):
    return ctx.get_buffer_numpy(), (ctx.get_depth_buffer() if mode != "nz" else None)


def oracle_frame(W, H, alpha, mode, draws, m=XFORM, ct=(1.0, 1.0, 1.0, 1.0), before=None, clear=CLEAR):
    """(framebuffer, depth or None) of the oracle after the colour-mesh draws
    [(mesh, M), ...] as soups; before(ctx) runs after the clears."""
    ctx = scenes.OracleFactory().context(W, H, alpha)
    begin_frame(ctx, mode, m, ct, clear=clear)
    if before:
        before(ctx)
    for mesh, M in draws:
        xy, z, attr = expand(mesh, M)
        if xy.shape[0]:
            ctx.draw_triangles(xy, attr, z=z, gouraud=bool(mesh["gouraud"]))
    return read_frame(ctx, mode)


def textured_batch(mesh, M, tex, m=XFORM, ct=(0.9, 0.8, 0.7, 1.0)):
    xy, z, uv = expand(mesh, M)
    return dict(xy=xy, uv=uv, z=z, tex=tex, ct=tuple(ct), m=tuple(m))

"""The numpy reference of vertex lighting (DESIGN.md §3 "Vertex lighting") and
the scene its tests share.

lit_colors restates the light pass with explicit elementwise products and sums
in the specified order (no `@`, no np.dot, as mesh_ref.vertex_stage explains).
Lighting comes before everything else that reads colours, so a lit soup is
mesh_ref.expand, mesh_clip_ref.clip_soup or mesh_inst_ref.instanced_soup of
dict(mesh, colors=lit) -- for an instanced draw instance by instance, each
under its own normal matrix, the tint multiplying the lit colours -- and the
expected frames are the existing oracle_frame helpers over those meshes.

A mesh is mesh_ref's dict with normals (nv, 3); a normal matrix is row-major
3x3 ((9,) or (3, 3)), None the identity; lights are rows (dx, dy, dz, cr, cg,
cb), d towards the light.
"""
import numpy as np

import mesh_clip_ref as MC
import mesh_inst_ref as MI
import mesh_ref as MR
import scenes

IDENT9 = np.eye(3).reshape(9)
DEFAULT_AMBIENT = (1.0, 1.0, 1.0)
MAX_LIGHTS = 8


def _lights(lights):
    return np.zeros((0, 6)) if lights is None else np.asarray(lights, dtype=np.float64).reshape(-1, 6)


def lit_colors(mesh, N=None, ambient=None, lights=None):
    """(nv, 4): the lit vertex colours of `mesh` under the normal matrix N, the
    ambient colour (None: (1, 1, 1)) and the lights, in order."""
    col = np.asarray(mesh["colors"], dtype=np.float64).reshape(-1, 4)
    nrm = np.asarray(mesh["normals"], dtype=np.float64).reshape(-1, 3)
    N = IDENT9 if N is None else np.asarray(N, dtype=np.float64).reshape(9)
    A = DEFAULT_AMBIENT if ambient is None else np.asarray(ambient, dtype=np.float64).reshape(3)
    nx, ny, nz = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    with np.errstate(all="ignore"):
        wx = (N[0] * nx + N[1] * ny) + N[2] * nz
        wy = (N[3] * nx + N[4] * ny) + N[5] * nz
        wz = (N[6] * nx + N[7] * ny) + N[8] * nz
        acc = [np.full(col.shape[0], A[c], dtype=np.float64) for c in range(3)]
        for L in _lights(lights):
            dot = (wx * L[0] + wy * L[1]) + wz * L[2]
            d = np.where(dot > 0, dot, 0.0)
            for c in range(3):
                acc[c] = acc[c] + d * L[3 + c]
        out = col.copy()
        for c in range(3):
            p = col[:, c] * acc[c]
            out[:, c] = np.where(p < 0, 0.0, np.where(p > 1, 1.0, p))
    return out


def lit_mesh(mesh, N=None, ambient=None, lights=None):
    """`mesh` with its colours replaced by the lit ones: what every later stage reads."""
    return dict(mesh, colors=lit_colors(mesh, N, ambient, lights))


def lit_soup(mesh, M, N=None, ambient=None, lights=None, w_near=0.0, cull=0):
    """(xy, z, attr) of a lit single draw under the clip state."""
    lm = lit_mesh(mesh, N, ambient, lights)
    if w_near > 0 or cull != 0:
        return MC.clip_soup(lm, M, w_near, cull)[:3]
    return MR.expand(lm, M)


def instance_meshes(mesh, mats, normals=None, tint=None, ambient=None, lights=None):
    """[(mesh_k, M_k), ...]: the K single unlit draws a lit instanced draw
    stands for -- instance k lit under normals[k], then tinted."""
    mats = np.asarray(mats, dtype=np.float64).reshape(-1, 16)
    K = mats.shape[0]
    nm = None if normals is None else np.asarray(normals, dtype=np.float64).reshape(K, 9)
    tn = None if tint is None else np.asarray(tint, dtype=np.float64).reshape(K, 4)
    return [(MI.tinted(lit_mesh(mesh, None if nm is None else nm[k], ambient, lights), None if tn is None else tn[k]),
             mats[k]) for k in range(K)]


def lit_instanced_soup(mesh, mats, normals=None, tint=None, ambient=None, lights=None, w_near=0.0, cull=0,
                       counts=None):
    """(xy, z, attr) of a lit instanced draw: the instances' soups in order."""
    clip = w_near > 0 or cull != 0
    parts = []
    for m, M in instance_meshes(mesh, mats, normals, tint, ambient, lights):
        parts.append(MC.clip_soup(m, M, w_near, cull)[:3] if clip else MR.expand(m, M))
        if counts is not None:
            counts.append(parts[-1][0].shape[0])
    widths = (6, 3, MI.stride(mesh))
    return tuple(np.ascontiguousarray(np.concatenate([p[i] for p in parts], axis=0)) if parts
                 else np.zeros((0, widths[i])) for i in range(3))


def oracle_frame(W, H, alpha, mode, draws, w_near=0.0, cull=0, **kw):
    """The oracle's frame of the unlit draws [(mesh, M), ...] (lit_mesh /
    instance_meshes made them) under the clip state."""
    if w_near > 0 or cull != 0:
        return MC.oracle_frame(W, H, alpha, mode, [(m, M, w_near, cull) for m, M in draws], **kw)
    return MR.oracle_frame(W, H, alpha, mode, draws, **kw)


# ---- meshes and the shared scene ------------------------------------------------
def sphere_normals(rows=10, cols=16):
    """The analytic unit normals (sinT cosP, cosT, sinT sinP) of the sphere that
    mesh_ref.sphere3d displaces, on its vertex grid: (nv, 3)."""
    th = np.linspace(0, np.pi, rows + 1)
    ph = np.linspace(0, 2 * np.pi, cols + 1)
    Tm, Pm = np.meshgrid(th, ph, indexing="ij")
    return np.ascontiguousarray(np.stack([np.sin(Tm) * np.cos(Pm), np.cos(Tm), np.sin(Tm) * np.sin(Pm)], -1).reshape(-1, 3))


def lit_sphere3d(rows=10, cols=16, **kw):
    """mesh_ref.sphere3d with its analytic normals."""
    return dict(MR.sphere3d(rows, cols, **kw), normals=sphere_normals(rows, cols))


def random_lit_mesh(nv, n, seed):
    """mesh_ref.random_mesh with random unit-ish normals (length within 1e-15 of 1)."""
    g = scenes.rng(seed + 77)
    v = g.normal(size=(nv, 3))
    return dict(MR.random_mesh(nv, n, seed), normals=v / np.sqrt((v * v).sum(axis=1))[:, None])


def random_lights(nl, seed):
    """(ambient (3,), lights (nl, 6)): unit directions, colours that let some channels reach 1."""
    g = scenes.rng(seed + 5)
    d = g.normal(size=(nl, 3))
    d = d / np.sqrt((d * d).sum(axis=1))[:, None]
    return g.uniform(0.05, 0.3, size=3), np.concatenate([d, g.uniform(0.1, 1.6, size=(nl, 3))], axis=1)


AMBIENT = (0.15, 0.12, 0.2)
LIGHTS = np.array([[0.6, 0.64, -0.48, 1.6, 1.3, 1.0],
                   [-0.8, 0.0, 0.6, 0.2, 0.5, 0.9],
                   [0.0, -1.0, 0.0, 0.3, 0.3, 0.1]])
LIGHTS.setflags(write=False)


def rotation3(ax=0.3, ay=0.5):
    """The second normal matrix of the scene: mesh_ref.rotation's 3x3, (9,)."""
    return np.ascontiguousarray(MR.rotation(ax, ay)[:3, :3].reshape(9))

"""The numpy reference of instanced mesh draws (DESIGN.md §3 "Instanced mesh
draws") and the scene their tests share.

An instanced draw of a mesh under matrices M_0 .. M_{K-1} rasterises, by
definition, the concatenation in instance order of the soups the K single
draws would rasterise: mesh_ref.expand of the (tinted) mesh with the clip stage
off, mesh_clip_ref.clip_soup of it with the stage on.  A tint multiplies the
(nv, 4) vertex colours elementwise, in f64, before anything else -- as if the
mesh had been created with those colours.

A mesh is mesh_ref's dict; matrices are row-major 4x4, (K, 16).
"""
import functools

import numpy as np

import mesh_clip_ref as MC
import mesh_ref as MR
import persp_ref as P

W, H = 130, 97             # the target of tests/test_mesh_gpu.py: 3 x 4 tiles, partial right and bottom tiles
NEAR = 0.05                # the near plane of tests/test_mesh_clip_gpu.py


def stride(mesh):
    return 6 if "uv" in mesh else (12 if mesh["gouraud"] else 4)


def tinted(mesh, tint_k):
    """`mesh` with its vertex colours times tint_k (4,); None: the mesh itself."""
    if tint_k is None:
        return mesh
    return dict(mesh, colors=np.asarray(mesh["colors"], dtype=np.float64) * np.asarray(tint_k, dtype=np.float64))


def instance_meshes(mesh, mats, tint=None):
    """[(tinted mesh_k, M_k), ...]: the K single draws an instanced draw stands for."""
    mats = np.asarray(mats, dtype=np.float64).reshape(-1, 16)
    return [(tinted(mesh, None if tint is None else np.asarray(tint).reshape(-1, 4)[k]), mats[k])
            for k in range(mats.shape[0])]


def instanced_soup(mesh, mats, tint=None, w_near=0.0, cull=0, persp=False, counts=None):
    """(xy (N, 6), z (N, 3), attr (N, 12 | 4 | 6), q (N, 3) or None) of the
    instanced draw: the instances' soups in instance order, each in its own
    (stable) order.  The clip stage runs when w_near > 0 or cull != 0; q only
    for a perspective textured draw.  counts (a list) receives each instance's
    triangle count."""
    textured = "uv" in mesh
    assert not (textured and tint is not None)
    clip = w_near > 0 or cull != 0
    parts = []
    for m, M in instance_meshes(mesh, mats, tint):
        if textured and persp:
            part = P.clip_soup_q(m, M, w_near, cull, True)[:4] if clip else P.expand_q(m, M)
        else:
            part = (MC.clip_soup(m, M, w_near, cull)[:3] if clip else MR.expand(m, M)) + (None,)
        parts.append(part)
        if counts is not None:
            counts.append(part[0].shape[0])
    cat = lambda i, w: (np.ascontiguousarray(np.concatenate([p[i] for p in parts], axis=0)) if parts
                        else np.zeros((0, w)))
    q = cat(3, 3) if textured and persp else None
    return cat(0, 6), cat(1, 3), cat(2, stride(mesh)), q


def textured_batch(mesh, mats, tex, w_near=0.0, cull=0, persp=False, m=MR.XFORM, ct=(0.9, 0.8, 0.7, 1.0)):
    """The concatenated soup as one batch of textured_ref / persp_ref / bilinear_ref."""
    xy, z, uv, q = instanced_soup(mesh, mats, None, w_near, cull, persp)
    return dict(xy=xy, uv=uv, z=z, q=q if persp else np.ones((xy.shape[0], 3)), tex=tex, ct=tuple(ct), m=tuple(m))


def oracle_frame(Wd, Hd, alpha, mode, mesh, mats, tint=None, w_near=0.0, cull=0, m=MR.XFORM,
                 ct=(1.0, 1.0, 1.0, 1.0), clear=MR.CLEAR):
    """mesh_ref.oracle_frame / mesh_clip_ref.oracle_frame of the K single draws."""
    draws = instance_meshes(mesh, mats, tint)
    if w_near > 0 or cull != 0:
        return MC.oracle_frame(Wd, Hd, alpha, mode, [(a, M, w_near, cull) for a, M in draws], m=m, ct=ct, clear=clear)
    return MR.oracle_frame(Wd, Hd, alpha, mode, draws, m=m, ct=ct, clear=clear)


# ---- the shared scene ----------------------------------------------------------
def translate(x, y, z):
    A = np.eye(4)
    A[:3, 3] = (x, y, z)
    return A


@functools.lru_cache(maxsize=None)
def scene_matrices(k_random=7, seed=7):
    """(k_random + 3, 16): k_random placements M_k = P A_k of a scaled (0.25 ..
    0.6), translated sphere, then mesh_ref.behind_eye (partly at cw <= 0), a
    placement wholly off screen, and an exact copy of M_0 (every depth ties)."""
    Pm = MR.perspective(W, H).reshape(4, 4)
    g = np.random.default_rng(seed)
    mats = []
    for _ in range(k_random):
        s = g.uniform(0.25, 0.6)
        a, b, c = g.uniform(-1, 1, size=3)
        A = translate(1.6 * a, 1.12 * b, 1.4 * c)
        A[0, 0] = A[1, 1] = A[2, 2] = s
        mats.append(Pm @ A)
    mats.append(MR.behind_eye(W, H).reshape(4, 4))
    mats.append(Pm @ translate(50, 0, 0))
    mats.append(mats[0].copy())
    out = np.ascontiguousarray(np.stack(mats).reshape(-1, 16))
    out.setflags(write=False)
    return out


BEHIND, OFFSCREEN, DUPLICATE = -3, -2, -1   # the explicit instances, from the end


def scene_tints(K, seed=11, alpha=None):
    """(K, 4): colour factors in [0.3, 1]; alpha 1, or with alpha = (k, value)
    that one instance's alpha.  The duplicate instance (last) differs from
    instance 0 by construction (random)."""
    t = np.random.default_rng(seed).uniform(0.3, 1.0, size=(K, 4))
    t[:, 3] = 1.0
    if alpha is not None:
        t[alpha[0], 3] = alpha[1]
    return t

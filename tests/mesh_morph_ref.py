"""The numpy reference of morph targets (DESIGN.md §3 "Morph targets") and the
targets, weights and random morphs its tests share.

morph restates the morph pass with explicit elementwise products and sums in
index order and with the skip of zero-weight targets, which is part of the
definition.  A morphed mesh is an ordinary mesh: its expected soups and frames
are those of mesh_ref, mesh_clip_ref, mesh_inst_ref and mesh_light_ref over
dict(mesh, pos=..., normals=...); morph_posed is mesh_skin_ref.pose of it.

A morph is a dict: pos (nv, 3), dP (T, nv, 3), and normals (nv, 3) with dN
(T, nv, 3), or neither.
"""
import numpy as np

import mesh_light_ref as ML
import mesh_skin_ref as MS
import scenes


def morph(base_p, base_n, dP, dN, w):
    """(pos (nv, 3), nrm (nv, 3) or None):  X = px; for t in index order:
    if w_t == 0.0 skip (either sign; NaN is not zero); X = X + w_t * dPx[t][v]."""
    p = np.array(base_p, dtype=np.float64).reshape(-1, 3)
    nv = p.shape[0]
    dP = np.asarray(dP, dtype=np.float64).reshape(-1, nv, 3)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    assert w.shape[0] == dP.shape[0]
    n = None
    if base_n is not None:
        n = np.array(base_n, dtype=np.float64).reshape(nv, 3)
        dN = np.asarray(dN, dtype=np.float64).reshape(-1, nv, 3)
    with np.errstate(all="ignore"):
        for t in range(w.shape[0]):
            if w[t] == 0.0:
                continue
            p = p + w[t] * dP[t]                            # one rounded product, one rounded sum per component
            if n is not None:
                n = n + w[t] * dN[t]
    return p, n


def morphed(mesh, mo, w, normals=True):
    """`mesh` (a mesh_ref dict) under the morph: what every draw after
    morph_mesh reads.  normals False, or a morph without them: the mesh keeps
    its own."""
    use = normals and "normals" in mo and "normals" in mesh
    p, n = morph(mo["pos"], mo["normals"] if use else None, mo["dP"], mo["dN"] if use else None, w)
    out = dict(mesh, pos=p)
    if n is not None:
        out["normals"] = n
    return out


def morph_posed(mesh, mo, w, rig, palette, normals=True):
    """Morph, then skin: mesh_skin_ref.pose with the morph's output as the bind pose."""
    mm = morphed(mesh, mo, w, normals)
    use = normals and "normals" in mo and "normals" in mesh
    p, n = MS.pose(mm["pos"], mm["normals"] if use else None, rig["joints"], rig["weights"], palette)
    out = dict(mesh, pos=p)
    if n is not None:
        out["normals"] = n
    return out


# ---- the scene: mesh_light_ref.lit_sphere3d() under four targets ----------------------
def sphere_morph(mesh=None):
    """Bulge (the equator swells along its normals), squash (y shrinks, x and z
    spread), shear (x follows y) and a twist-like slide of the upper half, each
    with the normal deltas of the same displacement field (not renormalised)."""
    mesh = ML.lit_sphere3d() if mesh is None else mesh
    p, n = np.asarray(mesh["pos"]), np.asarray(mesh["normals"])
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    r = np.abs(p).max()
    band = np.exp(-(y / (0.45 * r)) ** 2)
    bulge = 0.45 * r * band[:, None] * n
    squash = np.stack([0.35 * x, -0.5 * y, 0.35 * z], axis=1)
    shear = np.stack([0.6 * y, np.zeros_like(y), 0.15 * y], axis=1)
    up = np.clip(y / r, 0.0, 1.0)
    slide = np.stack([0.5 * r * up * up, 0.2 * r * up, -0.3 * z * up], axis=1)
    dP = np.stack([bulge, squash, shear, slide])
    dN = np.stack([0.3 * band[:, None] * np.stack([n[:, 0], -n[:, 1], n[:, 2]], axis=1),
                   np.stack([-0.25 * n[:, 0], 0.5 * n[:, 1], -0.25 * n[:, 2]], axis=1),
                   np.stack([np.zeros_like(y), -0.6 * n[:, 0] - 0.15 * n[:, 2], np.zeros_like(y)], axis=1),
                   np.stack([-0.4 * up * n[:, 1], 0.3 * up * n[:, 0], 0.2 * up * n[:, 2]], axis=1)])
    return dict(pos=np.ascontiguousarray(p), normals=np.ascontiguousarray(n), dP=np.ascontiguousarray(dP),
                dN=np.ascontiguousarray(dN))


SCENE_WEIGHTS = (np.array([0.0, 0.0, 0.0, 0.0]),          # 0: the base
                 np.array([1.0, 0.0, 0.6, 0.35]),         # 1: three active targets, one of them at weight 1
                 np.array([-0.0, 0.8, -0.5, 0.0]))        # 2: two, and a negative zero


def scene_weights(which=1):
    return SCENE_WEIGHTS[which].copy()


# ---- random morphs -------------------------------------------------------------------------
def random_morph(mesh, T, seed, normals=True):
    """Random deltas in [-0.2, 0.2] over `mesh`'s positions (and normals)."""
    g = scenes.rng(seed + 71)
    nv = np.asarray(mesh["pos"]).shape[0]
    mo = dict(pos=np.ascontiguousarray(mesh["pos"], dtype=np.float64), dP=g.uniform(-0.2, 0.2, size=(T, nv, 3)))
    if normals and "normals" in mesh:
        mo["normals"] = np.ascontiguousarray(mesh["normals"], dtype=np.float64)
        mo["dN"] = g.uniform(-0.2, 0.2, size=(T, nv, 3))
    return mo


def scattered_weights(T, active, seed):
    """(T,) with `active` non-zero entries (None: all): scattered, except that
    one active target is the first or the last index by the seed's parity."""
    g = scenes.rng(seed + 5)
    w = np.zeros(T)
    k = T if active is None else min(active, T)
    if k == 0:
        return w
    edge = 0 if seed % 2 == 0 else T - 1
    rest = [t for t in g.permutation(T).tolist() if t != edge][:k - 1]
    for t in [edge] + rest:
        w[t] = g.uniform(-1.0, 1.0) or 0.5
    return w

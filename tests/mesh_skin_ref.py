"""The numpy reference of skinned meshes (DESIGN.md §3 "Skinned meshes") and the
rigs, palettes and scenes its tests share.

pose restates the skin pass with explicit elementwise products and sums in the
specified order (no `@`, no np.dot, as mesh_ref.vertex_stage explains).  A posed
mesh is an ordinary mesh: its expected soups and frames are those of mesh_ref,
mesh_clip_ref, mesh_inst_ref and mesh_light_ref over dict(mesh, pos=..., normals=...).

A rig is a dict: joints (nv, 4) uint32, weights (nv, 4), nb; a palette is (nb, 12),
one row-major 3x4 matrix [R | t] per bone.
"""
import numpy as np

import mesh_light_ref as ML
import mesh_ref as MR
import scenes


def same_bits(a, b):
    """Bit for bit, except that any NaN equals any NaN: an x86 host and the GPU
    generate different default NaNs (sign, payload)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def pose(bind_pos, bind_nrm, joints, weights, palette):
    """(pos (nv, 3), nrm (nv, 3) or None): the bind pose under the palette,
      x_k = ((B_k[0]*px + B_k[1]*py) + B_k[2]*pz) + B_k[3];  X = ((w0*x_0 + w1*x_1) + w2*x_2) + w3*x_3
      a_k = (B_k[0]*nx + B_k[1]*ny) + B_k[2]*nz;             NX = ((w0*a_0 + w1*a_1) + w2*a_2) + w3*a_3
    all four influences evaluated, every product and sum rounded."""
    p = np.asarray(bind_pos, dtype=np.float64).reshape(-1, 3)
    nv = p.shape[0]
    J = np.asarray(joints).reshape(nv, 4).astype(np.int64)
    Wt = np.asarray(weights, dtype=np.float64).reshape(nv, 4)
    pal = np.asarray(palette, dtype=np.float64).reshape(-1, 12)
    n = None if bind_nrm is None else np.asarray(bind_nrm, dtype=np.float64).reshape(nv, 3)
    out_p, out_n = np.empty((nv, 3)), (None if n is None else np.empty((nv, 3)))
    with np.errstate(all="ignore"):
        B = [pal[J[:, k]] for k in range(4)]              # (nv, 12) each
        for r in range(3):
            t = [((B[k][:, 4 * r] * p[:, 0] + B[k][:, 4 * r + 1] * p[:, 1]) + B[k][:, 4 * r + 2] * p[:, 2])
                 + B[k][:, 4 * r + 3] for k in range(4)]
            out_p[:, r] = ((Wt[:, 0] * t[0] + Wt[:, 1] * t[1]) + Wt[:, 2] * t[2]) + Wt[:, 3] * t[3]
            if n is not None:
                a = [(B[k][:, 4 * r] * n[:, 0] + B[k][:, 4 * r + 1] * n[:, 1]) + B[k][:, 4 * r + 2] * n[:, 2]
                     for k in range(4)]
                out_n[:, r] = ((Wt[:, 0] * a[0] + Wt[:, 1] * a[1]) + Wt[:, 2] * a[2]) + Wt[:, 3] * a[3]
    return out_p, out_n


def posed(mesh, rig, palette, normals=True):
    """`mesh` (a lit mesh_ref dict) posed: what every draw after the pose reads.
    normals False: a skin without bind normals -- the mesh keeps its own."""
    p, n = pose(mesh["pos"], mesh["normals"] if normals and "normals" in mesh else None,
                rig["joints"], rig["weights"], palette)
    out = dict(mesh, pos=p)
    if n is not None:
        out["normals"] = n
    return out


# ---- palettes ---------------------------------------------------------------------
def bone(ax=0.0, ay=0.0, t=(0.0, 0.0, 0.0), pivot=(0.0, 0.0, 0.0)):
    """(12,): the rotation mesh_ref.rotation(ax, ay) about `pivot`, then the translation t."""
    R = MR.rotation(ax, ay)[:3, :3]
    pv = np.asarray(pivot, dtype=np.float64)
    return np.ascontiguousarray(np.concatenate([R, (pv - R @ pv + np.asarray(t, dtype=np.float64))[:, None]], axis=1).reshape(12))


def identity_palette(nb):
    return np.ascontiguousarray(np.tile(bone(), (nb, 1)))


def scene_palette(which=1):
    """(3, 12) for sphere_rig: bone 0 (the top) stays, bones 1 and 2 are two
    rotations plus a translation; which = 0, 1, 2: three different poses."""
    s = (0.0, 1.0, -0.7)[which]
    if which == 0:
        return np.ascontiguousarray(np.stack([bone(), bone(0.2, -0.1, (0.1, 0.0, 0.0)), bone(-0.15, 0.3, (0.0, -0.1, 0.05))]))
    return np.ascontiguousarray(np.stack([bone(),
                                          bone(0.5 * s, 0.35 * s, (0.3 * s, 0.05, -0.1 * s), pivot=(0.0, 0.4, 0.0)),
                                          bone(-0.9 * s, 0.6 * s, (0.45 * s, -0.2 * s, 0.15), pivot=(0.0, -0.3, 0.0))]))


def random_palette(nb, seed):
    """(nb, 12): random rotations, translations in [-0.3, 0.3]^3."""
    g = scenes.rng(seed + 31)
    return np.ascontiguousarray(np.stack([bone(g.uniform(-1.5, 1.5), g.uniform(-1.5, 1.5), g.uniform(-0.3, 0.3, size=3))
                                          for _ in range(nb)]))


# ---- rigs ---------------------------------------------------------------------------
def sphere_rig(mesh=None):
    """A 3-bone rig of mesh_light_ref.lit_sphere3d() (187 vertices) by height:
    the top follows bone 0 alone (one non-zero weight), the band below it blends
    bones 0 and 1 (two), the rest all three with bone 1 twice (four)."""
    mesh = ML.lit_sphere3d() if mesh is None else mesh
    y = np.asarray(mesh["pos"])[:, 1]
    nv = y.shape[0]
    joints = np.tile(np.array([0, 1, 2, 1], dtype=np.uint32), (nv, 1))
    weights = np.zeros((nv, 4))
    top, band = y > 0.55, (y <= 0.55) & (y > 0.0)
    low = ~(top | band)
    weights[top] = (1.0, 0.0, 0.0, 0.0)
    a = (0.55 - y[band]) / 0.55                               # 0 at the top of the band, 1 at y = 0
    weights[band] = np.stack([1.0 - a, a, np.zeros_like(a), np.zeros_like(a)], axis=1)
    b = np.clip(-y[low] / 1.1, 0.0, 1.0)
    weights[low] = np.stack([0.1 * (1 - b), 0.55 * (1 - b) + 0.1 * b, 0.7 * b, 0.35 * (1 - b) + 0.2 * b], axis=1)
    return dict(joints=joints, weights=np.ascontiguousarray(weights), nb=3)


def random_rig(nv, nb, seed):
    """Random joints below nb and random weights that sum to 1 within rounding;
    about a third of the vertices have trailing zero weights (their joints stay
    random: a zero-weight joint is read all the same)."""
    g = scenes.rng(seed + 13)
    joints = g.integers(0, nb, size=(nv, 4)).astype(np.uint32)
    w = g.uniform(0.05, 1.0, size=(nv, 4))
    live = g.integers(1, 5, size=nv)
    live[g.uniform(size=nv) > 0.35] = 4
    w[np.arange(4)[None, :] >= live[:, None]] = 0.0
    return dict(joints=joints, weights=np.ascontiguousarray(w / w.sum(axis=1)[:, None]), nb=nb)

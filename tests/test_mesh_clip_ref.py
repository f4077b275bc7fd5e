"""CPU checks of the clip stage's numpy reference (tests/mesh_clip_ref.py):
it equals a scalar Python-float loop written independently, bit for bit; its
invariants (an unclipped triangle is the vertex stage's, shared cuts are
bit-identical, t in [0, 1], opaque stays opaque, the cull modes partition the
soup); and the scenes the GPU tests use contain every class of triangle."""
import struct

import numpy as np
import pytest

import mesh_clip_ref as CR
import mesh_ref as MR
import scenes

W, H = 130, 97
NAN = float("nan")


# ---- the independent restatement: one triangle at a time, Python floats --------
def _scalar_soup(mesh, M, w_near, cull):
    M = [float(v) for v in (MR.IDENT16 if M is None else np.asarray(M).reshape(16))]
    pos = np.asarray(mesh["pos"], dtype=np.float64).tolist()
    clip = []
    for px, py, pz in pos:
        clip.append(tuple(((M[4 * r] * px + M[4 * r + 1] * py) + M[4 * r + 2] * pz) + M[4 * r + 3] for r in range(4)))
    if "uv" in mesh:
        vattr, kind = np.asarray(mesh["uv"], dtype=np.float64).tolist(), "tex"
    else:
        vattr, kind = np.asarray(mesh["colors"], dtype=np.float64).tolist(), ("gouraud" if mesh["gouraud"] else "flat")

    def div(a, b):   # IEEE division (Python raises on a zero divisor)
        return float(np.float64(a) / np.float64(b))

    def corner(i):
        cx, cy, cz, cw = clip[i]
        p = (div(cx, cw), div(cy, cw), div(cz, cw)) if cw > 0 else (NAN, NAN, NAN)
        return p + (list(vattr[i]),)

    def cut(ia, ib):
        a, b = clip[ia], clip[ib]
        t = div(a[3] - w_near, a[3] - b[3])
        q = [a[c] + (b[c] - a[c]) * t for c in range(3)]
        A = [va + (vb - va) * t for va, vb in zip(vattr[ia], vattr[ib])]
        return (div(q[0], w_near), div(q[1], w_near), div(q[2], w_near), A)

    xy, z, attr, counts = [], [], [], []
    with np.errstate(all="ignore"):
        for tri in np.asarray(mesh["idx"]).reshape(-1, 3).tolist():
            ins = [(clip[i][3] >= w_near) if w_near > 0 else True for i in tri]
            poly = []
            for k in range(3):
                j = (k + 1) % 3
                if ins[k]:
                    poly.append(corner(tri[k]))
                if ins[k] != ins[j]:
                    poly.append(cut(tri[k], tri[j]) if ins[k] else cut(tri[j], tri[k]))
            out = []
            if len(poly) >= 3:
                out.append((poly[0], poly[1], poly[2]))
            if len(poly) == 4:
                out.append((poly[0], poly[2], poly[3]))
            made = 0
            for p0, p1, p2 in out:
                a2 = (p1[0] - p0[0]) * (p2[1] - p0[1]) - (p2[0] - p0[0]) * (p1[1] - p0[1])
                if (cull == 1 and a2 > 0) or (cull == 2 and a2 < 0):
                    continue
                xy.append([p0[0], p0[1], p1[0], p1[1], p2[0], p2[1]])
                z.append([p0[2], p1[2], p2[2]])
                attr.append(list(vattr[tri[0]]) if kind == "flat" else p0[3] + p1[3] + p2[3])
                made += 1
            counts.append(made)
    stride = {"tex": 6, "gouraud": 12, "flat": 4}[kind]
    return (np.array(xy, dtype=np.float64).reshape(-1, 6), np.array(z, dtype=np.float64).reshape(-1, 3),
            np.array(attr, dtype=np.float64).reshape(-1, stride), np.array(counts, dtype=np.int64))


def _small_mesh(kind, seed):
    mesh = MR.random_mesh(40, 150, seed)
    if kind == "flat":
        mesh["gouraud"] = False
    elif kind == "tex":
        del mesh["colors"], mesh["gouraud"]
        mesh["uv"] = scenes.rng(seed + 1).uniform(-3, 40, size=(40, 2))
    return mesh


@pytest.mark.parametrize("kind", ["gouraud", "flat", "tex"])
def test_reference_equals_the_scalar_loop(kind):
    mats = {"perspective": MR.perspective(W, H, d=0.9), "affine": MR.affine(W, H), "identity": None}
    clipped = 0
    for seed, (name, M) in enumerate(mats.items()):
        mesh = _small_mesh(kind, 11 + seed)
        for w_near in (0.0, 0.05, 0.5):
            for cull in (0, 1, 2):
                got = CR.clip_soup(mesh, M, w_near, cull)
                want = _scalar_soup(mesh, M, w_near, cull)
                for g, w, what in zip(got, want, ("xy", "z", "attr", "counts")):
                    assert g.shape == w.shape, (name, w_near, cull, what, g.shape, w.shape)
                    assert scenes.bits_equal(g, w) if what != "counts" else np.array_equal(g, w), (name, w_near, cull, what)
                if name == "perspective" and w_near > 0 and cull == 0:
                    clipped += int(((got[3] == 2).sum() > 0) and (got[3] == 0).sum() > 0)
    assert clipped == 2   # the perspective case cuts quads and drops triangles at both planes


def _sphere_behind():
    return MR.sphere3d(), MR.behind_eye(W, H)


def test_unclipped_triangles_are_the_vertex_stage_bitwise():
    mesh, M = _sphere_behind()
    info = {}
    xy, z, attr, counts = CR.clip_soup(mesh, M, 0.05, 0, info)
    wxy, wz, wattr = MR.expand(mesh, M)
    whole = info["inside"] == 3
    assert whole.sum() > 100 and (counts[whole] == 1).all()
    first = np.cumsum(counts) - counts           # offset of each source triangle's first output
    rows = first[whole]
    assert scenes.bits_equal(xy[rows], wxy[whole]) and scenes.bits_equal(z[rows], wz[whole])
    assert scenes.bits_equal(attr[rows], wattr[whole])
    # and with the plane off the whole soup is expand's (NaN where a vertex is behind the eye)
    xy0, z0, attr0, counts0 = CR.clip_soup(mesh, M, 0.0, 0)
    assert (counts0 == 1).all() and np.isnan(wxy).any()
    assert np.array_equal(xy0.view(np.uint64), wxy.view(np.uint64)) and np.array_equal(z0.view(np.uint64), wz.view(np.uint64))
    assert scenes.bits_equal(attr0, wattr)


@pytest.mark.parametrize("scene", ["sphere", "random"])
def test_output_count_by_class(scene):
    mesh, M, w = (_sphere_behind() + (0.05,)) if scene == "sphere" else \
        (MR.random_mesh(1000, 3000, 5), MR.perspective(W, H, d=0.9), 0.25)
    xy, z, attr, counts = CR.clip_soup(mesh, M, w, 0)
    m = CR.inside_counts(mesh, M, w)
    c = [int((m == k).sum()) for k in range(4)]
    assert xy.shape[0] == counts.sum() == c[1] + 2 * c[2] + c[3]
    assert np.array_equal(counts, np.array([0, 1, 2, 1])[m])


def test_shared_cut_vertices_are_bit_identical():
    mesh, M = _sphere_behind()
    info = {}
    CR.clip_soup(mesh, M, 0.05, 0, info)
    idx = mesh["idx"].astype(np.int64)
    seen = {}
    for t in np.flatnonzero((info["inside"] == 1) | (info["inside"] == 2)):
        for s in range(int(info["fill"][t])):
            a, b = int(info["sa"][t, s]), int(info["sb"][t, s])
            if a != b:
                key = (int(idx[t, a]), int(idx[t, b]))
                bits = struct.pack("<3d", info["x"][t, s], info["y"][t, s], info["z"][t, s])
                seen.setdefault(key, []).append((int(t), bits))
    shared = [v for v in seen.values() if len({t for t, _ in v}) >= 2]
    assert len(shared) >= 20, len(shared)
    # both directions of the edge occur among them (k -> k + 1 in one triangle, k + 1 -> k in its neighbour)
    for v in seen.values():
        assert len({bits for _, bits in v}) == 1
    # an edge is never cut from both ends
    assert not any((b, a) in seen for a, b in seen)


@pytest.mark.parametrize("w_near", [0.05, 0.5])
def test_cut_parameter_lies_in_the_unit_interval(w_near):
    info = {}
    CR.clip_soup(MR.random_mesh(1000, 3000, 5), MR.perspective(W, H, d=0.9), w_near, 0, info)
    t = info["t"]
    assert t.size > 500 and np.isfinite(t).all() and (t >= 0).all() and (t <= 1).all()


def test_opaque_alpha_stays_exactly_one():
    mesh, M = _sphere_behind()
    assert (mesh["colors"][:, 3] == 1).all()
    xy, z, attr, counts = CR.clip_soup(mesh, M, 0.05, 0)
    assert (counts == 2).any() and (attr[:, 3::4] == 1.0).all()
    # (a translucent mesh's alpha is interpolated)
    blended = MR.sphere3d(alpha=(0.2, 0.9))
    a = CR.clip_soup(blended, M, 0.05, 0)[2][:, 3::4]
    assert (a != 1.0).all() and a.min() >= 0.2 and a.max() <= 0.9


@pytest.mark.parametrize("w_near", [0.0, 0.05])
def test_cull_modes_partition_the_soup(w_near):
    # (seen from inside, the sphere's triangles all face one way: the clipped case takes the random mesh)
    mesh, M = (MR.sphere3d(), MR.perspective(W, H)) if w_near == 0 else \
        (MR.random_mesh(1000, 3000, 5), MR.perspective(W, H, d=0.9))
    full = CR.clip_soup(mesh, M, w_near, 0)
    a2 = CR.area2(full[0])
    with np.errstate(invalid="ignore"):
        pos, neg = a2 > 0, a2 < 0
    rest = ~pos & ~neg                         # zero or NaN: never culled
    assert pos.sum() > 50 and neg.sum() > 50 and rest.sum() > 0
    assert pos.sum() + neg.sum() + rest.sum() == full[0].shape[0]
    for cull, dropped in ((1, pos), (2, neg)):
        got = CR.clip_soup(mesh, M, w_near, cull)
        for g, f in zip(got[:3], full[:3]):
            assert g.shape[0] == (~dropped).sum()
            assert np.array_equal(g.view(np.uint64), f[~dropped].view(np.uint64))
        assert got[3].sum() == (~dropped).sum() and (got[3] <= full[3]).all()


def test_cull_without_a_plane_keeps_triangles_behind_the_eye():
    """With w_near == 0 the cull sees the vertex stage's NaN: never culled."""
    mesh, M = _sphere_behind()
    wxy = MR.expand(mesh, M)[0]
    nan_tris = np.isnan(wxy).any(axis=1)
    assert nan_tris.sum() > 50
    for cull in (1, 2):
        xy, _, _, counts = CR.clip_soup(mesh, M, 0.0, cull)
        assert (counts[nan_tris] == 1).all() and np.isnan(xy).any(axis=1).sum() == nan_tris.sum()


# ---- the scenes of tests/test_mesh_clip_gpu.py cover every class ----------------
def test_sphere_behind_the_eye_classes():
    mesh, M = _sphere_behind()
    m = CR.inside_counts(mesh, M, 0.05)
    assert [int((m == k).sum()) for k in range(4)] == [52, 22, 28, 218]


def test_random_mesh_classes():
    m = CR.inside_counts(MR.random_mesh(1000, 3000, 5), MR.perspective(W, H, d=0.9), 0.25)
    assert [int((m == k).sum()) for k in range(4)] == [9, 216, 1069, 1706]


def test_sphere_under_the_perspective_matrix_areas():
    mesh, M = MR.sphere3d(), MR.perspective(W, H)
    assert (CR.inside_counts(mesh, M, 0.05) == 3).all()
    a2 = CR.area2(CR.clip_soup(mesh, M, 0.05, 0)[0])
    assert [int((a2 > 0).sum()), int((a2 < 0).sum()), int((a2 == 0).sum())] == [184, 109, 27]
    assert np.array_equal(a2, CR.area2(MR.expand(mesh, M)[0]))

"""The perspective-correct texture reference (tests/persp_ref.py) checked on
the CPU: its numpy arithmetic against a scalar Python-float loop, against the
analytic inverse homography of a receding quad, against textured_ref when every
q is 1, the mesh front end's q, and that the scenes of the GPU tests
(tests/test_persp_gpu.py) tell perspective-correct from affine sampling."""
import functools

import numpy as np
import pytest

import mesh_clip_ref as MC
import mesh_ref as MR
import persp_ref as P
import scenes
import textured_ref as T

W, H = P.W, P.H


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 1. numpy == scalar loop ------------------------------------------------------
def _scalar_uv(xy, uv, q, m, px, py):
    """The specification, one Python float operation at a time."""
    sx = [m[0] * xy[2 * k] + m[2] * xy[2 * k + 1] + m[4] for k in range(3)]
    sy = [m[1] * xy[2 * k] + m[3] * xy[2 * k + 1] + m[5] for k in range(3)]
    e1x, e1y, e2x, e2y = sx[1] - sx[0], sy[1] - sy[0], sx[2] - sx[0], sy[2] - sy[0]
    den = e1x * e2y - e2x * e1y
    inv = 1.0 / den
    dx, dy = px - sx[0], py - sy[0]
    w1 = (dx * e2y - e2x * dy) * inv
    w2 = (e1x * dy - dx * e1y) * inv
    a = [uv[2 * k] * q[k] for k in range(3)]
    b = [uv[2 * k + 1] * q[k] for k in range(3)]
    U = a[0] + (a[1] - a[0]) * w1 + (a[2] - a[0]) * w2
    V = b[0] + (b[1] - b[0]) * w1 + (b[2] - b[0]) * w2
    Q = q[0] + (q[1] - q[0]) * w1 + (q[2] - q[0]) * w2
    r = 1.0 / Q
    return U * r, V * r


def test_numpy_restatement_equals_a_scalar_loop():
    b = P.soup(W, H, 50, 3, T.texture_rgb(), spread=40.0, m=T.XFORM)
    g = scenes.rng(17)
    checked = 0
    for t in range(50):
        px = np.floor(g.uniform(0, W, 40))
        py = np.floor(g.uniform(0, H, 40))
        u, v, _, _ = P.fragment_uv(b["xy"][t], b["uv"][t], b["q"][t], b["m"], px, py)
        for i in range(40):
            su, sv = _scalar_uv([float(c) for c in b["xy"][t]], [float(c) for c in b["uv"][t]],
                                [float(c) for c in b["q"][t]], [float(c) for c in b["m"]], float(px[i]), float(py[i]))
            assert _bits([u[i], v[i]], [su, sv]), (t, i)
            checked += 1
    assert checked == 2000


def test_oracle_payload_equals_the_numpy_restatement():
    """expected_payload's U, V, Q come from the oracle's Gouraud interpolation:
    its texels equal those of fragment_uv at every covered pixel."""
    b = P.soup(W, H, 50, 3, T.texture_rgb(), spread=40.0, m=T.XFORM)
    info = {}
    P.expected_payload(W, H, False, P.BG, "nz", 0, [b], info)
    idx = P._oracle_pass(W, H, "nz", 0, [b], True)[0][..., 0]
    ys, xs = np.nonzero(info["covered"])
    assert ys.size > 0.5 * W * H
    for t in np.unique(idx[ys, xs]).astype(int):
        sel = idx[ys, xs] == t
        u, v, _, _ = P.fragment_uv(b["xy"][t], b["uv"][t], b["q"][t], b["m"], xs[sel], ys[sel])
        assert np.array_equal(T.sample(b["tex"], u, v)[1], info["tids"][ys[sel], xs[sel]]), t


# ---- 2. the analytic inverse homography ---------------------------------------------
TW_, TH_ = 37, 23
QUAD_POS = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [-1.0, 1.0, 0.0]])
QUAD_UV = np.array([[0.0, 0.0], [TW_, 0.0], [TW_, TH_], [0.0, TH_]])
QUAD_IDX = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32)
# cw = d + s X + t Y over the quad [-1, 1]^2 (z = 0); screen = centre + A (X, -Y) / cw; z = 0.5.
# Rows: cx = A X + (W/2) cw, cy = -A Y + (H/2) cw, cz = 0.5 cw, cw.
QUADS = {   # cw ratio: the matrix
    1.7: np.array([139.0, 13.0, 0.0, 195.0, 29.1, -90.3, 0.0, 145.5, 0.3, 0.1, 0.0, 1.5, 0.6, 0.2, 0.0, 3.0]),
    6.0: np.array([112.0, 13.0, 0.0, 91.0, 38.8, -50.3, 0.0, 67.9, 0.4, 0.1, 0.0, 0.7, 0.8, 0.2, 0.0, 1.4]),
    38.0: np.array([88.75, 12.935, 0.0, 65.0, 36.375, -30.3485, 0.0, 48.5, 0.375, 0.0995, 0.0, 0.5, 0.75, 0.199, 0.0, 1.0]),
}


def _quad_mesh():
    return dict(pos=QUAD_POS, idx=QUAD_IDX, uv=QUAD_UV)


@pytest.mark.parametrize("ratio", sorted(QUADS))
def test_restatement_equals_the_inverse_homography(ratio):
    """A wrong formula is off by whole texels (the affine one by up to 5, 16 and
    26 on these quads); f64 rounding leaves 6e-14, 6e-14 and 5e-12 texel.
    Tolerance 1e-9 texel."""
    M = QUADS[ratio]
    cw = MC.clip_coords(QUAD_POS, M)[3]
    assert cw.min() > 0 and abs(cw.max() / cw.min() - ratio) < 0.03 * ratio, cw
    xy, z, uv, q = P.expand_q(_quad_mesh(), M)
    assert _bits(q, 1.0 / cw[QUAD_IDX.astype(np.int64)])
    Mm = M.reshape(4, 4)
    Hm = Mm[np.ix_([0, 1, 3], [0, 1, 3])]          # (X, Y, 1) -> (cx, cy, cw)
    Hi = np.linalg.inv(Hm)
    ys, xs = np.mgrid[0:H, 0:W]
    px, py = xs.ravel().astype(np.float64), ys.ravel().astype(np.float64)
    back = Hi @ np.stack([px, py, np.ones_like(px)])
    X, Y = back[0] / back[2], back[1] / back[2]
    ua, va = (X + 1) * 0.5 * TW_, (Y + 1) * 0.5 * TH_
    worst, wrong_affine, covered = 0.0, 0, 0
    for t in range(2):
        u, v, w1, w2 = P.fragment_uv(xy[t], uv[t], q[t], T.IDENT, px, py)
        au, av, _, _ = P.fragment_uv(xy[t], uv[t], np.ones(3), T.IDENT, px, py)
        ins = (w1 >= 0) & (w2 >= 0) & (w1 + w2 <= 1)
        assert ins.sum() > 300
        worst = max(worst, float(np.abs(u - ua)[ins].max()), float(np.abs(v - va)[ins].max()))
        covered += int(ins.sum())
        wrong_affine += int(((np.floor(au) != np.floor(ua)) | (np.floor(av) != np.floor(va)))[ins].sum())
    assert worst < 1e-9, worst
    assert wrong_affine >= 0.9 * covered, (wrong_affine, covered)   # (the affine map is visibly wrong here)


# ---- 3. the GPU scenes discriminate ---------------------------------------------------
@pytest.mark.parametrize("mode", T.MODES)
def test_soup_scenes_discriminate(mode):
    bs = P.soup_batches("opaque")
    share, cov = P.affine_share(W, H, mode, P.CLEAR, bs)
    assert share >= 0.5 and cov >= 0.5, (share, cov)
    for kind in P.KINDS:
        assert all(P.q_spread(b["q"]) >= 1.5 for b in P.soup_batches(kind))


@pytest.mark.parametrize("name", ["perspective", "behind_eye"])
def test_mesh_scenes_discriminate(name):
    tex = P.mesh_texture()
    for near, cull in P.MESH_STATES:
        b = P.mesh_batch(P.mesh_scene(), P.mesh_matrix(name), tex, near, cull)
        share, cov = P.affine_share(W, H, "zw", P.FAR, [b])
        if (name, near, cull) in P.MESH_EMPTY:
            assert cov == 0.0
            continue
        assert share >= 0.5 and cov >= 0.3, (name, near, cull, share, cov)
        # q spans a factor of 1.5 within some triangle the rasters keep
        assert P.q_spread(b["q"][MR.kept(b["xy"], b["m"])]) >= 1.5, (name, near, cull)


# ---- 4. q == 1: textured_ref's frames ---------------------------------------------------
@pytest.mark.parametrize("mode", T.MODES)
def test_unit_q_equals_the_affine_reference(mode):
    for kind in ("opaque", "rgba_texture"):
        bs = [dict(b, q=np.ones_like(b["q"])) for b in P.soup_batches(kind)]
        fn, tfn = (P.expected_payload, T.expected_payload) if kind == "opaque" else (P.expected_loop, T.expected_loop)
        for alpha in (False, True):
            got = fn(W, H, alpha, P.BG, mode, P.CLEAR, bs)
            want = tfn(W, H, alpha, P.BG, mode, P.CLEAR, bs)
            assert scenes.bits_equal(got[0], want[0]), (kind, mode, alpha)
            if want[1] is not None:
                assert np.array_equal(got[1], want[1]), (kind, mode, alpha)


def test_both_derivations_agree_on_an_opaque_batch():
    bs = P.soup_batches("opaque")
    for mode in T.MODES:
        a = P.expected_payload(W, H, False, P.BG, mode, P.CLEAR, bs)
        b = P.expected_loop(W, H, False, P.BG, mode, P.CLEAR, bs)
        assert scenes.bits_equal(a[0], b[0]), mode
        if a[1] is not None:
            assert np.array_equal(a[1], b[1]), mode


# ---- 5. clip_soup_q ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _behind():
    return MR.behind_eye(W, H)


def test_clip_soup_q_corners_and_cuts():
    mesh = P.mesh_scene()
    M = _behind()
    info = {}
    xy, z, uv, counts = MC.clip_soup(mesh, M, P.NEAR, 0, info)
    qxy, qz, quv, q, qcounts = P.clip_soup_q(mesh, M, P.NEAR, 0)
    assert _bits(qxy, xy) and _bits(qz, z) and _bits(quv, uv) and np.array_equal(counts, qcounts)
    assert q.shape == (xy.shape[0], 3) and (counts == 2).any() and (counts == 1).any() and (counts == 0).any()
    idx = mesh["idx"].astype(np.int64)
    cw = MC.clip_coords(mesh["pos"], M)[3][idx]
    # by hand, triangle by triangle: a corner's 1 / cw, a cut's 1 / w_near
    o, cuts, corners = 0, 0, 0
    for t in range(idx.shape[0]):
        slots = [(int(info["sa"][t, s]), int(info["sb"][t, s])) for s in range(int(info["fill"][t]))]
        for half in ([0, 1, 2], [0, 2, 3])[:int(counts[t])]:
            for c, s in enumerate(half):
                a, b = slots[s]
                want = 1.0 / P.NEAR if a != b else 1.0 / float(cw[t, a])
                assert _bits([q[o, c]], [want]), (t, half, c)
                cuts += a != b
                corners += a == b
            o += 1
    assert o == xy.shape[0] and cuts > 10 and corners > 10


def test_shared_cut_vertices_are_identical():
    """Two triangles that share a cut edge get the same (x, y, z, u, v, q)."""
    mesh = P.mesh_scene()
    M = _behind()
    info = {}
    MC.clip_soup(mesh, M, P.NEAR, 0, info)
    xy, z, uv, q, counts = P.clip_soup_q(mesh, M, P.NEAR, 0)
    idx = mesh["idx"].astype(np.int64)
    # every output corner keyed by the mesh edge (or vertex) it came from
    seen, shared = {}, 0
    o = 0
    for t in range(idx.shape[0]):
        slots = [(int(info["sa"][t, s]), int(info["sb"][t, s])) for s in range(int(info["fill"][t]))]
        for half in ([0, 1, 2], [0, 2, 3])[:int(counts[t])]:
            for c, s in enumerate(half):
                a, b = slots[s]
                key = (int(idx[t, a]), int(idx[t, b]))
                val = np.array([xy[o, 2 * c], xy[o, 2 * c + 1], z[o, c], uv[o, 2 * c], uv[o, 2 * c + 1], q[o, c]])
                if key in seen and key[0] != key[1]:
                    shared += 1
                    assert _bits(seen[key], val), key
                seen[key] = val
            o += 1
    assert shared >= 5, shared


def test_clip_soup_q_state_off_is_mesh_clip_ref():
    mesh = P.mesh_scene()
    for near, cull in ((P.NEAR, 0), (P.NEAR, 1), (0.0, 2)):
        xy, z, uv, counts = MC.clip_soup(mesh, _behind(), near, cull)
        qxy, qz, quv, q, qcounts = P.clip_soup_q(mesh, _behind(), near, cull, persp=False)
        assert _bits(qxy, xy) and _bits(qz, z) and _bits(quv, uv) and np.array_equal(counts, qcounts)
        assert np.array_equal(q, np.ones((xy.shape[0], 3)))
    # and under an affine matrix q is 1 with the state on: cw == 1
    xy, z, uv, q = P.expand_q(mesh, MR.affine(W, H))
    assert np.array_equal(q, np.ones_like(q))
    qq = P.clip_soup_q(mesh, MR.affine(W, H), P.NEAR, 1)[3]
    assert qq.size and np.array_equal(qq, np.ones_like(qq))

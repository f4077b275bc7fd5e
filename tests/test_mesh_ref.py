"""CPU checks of the mesh reference (tests/mesh_ref.py): the vertex stage is
the specified expression, an indexed sphere reproduces scenes.sphere_mesh's
soup, and the scenes of tests/test_mesh_gpu.py exercise what that file says
they do -- on the reference alone, no GPU."""
import numpy as np

import mesh_ref as MR
import scenes
import textured_ref as T

W, H = 130, 97


def _loop(pos, M):
    """The vertex stage in plain Python floats."""
    out = []
    for px, py, pz in pos.tolist():
        c = [((M[4 * r] * px + M[4 * r + 1] * py) + M[4 * r + 2] * pz) + M[4 * r + 3] for r in range(4)]
        if not c[3] > 0:
            out.append((float("nan"),) * 3)
        else:
            out.append((c[0] / c[3], c[1] / c[3], c[2] / c[3]))
    return np.array(out)


def test_vertex_stage_is_the_specified_expression():
    g = scenes.rng(5)
    pos = g.uniform(-2, 2, size=(400, 3))
    for M in (MR.perspective(W, H), MR.behind_eye(W, H), MR.affine(W, H), g.uniform(-3, 3, size=16)):
        M = [float(v) for v in M]
        got = np.stack(MR.vertex_stage(pos, M), axis=-1)
        want = _loop(pos, M)
        assert scenes.bits_equal(got, want)
    assert np.isnan(want).any() and np.isfinite(want).any()   # (the random matrix: both sides of the eye plane)
    # cw == 0 and a NaN cw are behind the eye too
    M = [1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0]
    got = np.stack(MR.vertex_stage(np.array([[1.0, 2.0, 0.0], [1.0, 2.0, np.nan], [1.0, 2.0, 4.0]]), M), axis=-1)
    assert np.isnan(got[:2]).all() and got[2].tolist() == [0.25, 0.5, 1.0]


def test_affine_matrix_is_exact():
    pos = scenes.rng(6).uniform(-2, 2, size=(300, 3))
    M = MR.affine(W, H)
    assert M[12:].tolist() == [0.0, 0.0, 0.0, 1.0]
    x, y, z = MR.vertex_stage(pos, M)
    px, py, pz = pos.T
    assert scenes.bits_equal(x, ((M[0] * px + M[1] * py) + M[2] * pz) + M[3])
    assert scenes.bits_equal(y, ((M[4] * px + M[5] * py) + M[6] * pz) + M[7])
    assert scenes.bits_equal(z, ((M[8] * px + M[9] * py) + M[10] * pz) + M[11])
    # the identity leaves positions alone
    assert scenes.bits_equal(np.stack(MR.vertex_stage(pos, None), -1), pos)


def test_indexed_sphere_reproduces_the_soup():
    for rows, cols in ((7, 11), (20, 40)):
        mesh = MR.sphere_screen_mesh(W, H, rows, cols)
        assert mesh["pos"].shape[0] == (rows + 1) * (cols + 1) and mesh["idx"].max() == mesh["pos"].shape[0] - 1
        xy, z, c = scenes.sphere_mesh(W, H, rows, cols)
        gxy, gz, gc = MR.expand(mesh, None)
        assert scenes.bits_equal(gxy, xy) and scenes.bits_equal(gz, z) and scenes.bits_equal(gc, c)
        flat = dict(mesh, gouraud=False)
        assert scenes.bits_equal(MR.expand(flat, None)[2], c[:, :4])   # the provoking vertex is i0


def test_scene_conditions():
    """What tests/test_mesh_gpu.py relies on, from the reference alone."""
    mesh = MR.sphere3d()
    # the perspective and affine scenes: depths inside (0.05, 0.95) on both
    # sides of the cleared depth, most triangles kept, the frame well covered
    for M in (MR.perspective(W, H), MR.affine(W, H)):
        xy, z, _ = MR.expand(mesh, M)
        assert np.isfinite(xy).all() and z.min() > 0.05 and z.max() < 0.95
        zq = MR.CLEAR / 4294967295.0
        assert (z < zq).any() and (z > zq).any()
        assert MR.kept(xy, MR.XFORM).mean() >= 0.9   # (all but the poles' degenerate triangles)
    fb, depth = MR.oracle_frame(W, H, False, "zw", [(mesh, MR.perspective(W, H))])
    covered = depth != MR.CLEAR
    assert 0.2 < covered.mean() < 0.95, covered.mean()
    # behind the eye: between 10 % and 90 % of the triangles are dropped, and a
    # kept triangle has a coordinate beyond 1e7 (the huge-coordinate rule)
    bmesh = MR.behind_eye_mesh()
    xy, z, _ = MR.expand(bmesh, MR.behind_eye(W, H))
    keep = MR.kept(xy, MR.XFORM)
    assert 0.1 <= 1 - keep.mean() <= 0.9, keep.mean()
    assert np.isnan(xy).any()
    assert (np.abs(MR.xform(MR.XFORM, xy[keep])) > 1e7).any()
    fb, depth = MR.oracle_frame(W, H, False, "zw", [(bmesh, MR.behind_eye(W, H))], clear=0xFFFFFFFF)
    assert (depth != 0xFFFFFFFF).mean() > 0.1
    # the translucent mesh is translucent, the textured one runs past the texture
    assert (MR.sphere3d(alpha=(0.2, 0.9))["colors"][:, 3] < 1).all()
    uv = MR.sphere3d(uv_size=(37, 23))["uv"]
    assert uv[:, 0].min() < 0 and uv[:, 0].max() > 37 and uv[:, 1].min() < 0 and uv[:, 1].max() > 23
    assert T.texture_rgb().shape == (23, 37, 3)

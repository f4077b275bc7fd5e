"""CPU checks of the skinning reference (tests/mesh_skin_ref.py) and of the scene
tests/test_mesh_skin_gpu.py draws: the conditions that make those tests
discriminate -- a pose that moves the picture, posed normals that change the
lighting, a sum that depends on the order of the influences, posed triangles
that cross the near plane -- asserted on the reference and the oracle alone, so
that no GPU test can pass vacuously."""
import os
import re

import numpy as np

import mesh_clip_ref as MC
import mesh_inst_ref as MI
import mesh_light_ref as ML
import mesh_ref as MR
import mesh_skin_ref as MS
import scenes

W, H = MI.W, MI.H
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"CreateMeshSkin": 6, "DestroyMeshSkin": 1, "GetMeshSkinBoneCount": 1, "PoseMesh": 4, "PoseMeshDevice": 4,
         "GetMeshPositions": 2, "GetMeshNormals": 2}


def test_the_new_symbols_are_declared_and_in_the_abi_table():
    from libnativecpurenderer_amd import _abi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "libNativeCPURenderer.h")).read(), flags=re.S)
    for s, arity in ARITY.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % s, text)
        assert m, s
        assert len(m.group(1).split(",")) == arity, s
        assert s in _abi.HIP_LIBRARY_ABI, s
        assert len(_abi.HIP_LIBRARY_ABI[s][1]) == arity, s


def test_the_python_surface_is_there():
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    assert callable(R.MeshSkin) and callable(R.RenderContext.pose_mesh) and callable(R.RenderContext.pose_mesh_device)
    assert callable(R.Mesh.positions) and callable(R.Mesh.normals)


def _scalar_pose(p, n, J, Wt, pal):
    """One vertex, in Python floats, written from the specification."""
    B = [[float(x) for x in pal[int(J[k])]] for k in range(4)]
    w = [float(x) for x in Wt]
    px, py, pz = (float(x) for x in p)
    out = []
    for r in range(3):
        t = [((B[k][4 * r] * px + B[k][4 * r + 1] * py) + B[k][4 * r + 2] * pz) + B[k][4 * r + 3] for k in range(4)]
        out.append(((w[0] * t[0] + w[1] * t[1]) + w[2] * t[2]) + w[3] * t[3])
    if n is not None:
        nx, ny, nz = (float(x) for x in n)
        for r in range(3):
            a = [(B[k][4 * r] * nx + B[k][4 * r + 1] * ny) + B[k][4 * r + 2] * nz for k in range(4)]
            out.append(((w[0] * a[0] + w[1] * a[1]) + w[2] * a[2]) + w[3] * a[3])
    return out


def test_the_reference_equals_a_scalar_loop():
    for nv, nb, seed in ((40, 1, 1), (40, 5, 2), (33, 64, 3)):
        mesh, rig, pal = ML.random_lit_mesh(nv, 4, seed), MS.random_rig(nv, nb, seed), MS.random_palette(nb, seed)
        p, n = MS.pose(mesh["pos"], mesh["normals"], rig["joints"], rig["weights"], pal)
        want = np.array([_scalar_pose(mesh["pos"][v], mesh["normals"][v], rig["joints"][v], rig["weights"][v], pal)
                         for v in range(nv)])
        assert scenes.bits_equal(p, np.ascontiguousarray(want[:, :3])), (nv, nb)
        assert scenes.bits_equal(n, np.ascontiguousarray(want[:, 3:])), (nv, nb)
        p2, n2 = MS.pose(mesh["pos"], None, rig["joints"], rig["weights"], pal)
        assert n2 is None and scenes.bits_equal(p2, p)


def test_single_influence_identity_bones_give_the_bind_pose():
    mesh = ML.lit_sphere3d()
    nv = mesh["pos"].shape[0]
    rig = MS.random_rig(nv, 7, seed=5)
    weights = np.zeros((nv, 4))
    weights[:, 0] = 1.0
    p, n = MS.pose(mesh["pos"], mesh["normals"], rig["joints"], weights, MS.identity_palette(7))
    assert (p == mesh["pos"]).all() and (n == mesh["normals"]).all()
    # a zero weight contributes a signed zero, not nothing: -0.0 in the bind pose comes out as +0.0, still == 0
    pos = mesh["pos"].copy()
    pos[3] = (-0.0, 1.0, -2.0)
    assert (MS.pose(pos, None, rig["joints"], weights, MS.identity_palette(7))[0] == pos).all()


def test_the_rig_mixes_one_two_and_four_influences_and_pins_the_order():
    mesh, rig = ML.lit_sphere3d(), MS.sphere_rig()
    assert mesh["pos"].shape == (187, 3) and rig["nb"] == 3 and int(rig["joints"].max()) == 2
    live = (rig["weights"] != 0).sum(axis=1)
    assert {1, 2, 4} <= set(live.tolist())                       # (17, 68 and 85 vertices; 17 at b = 0 have three)
    assert np.abs(rig["weights"].sum(axis=1) - 1).max() < 1e-15
    pal = MS.scene_palette(1)
    p, n = MS.pose(mesh["pos"], mesh["normals"], rig["joints"], rig["weights"], pal)
    rp, rn = MS.pose(mesh["pos"], mesh["normals"], rig["joints"][:, ::-1], rig["weights"][:, ::-1], pal)
    assert (p.view(np.uint64) != rp.view(np.uint64)).any(axis=1).sum() >= 1
    assert (n.view(np.uint64) != rn.view(np.uint64)).any(axis=1).sum() >= 1
    assert np.abs(p - rp).max() < 1e-15 and np.abs(n - rn).max() < 1e-15
    # rigid bones and weights that sum to 1 keep blended normals near unit length, not at it: nothing renormalises
    assert np.abs((n * n).sum(axis=1) - 1).max() > 1e-3
    # posing starts from the bind pose: the three scene poses differ pairwise
    poses = [MS.pose(mesh["pos"], None, rig["joints"], rig["weights"], MS.scene_palette(k))[0] for k in range(3)]
    for a in range(3):
        for b in range(a + 1, 3):
            assert (poses[a] != poses[b]).any(axis=1).sum() > 100


def test_the_posed_frame_differs_from_the_bind_pose_frame():
    mesh, rig, M = ML.lit_sphere3d(), MS.sphere_rig(), MR.perspective(W, H)
    bind = MR.oracle_frame(W, H, False, "zw", [(mesh, M)])
    frames = [bind]
    for k in (0, 1, 2):
        f = MR.oracle_frame(W, H, False, "zw", [(MS.posed(mesh, rig, MS.scene_palette(k)), M)])
        for other in frames:
            assert (f[0].view(np.uint64) != other[0].view(np.uint64)).any(axis=-1).sum() > 1000, k
        frames.append(f)


def test_the_posed_lit_frame_differs_from_the_one_lit_with_bind_normals():
    mesh, rig, M = ML.lit_sphere3d(), MS.sphere_rig(), MR.perspective(W, H)
    pm = MS.posed(mesh, rig, MS.scene_palette(1))
    lit = MR.oracle_frame(W, H, False, "zw", [(ML.lit_mesh(pm, None, ML.AMBIENT, ML.LIGHTS), M)])
    stale = MR.oracle_frame(W, H, False, "zw", [(ML.lit_mesh(dict(pm, normals=mesh["normals"]), None, ML.AMBIENT, ML.LIGHTS), M)])
    assert (lit[0].view(np.uint64) != stale[0].view(np.uint64)).any(axis=-1).sum() > 1000
    assert np.array_equal(lit[1], stale[1])                       # the same positions: the same depth
    assert not scenes.bits_equal(MS.posed(mesh, rig, MS.scene_palette(1), normals=False)["normals"], pm["normals"])


def test_the_clip_scene_cuts_posed_triangles():
    mesh, rig, M = ML.lit_sphere3d(), MS.sphere_rig(), MR.behind_eye(W, H)
    pm = MS.posed(mesh, rig, MS.scene_palette(1))
    info, bind_info = {}, {}
    MC.clip_soup(pm, M, MI.NEAR, 0, info=info)
    MC.clip_soup(mesh, M, MI.NEAR, 0, info=bind_info)
    cut = (info["inside"] == 1) | (info["inside"] == 2)
    assert cut.sum() >= 10 and (info["inside"] == 0).sum() >= 1 and (info["inside"] == 3).sum() >= 1
    assert not np.array_equal(info["inside"], bind_info["inside"])      # the pose moved triangles across the plane
    # ... and triangles whose vertices were moved by the pose are among the cut ones
    moved = (pm["pos"] != mesh["pos"]).any(axis=1)[mesh["idx"].astype(np.int64)].any(axis=1)
    assert (cut & moved).sum() >= 10


def test_the_nan_rule_of_the_comparison():
    a = np.array([1.0, np.nan, -0.0])
    b = a.copy()
    b[1] = -np.nan
    assert MS.same_bits(a, b) and not scenes.bits_equal(a, b)
    assert not MS.same_bits(a, np.array([1.0, np.nan, 0.0])) and not MS.same_bits(a, np.array([1.0, 2.0, -0.0]))

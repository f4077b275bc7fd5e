"""CPU checks of the morph reference (tests/mesh_morph_ref.py) and of the scene
tests/test_mesh_morph_gpu.py draws: the conditions that make those tests
discriminate -- the skip of zero weights, the two identities of the fused call,
a morph that moves the picture -- asserted on the reference and the oracle
alone, and the new symbols in the header, the ABI table and the built library."""
import os
import re

import numpy as np

import mesh_inst_ref as MI
import mesh_light_ref as ML
import mesh_morph_ref as MM
import mesh_ref as MR
import mesh_skin_ref as MS
import scenes

W, H = MI.W, MI.H
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"CreateMeshMorph": 6, "DestroyMeshMorph": 1, "GetMeshMorphTargetCount": 1, "MorphMesh": 4,
         "MorphMeshDevice": 4, "PoseMeshMorphed": 6, "PoseMeshMorphedDevice": 6}


def test_the_new_symbols_are_declared_exported_and_in_the_abi_table():
    from libnativecpurenderer_amd import _abi, _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "libNativeCPURenderer.h")).read(), flags=re.S)
    lib = _lib.load()
    assert len(ARITY) == 7
    for s, arity in ARITY.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % s, text)
        assert m, s
        assert len(m.group(1).split(",")) == arity, s
        assert s in _abi.HIP_LIBRARY_ABI and s in _abi.DEVICE_ABI, s
        assert len(_abi.HIP_LIBRARY_ABI[s][1]) == arity, s
        assert hasattr(lib, s), s


def test_the_python_surface_is_there():
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    assert callable(R.MeshMorph)
    for name in ("morph_mesh", "morph_mesh_device", "pose_mesh_morphed", "pose_mesh_morphed_device"):
        assert callable(getattr(R.RenderContext, name)), name
    assert isinstance(R.MeshMorph.target_count, property)


def _scalar_morph(p, dP, w):
    """One vertex's three components, in Python floats, written from the specification."""
    out = []
    for c in range(3):
        X = float(p[c])
        for t in range(len(w)):
            if float(w[t]) == 0.0:
                continue
            X = X + float(w[t]) * float(dP[t][c])
        out.append(X)
    return out


def test_the_reference_equals_a_scalar_loop():
    for nv, T, active, seed in ((40, 1, None, 1), (33, 5, 3, 2), (17, 33, 9, 3), (9, 6, 0, 4)):
        mesh = ML.random_lit_mesh(nv, 4, seed)
        mo, w = MM.random_morph(mesh, T, seed), MM.scattered_weights(T, active, seed)
        assert (w != 0).sum() == (T if active is None else active)
        p, n = MM.morph(mo["pos"], mo["normals"], mo["dP"], mo["dN"], w)
        want_p = np.array([_scalar_morph(mo["pos"][v], mo["dP"][:, v], w) for v in range(nv)])
        want_n = np.array([_scalar_morph(mo["normals"][v], mo["dN"][:, v], w) for v in range(nv)])
        assert scenes.bits_equal(p, want_p) and scenes.bits_equal(n, want_n), (nv, T)
        p2, n2 = MM.morph(mo["pos"], None, mo["dP"], None, w)
        assert n2 is None and scenes.bits_equal(p2, p)
    # the order of the sum is pinned: reversing the targets changes bits somewhere
    mesh = ML.lit_sphere3d()
    mo, w = MM.random_morph(mesh, 5, 9), MM.scattered_weights(5, None, 9)
    a = MM.morph(mo["pos"], None, mo["dP"], None, w)[0]
    b = MM.morph(mo["pos"], None, mo["dP"][::-1], None, w[::-1])[0]
    assert (a.view(np.uint64) != b.view(np.uint64)).any() and np.abs(a - b).max() < 1e-14


def test_zero_weights_return_the_base_bits_and_skip_non_finite_deltas():
    mesh = ML.lit_sphere3d()
    mo = MM.random_morph(mesh, 4, 3)
    mo["pos"][3] = (-0.0, 1.0, -2.0)
    mo["normals"][5, 2] = -0.0
    for zero in (0.0, -0.0):
        p, n = MM.morph(mo["pos"], mo["normals"], mo["dP"], mo["dN"], np.full(4, zero))
        assert scenes.bits_equal(p, mo["pos"]) and scenes.bits_equal(n, mo["normals"])
        assert np.signbit(p[3, 0]) and np.signbit(n[5, 2])
    # without the skip -0.0 + 0.0 * d would be +0.0, and 0 * inf NaN
    bad = dict(mo, dP=mo["dP"].copy(), dN=mo["dN"].copy())
    bad["dP"][1, 10] = (np.nan, np.inf, -np.inf)
    bad["dN"][2, 11] = np.nan
    for zero in (0.0, -0.0):
        w = np.array([0.5, zero, zero, -0.25])
        p, n = MM.morph(bad["pos"], bad["normals"], bad["dP"], bad["dN"], w)
        assert np.isfinite(p).all() and np.isfinite(n).all()
        q, m = MM.morph(mo["pos"], mo["normals"], mo["dP"], mo["dN"], w)
        assert scenes.bits_equal(p, q) and scenes.bits_equal(n, m)
    # a NaN weight is not zero: its target is applied, and everything becomes NaN
    p, _ = MM.morph(mo["pos"], None, mo["dP"], None, np.array([0.0, np.nan, 0.0, 0.0]))
    assert np.isnan(p).all()


def test_the_two_identities_hold_in_numpy():
    mesh, rig = ML.lit_sphere3d(), MS.sphere_rig()
    mo, pal = MM.sphere_morph(mesh), MS.scene_palette(1)
    # I1: morph, read back, a skin with that bind pose, pose
    w = MM.scene_weights(1)
    fused = MM.morph_posed(mesh, mo, w, rig, pal)
    mp, mn = MM.morph(mo["pos"], mo["normals"], mo["dP"], mo["dN"], w)
    p, n = MS.pose(mp, mn, rig["joints"], rig["weights"], pal)
    assert scenes.bits_equal(fused["pos"], p) and scenes.bits_equal(fused["normals"], n)
    assert not scenes.bits_equal(p, MS.posed(mesh, rig, pal)["pos"])
    # I2: all weights zero == pose_mesh with the morph's base as the bind pose
    zero = MM.morph_posed(mesh, mo, MM.scene_weights(0), rig, pal)
    plain = MS.posed(dict(mesh, pos=mo["pos"], normals=mo["normals"]), rig, pal)
    assert scenes.bits_equal(zero["pos"], plain["pos"]) and scenes.bits_equal(zero["normals"], plain["normals"])


def test_the_scene_weights_and_the_morphed_frame():
    ws = [MM.scene_weights(k) for k in range(3)]
    assert not ws[0].any() and np.signbit(ws[2][0])
    assert (ws[1] == 1.0).any() and (ws[1] != 0).sum() >= 3 and (ws[2] != 0).sum() >= 2
    mesh, M = ML.lit_sphere3d(), MR.perspective(W, H)
    mo = MM.sphere_morph(mesh)
    assert mo["dP"].shape == (4, 187, 3) and mo["dN"].shape == (4, 187, 3)
    base = MR.oracle_frame(W, H, False, "zw", [(mesh, M)])
    background = base[0][0, 0]
    covered = (base[0] != background).any(axis=-1)
    frames = [base]
    for k in (1, 2):
        f = MR.oracle_frame(W, H, False, "zw", [(MM.morphed(mesh, mo, ws[k]), M)])
        for other in frames:
            changed = (f[0].view(np.uint64) != other[0].view(np.uint64)).any(axis=-1)
            assert changed.sum() >= covered.sum() / 4, (k, int(changed.sum()), int(covered.sum()))
        frames.append(f)
    # the morphed normals change the lighting at unchanged positions
    mm = MM.morphed(mesh, mo, ws[1])
    lit = MR.oracle_frame(W, H, False, "zw", [(ML.lit_mesh(mm, None, ML.AMBIENT, ML.LIGHTS), M)])
    stale = MR.oracle_frame(W, H, False, "zw", [(ML.lit_mesh(dict(mm, normals=mesh["normals"]), None, ML.AMBIENT, ML.LIGHTS), M)])
    assert (lit[0].view(np.uint64) != stale[0].view(np.uint64)).any(axis=-1).sum() > 1000
    assert np.array_equal(lit[1], stale[1])


def test_scattered_weights_cover_first_only_and_last_only():
    for T in (1, 2, 5, 33):
        for active in (0, 1, 3, 4, 5, 8, 9, None):
            for seed in (0, 1):
                w = MM.scattered_weights(T, active, seed)
                assert (w != 0).sum() == (T if active is None else min(active, T))
    assert MM.scattered_weights(33, 1, 0)[0] != 0 and MM.scattered_weights(33, 1, 1)[32] != 0

"""CPU checks of the instanced-draw reference (tests/mesh_inst_ref.py) and of
the scene tests/test_mesh_instanced_gpu.py draws: the conditions that make
those frame tests discriminate -- overlapping instances, an order-dependent
blend, an instance behind the eye, one off screen, one that ties every depth,
a near plane that cuts some instances and spares others -- asserted on the
oracle alone, so that no GPU test can pass vacuously."""
import os
import re

import numpy as np

import mesh_clip_ref as MC
import mesh_inst_ref as MI
import mesh_ref as MR
import scenes

W, H = MI.W, MI.H
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("DrawMeshInstanced", "DrawTexturedMeshInstanced", "DrawMeshInstancedDevice",
               "DrawTexturedMeshInstancedDevice", "AssembleMeshInstanced")


def _covered(mesh, M, mode="nz"):
    """Pixels the single draw (mesh, M) writes on a cleared frame."""
    bg = MR.oracle_frame(W, H, False, mode, [])[0]
    fb = MR.oracle_frame(W, H, False, mode, [(mesh, M)], clear=0xFFFFFFFF)[0]
    return (fb.view(np.uint64) != bg.view(np.uint64)).any(axis=-1)


def test_the_new_symbols_are_declared_and_in_the_abi_table():
    from libnativecpurenderer_amd import _abi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "libNativeCPURenderer.h")).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _abi.HIP_LIBRARY_ABI, s
    assert len(_abi.HIP_LIBRARY_ABI["AssembleMeshInstanced"][1]) == 11
    assert len(_abi.HIP_LIBRARY_ABI["DrawMeshInstanced"][1]) == 5


def test_one_instance_is_expand_bit_for_bit():
    for mesh in (MR.sphere3d(), MR.sphere3d(gouraud=False), MR.sphere3d(uv_size=(37, 23))):
        M = MR.perspective(W, H)
        xy, z, attr, q = MI.instanced_soup(mesh, M.reshape(1, 16))
        wxy, wz, wattr = MR.expand(mesh, M)
        assert q is None
        assert scenes.bits_equal(xy, wxy) and scenes.bits_equal(z, wz) and scenes.bits_equal(attr, wattr)
    mesh = MR.sphere3d()
    t = np.array([[0.5, 0.25, 0.75, 1.0]])
    attr = MI.instanced_soup(mesh, M.reshape(1, 16), t)[2]
    assert scenes.bits_equal(attr, MR.expand(dict(mesh, colors=mesh["colors"] * t[0]), M)[2])
    assert attr.shape == (320, 12) and not scenes.bits_equal(attr, MR.expand(mesh, M)[2])
    empty = MI.instanced_soup(mesh, np.zeros((0, 16)))
    assert empty[0].shape == (0, 6) and empty[1].shape == (0, 3) and empty[2].shape == (0, 12)


def test_instance_order_and_counts():
    mesh = MR.sphere3d()
    mats = MI.scene_matrices()
    counts = []
    xy, z, attr, _ = MI.instanced_soup(mesh, mats, counts=counts)
    assert counts == [320] * 10 and xy.shape == (3200, 6)
    for k in (0, 4, 9):
        wxy, wz, _ = MR.expand(mesh, mats[k])
        assert np.array_equal(xy[320 * k:320 * (k + 1)], wxy, equal_nan=True)
        assert np.array_equal(z[320 * k:320 * (k + 1)], wz, equal_nan=True)


def test_random_instances_overlap_and_the_blend_depends_on_their_order():
    mats = MI.scene_matrices()
    assert mats.shape == (10, 16)
    mesh = MR.sphere3d()
    cov = [_covered(mesh, mats[k]) for k in range(7)]
    assert all(c.any() for c in cov)
    shared = max(int((cov[a] & cov[b]).sum()) for a in range(7) for b in range(a + 1, 7))
    assert shared >= 100, shared         # (instances 2 and 3 share 545 pixels)
    blended = MR.sphere3d(alpha=(0.2, 0.9))
    fwd = MI.oracle_frame(W, H, True, "nz", blended, mats)[0]
    rev = MI.oracle_frame(W, H, True, "nz", blended, mats[::-1])[0]
    assert (fwd.view(np.uint64) != rev.view(np.uint64)).any(axis=-1).sum() >= 100


def test_the_explicit_instances():
    mats = MI.scene_matrices()
    mesh = MR.sphere3d()
    x = MR.vertex_stage(mesh["pos"], mats[MI.BEHIND])[0]
    assert np.isnan(x).any() and np.isfinite(x).any()
    assert not _covered(mesh, mats[MI.OFFSCREEN]).any()
    # (50 units along the model's x: far off screen, and under this view's rotation also behind the eye)
    assert not MR.kept(MR.expand(mesh, mats[MI.OFFSCREEN])[0], MR.XFORM).any()
    assert np.array_equal(mats[MI.DUPLICATE], mats[0])
    tint = MI.scene_tints(10)
    assert not np.array_equal(tint[MI.DUPLICATE], tint[0])
    # LESS + write: the duplicate ties every depth of instance 0 and loses every pixel
    with_dup = MI.oracle_frame(W, H, False, "zw", mesh, mats, tint)
    without = MI.oracle_frame(W, H, False, "zw", mesh, mats[:-1], tint[:-1])
    assert scenes.bits_equal(with_dup[0], without[0]) and np.array_equal(with_dup[1], without[1])
    # no depth test: it covers every pixel instance 0 covers
    c0 = _covered(mesh, mats[0])
    both = MI.oracle_frame(W, H, False, "nz", mesh, mats[[0, -1]], tint[[0, -1]])[0]
    dup = MI.oracle_frame(W, H, False, "nz", mesh, mats[[-1]], tint[[-1]])[0]
    first = MI.oracle_frame(W, H, False, "nz", mesh, mats[[0]], tint[[0]])[0]
    assert c0.sum() > 100
    assert scenes.bits_equal(both[c0], dup[c0]) and not scenes.bits_equal(both[c0], first[c0])


def test_the_near_plane_cuts_some_instances_and_spares_others():
    mats = MI.scene_matrices()
    mesh = MR.sphere3d()
    counts = []
    MI.instanced_soup(mesh, mats, w_near=MI.NEAR, counts=counts)
    assert sum(counts) != 10 * 320
    inside = [MC.inside_counts(mesh, M, MI.NEAR) for M in mats]
    cut = [bool(((i == 1) | (i == 2)).any()) for i in inside]
    whole = [bool((i == 3).all()) for i in inside]
    assert any(cut) and any(whole)
    assert counts[int(np.flatnonzero(whole)[0])] == 320
    assert cut[MI.BEHIND + 10] and counts[MI.BEHIND + 10] == 22 + 2 * 28 + 218   # (tests/test_mesh_clip_gpu.py's count)
    for cull in (1, 2):
        c = []
        MI.instanced_soup(mesh, mats, w_near=MI.NEAR, cull=cull, counts=c)
        assert 0 < sum(c) < sum(counts)


def test_tinted_cut_vertices_interpolate_tinted_colours():
    mats = MI.scene_matrices()
    mesh = MR.sphere3d()
    tint = MI.scene_tints(10)
    k = MI.BEHIND + 10
    attr = MI.instanced_soup(mesh, mats, tint, w_near=MI.NEAR)[2]
    plain = MI.instanced_soup(mesh, mats, None, w_near=MI.NEAR)[2]
    assert attr.shape == plain.shape and not scenes.bits_equal(attr, plain)
    one = MC.clip_soup(dict(mesh, colors=mesh["colors"] * tint[k]), mats[k], MI.NEAR, 0)[2]
    c = []
    MI.instanced_soup(mesh, mats, w_near=MI.NEAR, counts=c)
    at = sum(c[:k])
    assert scenes.bits_equal(attr[at:at + c[k]], one)

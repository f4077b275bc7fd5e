"""CPU checks of tests/modulate_ref.py: its two derivations agree, the feature's
two identities hold in the reference, the scenes the GPU tests draw meet their
own conditions (so those tests cannot pass vacuously), and the new entry points
are declared in the header and the ABI table."""
import functools
import os
import re

import numpy as np

import bilinear_ref as BL
import mesh_clip_ref as MC
import mesh_light_ref as ML
import modulate_ref as M
import persp_ref as P
import scenes
import textured_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, BG, CLEAR, FAR = M.W, M.H, M.BG, M.CLEAR, M.FAR

SOUP_ENTRIES = ("DrawTexturedTrianglesModulated", "DrawTexturedTrianglesModulatedDevice")
MESH_ENTRIES = ("CreateTexturedColorMesh", "DrawTexturedMeshLit", "AssembleTexturedColorMesh")


def _same(a, b, what):
    assert scenes.bits_equal(a[0], b[0]), (what, scenes.first_mismatch(a[0], b[0]))
    if b[1] is not None:
        assert np.array_equal(a[1], b[1]), (what, "depth")


def test_entry_points_are_declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "libNativeCPURenderer.h")).read(), flags=re.S)
    from libnativecpurenderer_amd import _abi
    for name in SOUP_ENTRIES + MESH_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _abi.HIP_LIBRARY_ABI, name


@functools.lru_cache(maxsize=None)
def _payload(kind_persp_filt, mode="zw"):
    persp, filt = kind_persp_filt
    info = {}
    want = M.expected_payload(W, H, False, BG, mode, CLEAR, M.soup_batches("opaque", persp), info, filt=filt)
    return want, info


def test_derivations_agree_on_the_opaque_scenes():
    for filt in (0, 1):
        for mode in T.MODES:
            bs = M.soup_batches("opaque", True)
            _same(M.expected_loop(W, H, True, BG, mode, CLEAR, bs, filt=filt),
                  M.expected_payload(W, H, True, BG, mode, CLEAR, bs, filt=filt), f"{mode} filter {filt}")
    bs = M.small_batches("opaque")
    _same(M.expected_loop(M.W2, M.H2, False, BG, "zw", CLEAR, bs), M.expected_payload(M.W2, M.H2, False, BG, "zw", CLEAR, bs),
          "small frame")


def test_identity_unit_colours_give_the_perspective_frame():
    """I1, in the reference: T * 1.0 is T."""
    for persp in (False, True):
        for filt in (0, 1):
            bs = [M.ones_colours(b) for b in M.soup_batches("opaque", persp)]
            _same(M.expected_payload(W, H, True, BG, "zw", CLEAR, bs, filt=filt),
                  BL.expected_payload(W, H, True, BG, "zw", CLEAR, bs, filt=filt), f"I1 opaque persp={persp} filter {filt}")
    bs = [M.ones_colours(b) for b in M.soup_batches("blended")]
    _same(M.expected_loop(W, H, True, BG, "zw", CLEAR, bs, filt=1), BL.expected_loop(W, H, True, BG, "zw", CLEAR, bs, filt=1),
          "I1 blended")


def test_identity_unit_texture_gives_the_gouraud_frame():
    """I2, in the reference, nearest filter: 1.0 * G is G -- against the oracle's own Gouraud draw."""
    for kind, fn in (("opaque", M.expected_payload), ("blended", M.expected_loop)):
        for mode in T.MODES:
            bs = [M.ones_texture(b) for b in M.soup_batches(kind)]
            _same(fn(W, H, True, BG, mode, CLEAR, bs, filt=0), M.expected_gouraud(W, H, True, BG, mode, CLEAR, bs),
                  f"I2 {kind} {mode}")


def test_dense_tile_overflows_every_record_table():
    b = M.dense_batch()
    info = {}
    M.expected_payload(W, H, False, BG, "zw", FAR, [b], info)
    most = max(M.tile_winners(info["idx"], tx, ty) for tx in range(3) for ty in range(4))
    assert most > M.GOURAUD_RT, most
    assert M.tile_winners(info["idx"], 1, 1) == most


def test_scene_conditions():
    for persp in (False, True):
        want, info = _payload((persp, 0))
        cov = info["covered"]
        assert cov.mean() >= 0.5
        # at least half of the covered pixels are tinted: some channel's G is not 1
        assert ((info["G"] != 1.0).any(axis=2) & cov).sum() >= 0.5 * cov.sum()
        # all four sampler clamps fire (either batch's texture)
        fired = np.zeros(4, dtype=bool)
        t0 = 0
        for b in M.soup_batches("opaque", persp):
            sel = cov & (info["idx"] >= t0) & (info["idx"] < t0 + b["xy"].shape[0])
            t0 += b["xy"].shape[0]
            fired |= np.array(M.clamps_fired(b["tex"], info["u"][sel], info["v"][sel]))
        assert fired.all(), fired
    # the modulated frame is neither the plain textured frame nor the Gouraud one
    want, _ = _payload((True, 0))
    bs = M.soup_batches("opaque", True)
    assert not scenes.bits_equal(want[0], BL.expected_payload(W, H, False, BG, "zw", CLEAR, bs, filt=0)[0])
    assert not scenes.bits_equal(want[0], M.expected_gouraud(W, H, False, BG, "zw", CLEAR, bs)[0])
    # nor does the filter or the perspective divide leave it unchanged
    assert not scenes.bits_equal(want[0], _payload((True, 1))[0][0])
    assert not scenes.bits_equal(want[0], _payload((False, 0))[0][0])
    for b in M.soup_batches("opaque", True) + [M.dense_batch()] + M.small_batches("opaque"):
        assert P.q_spread(b["q"]) >= 2
        assert M.is_opaque(b)
    assert all((b["q"] == 1).all() for b in M.soup_batches("opaque", False))
    for b in M.soup_batches("blended") + M.small_batches("blended"):
        a = M.batch_rgba(b)[:, :, 3]
        assert b["tex"].shape[2] == 4 and b["ct"][3] == 0.5 and (a > 0.2).all() and (a < 0.9).all()
    # the loop derivation's condition
    for kind in M.KINDS:
        for b in M.soup_batches(kind) + M.small_batches(kind) + [M.dense_batch()]:
            assert np.nanmax(b["z"]) <= 0.99


def test_uvc_layout():
    b = M.soup_batches("blended")[0]
    a = M.uvc(b).reshape(-1, 3, 6)
    assert np.array_equal(a[:, :, 0:2], b["uv"].reshape(-1, 3, 2))
    assert np.array_equal(a[:, :, 2:6], M.batch_rgba(b))
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    assert np.array_equal(R.interleave_uv_colors(b["uv"], b["rgba"]), M.uvc(b))


# ---- the mesh scenes ------------------------------------------------------------------------
def test_mesh_scene_conditions():
    """A lit colour channel clamps to exactly 1.0; the near plane cuts at least one triangle into two and one
    into one; q varies within the triangles of the perspective scene and is 1 everywhere without the state."""
    mesh = M.lit_textured_sphere()
    lit = ML.lit_colors(mesh, ML.rotation3(), ML.AMBIENT, ML.LIGHTS)
    assert (lit[:, 0:3] == 1.0).any() and (lit[:, 0:3] < 1.0).any()
    cm, _ = M.mesh_twins(mesh)
    counts = MC.clip_soup(cm, P.mesh_matrix("behind_eye"), P.NEAR, 0)[3]
    assert (counts == 2).any() and (counts == 1).any()
    # 1/cw varies within the triangles of the sphere under mesh_ref.perspective (cw runs over about 2 .. 4 across
    # the whole mesh), and by more than a factor 2 once the near plane cuts the behind-the-eye view
    assert P.q_spread(M.mesh_soup(mesh, P.mesh_matrix("perspective"))[3]) >= 1.25
    assert P.q_spread(M.mesh_soup(mesh, P.mesh_matrix("behind_eye"), w_near=P.NEAR)[3]) >= 2
    assert (M.mesh_soup(mesh, P.mesh_matrix("perspective"), persp=False)[3] == 1.0).all()
    b = M.mesh_batch(mesh, P.mesh_matrix("perspective"), P.mesh_texture(False), lit=True, N=ML.rotation3(),
                     ambient=ML.AMBIENT, lights=ML.LIGHTS)
    assert np.nanmax(b["z"]) <= 0.99 and M.is_opaque(b)


def test_mesh_soup_is_the_two_existing_soups_side_by_side():
    """uvc interleaves the textured twin's uv with the colour twin's (lit) colours, clipped or not."""
    mesh = M.random_textured_color_mesh(257, 300, seed=4)
    Mx = P.mesh_matrix("behind_eye")
    amb, lights = ML.random_lights(3, seed=9)
    for near, cull in ((0.0, 0), (P.NEAR, 2)):
        xy, z, a, q = M.mesh_soup(mesh, Mx, True, ML.rotation3(), amb, lights, near, cull)
        want = ML.lit_soup(M.mesh_twins(mesh)[0], Mx, ML.rotation3(), amb, lights, near, cull)
        a = a.reshape(-1, 3, 6)
        assert scenes.bits_equal(xy, want[0]) and scenes.bits_equal(np.ascontiguousarray(a[:, :, 2:6].reshape(-1, 12)), want[2])
        _, tm = M.mesh_twins(mesh)
        uvq = P.clip_soup_q(tm, Mx, near, cull) if near > 0 else P.expand_q(tm, Mx)
        assert scenes.bits_equal(np.ascontiguousarray(a[:, :, 0:2].reshape(-1, 6)), uvq[2]) and scenes.bits_equal(q, uvq[3])

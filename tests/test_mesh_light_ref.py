"""CPU checks of the vertex-lighting reference (tests/mesh_light_ref.py) and of
the scene tests/test_mesh_light_gpu.py draws: the conditions that make those
tests discriminate -- back-facing lights, channels clamped at 1, a sum that
depends on the order of the lights, a normal matrix that changes every vertex,
lit colours at the cut vertices, a tint after the lighting -- asserted on the
reference and the oracle alone, so that no GPU test can pass vacuously."""
import os
import re

import numpy as np

import mesh_clip_ref as MC
import mesh_inst_ref as MI
import mesh_light_ref as ML
import mesh_ref as MR
import scenes

W, H = MI.W, MI.H
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"CreateLitMesh": 7, "UpdateMeshNormals": 2, "GetMeshLit": 1, "SetMeshLights": 4, "GetMeshLightCount": 1,
         "DrawMeshLit": 4, "DrawMeshLitInstanced": 6, "DrawMeshLitInstancedDevice": 6, "AssembleMeshLit": 9,
         "AssembleMeshLitInstanced": 11}


def test_the_new_symbols_are_declared_and_in_the_abi_table():
    from libnativecpurenderer_amd import _abi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "libNativeCPURenderer.h")).read(), flags=re.S)
    for s, arity in ARITY.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % s, text)
        assert m, s
        assert len(m.group(1).split(",")) == arity, s
        assert s in _abi.HIP_LIBRARY_ABI, s
        assert len(_abi.HIP_LIBRARY_ABI[s][1]) == arity, s


def _dots(mesh, N, lights):
    """(nv, nl): the light pass's dot products, in its order."""
    nrm, N = mesh["normals"], np.asarray(N).reshape(9)
    w = [(N[3 * r] * nrm[:, 0] + N[3 * r + 1] * nrm[:, 1]) + N[3 * r + 2] * nrm[:, 2] for r in range(3)]
    return np.stack([(w[0] * L[0] + w[1] * L[1]) + w[2] * L[2] for L in lights], axis=1)


def test_the_scene_has_back_faces_clamped_channels_and_an_order_sensitive_sum():
    mesh = ML.lit_sphere3d()
    assert mesh["normals"].shape == (187, 3)
    assert np.abs((mesh["normals"] ** 2).sum(axis=1) - 1).max() < 1e-15
    lit = ML.lit_colors(mesh, None, ML.AMBIENT, ML.LIGHTS)
    assert (~(_dots(mesh, ML.IDENT9, ML.LIGHTS) > 0)).sum() >= 1        # (300 of the 561 pairs give d = 0)
    assert (lit[:, :3] == 1.0).sum() >= 1 and (mesh["colors"][:, :3] == 1.0).sum() == 0   # (22 clamped values)
    rev = ML.lit_colors(mesh, None, ML.AMBIENT, ML.LIGHTS[::-1])
    order = (lit.view(np.uint64) != rev.view(np.uint64)).any(axis=1)
    assert order.sum() >= 1                                             # (42 vertices)
    assert np.abs(lit - rev).max() < 1e-15
    rot = ML.lit_colors(mesh, ML.rotation3(), ML.AMBIENT, ML.LIGHTS)
    assert (lit.view(np.uint64) != rot.view(np.uint64)).any(axis=1).all()   # every vertex
    for c in (lit, rev, rot):
        assert scenes.bits_equal(c[:, 3], mesh["colors"][:, 3])
        assert (c >= 0).all() and (c <= 1).all()


def test_the_lit_frame_differs_from_the_unlit_one():
    mesh, M = ML.lit_sphere3d(), MR.perspective(W, H)
    unlit = MR.oracle_frame(W, H, False, "zw", [(mesh, M)])
    for N in (None, ML.rotation3()):
        lit = MR.oracle_frame(W, H, False, "zw", [(ML.lit_mesh(mesh, N, ML.AMBIENT, ML.LIGHTS), M)])
        assert (lit[0].view(np.uint64) != unlit[0].view(np.uint64)).any(axis=-1).sum() > 1000
        assert np.array_equal(lit[1], unlit[1])          # the depth is the unlit mesh's
    flat = ML.lit_sphere3d(gouraud=False)
    lf = MR.oracle_frame(W, H, False, "zw", [(ML.lit_mesh(flat, None, ML.AMBIENT, ML.LIGHTS), M)])
    assert not scenes.bits_equal(lf[0], lit[0])


def test_default_lights_reproduce_expand_bit_for_bit():
    M = MR.perspective(W, H)
    for mesh in (ML.lit_sphere3d(), ML.lit_sphere3d(gouraud=False), ML.lit_sphere3d(alpha=(0.2, 0.9)),
                 ML.random_lit_mesh(257, 300, seed=4)):
        assert scenes.bits_equal(ML.lit_colors(mesh), mesh["colors"])
        assert scenes.bits_equal(ML.lit_colors(mesh, ML.rotation3()), mesh["colors"])
        for a, b in zip(ML.lit_soup(mesh, M), MR.expand(mesh, M)):
            assert scenes.bits_equal(a, b)


def _scalar_lit(col, nrm, N, A, lights):
    """One vertex, in Python floats, written from the specification."""
    wx = (N[0] * nrm[0] + N[1] * nrm[1]) + N[2] * nrm[2]
    wy = (N[3] * nrm[0] + N[4] * nrm[1]) + N[5] * nrm[2]
    wz = (N[6] * nrm[0] + N[7] * nrm[1]) + N[8] * nrm[2]
    acc = [float(A[0]), float(A[1]), float(A[2])]
    for L in lights:
        dot = (wx * L[0] + wy * L[1]) + wz * L[2]
        d = dot if dot > 0 else 0.0
        for c in range(3):
            acc[c] = acc[c] + d * L[3 + c]
    out = []
    for c in range(3):
        p = col[c] * acc[c]
        out.append(0.0 if p < 0 else (1.0 if p > 1 else p))
    return out + [col[3]]


def test_the_reference_equals_a_scalar_loop():
    mesh = ML.random_lit_mesh(40, 5, seed=9)
    mesh["colors"][3] = (-0.5, 0.2, 2.0, 0.3)            # a negative product, and one past 1 before any light
    for nl in (0, 1, 3, 8):
        A, lights = ML.random_lights(nl, seed=nl)
        for N in (ML.IDENT9, ML.rotation3()):
            got = ML.lit_colors(mesh, N, A, lights)
            want = np.array([_scalar_lit([float(x) for x in mesh["colors"][v]], [float(x) for x in mesh["normals"][v]],
                                         [float(x) for x in N], A, [[float(x) for x in L] for L in lights])
                             for v in range(40)])
            assert scenes.bits_equal(got, want), nl
    assert got[3, 0] == 0.0


def test_a_nan_normal_gives_no_light_not_nan():
    mesh = ML.random_lit_mesh(8, 2, seed=1)
    mesh["normals"][2] = np.nan
    mesh["normals"][5] = (np.inf, 0.0, 0.0)              # 0 * inf in the identity's rows: NaN as well
    lit = ML.lit_colors(mesh, None, ML.AMBIENT, ML.LIGHTS)
    assert np.isfinite(lit).all()
    for v in (2, 5):
        assert scenes.bits_equal(lit[v, :3], mesh["colors"][v, :3] * np.array(ML.AMBIENT))
    # a NaN product stays NaN: only the dot is guarded
    mesh["colors"][1, 0] = np.nan
    assert np.isnan(ML.lit_colors(mesh, None, ML.AMBIENT, ML.LIGHTS)[1, 0])
    neg = ML.LIGHTS.copy()
    neg[0, 3:] = (-2.0, -2.0, -2.0)                       # a negative light colour: sums below 0 clamp to 0
    assert (ML.lit_colors(ML.lit_sphere3d(), None, ML.AMBIENT, neg)[:, :3] == 0.0).any()


def test_a_cut_vertex_interpolates_lit_colours():
    mesh, M = ML.lit_sphere3d(), MR.behind_eye(W, H)
    info = {}
    xy, z, attr = ML.lit_soup(mesh, M, None, ML.AMBIENT, ML.LIGHTS, w_near=MI.NEAR)
    base = MC.clip_soup(mesh, M, MI.NEAR, 0, info=info)[2]
    assert info["t"].size > 0 and attr.shape == base.shape
    # the corners that are no cut carry lit colours; the cuts are not what lighting the interpolated base colour gives
    lit = ML.lit_colors(mesh, None, ML.AMBIENT, ML.LIGHTS)
    whole = np.flatnonzero(info["inside"] == 3)
    at = np.cumsum(np.r_[0, MC.clip_soup(mesh, M, MI.NEAR, 0)[3]])
    t = int(whole[0])
    assert scenes.bits_equal(attr[at[t]], lit[mesh["idx"][t].astype(np.int64)].reshape(12))
    # a triangle with one vertex inside: its cuts are lit_a + (lit_b - lit_a) * t
    one = int(np.flatnonzero(info["inside"] == 1)[0])
    sa, sb = info["sa"][one], info["sb"][one]
    cw = MC.clip_coords(mesh["pos"], M)[3][mesh["idx"][one].astype(np.int64)]
    la = lit[mesh["idx"][one].astype(np.int64)]
    for s in range(3):
        if sa[s] == sb[s]:
            want = la[sa[s]]
        else:
            tt = (cw[sa[s]] - MI.NEAR) / (cw[sa[s]] - cw[sb[s]])
            want = la[sa[s]] + (la[sb[s]] - la[sa[s]]) * tt
        assert scenes.bits_equal(attr[at[one], 4 * s:4 * s + 4], want)
    assert not scenes.bits_equal(attr[at[one]], base[at[one]])


def test_a_tinted_instance_is_lit_times_tint():
    mesh = ML.lit_sphere3d()
    mats = MI.scene_matrices()[:3]
    normals = np.stack([ML.IDENT9, ML.rotation3(), ML.rotation3(-0.7, 1.9)])
    tint = MI.scene_tints(3)
    attr = ML.lit_instanced_soup(mesh, mats, normals, tint, ML.AMBIENT, ML.LIGHTS)[2]
    idx = mesh["idx"].astype(np.int64)
    for k in range(3):
        lit = ML.lit_colors(mesh, normals[k], ML.AMBIENT, ML.LIGHTS)
        assert scenes.bits_equal(attr[320 * k:320 * (k + 1)], (lit * tint[k])[idx].reshape(320, 12))
        wrong = ML.lit_colors(dict(mesh, colors=mesh["colors"] * tint[k]), normals[k], ML.AMBIENT, ML.LIGHTS)
        assert not scenes.bits_equal(attr[320 * k:320 * (k + 1)], wrong[idx].reshape(320, 12))
    # instance k's colours come from normal matrix k
    same = ML.lit_instanced_soup(mesh, mats, None, tint, ML.AMBIENT, ML.LIGHTS)[2]
    assert scenes.bits_equal(attr[:320], same[:320]) and not scenes.bits_equal(attr[320:640], same[320:640])

"""The frame vocabulary on the oracle alone (no GPU): its lowerings are what
tests/frame_ops.py claims, and the frames its strategies generate -- exactly
the examples tests/test_fuzz_mixed_gpu.py runs -- are worth running."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import bilinear_ref as B
import frame_anim as A
import frame_ops as F
import mesh_clip_ref as MC
import mesh_light_ref as ML
import mesh_ref as MR
import mesh_skin_ref as MS
import modulate_ref as MD
import persp_ref as P
import scenes
import textured_ref as T
import wrap_ref as WR


def test_flat_colours_on_a_2x2_texture_is_texel_zero():
    g = scenes.rng(11)
    for ch in (3, 4):
        tex = g.uniform(0, 1, size=(2, 2, ch))
        uv = np.concatenate([g.uniform(-1e6, 1e6, size=(500, 2)), g.uniform(-3, 5, size=(500, 2)),
                             [[0.0, 0.0], [1.0, 1.0], [-0.0, 2.0], [1e300, -1e300], [0.999, 1.001]]])
        want = np.concatenate([tex[0, 0], [1.0]])[:4] if ch == 3 else tex[0, 0]
        got = T.flat_colours(tex, uv)
        assert got.shape == (uv.shape[0], 4)
        assert scenes.bits_equal(got, np.ascontiguousarray(np.broadcast_to(want, got.shape)))


@pytest.mark.parametrize("space", ["screen", "model"])
def test_unshared_mesh_expands_to_its_soup(space):
    spec = ("tu", space, 57, 1234, 0.3)
    mesh = F.mesh_dict(spec, 140, 110)
    xy, z, uv = F.mesh_soup(spec, 140, 110)
    assert sorted(mesh["idx"].reshape(-1).tolist()) == list(range(3 * 57))      # a permutation: no vertex shared
    assert not np.array_equal(mesh["idx"].reshape(-1), np.arange(3 * 57))
    for M in (None, MR.IDENT16):
        gxy, gz, guv = MR.expand(mesh, M)
        assert scenes.bits_equal(gxy, xy) and scenes.bits_equal(gz, z) and scenes.bits_equal(guv, uv)
    assert np.array_equal(uv[:, 0:2], uv[:, 2:4]) and np.array_equal(uv[:, 0:2], uv[:, 4:6])   # one UV per triangle


# ---- the lowerings of the state frames ------------------------------------------
def _constant_uv_batch(n=14, seed=3):
    """A small soup with one (u, v) per triangle on a 9 x 7 RGBA texture: inside
    it, past every edge, on texel centres and borders."""
    tex = scenes.rng(seed).uniform(0, 1, size=(7, 9, 4))
    b = T.soup(60, 40, n, seed, tex, spread=25.0, ct=(0.9, 0.8, 0.7, 0.5))
    g = scenes.rng(seed + 1)
    uv = np.stack([g.uniform(-2, 11, n), g.uniform(-2, 9, n)], axis=1)
    uv[:4] = [[0.0, 0.0], [8.0, 6.0], [3.5, 2.0], [7.999, 5.999]]
    return dict(b, uv=np.ascontiguousarray(np.repeat(uv[:, None], 3, axis=1).reshape(n, 6)))


@pytest.mark.parametrize("mode", ["zw", "nz"])
def test_constant_uv_bilinear_is_a_flat_colour(oracle, mode):
    """frame_ops' lowering (flat draw_triangles of sample_bilinear at the
    triangle's UV) against bilinear_ref's per-fragment derivations."""
    b = _constant_uv_batch()
    ctx = oracle.context(60, 40, True)
    ctx.set_color(*B.BG)
    T._set_depth_mode(ctx, mode)
    if mode != "nz":
        ctx.clear_depth(B.CLEAR)
    ctx.set_transform(*b["m"])
    ctx.set_color_transform(*b["ct"])
    flat = F.textured_colours(b["tex"], b["uv"], 1)
    assert not scenes.bits_equal(flat, F.textured_colours(b["tex"], b["uv"], 0))
    ctx.draw_triangles(b["xy"], flat, z=b["z"], gouraud=False)
    got = ctx.get_buffer_numpy()
    info = {}
    want, depth = B.expected_loop(60, 40, True, B.BG, mode, B.CLEAR, [b], info)
    assert info["covered"].mean() > 0.3
    assert scenes.bits_equal(got, want)
    if mode != "nz":
        assert scenes.bits_equal(ctx.get_depth_buffer(), depth)
        opaque = dict(b, tex=np.ascontiguousarray(b["tex"][..., :3]), ct=(0.9, 0.8, 0.7, 1.0))
        ctx = oracle.context(60, 40, False)
        ctx.set_color(*B.BG)
        T._set_depth_mode(ctx, mode)
        ctx.clear_depth(B.CLEAR)
        ctx.set_transform(*opaque["m"])
        ctx.set_color_transform(*opaque["ct"])
        ctx.draw_triangles(opaque["xy"], F.textured_colours(opaque["tex"], opaque["uv"], 1), z=opaque["z"], gouraud=False)
        want, depth = B.expected_payload(60, 40, False, B.BG, mode, B.CLEAR, [opaque])
        assert scenes.bits_equal(ctx.get_buffer_numpy(), want) and scenes.bits_equal(ctx.get_depth_buffer(), depth)


def test_power_of_two_q_returns_the_uv_bit_for_bit():
    g = scenes.rng(21)
    u = np.concatenate([g.uniform(-1e6, 1e6, 4000), g.uniform(-3, 43, 4000), 10.0 ** g.uniform(-200, 200, 2000),
                        [0.0, -0.0, 1.0, 36.999999999999996]])
    v = g.permutation(u)
    for q in F.Q_VALUES:
        qs = np.full(u.shape, q)
        U, V = u * qs, v * qs                       # the payload products, constant over the triangle
        gu, gv = P.persp_uv(U, V, qs)
        assert scenes.bits_equal(gu, u) and scenes.bits_equal(gv, v)
    xy, z, uv, q = F.perspective_soup(50, 97, 61, 5, 40.0, (37, 23))
    assert set(np.unique(q)) <= set(F.Q_VALUES) and len(np.unique(q)) == len(F.Q_VALUES)
    assert (q == q[:, :1]).all() and (uv.reshape(-1, 3, 2) == uv.reshape(-1, 3, 2)[:, :1]).all()
    px, py = np.meshgrid(np.arange(0.5, 97, 7.0), np.arange(0.5, 61, 5.0))
    for t in range(50):                             # and through the whole per-fragment expression
        fu, fv, _, _ = P.fragment_uv(xy[t], uv[t], q[t], T.IDENT, px.ravel(), py.ravel())
        ok = np.isfinite(fu)
        assert ok.any() and (fu[ok] == uv[t, 0]).all() and (fv[ok] == uv[t, 1]).all()


def test_affine_matrices_give_q_exactly_one():
    for spec in (("tu", "model", 40, 7, 1.0), ("tu", "screen", 40, 8, 0.3), ("ts", "model", 4, 5, 9)):
        mesh = F.mesh_dict(spec, 97, 61)
        mats = [F.mesh_matrix(spec[1], m, 97, 61) for m in range(4)]
        labels, inst = F.instance_matrices(spec[1], 12, 5, 97, 61)
        mats += list(zip(labels, inst))
        assert {lab for lab, _ in mats} >= ({"affine", "perspective"} if spec[1] == "model" else {"none", "ident"})
        for label, M in mats:
            q = P.expand_q(mesh, M)[3]
            if label == "perspective":
                assert not (q == 1.0).all()
            else:
                assert scenes.bits_equal(q, np.ones_like(q)), label
                for near in F.NEAR_VALUES:          # cw == 1 >= every near plane: nothing is cut, q stays 1
                    cq = P.clip_soup_q(mesh, M, near, 1, True)[3]
                    assert scenes.bits_equal(cq, np.ones_like(cq))


def test_a_cut_vertex_of_a_constant_uv_triangle_keeps_its_uv():
    spec = ("tu", "model", 150, 11, 1.0)
    mesh = F.mesh_dict(spec, 97, 61)
    M = MR.behind_eye(97, 61)
    full = MR.expand(mesh, M)[2]
    cut = 0
    for near in F.NEAR_VALUES[1:]:
        info = {}
        xy, z, uv, counts = MC.clip_soup(mesh, M, near, 0, info)
        inside = info["inside"]
        cut += int(((inside == 1) | (inside == 2)).sum())
        src = np.repeat(np.arange(150), counts)     # the source triangle of every output triangle
        assert scenes.bits_equal(uv, np.ascontiguousarray(full[src]))
        assert (uv.reshape(-1, 3, 2) == uv.reshape(-1, 3, 2)[:, :1]).all()
    assert cut >= 20, "the near planes cut too few triangles to show anything"


# ---- the lowerings of the anim frames (tests/frame_anim.py) -----------------------
ANIM_WRAPS = ((0, 0), (1, 2), (2, 1))


def test_the_clamp_wrap_lowering_is_textured_colours_bit_for_bit():
    g = scenes.rng(31)
    for w, h, ch in ((2, 2, 3), (9, 7, 4), (5, 3, 3), (37, 23, 4)):
        tex = g.uniform(-0.2, 1.3, size=(h, w, ch))
        uv = np.concatenate([np.stack([g.uniform(-3, w + 3, 3000), g.uniform(-3, h + 3, 3000)], axis=1),
                             np.stack([g.uniform(-2 * w, 3 * w, 3000), g.uniform(-2 * h, 3 * h, 3000)], axis=1),
                             g.uniform(-1e6, 1e6, size=(500, 2)),
                             [[0.0, 0.0], [-0.0, h - 1.0], [w - 1.0, h - 1.0], [w - 2.0, h - 2.0], [np.nan, 1.0],
                              [1e300, -1e300], [w - 1.0000000001, 0.5]]])
        for filt in (0, 1):
            want = F.textured_colours(tex, uv, filt)
            got = A.wrapped_colours(tex, uv, filt, (0, 0))
            assert got.shape == want.shape and scenes.bits_equal(got, want), (w, h, ch, filt)
            if (w, h) != (2, 2):
                assert not scenes.bits_equal(A.wrapped_colours(tex, uv, filt, (1, 2)), want)


def _oracle_gouraud(oracle, W, H, b, colours, clear=MD.CLEAR):
    """The frame and depth of the lowering: one Gouraud draw_triangles of `colours`."""
    ctx = oracle.context(W, H, True)
    ctx.set_color(*MD.BG)
    T._set_depth_mode(ctx, "zw")
    ctx.clear_depth(clear)
    ctx.set_transform(*b["m"])
    ctx.set_color_transform(*b["ct"])
    if b["xy"].shape[0]:
        ctx.draw_triangles(b["xy"], colours, z=b["z"], gouraud=True)
    return ctx.get_buffer_numpy(), ctx.get_depth_buffer()


@pytest.mark.parametrize("blended", [False, True], ids=["opaque", "blended"])
@pytest.mark.parametrize("lowering", ["flat-nearest", "flat-bilinear", "gouraud-nearest"])
def test_the_mtri_lowerings_match_the_per_fragment_derivation(oracle, lowering, blended):
    """Both lowerings of a modulated soup (frame_anim: a Gouraud draw_triangles of
    corner colour times the texel at the triangle's one (u, v)) against
    wrap_ref.expected_loop, which samples and multiplies fragment by fragment:
    under every wrap pair the fixed sequences and the generator's sandwiches
    use, with one power-of-two q per triangle."""
    W, H = MD.W2, MD.H2
    colkind, filt = lowering.split("-")[0], int(lowering.endswith("bilinear"))
    tex = A.pow2_array(7, 4 if blended else 3) if colkind == "gouraud" else WR.texture(5, 3, 4 if blended else 3)
    h, w, _ = tex.shape
    xy, _, uv, rgba, q = A.modulated_soup(36, W, H, 5 + blended, 25.0, colkind, blended, "pow2", (w, h))
    z = scenes.rng(9).uniform(0.05, 0.95, size=(36, 3))
    assert len(np.unique(q)) >= 4 and (uv.reshape(-1, 3, 2) == uv.reshape(-1, 3, 2)[:, :1]).all()
    rgb = rgba.reshape(-1, 3, 4)
    assert ((rgb == rgb[:, :1]).all()) == (colkind == "flat") and ((rgb[..., 3] == 1).all()) != blended
    b = dict(xy=xy, uv=uv, z=z, q=q, rgba=rgba, tex=tex, ct=MD.CT_BLEND if blended else MD.CT, m=T.IDENT)
    frames = []
    for wrap in ANIM_WRAPS:
        info = {}
        want, depth = WR.expected_loop(W, H, True, MD.BG, "zw", MD.CLEAR, [b], info, filt=filt, wrap=wrap)
        assert info["covered"].mean() > 0.3
        fu, fv = info["frags"][0]
        assert (WR.outside(fu, w) | WR.outside(fv, h)).mean() > 0.4        # most fragments sample past the clamp's range
        got = _oracle_gouraud(oracle, W, H, b, A.modulated_colours(tex, uv, rgba, filt, wrap))
        assert scenes.bits_equal(got[0], want) and scenes.bits_equal(got[1], depth), (lowering, blended, wrap)
        frames.append(want)
    assert not scenes.bits_equal(frames[0], frames[1]) and not scenes.bits_equal(frames[1], frames[2])


@pytest.mark.parametrize("wrap", ANIM_WRAPS)
def test_the_lit_textured_colour_mesh_lowering_matches_the_per_fragment_derivation(oracle, wrap):
    """A "tl" mesh under lights, a near plane and a cull mode (cut vertices
    occur): modulate_ref.mesh_batch through wrap_ref.expected_loop against the
    Gouraud draw of its corner colours times the texel at each triangle's UV."""
    W, H = MD.W2, MD.H2
    spec = ("tl", "model", 50, 12, 1.0)
    mesh = A.texc_dict(spec, W, H)
    assert sorted(mesh["idx"].reshape(-1).tolist()) == list(range(150))
    tex = A.pow2_array(spec[3], 3 + spec[3] % 2)
    assert set(np.unique(tex)) <= set(A.POW2_VALUES) and 2 <= min(tex.shape[:2]) and max(tex.shape[:2]) <= 9
    M, N = MR.behind_eye(W, H), F.normal_matrix(5)
    ambient, lights = ML.random_lights(3, 4)
    info = {}
    counts = MC.clip_soup(MD.mesh_twins(mesh)[0], M, 0.5, 1, info)[3]
    assert int(((info["inside"] == 1) | (info["inside"] == 2)).sum()) >= 5 and 0 < counts.sum() != 50
    b = MD.mesh_batch(mesh, M, tex, m=T.IDENT, lit=True, N=N, ambient=ambient, lights=lights, w_near=0.5, cull=1, persp=False)
    n = b["xy"].shape[0]
    assert (b["uv"].reshape(n, 3, 2) == b["uv"].reshape(n, 3, 2)[:, :1]).all()      # a cut vertex keeps the constant UV
    b["z"] = np.clip(b["z"], 0.0, 0.99)
    info = {}
    want, depth = WR.expected_loop(W, H, True, MD.BG, "zw", MD.FAR, [b], info, filt=0, wrap=wrap)
    assert info["covered"].mean() > 0.1
    got = _oracle_gouraud(oracle, W, H, b, A.modulated_colours(tex, b["uv"], b["rgba"], 0, wrap), MD.FAR)
    assert scenes.bits_equal(got[0], want) and scenes.bits_equal(got[1], depth)


def test_a_pose_starts_from_the_bind_pose_and_a_normal_less_skin_keeps_the_normals(oracle):
    res = dict(texs=[], bufs=[], meshes=[("l", "model", 4, 6, 3, True, False)],
               rigs=[(0, 5, 41, True, 0), (0, 3, 42, False, 0)], morphs=[(0, 5, 43, True)])

    def after(ops):
        r = A._AnimRun(oracle, (97, 61, True, F.KNOBS_OFF, res, ops))
        r.run()
        return r.meshes[0][1], r.bind[id(r.meshes[0])]

    first, bind = after([("pose", 0, 7, "host", "main")])
    assert not scenes.bits_equal(first["pos"], bind[0]) and not scenes.bits_equal(first["normals"], bind[1])
    moved, _ = after([("pose", 0, 7, "host", "main"), ("lmesh2", 0, 1, None, 13)])
    assert not scenes.bits_equal(moved["pos"], first["pos"]) and not scenes.bits_equal(moved["normals"], first["normals"])
    again, _ = after([("pose", 0, 7, "host", "main"), ("lmesh2", 0, 1, None, 13), ("morph", 0, 3, None, "host", "aux"),
                      ("pose", 0, 7, "host", "main")])
    assert scenes.bits_equal(again["pos"], first["pos"]) and scenes.bits_equal(again["normals"], first["normals"])
    bare, _ = after([("lmesh2", 0, 1, None, 13), ("pose", 1, 8, "host", "main")])
    rig = MS.random_rig(bind[0].shape[0], 3, 42)
    assert scenes.bits_equal(bare["pos"], MS.pose(bind[0], None, rig["joints"], rig["weights"], A.palette("model", 3, 8, 97, 61))[0])
    assert scenes.bits_equal(bare["normals"], moved["normals"]) and not scenes.bits_equal(bare["normals"], bind[1])


# ---- the interpreter ---------------------------------------------------------------
FIXED = (97, 61, True, F.KNOBS_OFF,
         dict(texs=[(9, 7, 4, "u8", 5, None), (20, 11, 3, "f64", 6, (5, 4))],
              bufs=[("c", 40, 1, 40.0, True, False), ("t", 30, 2, 40.0, "const")],
              meshes=[("c", "model", 4, 6, 3, True, False), ("tu", "screen", 20, 4, 0.3)]),
         [("tri", "dev8", 50, 7, 40.0, False, True), ("buf2", 1, ("res", 0), 1.5), ("mesh2", 0, 2, ("res", 0), 9),
          ("tex", ("snap", "main", True), [3.0, 4.0, 50.0, 30.0]), ("aux", "tri", [0.2, 0.3, 0.4, 0.3], [1.0, 2.0, 3.0, 4.0]),
          ("ttri", "host", 30, 8, 40.0, "const", ("snap", "aux", True)), ("getcolor", 30.0, 20.0), ("readdepth",),
          ("mesh", 1, 1, ("res", 1)), ("ttri", "dev", 20, 9, 6.0, "free", ("tiny", 3, 4)), ("gather",),
          ("resize", 50, 40), ("buf", 0, ("tiny", 1, 3)), ("stex", ("res", 1), [1.0, 2.0, 30.0, 30.0], [0.1, 0.9, 0.2, 0.8])])


def test_run_on_the_oracle_is_deterministic(oracle):
    a, b = F.run(oracle, FIXED), F.run(oracle, FIXED)
    assert F.mismatches(a, b) == [] and len(a["probes"]) == 2
    assert a["batches"] == b["batches"] and len(a["batches"]) == 10
    assert a["f64"].shape == (40, 50, 4)
    bare = F.run(oracle, FIXED, triangles=False)
    assert bare["batches"] == [] and not scenes.bits_equal(bare["f64"], a["f64"])
    assert F.kinds(FIXED) <= set(F.ALL_KINDS)
    _state_operations_are_deterministic(oracle)
    _anim_operations_are_deterministic(oracle)


STATE_FIXED = (97, 61, True, F.KNOBS_OFF,
               dict(texs=[(9, 7, 4, "u8", 5, None), (20, 11, 3, "f64", 6, None)], bufs=[("t", 30, 2, 40.0, "free")],
                    meshes=[("l", "model", 4, 6, 3, True, False), ("tu", "model", 20, 4, 0.3), ("ts", "screen", 3, 3, 8),
                            ("c", "screen", 3, 4, 9, False, True)]),
               [("lights", 4, 8), ("near", 0.5), ("cull", 2), ("lmesh", 0, 2, 12), ("mpersp", True), ("filter", 1),
                ("mesh", 1, 1, ("res", 0)), ("mesh", 1, 0, ("res", 1)), ("mesh", 2, 1, ("res", 0)), ("buf", 0, ("res", 0)),
                ("meshi", 1, 3, 21, None, "host"), ("meshi", 3, 4, 22, "alpha", "dev8"), ("lights", 5, 0),
                ("lmesh2", 0, 1, None, 13), ("near", F.NEAR_VALUES[2]), ("cull", 1), ("lmeshi", 0, 5, 23, "opaque", "dev"),
                ("ptri", "dev8", 30, 24, 40.0, ("res", 1)), ("lights", None, 0), ("lmeshi", 0, 2, 24, "alpha", "host"),
                ("filter", 0), ("near", 0.0), ("cull", 0), ("mpersp", False), ("mesh2", 0, 2, ("res", 0), 14)])


def _state_operations_are_deterministic(oracle):
    """The same for a frame that uses every operation of the state vocabulary."""
    a, b = F.run(oracle, STATE_FIXED), F.run(oracle, STATE_FIXED)
    assert F.mismatches(a, b) == [] and a["batches"] == b["batches"] and a["counts"] == b["counts"]
    assert len(a["counts"]) == 12 and {k for k, _, _ in a["batches"]} == {"mesh", "textured", "instanced", "lit"}
    assert any(got < full for full, got in a["counts"]) and any(got > 0 for _, got in a["counts"])
    bare = F.run(oracle, STATE_FIXED, triangles=False)
    assert bare["batches"] == [] and not scenes.bits_equal(bare["f64"], a["f64"])
    used = F.kinds(STATE_FIXED)
    assert used <= set(F.ALL_KINDS) and set(F.STATE_KINDS) <= used, set(F.STATE_KINDS) - used
    # every state reaches the frame: the same operations with the five setters left out draw another one
    plain = STATE_FIXED[:5] + ([op for op in STATE_FIXED[5] if op[0] not in F.STATE5_OPS],)
    assert not scenes.bits_equal(F.run(oracle, plain)["f64"], a["f64"])
    stats = F.state_stats(STATE_FIXED)
    assert stats == dict(two_states=True, changed_between=True, meets_others=True)


ANIM_FIXED = (97, 61, True, F.KNOBS_OFF,
              dict(texs=[(9, 7, 4, "u8", 5, None), (20, 11, 3, "f64", 6, None)], bufs=[("t", 30, 2, 40.0, "tiled")],
                   meshes=[("l", "model", 4, 6, 3, True, False), ("tl", "model", 30, 4, 0.6), ("tc", "screen", 25, 5, 0.3),
                           ("tu", "model", 20, 6, 0.3)],
                   rigs=[(0, 5, 41, True, 0), (1, 129, 42, True, 2), (3, 1, 44, False, 1)],
                   morphs=[(0, 5, 43, True), (2, 2, 45, False), (1, 9, 46, True)]),
              [("lights", 4, 3), ("wrap", 1, 2), ("mtri", "host", 30, 51, 40.0, "flat", False, None, ("res", 0)),
               ("filter", 1), ("mtri", "dev8", 30, 52, 40.0, "gouraud", True, "pow2", ("pow2", 3, 4)),
               ("ttri", "dev", 30, 53, 40.0, "tiled", ("res", 1)), ("buf", 0, ("pow2", 9, 3)),
               ("lmesh", 0, 2, 12), ("pose", 0, 7, "host", "main"), ("lmesh", 0, 2, 12), ("near", 0.5), ("cull", 1),
               ("mesh", 1, 2, ("res", 0)), ("posemorph", 1, 8, 9, 3, "dev", "aux"), ("lmesh", 1, 2, 13),
               ("wrap", 2, 1), ("mesh", 2, 1, ("res", 0)), ("morph", 1, 10, 1, "host", "main"), ("mesh", 2, 0, ("res", 0)),
               ("variant", 0, 1), ("posemorph", 0, 11, 12, None, "host", "main"), ("meshi", 0, 3, 21, "alpha", "host"),
               ("lmeshi", 0, 2, 22, None, "dev"), ("pose", 2, 14, "dev", "main"), ("mesh2", 3, 1, ("res", 1), 15),
               ("ttri", "host", 20, 54, 6.0, "free", ("tiny", 3, 4)), ("wrap", 0, 0), ("filter", 0), ("near", 0.0),
               ("cull", 0), ("mesh", 0, 1, ("res", 0))])


def _anim_operations_are_deterministic(oracle):
    """The same for a frame that uses every operation of the anim vocabulary."""
    a, b = A.run(oracle, ANIM_FIXED), A.run(oracle, ANIM_FIXED)
    assert A.mismatches(a, b) == [] and a["batches"] == b["batches"] and a["counts"] == b["counts"]
    assert {k for k, _, _ in a["batches"]} == {"modulated", "textured", "mesh", "instanced", "lit"}
    assert a["posed"] == 4 and a["posed_between"] == 4 and a["wrapped"][1] > 0.4 * a["wrapped"][0] > 0
    assert any(got < full for full, got in a["counts"]) and np.isfinite(a["f64"]).all()
    bare = A.run(oracle, ANIM_FIXED, triangles=False)
    assert bare["batches"] == [] and not scenes.bits_equal(bare["f64"], a["f64"])
    used = A.kinds(ANIM_FIXED)
    assert used <= set(A.ALL_KINDS) and used >= set(A.ANIM_KINDS), set(A.ANIM_KINDS) - used
    # the wrap and the poses reach the frame: without either the same operations draw another one
    for gone in (("wrap",), A.POSE_OPS):
        plain = ANIM_FIXED[:5] + ([op for op in ANIM_FIXED[5] if op[0] not in gone],)
        assert not scenes.bits_equal(A.run(oracle, plain)["f64"], a["f64"]), gone
    stats = A.state_stats(ANIM_FIXED)
    assert stats["posed_between"] and stats["wrap_between"] and stats["two_states"]
    assert {"modulated"} <= set().union(*A.batch_kinds(ANIM_FIXED)[0])


def _digest(size):
    frames = []
    A.for_each_frame(size, frames.append)
    return hashlib.sha256(repr(frames[:20]).encode()).hexdigest()


_DIGESTS = """
import hashlib, sys
sys.path[:0] = [{tests!r}, {root!r}]
for name in {imports!r}:
    __import__(name)
import frame_ops as F
for size in ("small", "large", "small-state", "large-state"):
    frames = []
    F.for_each_frame(size, frames.append)
    print(size, hashlib.sha256(repr(frames[:20]).encode()).hexdigest())
"""


_ANIM_DIGESTS = """
import hashlib, sys
sys.path[:0] = [{tests!r}, {root!r}]
for name in {imports!r}:
    __import__(name)
import frame_anim as A
for size in ("small-anim", "large-anim"):
    frames = []
    A.for_each_frame(size, frames.append)
    print(size, hashlib.sha256(repr(frames[:20]).encode()).hexdigest())
"""


def _fresh_digests(imports=(), script=None):
    """{size: digest of repr of the first 20 frames} in a fresh interpreter that
    imports `imports`, then frame_ops."""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = (script or _DIGESTS).format(tests=tests, root=os.path.dirname(tests), imports=tuple(imports))
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True).stdout
    return dict(line.split() for line in out.splitlines())


def test_the_old_example_streams_are_what_they_were():
    """The "small" and "large" examples are the regression record.  Their
    makers are pure functions of the five drawn arguments, pinned here on a
    fixed argument list.  What hypothesis draws for those arguments depends on
    the integer constants in the project modules a process has imported
    (frame_ops.py, at _stable_seed), so the digest of the first 20 examples is
    pinned where that set is fixed: in a fresh interpreter that imports
    frame_ops alone.  All four digests are the parent commit's, computed
    before the state frames were added."""
    pure = {}
    for name, make in (("small", F.make_small_frame), ("large", F.make_large_frame)):
        frames = [make(1000003 * s + 17, 7 * s + 1, bool(s & 1), F.KNOB_VALUES["fmt"][s % 3], 10) for s in range(20)]
        pure[name] = hashlib.sha256(repr(frames).encode()).hexdigest()
    assert pure == dict(small="fecaaa06a176d2bf2229951e96797e706d3a20c18e9db91a7fa3917a76184d57",
                        large="57f693796f265a5449e5a519d3d86c4a8cd9c954b77e9b22845ee2a74c35e62a")
    alone = _fresh_digests()
    assert alone["small"] == "b74c46a1eb7793abbb0177b2555ef9a0f79a222212dd31de4fe1bfeff9ddcdae"
    assert alone["large"] == "07effb809ee42c79aed22c9026ae5340ef15728ec0bd561e69d063a638c5c628"


def test_the_state_examples_are_the_same_in_every_process():
    """The CPU test below vouches for the examples the GPU tests run only if
    both draw the same ones: whatever this process has imported, and in a
    fresh interpreter with and without the library's binding and the largest
    GPU test module imported first."""
    here = {size: _digest(size) for size in ("small-state", "large-state", "small-anim", "large-anim")}
    alone = _fresh_digests()
    other = _fresh_digests(("libnativecpurenderer_amd.libNativeCPURendererPybind", "test_parity_gpu"))
    alone.update(_fresh_digests(script=_ANIM_DIGESTS))
    other.update(_fresh_digests(("libnativecpurenderer_amd.libNativeCPURendererPybind", "test_parity_gpu"), _ANIM_DIGESTS))
    for size, digest in here.items():
        assert alone[size] == digest and other[size] == digest, size
    # (the old examples do move with the imports: the reason the state frames draw their seeds differently)
    assert (other["small"], other["large"]) != (alone["small"], alone["large"])


def _fraction(flags):
    return sum(bool(f) for f in flags) / max(len(flags), 1)


@pytest.mark.parametrize("size", ["small", "large", "small-state", "large-state", "small-anim", "large-anim"])
def test_generated_frames_are_worth_running(oracle, size):
    """The examples of the GPU property tests (the same strategies, settings
    and derandomize=True, frame_ops.for_each_frame / frame_anim.for_each_frame),
    on the oracle only."""
    frames, changed, finite, outs = [], [], [], []
    run = A.run if size.endswith("-anim") else F.run

    def visit(fr):
        frames.append(fr)
        out = run(oracle, fr)
        outs.append(out)
        finite.append(all(np.isfinite(a).all() for a in [out["f64"]] + [p for p in out["probes"] if p.dtype == np.float64]))
        if out["batches"]:
            bare = run(oracle, fr, triangles=False)
            changed.append(not scenes.bits_equal(out["f64"], bare["f64"]))

    A.for_each_frame(size, visit)
    assert len(frames) >= {"small": 150, "large": 20}[size.split("-")[0]]
    assert all(finite), "an oracle frame holds a NaN or an infinity"
    report = {}
    if size.startswith("small"):
        # (the old frames: the kinds they were written for; the state frames: every kind)
        # (the anim frames: every kind may occur, every new kind must)
        wanted = F.BASE_KINDS if size == "small" else A.ANIM_KINDS if size == "small-anim" else F.ALL_KINDS
        used = [A.kinds(fr) if size == "small-anim" else F.kinds(fr) for fr in frames]
        assert set().union(*used) <= set(A.ALL_KINDS if size == "small-anim" else wanted)
        for k in wanted:
            report[k] = _fraction([k in u for u in used])
        low = {k: v for k, v in report.items() if v < 0.10}
        assert not low, f"operation kinds in fewer than 10 % of the frames: {low}"
        for knob, values in F.KNOB_VALUES.items():
            for v in values:
                f = _fraction([fr[3][knob] == v for fr in frames])
                assert f >= 0.15, f"knob {knob}={v!r} in {f:.0%} of the frames"
        batch_kinds = A.batch_kinds if size == "small-anim" else F.batch_kinds
        mixed = _fraction([any(len(e) >= 2 for e in batch_kinds(fr)[0]) for fr in frames])
        assert mixed >= 0.30, f"{mixed:.0%} of the frames mix triangle kinds in one depth buffer"
        four = _fraction([batch_kinds(fr)[1] >= 4 for fr in frames])
        assert four >= 0.25, f"{four:.0%} of the frames hold four or more triangle batches"
    if size == "small-state":
        stats = [F.state_stats(fr) for fr in frames]
        two = _fraction([s["two_states"] for s in stats])
        assert two >= 0.30, f"{two:.0%} of the frames hold a mesh draw under two or more non-default states"
        between = _fraction([s["changed_between"] for s in stats])
        assert between >= 0.20, f"{between:.0%} of the frames change a state between two unsynchronised batches"
        meets = _fraction([s["meets_others"] for s in stats])
        assert meets >= 0.25, f"{meets:.0%} of the frames hold a lit or instanced draw beside another kind"
    if size == "small-anim":
        stats = [A.state_stats(fr) for fr in frames]
        posed = _fraction([s["posed_between"] for s in stats])
        assert posed >= 0.20, f"{posed:.0%} of the frames pose a mesh between two unsynchronised draws of it"
        assert [s["posed_between"] for s in stats] == [o["posed_between"] > 0 for o in outs]    # (as the interpreter counts)
        between = _fraction([s["wrap_between"] for s in stats])
        assert between >= 0.20, f"{between:.0%} of the frames change the wrap between two unsynchronised textured batches"
        mod = _fraction([any("modulated" in e and len(e) >= 2 for e in A.batch_kinds(fr)[0]) for fr in frames])
        assert mod >= 0.25, f"{mod:.0%} of the frames hold a modulated batch beside another kind"
    if size.endswith("-anim"):
        # constant-UV triangles drawn under a non-clamp wrap: how many sample outside [0, n-1) on a wrapped axis,
        # where the wrap differs from the clamp (wrap_ref.outside, the 40 % of tests/test_wrap_ref.py)
        total, outside = np.sum([o["wrapped"] for o in outs], axis=0)
        assert total > 1000 and outside >= 0.40 * total, f"{outside} of {total} wrapped triangles sample past the clamp range"
        assert _fraction([o["posed"] > 0 for o in outs]) >= 0.5
        for fr in frames:
            meshes, rigs, morphs = fr[4]["meshes"], fr[4]["rigs"], fr[4]["morphs"]
            assert any(m[0] in A.TEXC for m in meshes)                        # (which is also the pow2-eligible draw)
            assert any(meshes[i][0] in ("l", "tl") for i, *_ in rigs + morphs)
            assert all(nb in A.BONE_COUNTS for _, nb, *_ in rigs) and all(t in A.TARGET_COUNTS for _, t, *_ in morphs)
            assert fr[0] <= (140 if size == "small-anim" else 700) and fr[1] <= (110 if size == "small-anim" else 420)
            for op in fr[5]:
                if op[0] in ("meshi", "lmeshi"):
                    spec = meshes[A.mesh_of(fr, op)]
                    n = 2 * spec[2] * spec[3] if spec[0] in ("c", "l", "ts") else spec[2]
                    assert op[2] == 1 or op[2] * n <= (600 if size == "small-anim" else 4000)
                    assert size == "small-anim" or op[2] == 1 or op[2] * 1.2 * fr[0] * fr[1] <= F.LARGE["budget"]
                if op[0] == "wrap":
                    assert 0 <= op[1] <= 2 and 0 <= op[2] <= 2
    if size.endswith("-state"):         # the sizes the state frames promise
        for fr in frames:
            meshes = fr[4]["meshes"]
            tri = [m[2] if m[0] == "tu" else 2 * m[2] * m[3] for m in meshes]
            lit = [t for m, t in zip(meshes, tri) if m[0] == "l"]
            for op in fr[5]:
                if op[0] in ("meshi", "lmeshi"):
                    n = tri[op[1] % len(tri)] if op[0] == "meshi" else lit[op[1] % len(lit)]
                    if size == "small-state":
                        assert 1 <= op[2] <= 6 and (op[2] == 1 or op[2] * n <= 600) and n <= 200
                        assert fr[0] <= 140 and fr[1] <= 110
                    else:
                        assert 1 <= op[2] <= 40 and (op[2] == 1 or op[2] * n <= 4000)
                        assert op[2] == 1 or op[2] * 1.2 * fr[0] * fr[1] <= F.LARGE["budget"]
                if op[0] == "lights":
                    assert 0 <= op[2] <= 8
    assert len(changed) >= len(frames) // 2
    assert _fraction(changed) >= 0.80, f"the triangles change {_fraction(changed):.0%} of the frames that hold some"

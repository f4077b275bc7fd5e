"""Morph targets on the GPU, bit for bit (DESIGN.md §3 "Morph targets"): the
arrays morph_mesh and pose_mesh_morphed leave in the mesh against the numpy
reference (tests/mesh_morph_ref.py), for host and device weights, with and
without normals, for both skin kernels; the two identities of the fused call;
every kind of mesh draw after a morph against the CPU oracle's frame of the
reference mesh and against the same draw after update_positions /
update_normals; the ordering of a morph between draws with no flush, a batch's
overflow re-run included; repeats, non-finite input, the error cases, an empty
morph and the timing names.  NaNs compare as NaN (mesh_skin_ref.same_bits).  The
scene's own conditions are checked on the CPU in tests/test_mesh_morph_ref.py."""
import functools

import numpy as np
import pytest

import mesh_clip_ref as MC
import mesh_inst_ref as MI
import mesh_light_ref as ML
import mesh_morph_ref as MM
import mesh_ref as MR
import mesh_skin_ref as MS
import scenes
import textured_ref as T

pytestmark = pytest.mark.gpu

W, H = MI.W, MI.H
CT = (0.9, 0.8, 0.7, 1.0)
NEAR = MI.NEAR
A, LIGHTS = ML.AMBIENT, ML.LIGHTS
ROT = ML.rotation3()
FAR = 0xFFFFFFFF
ACTIVE = (0, 1, 3, 4, 5, 8, 9, None)     # both sides of an unroll-by-4 tail; None: every target


def _R():
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    return R


def _gpu_mesh(mesh, lit=True):
    if "uv" in mesh:
        return _R().Mesh(mesh["pos"], mesh["idx"], uv=mesh["uv"])
    return _R().Mesh(mesh["pos"], mesh["idx"], colors=mesh["colors"], gouraud=mesh["gouraud"],
                     normals=mesh["normals"] if lit and "normals" in mesh else None)


def _gpu_morph(mo, normals=True):
    if normals and "normals" in mo:
        return _R().MeshMorph(mo["pos"], mo["dP"], base_normals=mo["normals"], delta_normals=mo["dN"])
    return _R().MeshMorph(mo["pos"], mo["dP"])


def _gpu_skin(mesh, rig, normals=True):
    return _R().MeshSkin(mesh["pos"], rig["joints"], rig["weights"], rig["nb"],
                         bind_normals=mesh["normals"] if normals and "normals" in mesh else None)


def _same(got, want, what):
    assert scenes.bits_equal(got[0], want[0]), (what, scenes.first_mismatch(got[0], want[0]))
    if want[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "depth", scenes.first_mismatch(got[1], want[1]))


def _same_arrays(got, want, what):
    assert MS.same_bits(got, want), (what, scenes.first_mismatch(got, want))


def _ctx(gpu, near=0.0, cull=0, clear=MR.CLEAR):
    ctx = gpu.context(W, H, False)
    MR.begin_frame(ctx, "zw", MR.XFORM, CT, clear=clear)
    ctx.set_mesh_near_plane(near)
    ctx.set_mesh_cull(cull)
    ctx.set_mesh_lights(A, LIGHTS)
    return ctx


def _persp():
    return MR.perspective(W, H)


def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _morph_call(ctx, gm, gmo, w, form):
    """morph_mesh in the host form (the caller's array is overwritten afterwards) or the device form; returns what
    must stay alive until the kernel has run."""
    if form == "host":
        mine = w.copy()
        ctx.morph_mesh(gm, gmo, mine)
        mine[:] = np.nan
        return None
    dev = _device(w)
    ctx.morph_mesh_device(gm, gmo, dev)
    return dev


# ---- 1. the morphed arrays against the reference -----------------------------------------------
@pytest.mark.parametrize("nv", [1, 187, 255, 256, 257])
def test_morphed_arrays_match_the_reference(gpu, nv):
    ctx = gpu.context(8, 8, False)
    mesh = ML.lit_sphere3d() if nv == 187 else ML.random_lit_mesh(nv, 2, seed=nv)
    case = 0
    for Tn in (1, 2, 5, 33) + ((1024,) if nv == 1 else ()):
        mo = MM.random_morph(mesh, Tn, seed=nv + Tn)
        for normals in (True, False):
            gm, gmo = _gpu_mesh(mesh), _gpu_morph(mo, normals)
            assert (gmo.target_count, gmo.vertex_count, gmo.has_normals) == (Tn, nv, normals)
            for active in sorted({Tn if a is None else min(a, Tn) for a in ACTIVE}):
                case += 1
                w = MM.scattered_weights(Tn, active, seed=case)
                if active < Tn:
                    w[int(np.flatnonzero(w == 0)[0])] = -0.0
                want = MM.morphed(mesh, mo, w, normals)
                form = ("host", "device")[case % 2]
                keep = _morph_call(ctx, gm, gmo, w, form)
                what = (nv, Tn, normals, active, form)
                _same_arrays(gm.positions(), want["pos"], what + ("positions",))
                _same_arrays(gm.normals(), want["normals"], what + ("normals",))    # (a normal-less morph: the mesh's own)
                del keep
            # the other form once per morph, all targets active
            w = MM.scattered_weights(Tn, None, seed=case + 7)
            want = MM.morphed(mesh, mo, w, normals)
            for form in ("host", "device"):
                keep = _morph_call(ctx, gm, gmo, w, form)
                _same_arrays(gm.positions(), want["pos"], (nv, Tn, normals, form))
                _same_arrays(gm.normals(), want["normals"], (nv, Tn, normals, form))
                del keep
    assert ctx.get_kernel_timing("mesh_morph") == (0.0, 0)      # (timing is off: nothing is recorded)


def test_an_unlit_mesh_under_a_morph_with_normals(gpu):
    mesh = ML.lit_sphere3d()
    mo, w = MM.sphere_morph(mesh), MM.scene_weights(1)
    plain, gmo, ctx = _gpu_mesh(mesh, lit=False), _gpu_morph(MM.sphere_morph(mesh)), gpu.context(8, 8, False)
    ctx.morph_mesh(plain, gmo, w)
    _same_arrays(plain.positions(), MM.morphed(mesh, mo, w)["pos"], "an unlit mesh")
    with pytest.raises(RuntimeError, match="GetMeshNormals"):
        plain.normals()
    _R().lib.ClearLastError()


# ---- 2. fused with skinning ------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 3, 128, 129])
def test_the_fused_call_matches_morph_then_pose(gpu, nb):
    ctx = gpu.context(8, 8, False)
    mesh = ML.lit_sphere3d()
    nv = 187
    rig = MS.sphere_rig() if nb == 3 else MS.random_rig(nv, nb, seed=nb)
    mo = MM.sphere_morph(mesh) if nb == 3 else MM.random_morph(mesh, 9, seed=nb)
    Tn = mo["dP"].shape[0]
    gm, gmo = _gpu_mesh(mesh), _gpu_morph(mo)
    skins = {True: _gpu_skin(mesh, rig), False: _gpu_skin(mesh, rig, normals=False)}
    case = 0
    for variant in (1, 2):
        for form in ("host", "device"):
            for active in (0, 3, None):
                case += 1
                skin = skins[case % 2 == 0]                 # (whether the skin has bind normals does not matter)
                skin.set_variant(variant)
                w = MM.scattered_weights(Tn, active, seed=case + nb)
                pal = MS.random_palette(nb, seed=case + 3 * nb)
                want = MM.morph_posed(mesh, mo, w, rig, pal)
                if form == "host":
                    mine_p, mine_w = pal.reshape(nb, 3, 4).copy(), w.copy()
                    ctx.pose_mesh_morphed(gm, skin, mine_p, gmo, mine_w)
                    mine_p[:] = np.nan
                    mine_w[:] = np.nan
                    keep = None
                else:
                    keep = (_device(pal), _device(w))
                    ctx.pose_mesh_morphed_device(gm, skin, keep[0], gmo, keep[1])
                what = (nb, variant, form, active)
                _same_arrays(gm.positions(), want["pos"], what + ("positions",))
                _same_arrays(gm.normals(), want["normals"], what + ("normals",))
                del keep
    # a normal-less morph: positions only, the mesh keeps the normals it has
    bare = _gpu_morph(mo, normals=False)
    before = gm.normals()
    w, pal = MM.scattered_weights(Tn, 3, seed=77), MS.random_palette(nb, seed=78)
    ctx.pose_mesh_morphed(gm, skins[True], pal, bare, w)
    _same_arrays(gm.positions(), MM.morph_posed(mesh, mo, w, rig, pal, normals=False)["pos"], (nb, "normal-less morph"))
    assert scenes.bits_equal(gm.normals(), before)
    assert ctx.get_kernel_timing("mesh_morph_skin") == (0.0, 0)


def test_the_two_identities_on_the_device(gpu):
    R = _R()
    mesh, rig = ML.lit_sphere3d(), MS.sphere_rig()
    mo, pal, ctx = MM.sphere_morph(mesh), MS.scene_palette(1), gpu.context(8, 8, False)
    gm, gmo, skin = _gpu_mesh(mesh), _gpu_morph(mo), _gpu_skin(mesh, rig)
    # I1: morph, read back, a skin with that as its bind pose, pose
    w = MM.scene_weights(1)
    ctx.pose_mesh_morphed(gm, skin, pal, gmo, w)
    fused = (gm.positions(), gm.normals())
    ctx.morph_mesh(gm, gmo, w)
    mid = (gm.positions(), gm.normals())
    skin2 = R.MeshSkin(mid[0], rig["joints"], rig["weights"], 3, bind_normals=mid[1])
    ctx.pose_mesh(gm, skin2, pal)
    _same_arrays(gm.positions(), fused[0], "I1 positions")
    _same_arrays(gm.normals(), fused[1], "I1 normals")
    # pose_mesh after morph_mesh starts from the skin's bind pose and overwrites the morph
    ctx.morph_mesh(gm, gmo, w)
    ctx.pose_mesh(gm, skin, pal)
    _same_arrays(gm.positions(), MS.posed(mesh, rig, pal)["pos"], "pose_mesh overwrites the morph")
    # I2: all weights zero == pose_mesh with the morph's base as the bind pose (a base that differs from the mesh's)
    moved = dict(mo, pos=mo["pos"] + 0.125, normals=-mo["normals"])
    moved["pos"][3] = (-0.0, 1.0, -2.0)
    gmo2 = _gpu_morph(moved)
    skin3 = R.MeshSkin(moved["pos"], rig["joints"], rig["weights"], 3, bind_normals=moved["normals"])
    for zero in (0.0, -0.0):
        ctx.pose_mesh_morphed(gm, skin, pal, gmo2, np.full(4, zero))
        got = (gm.positions(), gm.normals())
        ctx.pose_mesh(gm, skin3, pal)
        _same_arrays(got[0], gm.positions(), "I2 positions")
        _same_arrays(got[1], gm.normals(), "I2 normals")
        # ... and morph_mesh alone returns the base, bit for bit, -0.0 included
        ctx.morph_mesh(gm, gmo2, np.full(4, zero))
        assert scenes.bits_equal(gm.positions(), moved["pos"]) and scenes.bits_equal(gm.normals(), moved["normals"])


# ---- 3. every draw of a morphed mesh and of a morphed-and-posed mesh ----------------------------------
def _tex():
    return T.texture_rgb()


@functools.lru_cache(maxsize=None)
def _scene(how, posed):
    """(base mesh, reference mesh after the morph (and pose), oracle frame of the draw `how` of it)."""
    mesh = MR.sphere3d(uv_size=(37, 23)) if how == "textured" else ML.lit_sphere3d()
    mo, w = MM.sphere_morph(ML.lit_sphere3d()), MM.scene_weights(1)
    rm = MM.morph_posed(mesh, mo, w, MS.sphere_rig(), MS.scene_palette(1)) if posed else MM.morphed(mesh, mo, w)
    M = _persp()
    if how == "gouraud":
        want = MR.oracle_frame(W, H, False, "zw", [(rm, M)], ct=CT)
    elif how == "lit":
        want = MR.oracle_frame(W, H, False, "zw", [(ML.lit_mesh(rm, ROT, A, LIGHTS), M)], ct=CT)
    elif how == "textured":
        want = T.expected_payload(W, H, False, MR.BG, "zw", MR.CLEAR, [MR.textured_batch(rm, M, _tex(), ct=CT)])
    elif how == "instanced":
        want = MI.oracle_frame(W, H, False, "zw", rm, MI.scene_matrices(), MI.scene_tints(MI.scene_matrices().shape[0]), ct=CT)
    elif how == "clipped":
        want = MC.oracle_frame(W, H, False, "zw", [(rm, MR.behind_eye(W, H), NEAR, 2)], ct=CT, clear=FAR)
        base = MC.oracle_frame(W, H, False, "zw", [(mesh, MR.behind_eye(W, H), NEAR, 2)], ct=CT, clear=FAR)
        assert (want[0].view(np.uint64) != base[0].view(np.uint64)).any(axis=-1).sum() > 1000
    for a in want:
        if a is not None:
            a.setflags(write=False)
    return mesh, rm, want


def _draw(gpu, ctx, gm, how):
    if how == "gouraud":
        ctx.draw_mesh(gm, _persp())
    elif how == "lit":
        ctx.draw_mesh_lit(gm, _persp(), ROT)
    elif how == "textured":
        ctx.draw_mesh(gm, _persp(), texture=gpu.texture(_tex()))
    elif how == "instanced":
        ctx.draw_mesh_instanced(gm, MI.scene_matrices(), tint=MI.scene_tints(MI.scene_matrices().shape[0]))
    elif how == "clipped":
        ctx.draw_mesh(gm, MR.behind_eye(W, H))


@pytest.mark.parametrize("posed", [False, True], ids=["morphed", "morphed_and_posed"])
@pytest.mark.parametrize("how", ["gouraud", "lit", "textured", "instanced", "clipped"])
def test_draws_of_a_morphed_mesh(gpu, how, posed):
    mesh, rm, want = _scene(how, posed)
    near, cull, clear = (NEAR, 2, FAR) if how == "clipped" else (0.0, 0, MR.CLEAR)
    base = ML.lit_sphere3d()
    gm, gmo = _gpu_mesh(mesh), _gpu_morph(MM.sphere_morph(base))
    ctx = _ctx(gpu, near=near, cull=cull, clear=clear)
    if posed:
        ctx.pose_mesh_morphed(gm, _gpu_skin(base, MS.sphere_rig()), MS.scene_palette(1), gmo, MM.scene_weights(1))
    else:
        ctx.morph_mesh(gm, gmo, MM.scene_weights(1))
    _draw(gpu, ctx, gm, how)
    got = MR.read_frame(ctx, "zw")
    _same(got, want, (how, posed, "on the device, against the oracle"))
    # the numpy result uploaded, on a second context
    gm2 = _gpu_mesh(mesh)
    gm2.update_positions(rm["pos"])
    if gm2.lit:
        gm2.update_normals(rm["normals"])
    ctx2 = _ctx(gpu, near=near, cull=cull, clear=clear)
    _draw(gpu, ctx2, gm2, how)
    _same(got, MR.read_frame(ctx2, "zw"), (how, posed, "against update_positions / update_normals"))
    assert ctx.mesh_last_triangle_count == ctx2.mesh_last_triangle_count > 0


# ---- 4. ordering: no flush between a draw, a morph and the next draw --------------------------------------
@functools.lru_cache(maxsize=None)
def _morph_frame(which):
    mesh = ML.lit_sphere3d()
    want = MR.oracle_frame(W, H, False, "zw", [(MM.morphed(mesh, MM.sphere_morph(mesh), MM.scene_weights(which)), _persp())], ct=CT)
    for a in want:
        a.setflags(write=False)
    return want


@pytest.mark.parametrize("cap", [0, 50])
def test_a_morph_falls_between_the_draws_around_it(gpu, cap):
    """cap 50: A's batch overflows and is re-run when A is next settled, after the morph call: it still shows morph 2."""
    mesh = ML.lit_sphere3d()
    mo = MM.sphere_morph(mesh)
    assert not scenes.bits_equal(_morph_frame(2)[0], _morph_frame(1)[0])
    for morpher in ("A", "B"):
        gm, gmo = _gpu_mesh(mesh), _gpu_morph(mo)
        a, b = _ctx(gpu), _ctx(gpu)
        a.set_pair_capacity_override(cap)
        a.morph_mesh(gm, gmo, MM.scene_weights(2))
        a.draw_mesh(gm, _persp())
        (a if morpher == "A" else b).morph_mesh(gm, gmo, MM.scene_weights(1))
        b.draw_mesh(gm, _persp())
        _same(MR.read_frame(b, "zw"), _morph_frame(1), ("drawn after the morph", cap, morpher))
        _same(MR.read_frame(a, "zw"), _morph_frame(2), ("drawn before the morph", cap, morpher))
        _same_arrays(gm.positions(), MM.morphed(mesh, mo, MM.scene_weights(1))["pos"], ("the mesh holds morph 1", cap, morpher))


# ---- 5. repeats -----------------------------------------------------------------------------------------
def test_the_same_weights_give_the_same_bits_after_any_other_call(gpu):
    mesh, rig = ML.lit_sphere3d(), MS.sphere_rig()
    mo, ctx = MM.sphere_morph(mesh), gpu.context(8, 8, False)
    gm, gmo, skin = _gpu_mesh(mesh), _gpu_morph(mo), _gpu_skin(mesh, rig)
    first = {}
    for step in ("m1", "m2", "m1", "p1", "m1", "f1", "f2", "f1", "m0", "f1", "m1"):
        k = int(step[1])
        if step[0] == "m":
            ctx.morph_mesh(gm, gmo, MM.scene_weights(k))
            want = MM.morphed(mesh, mo, MM.scene_weights(k))
        elif step[0] == "p":
            ctx.pose_mesh(gm, skin, MS.scene_palette(k))
            want = MS.posed(mesh, rig, MS.scene_palette(k))
        else:
            ctx.pose_mesh_morphed(gm, skin, MS.scene_palette(k), gmo, MM.scene_weights(k))
            want = MM.morph_posed(mesh, mo, MM.scene_weights(k), rig, MS.scene_palette(k))
        got = (gm.positions(), gm.normals())
        _same_arrays(got[0], want["pos"], step)
        _same_arrays(got[1], want["normals"], step)
        prev = first.setdefault(step, got)
        assert scenes.bits_equal(got[0], prev[0]) and scenes.bits_equal(got[1], prev[1]), step


# ---- 6. non-finite input ----------------------------------------------------------------------------------
def test_non_finite_weights_and_deltas(gpu):
    R = _R()
    mesh = ML.lit_sphere3d()
    mo = MM.sphere_morph(mesh)
    dP, dN = np.concatenate([mo["dP"], mo["dP"][:2]]), np.concatenate([mo["dN"], mo["dN"][:2]])
    dP[1, 20:30] = np.nan               # target 1, active: ten vertices go NaN
    dP[2, 40] = (np.inf, 0.0, -np.inf)  # target 2, active: one vertex goes infinite
    dN[1, 25] = np.nan                  # (a vertex whose position is NaN too: its triangles are dropped)
    dP[4] = np.nan                      # target 4 under a zero weight and target 5 under a negative zero: skipped
    dN[5] = np.inf
    bad = dict(mo, dP=dP, dN=dN)
    w = np.array([0.5, 0.25, 1.0, 0.0, 0.0, -0.0])
    want = MM.morphed(mesh, bad, w)
    assert np.isnan(want["pos"]).any() and np.isinf(want["pos"]).any() and np.isnan(want["normals"]).any()
    assert np.isfinite(want["pos"]).all(axis=1).sum() == 187 - 11
    gm, gmo, ctx = _gpu_mesh(mesh), _gpu_morph(bad), _ctx(gpu)
    R.lib.ClearLastError()
    assert R.lib.MorphMesh(ctx._ptr, gm._ptr, gmo._ptr, w.ctypes.data)
    ctx.draw_mesh(gm, _persp())
    ctx.draw_mesh_lit(gm, _persp(), ROT)
    ctx.flush()
    assert ctx.mesh_last_triangle_count == 320
    assert not R.lib.GetLastErrorString()
    _same_arrays(gm.positions(), want["pos"], "positions")
    _same_arrays(gm.normals(), want["normals"], "normals")
    frame = ctx.get_buffer_numpy()                             # (a triangle with a NaN vertex is dropped by the rasters)
    assert np.isfinite(frame).all() and (frame != frame[0, 0]).any(axis=-1).sum() > 1000
    # a NaN weight is not skipped, an infinite one neither: every vertex the target moves goes non-finite
    for wbad in (np.nan, np.inf):
        w2 = np.array([0.0, 0.0, 0.0, wbad, 0.0, 0.0])
        want2 = MM.morphed(mesh, bad, w2)
        assert not np.isfinite(want2["pos"]).all()
        ctx.morph_mesh(gm, gmo, w2)
        _same_arrays(gm.positions(), want2["pos"], ("weight", wbad))
        _same_arrays(gm.normals(), want2["normals"], ("weight", wbad))
        ctx.pose_mesh_morphed(gm, _gpu_skin(mesh, MS.sphere_rig()), MS.scene_palette(1), gmo, w2)
        want3 = MM.morph_posed(mesh, bad, w2, MS.sphere_rig(), MS.scene_palette(1))
        _same_arrays(gm.positions(), want3["pos"], ("fused, weight", wbad))
        _same_arrays(gm.normals(), want3["normals"], ("fused, weight", wbad))


# ---- 7. errors --------------------------------------------------------------------------------------------
def test_errors_latch_and_change_nothing(gpu):
    R = _R()
    lib = R.lib
    mesh, rig = ML.lit_sphere3d(), MS.sphere_rig()
    mo = MM.sphere_morph(mesh)
    gm, gmo, skin, ctx = _gpu_mesh(mesh), _gpu_morph(mo), _gpu_skin(mesh, rig), gpu.context(8, 8, False)
    ctx.morph_mesh(gm, gmo, MM.scene_weights(1))
    before = (gm.positions(), gm.normals())
    other = ML.random_lit_mesh(186, 2, seed=1)
    small, small_morph = _gpu_mesh(other), _gpu_morph(MM.random_morph(other, 4, seed=1))
    small_skin = _gpu_skin(other, MS.random_rig(186, 3, seed=1))
    P = lambda a: a.ctypes.data
    pos, nrm = np.ascontiguousarray(mo["pos"]), np.ascontiguousarray(mo["normals"])
    dP, dN = np.ascontiguousarray(mo["dP"]), np.ascontiguousarray(mo["dN"])
    w, pal = MM.scene_weights(2), np.ascontiguousarray(MS.scene_palette(2))
    c, m, s, o = ctx._ptr, gm._ptr, skin._ptr, gmo._ptr
    cases = {
        "CreateMeshMorph": {
            "T = 0": lambda: lib.CreateMeshMorph(187, P(pos), P(nrm), 0, P(dP), P(dN)),
            "T < 0": lambda: lib.CreateMeshMorph(187, P(pos), P(nrm), -1, P(dP), P(dN)),
            "T > 1024": lambda: lib.CreateMeshMorph(187, P(pos), P(nrm), 1025, P(dP), P(dN)),
            "nv < 0": lambda: lib.CreateMeshMorph(-1, P(pos), P(nrm), 4, P(dP), P(dN)),
            "nv beyond 32 bits": lambda: lib.CreateMeshMorph(1 << 32, P(pos), P(nrm), 4, P(dP), P(dN)),
            "NULL base positions": lambda: lib.CreateMeshMorph(187, None, P(nrm), 4, P(dP), P(dN)),
            "NULL position deltas": lambda: lib.CreateMeshMorph(187, P(pos), P(nrm), 4, None, P(dN)),
            "base normals alone": lambda: lib.CreateMeshMorph(187, P(pos), P(nrm), 4, P(dP), None),
            "normal deltas alone": lambda: lib.CreateMeshMorph(187, P(pos), None, 4, P(dP), P(dN)),
        },
        "MorphMesh": {
            "NULL context": lambda: lib.MorphMesh(None, m, o, P(w)),
            "NULL mesh": lambda: lib.MorphMesh(c, None, o, P(w)),
            "NULL morph": lambda: lib.MorphMesh(c, m, None, P(w)),
            "NULL weights": lambda: lib.MorphMesh(c, m, o, None),
            "a morph of another vertex count": lambda: lib.MorphMesh(c, m, small_morph._ptr, P(w)),
            "a mesh of another vertex count": lambda: lib.MorphMesh(c, small._ptr, o, P(w)),
        },
        "MorphMeshDevice": {
            "NULL mesh": lambda: lib.MorphMeshDevice(c, None, o, 4096),
            "NULL morph": lambda: lib.MorphMeshDevice(c, m, None, 4096),
            "NULL weights": lambda: lib.MorphMeshDevice(c, m, o, None),
            "a morph of another vertex count": lambda: lib.MorphMeshDevice(c, m, small_morph._ptr, 4096),
            "weights that are not 16-byte aligned": lambda: lib.MorphMeshDevice(c, m, o, 4096 + 8),
        },
        "PoseMeshMorphed": {
            "NULL context": lambda: lib.PoseMeshMorphed(None, m, s, P(pal), o, P(w)),
            "NULL mesh": lambda: lib.PoseMeshMorphed(c, None, s, P(pal), o, P(w)),
            "NULL skin": lambda: lib.PoseMeshMorphed(c, m, None, P(pal), o, P(w)),
            "NULL palette": lambda: lib.PoseMeshMorphed(c, m, s, None, o, P(w)),
            "NULL morph": lambda: lib.PoseMeshMorphed(c, m, s, P(pal), None, P(w)),
            "NULL weights": lambda: lib.PoseMeshMorphed(c, m, s, P(pal), o, None),
            "a skin of another vertex count": lambda: lib.PoseMeshMorphed(c, m, small_skin._ptr, P(pal), o, P(w)),
            "a morph of another vertex count": lambda: lib.PoseMeshMorphed(c, m, s, P(pal), small_morph._ptr, P(w)),
            "a mesh of another vertex count": lambda: lib.PoseMeshMorphed(c, small._ptr, s, P(pal), o, P(w)),
        },
        "PoseMeshMorphedDevice": {
            "NULL skin": lambda: lib.PoseMeshMorphedDevice(c, m, None, 4096, o, 8192),
            "NULL palette": lambda: lib.PoseMeshMorphedDevice(c, m, s, None, o, 8192),
            "NULL weights": lambda: lib.PoseMeshMorphedDevice(c, m, s, 4096, o, None),
            "a morph of another vertex count": lambda: lib.PoseMeshMorphedDevice(c, m, s, 4096, small_morph._ptr, 8192),
            "a palette that is not 16-byte aligned": lambda: lib.PoseMeshMorphedDevice(c, m, s, 4096 + 8, o, 8192),
            "weights that are not 16-byte aligned": lambda: lib.PoseMeshMorphedDevice(c, m, s, 4096, o, 8192 + 8),
        },
    }
    if R.device_count() > 1:                               # mesh, morph, skin and context not all on one device
        R.set_device(1)
        far_mesh, far_morph, far_skin, far_ctx = _gpu_mesh(mesh), _gpu_morph(mo), _gpu_skin(mesh, rig), gpu.context(8, 8, False)
        R.set_device(0)
        cases["MorphMesh"].update({
            "a mesh on another device": lambda: lib.MorphMesh(c, far_mesh._ptr, o, P(w)),
            "a morph on another device": lambda: lib.MorphMesh(c, m, far_morph._ptr, P(w)),
            "a context on another device": lambda: lib.MorphMesh(far_ctx._ptr, m, o, P(w)),
        })
        cases["PoseMeshMorphed"].update({
            "a skin on another device": lambda: lib.PoseMeshMorphed(c, m, far_skin._ptr, P(pal), o, P(w)),
            "a morph on another device": lambda: lib.PoseMeshMorphed(c, m, s, P(pal), far_morph._ptr, P(w)),
        })
    for name, group in cases.items():
        for what, call in group.items():
            lib.ClearLastError()
            assert not call(), (name, what)
            msg = lib.GetLastErrorString().decode()
            assert msg.startswith(name + ":"), (name, what, msg)
            lib.ClearLastError()
            assert scenes.bits_equal(gm.positions(), before[0]) and scenes.bits_equal(gm.normals(), before[1]), (name, what)
    # the binding: shape errors are ValueError before any call, a false return is RuntimeError with the message
    with pytest.raises(ValueError):
        ctx.morph_mesh(gm, gmo, np.zeros(3))
    with pytest.raises(ValueError):
        ctx.morph_mesh(gm, gmo, np.zeros((4, 1)))
    with pytest.raises(ValueError):
        ctx.morph_mesh(gm, small_morph, np.zeros(4))
    with pytest.raises(ValueError):
        ctx.morph_mesh_device(small, gmo, 4096)
    with pytest.raises(ValueError):
        ctx.pose_mesh_morphed(gm, skin, np.zeros((2, 12)), gmo, w)
    with pytest.raises(ValueError):
        ctx.pose_mesh_morphed(gm, skin, pal, gmo, np.zeros(5))
    with pytest.raises(ValueError):
        ctx.pose_mesh_morphed(gm, small_skin, pal, gmo, w)
    with pytest.raises(ValueError):
        R.MeshMorph(mo["pos"], mo["dP"][:, :100])
    with pytest.raises(ValueError):
        R.MeshMorph(mo["pos"], mo["dP"].reshape(4, -1))
    with pytest.raises(ValueError):
        R.MeshMorph(mo["pos"], mo["dP"], base_normals=mo["normals"])
    with pytest.raises(ValueError):
        R.MeshMorph(mo["pos"], mo["dP"], base_normals=mo["normals"], delta_normals=mo["dN"][:3])
    with pytest.raises(RuntimeError, match="CreateMeshMorph: the target count must be positive"):
        R.MeshMorph(mo["pos"], np.zeros((0, 187, 3)))
    with pytest.raises(RuntimeError, match="MorphMeshDevice: device weights must be 16-byte aligned"):
        ctx.morph_mesh_device(gm, gmo, 4096 + 8)
    lib.ClearLastError()
    assert scenes.bits_equal(gm.positions(), before[0]) and scenes.bits_equal(gm.normals(), before[1])


def test_an_empty_morph_does_nothing(gpu):
    R = _R()
    ctx = gpu.context(8, 8, False)
    gm = R.Mesh(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.uint32), colors=np.zeros((0, 4)), normals=np.zeros((0, 3)))
    gmo = R.MeshMorph(np.zeros((0, 3)), np.zeros((5, 0, 3)), base_normals=np.zeros((0, 3)), delta_normals=np.zeros((5, 0, 3)))
    skin = R.MeshSkin(np.zeros((0, 3)), np.zeros((0, 4), dtype=np.uint32), np.zeros((0, 4)), 2, bind_normals=np.zeros((0, 3)))
    R.lib.ClearLastError()
    ctx.morph_mesh(gm, gmo, np.ones(5))
    ctx.pose_mesh_morphed(gm, skin, MS.identity_palette(2), gmo, np.ones(5))
    assert (gmo.target_count, gmo.vertex_count) == (5, 0)
    assert gm.positions().shape == (0, 3) and gm.normals().shape == (0, 3)
    assert not R.lib.GetLastErrorString()


# ---- 8. timing ----------------------------------------------------------------------------------------------
def test_the_kernels_are_timed_as_mesh_morph_and_mesh_morph_skin(gpu):
    mesh, rig = ML.lit_sphere3d(), MS.sphere_rig()
    gm, gmo, skin = _gpu_mesh(mesh), _gpu_morph(MM.sphere_morph(mesh)), _gpu_skin(mesh, rig)
    ctx = gpu.context(8, 8, False)
    ctx.morph_mesh(gm, gmo, MM.scene_weights(1))                # timing off: nothing is recorded
    ctx.pose_mesh_morphed(gm, skin, MS.scene_palette(1), gmo, MM.scene_weights(1))
    ctx.flush()
    assert ctx.get_kernel_timing("mesh_morph") == (0.0, 0) and ctx.get_kernel_timing("mesh_morph_skin") == (0.0, 0)
    ctx.enable_kernel_timing(True)
    for k in (1, 2, 1):
        ctx.morph_mesh(gm, gmo, MM.scene_weights(k))
    for k in (1, 2):
        ctx.pose_mesh_morphed(gm, skin, MS.scene_palette(k), gmo, MM.scene_weights(k))
    ms, count = ctx.get_kernel_timing("mesh_morph")
    assert count == 3 and ms > 0
    ms, count = ctx.get_kernel_timing("mesh_morph_skin")
    assert count == 2 and ms > 0
    assert ctx.get_kernel_timing("mesh_skin")[1] == 0 and ctx.get_kernel_timing("mesh_vertex")[1] == 0

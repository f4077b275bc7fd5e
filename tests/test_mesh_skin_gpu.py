"""Skinned meshes on the GPU, bit for bit (DESIGN.md §3 "Skinned meshes"): the
arrays pose_mesh leaves in the mesh against the numpy reference
(tests/mesh_skin_ref.py), for the host and the device palette and for both
kernels; every kind of mesh draw after a pose against the CPU oracle's frame of
the posed reference mesh and against the same draw after update_positions /
update_normals with the numpy pose; the ordering of a pose between draws with no
flush, a batch's overflow re-run included; repeats, a skin without normals,
non-finite input and the error cases.  NaNs compare as NaN, not by payload (an
x86 host and the GPU generate different default NaNs).  The scene's own
conditions are checked on the CPU in tests/test_mesh_skin_ref.py."""
import functools

import numpy as np
import pytest

import mesh_clip_ref as MC
import mesh_inst_ref as MI
import mesh_light_ref as ML
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
FAR = 0xFFFFFFFF           # the depth clear of the behind-the-eye scene (its z runs past mesh_ref.CLEAR)
LDS_BOUND = 128            # SKIN_LDS_MAX_BONES: at most that many bones are staged in LDS


def _R():
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    return R


def _gpu_mesh(mesh, lit=True):
    if "uv" in mesh:
        return _R().Mesh(mesh["pos"], mesh["idx"], uv=mesh["uv"])
    return _R().Mesh(mesh["pos"], mesh["idx"], colors=mesh["colors"], gouraud=mesh["gouraud"],
                     normals=mesh["normals"] if lit and "normals" in mesh else None)


def _gpu_skin(mesh, rig, normals=True):
    return _R().MeshSkin(mesh["pos"], rig["joints"], rig["weights"], rig["nb"],
                         bind_normals=mesh["normals"] if normals and "normals" in mesh else None)


def _same(got, want, what):
    assert scenes.bits_equal(got[0], want[0]), (what, scenes.first_mismatch(got[0], want[0]))
    if want[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "depth", scenes.first_mismatch(got[1], want[1]))


def _same_arrays(got, want, what):
    assert MS.same_bits(got, want), (what, scenes.first_mismatch(got, want))


def _ctx(gpu, mode="zw", alpha=False, near=0.0, cull=0, clear=MR.CLEAR):
    ctx = gpu.context(W, H, alpha)
    MR.begin_frame(ctx, mode, MR.XFORM, CT, clear=clear)
    ctx.set_mesh_near_plane(near)
    ctx.set_mesh_cull(cull)
    ctx.set_mesh_lights(A, LIGHTS)
    return ctx


def _persp():
    return MR.perspective(W, H)


def _device_palette(pal):
    import torch
    return torch.from_numpy(np.ascontiguousarray(pal)).to("cuda:0")


# ---- 1. the posed arrays against the reference ------------------------------------------
@pytest.mark.parametrize("nv", [1, 187, 255, 256, 257])
def test_posed_arrays_match_the_reference(gpu, nv):
    ctx = gpu.context(8, 8, False)
    mesh = ML.lit_sphere3d() if nv == 187 else ML.random_lit_mesh(nv, 2, seed=nv)
    gm = _gpu_mesh(mesh)
    rigs = [MS.random_rig(nv, nb, seed=nv + nb) for nb in (1, 2, 64, LDS_BOUND, LDS_BOUND + 1)]
    if nv == 187:
        rigs.append(MS.sphere_rig())
    for rig in rigs:
        nb = rig["nb"]
        skin = _gpu_skin(mesh, rig)
        assert skin.bone_count == nb and skin.vertex_count == nv
        for variant in (0, 1, 2):                          # automatic, the palette from global memory, staged in LDS
            skin.set_variant(variant)
            for form in ("host", "device"):
                pal = MS.random_palette(nb, seed=10 * nb + variant + (form == "device"))
                want_p, want_n = MS.pose(mesh["pos"], mesh["normals"], rig["joints"], rig["weights"], pal)
                if form == "host":
                    mine = pal.reshape(nb, 3, 4).copy()
                    ctx.pose_mesh(gm, skin, mine)
                    mine[:] = np.nan                       # the caller's array is its own again
                else:
                    dev = _device_palette(pal)
                    ctx.pose_mesh_device(gm, skin, dev)    # (kept alive until positions() below has waited for the kernel)
                what = (nv, nb, variant, form)
                _same_arrays(gm.positions(), want_p, what + ("positions",))
                _same_arrays(gm.normals(), want_n, what + ("normals",))
                if form == "device":
                    del dev
        assert ctx.get_kernel_timing("mesh_skin") == (0.0, 0)   # (timing is off: nothing is recorded)


def test_the_skin_kernel_is_timed_as_mesh_skin(gpu):
    mesh, rig = ML.lit_sphere3d(), MS.sphere_rig()
    gm, skin, ctx = _gpu_mesh(mesh), _gpu_skin(mesh, rig), gpu.context(8, 8, False)
    ctx.enable_kernel_timing(True)
    for k in (1, 2, 1):
        ctx.pose_mesh(gm, skin, MS.scene_palette(k))
    ms, count = ctx.get_kernel_timing("mesh_skin")
    assert count == 3 and ms > 0
    assert ctx.get_kernel_timing("mesh_vertex")[1] == 0


# ---- 2. every draw of a posed mesh -------------------------------------------------------
def _tex():
    return T.texture_rgb()


@functools.lru_cache(maxsize=None)
def _scene(how):
    """(bind mesh, posed reference mesh, oracle frame of the draw `how` of it)."""
    if how == "textured":
        mesh = MR.sphere3d(uv_size=(37, 23))
    else:
        mesh = ML.lit_sphere3d(gouraud=how != "flat")
    pm = MS.posed(mesh, MS.sphere_rig(), MS.scene_palette(1))
    M = _persp()
    if how in ("gouraud", "flat"):
        want = MR.oracle_frame(W, H, False, "zw", [(pm, M)], ct=CT)
    elif how == "lit":
        want = MR.oracle_frame(W, H, False, "zw", [(ML.lit_mesh(pm, ROT, A, LIGHTS), M)], ct=CT)
    elif how == "textured":
        want = T.expected_payload(W, H, False, MR.BG, "zw", MR.CLEAR, [MR.textured_batch(pm, M, _tex(), ct=CT)])
    elif how == "instanced":
        want = MI.oracle_frame(W, H, False, "zw", pm, MI.scene_matrices(), MI.scene_tints(MI.scene_matrices().shape[0]), ct=CT)
    elif how == "clipped":
        want = MC.oracle_frame(W, H, False, "zw", [(pm, MR.behind_eye(W, H), NEAR, 2)], ct=CT, clear=FAR)
        bind = MC.oracle_frame(W, H, False, "zw", [(mesh, MR.behind_eye(W, H), NEAR, 2)], ct=CT, clear=FAR)
        assert (want[0].view(np.uint64) != bind[0].view(np.uint64)).any(axis=-1).sum() > 1000
    for a in want:
        if a is not None:
            a.setflags(write=False)
    return mesh, pm, want


def _draw(gpu, ctx, gm, how):
    if how in ("gouraud", "flat"):
        ctx.draw_mesh(gm, _persp())
    elif how == "lit":
        ctx.draw_mesh_lit(gm, _persp(), ROT)
    elif how == "textured":
        ctx.draw_mesh(gm, _persp(), texture=gpu.texture(_tex()))
    elif how == "instanced":
        ctx.draw_mesh_instanced(gm, MI.scene_matrices(), tint=MI.scene_tints(MI.scene_matrices().shape[0]))
    elif how == "clipped":
        ctx.draw_mesh(gm, MR.behind_eye(W, H))


@pytest.mark.parametrize("how", ["gouraud", "flat", "lit", "textured", "instanced", "clipped"])
def test_draws_of_a_posed_mesh(gpu, how):
    mesh, pm, want = _scene(how)
    near, cull, clear = (NEAR, 2, FAR) if how == "clipped" else (0.0, 0, MR.CLEAR)
    # posed on the device
    gm, skin = _gpu_mesh(mesh), _gpu_skin(mesh, MS.sphere_rig())
    ctx = _ctx(gpu, near=near, cull=cull, clear=clear)
    ctx.pose_mesh(gm, skin, MS.scene_palette(1))
    _draw(gpu, ctx, gm, how)
    got = MR.read_frame(ctx, "zw")
    _same(got, want, (how, "posed on the device, against the oracle"))
    # the numpy pose uploaded, on a second context
    gm2 = _gpu_mesh(mesh)
    gm2.update_positions(pm["pos"])
    if gm2.lit:
        gm2.update_normals(pm["normals"])
    ctx2 = _ctx(gpu, near=near, cull=cull, clear=clear)
    _draw(gpu, ctx2, gm2, how)
    _same(got, MR.read_frame(ctx2, "zw"), (how, "against update_positions / update_normals"))
    assert ctx.mesh_last_triangle_count == ctx2.mesh_last_triangle_count > 0


# ---- 3. ordering: no flush between a draw, a pose and the next draw --------------------------
@functools.lru_cache(maxsize=None)
def _pose_frame(which):
    mesh = ML.lit_sphere3d()
    want = MR.oracle_frame(W, H, False, "zw", [(MS.posed(mesh, MS.sphere_rig(), MS.scene_palette(which)), _persp())], ct=CT)
    for a in want:
        a.setflags(write=False)
    return want


@pytest.mark.parametrize("cap", [0, 50])
def test_a_pose_falls_between_the_draws_around_it(gpu, cap):
    """cap 50: A's batch overflows and is re-run when A is next settled, after the pose call: it still shows pose 0."""
    mesh, rig = ML.lit_sphere3d(), MS.sphere_rig()
    assert not scenes.bits_equal(_pose_frame(0)[0], _pose_frame(1)[0])
    for poser in ("A", "B"):
        gm, skin = _gpu_mesh(mesh), _gpu_skin(mesh, rig)
        a, b = _ctx(gpu), _ctx(gpu)
        a.set_pair_capacity_override(cap)
        a.pose_mesh(gm, skin, MS.scene_palette(0))
        a.draw_mesh(gm, _persp())
        (a if poser == "A" else b).pose_mesh(gm, skin, MS.scene_palette(1))
        b.draw_mesh(gm, _persp())
        _same(MR.read_frame(b, "zw"), _pose_frame(1), ("drawn after the pose", cap, poser))
        _same(MR.read_frame(a, "zw"), _pose_frame(0), ("drawn before the pose", cap, poser))
        _same_arrays(gm.positions(), MS.posed(mesh, rig, MS.scene_palette(1))["pos"], ("the mesh holds pose 1", cap, poser))


def test_a_lit_draw_keeps_the_normals_it_was_issued_under(gpu):
    mesh, rig = ML.lit_sphere3d(), MS.sphere_rig()
    gm, skin, ctx, later = _gpu_mesh(mesh), _gpu_skin(mesh, rig), _ctx(gpu), _ctx(gpu)
    ctx.pose_mesh(gm, skin, MS.scene_palette(1))
    ctx.draw_mesh_lit(gm, _persp(), ROT)
    ctx.pose_mesh(gm, skin, MS.scene_palette(2))
    later.draw_mesh_lit(gm, _persp(), ROT)
    _same(MR.read_frame(ctx, "zw"), _scene("lit")[2], "lit, issued before the second pose")
    pm2 = MS.posed(mesh, rig, MS.scene_palette(2))
    want2 = MR.oracle_frame(W, H, False, "zw", [(ML.lit_mesh(pm2, ROT, A, LIGHTS), _persp())], ct=CT)
    _same(MR.read_frame(later, "zw"), want2, "lit, issued after it")


# ---- 4. repeats, a skin without normals ------------------------------------------------------
def test_posing_starts_from_the_bind_pose(gpu):
    mesh, rig = ML.lit_sphere3d(), MS.sphere_rig()
    gm, skin, ctx = _gpu_mesh(mesh), _gpu_skin(mesh, rig), gpu.context(8, 8, False)
    first = None
    for k in (1, 2, 1, 1):
        ctx.pose_mesh(gm, skin, MS.scene_palette(k))
        pm = MS.posed(mesh, rig, MS.scene_palette(k))
        got = (gm.positions(), gm.normals())
        _same_arrays(got[0], pm["pos"], ("positions", k))
        _same_arrays(got[1], pm["normals"], ("normals", k))
        if k == 1:
            first = first or got
            assert scenes.bits_equal(got[0], first[0]) and scenes.bits_equal(got[1], first[1])
    # single-influence identity bones: == the bind pose
    w = np.zeros((187, 4))
    w[:, 0] = 1.0
    ident = _R().MeshSkin(mesh["pos"], rig["joints"], w, 3, bind_normals=mesh["normals"])
    ctx.pose_mesh(gm, ident, MS.identity_palette(3))
    assert (gm.positions() == mesh["pos"]).all() and (gm.normals() == mesh["normals"]).all()


def test_a_lit_mesh_posed_with_a_normal_less_skin_keeps_its_normals(gpu):
    mesh, rig = ML.lit_sphere3d(), MS.sphere_rig()
    gm, skin, ctx = _gpu_mesh(mesh), _gpu_skin(mesh, rig, normals=False), gpu.context(8, 8, False)
    assert not skin.has_normals
    ctx.pose_mesh(gm, skin, MS.scene_palette(1))
    pm = MS.posed(mesh, rig, MS.scene_palette(1), normals=False)
    _same_arrays(gm.positions(), pm["pos"], "positions")
    assert not scenes.bits_equal(pm["pos"], mesh["pos"])
    assert scenes.bits_equal(gm.normals(), mesh["normals"])
    # ... and an unlit mesh posed with a skin that has normals: positions only, no normals to read
    plain, full = _gpu_mesh(mesh, lit=False), _gpu_skin(mesh, rig)
    ctx.pose_mesh(plain, full, MS.scene_palette(1))
    _same_arrays(plain.positions(), pm["pos"], "an unlit mesh")
    with pytest.raises(RuntimeError, match="GetMeshNormals"):
        plain.normals()
    _R().lib.ClearLastError()


# ---- 5. non-finite input -------------------------------------------------------------------------
def test_non_finite_palette_and_weights(gpu):
    R = _R()
    mesh, rig = ML.lit_sphere3d(), MS.sphere_rig()
    # a fourth bone with an infinite and a NaN entry, read by vertices 20 .. 39 -- by half of them under a zero
    # weight -- and an infinite, a NaN and an all-zero weight elsewhere: the rest of the mesh stays finite
    joints, weights = rig["joints"].copy(), rig["weights"].copy()
    joints[20:40, 2] = 3
    weights[20:30, 2] = 0.0
    weights[5, 1] = np.inf
    weights[6, 0] = np.nan
    weights[7] = (0.0, 0.0, 0.0, 0.0)
    pal = np.concatenate([MS.scene_palette(1), MS.scene_palette(1)[2:]])
    pal[3, 3] = np.inf
    pal[3, 5] = np.nan
    want_p, want_n = MS.pose(mesh["pos"], mesh["normals"], joints, weights, pal)
    assert np.isnan(want_p).any() and np.isinf(want_p).any() and np.isnan(want_n).any()
    assert np.isfinite(want_p).all(axis=1).sum() > 150
    gm = _gpu_mesh(mesh)
    skin = R.MeshSkin(mesh["pos"], joints, weights, 4, bind_normals=mesh["normals"])
    ctx = _ctx(gpu)
    R.lib.ClearLastError()
    assert R.lib.PoseMesh(ctx._ptr, gm._ptr, skin._ptr, pal.ctypes.data)
    ctx.draw_mesh(gm, _persp())
    ctx.draw_mesh_lit(gm, _persp(), ROT)
    ctx.flush()
    assert ctx.mesh_last_triangle_count == 320
    assert not R.lib.GetLastErrorString()
    _same_arrays(gm.positions(), want_p, "positions")
    _same_arrays(gm.normals(), want_n, "normals")
    frame = ctx.get_buffer_numpy()                         # (a triangle with a NaN vertex is dropped by the rasters)
    assert np.isfinite(frame).all() and (frame != frame[0, 0]).any(axis=-1).sum() > 1000


# ---- 6. errors ---------------------------------------------------------------------------------------
def test_errors_latch_and_change_nothing(gpu):
    R = _R()
    lib = R.lib
    mesh, rig = ML.lit_sphere3d(), MS.sphere_rig()
    gm, skin, ctx = _gpu_mesh(mesh), _gpu_skin(mesh, rig), gpu.context(8, 8, False)
    ctx.pose_mesh(gm, skin, MS.scene_palette(1))
    before = (gm.positions(), gm.normals())
    other = ML.random_lit_mesh(186, 2, seed=1)
    small, small_skin = _gpu_mesh(other), _gpu_skin(other, MS.random_rig(186, 3, seed=1))
    P = lambda a: a.ctypes.data
    pos, nrm = np.ascontiguousarray(mesh["pos"]), np.ascontiguousarray(mesh["normals"])
    jn, wt = np.ascontiguousarray(rig["joints"]), np.ascontiguousarray(rig["weights"])
    bad = jn.copy()
    bad[100, 3] = 3                                         # == nb, under a zero... or any weight
    zero_w = wt.copy()
    zero_w[100, 3] = 0.0
    pal = np.ascontiguousarray(MS.scene_palette(2))
    out = np.zeros(187 * 3)
    c, m, s = ctx._ptr, gm._ptr, skin._ptr
    cases = {
        "CreateMeshSkin": {
            "nb = 0": lambda: lib.CreateMeshSkin(187, P(pos), P(nrm), P(jn), P(wt), 0),
            "nb < 0": lambda: lib.CreateMeshSkin(187, P(pos), P(nrm), P(jn), P(wt), -3),
            "nb beyond 32 bits": lambda: lib.CreateMeshSkin(187, P(pos), P(nrm), P(jn), P(wt), 1 << 32),
            "nv < 0": lambda: lib.CreateMeshSkin(-1, P(pos), P(nrm), P(jn), P(wt), 3),
            "NULL positions": lambda: lib.CreateMeshSkin(187, None, P(nrm), P(jn), P(wt), 3),
            "NULL joints": lambda: lib.CreateMeshSkin(187, P(pos), P(nrm), None, P(wt), 3),
            "NULL weights": lambda: lib.CreateMeshSkin(187, P(pos), P(nrm), P(jn), None, 3),
            "a joint == nb": lambda: lib.CreateMeshSkin(187, P(pos), P(nrm), P(bad), P(wt), 3),
            "a zero-weight joint == nb": lambda: lib.CreateMeshSkin(187, P(pos), P(nrm), P(bad), P(zero_w), 3),
            "a joint >= a smaller nb": lambda: lib.CreateMeshSkin(187, P(pos), P(nrm), P(jn), P(wt), 2),
        },
        "PoseMesh": {
            "NULL context": lambda: lib.PoseMesh(None, m, s, P(pal)),
            "NULL mesh": lambda: lib.PoseMesh(c, None, s, P(pal)),
            "NULL skin": lambda: lib.PoseMesh(c, m, None, P(pal)),
            "NULL palette": lambda: lib.PoseMesh(c, m, s, None),
            "a skin of another vertex count": lambda: lib.PoseMesh(c, m, small_skin._ptr, P(pal)),
            "a mesh of another vertex count": lambda: lib.PoseMesh(c, small._ptr, s, P(pal)),
        },
        "PoseMeshDevice": {
            "NULL mesh": lambda: lib.PoseMeshDevice(c, None, s, 4096),
            "NULL skin": lambda: lib.PoseMeshDevice(c, m, None, 4096),
            "NULL palette": lambda: lib.PoseMeshDevice(c, m, s, None),
            "a skin of another vertex count": lambda: lib.PoseMeshDevice(c, m, small_skin._ptr, 4096),
            "a palette that is not 16-byte aligned": lambda: lib.PoseMeshDevice(c, m, s, 4096 + 8),
        },
        "GetMeshPositions": {
            "NULL mesh": lambda: lib.GetMeshPositions(None, P(out)),
            "NULL output": lambda: lib.GetMeshPositions(m, None),
        },
        "GetMeshNormals": {
            "NULL mesh": lambda: lib.GetMeshNormals(None, P(out)),
            "NULL output": lambda: lib.GetMeshNormals(m, None),
            "an unlit mesh": lambda: lib.GetMeshNormals(_gpu_mesh(mesh, lit=False)._ptr, P(out)),
        },
    }
    if R.device_count() > 1:                               # mesh, skin and context not all on one device
        R.set_device(1)
        far_mesh, far_skin, far_ctx = _gpu_mesh(mesh), _gpu_skin(mesh, rig), gpu.context(8, 8, False)
        R.set_device(0)
        cases["PoseMesh"].update({
            "a mesh on another device": lambda: lib.PoseMesh(c, far_mesh._ptr, s, P(pal)),
            "a skin on another device": lambda: lib.PoseMesh(c, m, far_skin._ptr, P(pal)),
            "a context on another device": lambda: lib.PoseMesh(far_ctx._ptr, m, s, P(pal)),
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
        ctx.pose_mesh(gm, skin, np.zeros((2, 12)))
    with pytest.raises(ValueError):
        ctx.pose_mesh(gm, skin, np.zeros(36))
    with pytest.raises(ValueError):
        ctx.pose_mesh(gm, small_skin, pal)
    with pytest.raises(ValueError):
        R.MeshSkin(mesh["pos"], rig["joints"][:100], rig["weights"], 3)
    with pytest.raises(ValueError):
        R.MeshSkin(mesh["pos"], rig["joints"], rig["weights"][:, :3], 3)
    with pytest.raises(RuntimeError, match="CreateMeshSkin: joint out of range"):
        R.MeshSkin(mesh["pos"], rig["joints"], rig["weights"], 2)
    lib.ClearLastError()
    assert scenes.bits_equal(gm.positions(), before[0]) and scenes.bits_equal(gm.normals(), before[1])


def test_an_empty_skin_does_nothing(gpu):
    R = _R()
    ctx = gpu.context(8, 8, False)
    gm = R.Mesh(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.uint32), colors=np.zeros((0, 4)), normals=np.zeros((0, 3)))
    skin = R.MeshSkin(np.zeros((0, 3)), np.zeros((0, 4), dtype=np.uint32), np.zeros((0, 4)), 5, bind_normals=np.zeros((0, 3)))
    R.lib.ClearLastError()
    ctx.pose_mesh(gm, skin, MS.identity_palette(5))
    assert skin.bone_count == 5 and gm.positions().shape == (0, 3) and gm.normals().shape == (0, 3)
    assert not R.lib.GetLastErrorString()

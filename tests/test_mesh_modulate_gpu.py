"""Textured colour meshes on the GPU (CreateTexturedColorMesh, DrawTexturedMesh,
DrawTexturedMeshLit, AssembleTexturedColorMesh): the assembled soup against
tests/modulate_ref.py's mesh reference, frames bit for bit against the
oracle-derived frames, the identities with the unlit and the plain textured
draw, posing, updated normals, and the errors."""
import functools

import numpy as np
import pytest

import mesh_light_ref as ML
import mesh_ref as MR
import mesh_skin_ref as MS
import modulate_ref as M
import persp_ref as P
import scenes

pytestmark = pytest.mark.gpu

W, H, BG, FAR, CT = M.W, M.H, M.BG, M.FAR, M.CT
NEAR = P.NEAR
A, LIGHTS = ML.AMBIENT, ML.LIGHTS
ROT = ML.rotation3()


def _R():
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    return R


@pytest.fixture(autouse=True)
def _fresh_error_latch():
    _R().lib.ClearLastError()


def _gpu_mesh(mesh, lit=True):
    return _R().Mesh(mesh["pos"], mesh["idx"], colors=mesh["colors"], uv=mesh["uv"],
                     normals=mesh["normals"] if lit and "normals" in mesh else None)


def _same(got, want, what):
    assert scenes.bits_equal(got[0], want[0]), (what, scenes.first_mismatch(got[0], want[0]))
    if want[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "depth", scenes.first_mismatch(got[1], want[1]))


def _soup_same(got, want, what):
    """xy, z, uvc, q: the colours and uv bit for bit where they are numbers, any NaN equal to any NaN."""
    for name, g, w in zip(("xy", "z", "uvc", "q"), got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert MS.same_bits(g, w), (what, name, scenes.first_mismatch(g, w))


def _ctx(gpu, mode="zw", alpha=False, near=0.0, cull=0, persp=True, ct=CT, filt=0, lights=True, w=W, h=H):
    ctx = gpu.context(w, h, alpha)
    MR.begin_frame(ctx, mode, MR.XFORM, ct, bg=BG, clear=FAR)
    ctx.set_mesh_near_plane(near)
    ctx.set_mesh_cull(cull)
    ctx.set_mesh_perspective(persp)
    ctx.set_triangle_texture_filter(filt)
    if lights:
        ctx.set_mesh_lights(A, LIGHTS)
    return ctx


@functools.lru_cache(maxsize=None)
def _matrix(name):
    Mx = P.mesh_matrix(name)
    Mx.setflags(write=False)
    return Mx


# ---- the soup against the reference ----------------------------------------------------------
@pytest.mark.parametrize("nv", [1, 3, 255, 256, 257, 1000])
def test_assembled_soup_matches_the_reference(gpu, nv):
    mesh = M.random_textured_color_mesh(nv, max(2, 2 * nv), seed=nv)
    gm = _gpu_mesh(mesh)
    assert gm.lit and gm.vertex_count == nv
    Mx = _matrix("behind_eye")
    for nl in (0, 3, 8):
        amb, lights = ML.random_lights(nl, seed=nv + nl)
        for N in (None, ROT):
            for persp in (False, True):
                for near, cull in ((0.0, 0), (NEAR, 0), (NEAR, 1)):
                    ctx = _ctx(gpu, near=near, cull=cull, persp=persp, lights=False, w=8, h=8)
                    ctx.set_mesh_lights(amb, lights)
                    what = f"nv={nv} nl={nl} N={N is not None} persp={persp} near={near} cull={cull}"
                    got = ctx.assemble_textured_color_mesh(gm, Mx, N, lit=True)
                    want = M.mesh_soup(mesh, Mx, True, N, amb, lights, near, cull, persp)
                    _soup_same(got, want, what)
                    if nl == 3 and N is None:
                        got = ctx.assemble_textured_color_mesh(gm, Mx, ROT, lit=False)   # (normal matrix ignored)
                        _soup_same(got, M.mesh_soup(mesh, Mx, False, w_near=near, cull=cull, persp=persp), what + " unlit")


# ---- frames ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want(name, near, cull, persp, filt, rgba, lit, mode="zw", ct=CT):
    mesh = M.lit_textured_sphere()
    tex = P.mesh_texture(rgba)
    b = M.mesh_batch(mesh, _matrix(name), tex, ct=ct, lit=lit, N=ROT, ambient=A, lights=LIGHTS, w_near=near, cull=cull,
                     persp=persp)
    fn = M.expected_loop if rgba or ct[3] != 1 else M.expected_payload
    want = fn(W, H, rgba, BG, mode, FAR, [b], filt=filt)
    for a in want:
        if a is not None:
            a.setflags(write=False)
    return want, b["xy"].shape[0]


@pytest.mark.parametrize("persp", [False, True])
@pytest.mark.parametrize("filt", [0, 1])
def test_lit_sphere_on_both_rasters(gpu, filt, persp):
    mesh = M.lit_textured_sphere()
    gm = _gpu_mesh(mesh)
    tex = gpu.texture(P.mesh_texture(False))
    want, n = _want("perspective", 0.0, 0, persp, filt, False, True)
    for force in (False, True):
        ctx = _ctx(gpu, persp=persp, filt=filt)
        ctx.set_force_ordered_raster(force)
        ctx.draw_mesh_lit(gm, _matrix("perspective"), ROT, texture=tex)
        assert ctx.last_raster_path() == ("ordered" if force else "order-free")
        assert ctx.mesh_last_triangle_count == n == gm.triangle_count
        _same(MR.read_frame(ctx, "zw"), want, f"lit sphere filter={filt} persp={persp} force={force}")


@pytest.mark.parametrize("state", [(NEAR, 0), (NEAR, 1), (NEAR, 2)])
def test_near_plane_and_cull(gpu, state):
    near, cull = state
    mesh = M.lit_textured_sphere()
    gm = _gpu_mesh(mesh)
    tex = gpu.texture(P.mesh_texture(False))
    for name in ("behind_eye", "perspective"):
        for persp in (False, True):
            want, n = _want(name, near, cull, persp, 1, False, True)
            ctx = _ctx(gpu, near=near, cull=cull, persp=persp, filt=1)
            ctx.draw_mesh_lit(gm, _matrix(name), ROT, texture=tex)
            assert ctx.mesh_last_triangle_count == n
            _same(MR.read_frame(ctx, "zw"), want, f"{name} near={near} cull={cull} persp={persp}")


def test_rgba_texture_vertex_alpha_and_colour_transform(gpu):
    gm = _gpu_mesh(M.lit_textured_sphere())
    # an RGBA texture: the ordered raster, blended
    want, _ = _want("perspective", 0.0, 0, True, 0, True, True)
    ctx = _ctx(gpu, alpha=True)
    ctx.draw_mesh_lit(gm, _matrix("perspective"), ROT, texture=gpu.texture(P.mesh_texture(True)))
    assert ctx.last_raster_path() == "ordered"
    _same(MR.read_frame(ctx, "zw"), want, "rgba texture")
    # a colour transform with alpha: ordered too
    ctb = (0.5, 1.25, 0.75, 0.5)
    want, _ = _want("perspective", 0.0, 0, True, 0, False, True, ct=ctb)
    ctx = _ctx(gpu, ct=ctb)
    ctx.draw_mesh_lit(gm, _matrix("perspective"), ROT, texture=gpu.texture(P.mesh_texture(False)))
    assert ctx.last_raster_path() == "ordered"
    _same(MR.read_frame(ctx, "zw"), want, "colour transform")
    # vertex alpha below 1: the mesh is not opaque
    mesh = M.lit_textured_sphere(alpha=(0.2, 0.9))
    b = M.mesh_batch(mesh, _matrix("perspective"), P.mesh_texture(False), lit=True, N=ROT, ambient=A, lights=LIGHTS)
    ctx = _ctx(gpu)
    ctx.draw_mesh_lit(_gpu_mesh(mesh), _matrix("perspective"), ROT, texture=gpu.texture(P.mesh_texture(False)))
    assert ctx.last_raster_path() == "ordered"
    _same(MR.read_frame(ctx, "zw"), M.expected_loop(W, H, False, BG, "zw", FAR, [b]), "vertex alpha")


def test_unlit_draw_and_depth_modes(gpu):
    mesh = M.lit_textured_sphere()
    gm, plain = _gpu_mesh(mesh), _gpu_mesh(mesh, lit=False)
    assert gm.lit and not plain.lit
    tex = gpu.texture(P.mesh_texture(False))
    for mode in ("zw", "zt", "nz"):
        want, _ = _want("perspective", 0.0, 0, True, 0, False, False, mode)
        for g in (gm, plain):
            ctx = _ctx(gpu, mode=mode)
            ctx.draw_mesh(g, _matrix("perspective"), texture=tex)
            assert ctx.last_raster_path() == "order-free"
            _same(MR.read_frame(ctx, mode), want, f"unlit {mode}")


# ---- identities --------------------------------------------------------------------------------
def test_default_lights_give_the_unlit_frame(gpu):
    gm = _gpu_mesh(M.lit_textured_sphere())
    tex = gpu.texture(P.mesh_texture(False))
    for near, cull in ((0.0, 0), (NEAR, 1)):
        frames = []
        for lit in (True, False):
            ctx = _ctx(gpu, near=near, cull=cull, filt=1, lights=False)
            if lit:
                ctx.draw_mesh_lit(gm, _matrix("behind_eye"), ROT, texture=tex)
            else:
                ctx.draw_mesh(gm, _matrix("behind_eye"), texture=tex)
            frames.append(MR.read_frame(ctx, "zw"))
        _same(frames[0], frames[1], f"default lights near={near} cull={cull}")
        _same(frames[0], _want("behind_eye", near, cull, True, 1, False, False)[0], "and the reference's")


def test_unit_colours_give_the_plain_textured_meshes_frame(gpu):
    R = _R()
    mesh = M.lit_textured_sphere()
    ones = dict(mesh, colors=np.ones_like(mesh["colors"]))
    tex = gpu.texture(P.mesh_texture(False))
    for near, cull, persp, filt in ((0.0, 0, True, 0), (NEAR, 2, True, 1), (0.0, 0, False, 1)):
        frames = []
        for gm in (_gpu_mesh(ones), R.Mesh(mesh["pos"], mesh["idx"], uv=mesh["uv"])):
            ctx = _ctx(gpu, near=near, cull=cull, persp=persp, filt=filt)
            ctx.draw_mesh(gm, _matrix("perspective"), texture=tex)
            frames.append(MR.read_frame(ctx, "zw"))
        _same(frames[0], frames[1], f"unit colours near={near} cull={cull} persp={persp} filter={filt}")


# ---- posing, updated normals ---------------------------------------------------------------------
def test_posed_mesh_lit_textured_draw(gpu):
    mesh = M.lit_textured_sphere(rows=10, cols=16)
    rig = MS.sphere_rig(mesh)
    assert rig["nb"] == 3 and mesh["pos"].shape[0] == 187
    gm = _gpu_mesh(mesh)
    skin = _R().MeshSkin(mesh["pos"], rig["joints"], rig["weights"], 3, bind_normals=mesh["normals"])
    ctx = _ctx(gpu, filt=1)
    ctx.pose_mesh(gm, skin, MS.scene_palette(1))
    ctx.draw_mesh_lit(gm, _matrix("perspective"), ROT, texture=gpu.texture(P.mesh_texture(False)))
    posed = MS.posed(mesh, rig, MS.scene_palette(1))
    assert MS.same_bits(gm.normals(), posed["normals"])
    b = M.mesh_batch(posed, _matrix("perspective"), P.mesh_texture(False), lit=True, N=ROT, ambient=A, lights=LIGHTS)
    _same(MR.read_frame(ctx, "zw"), M.expected_payload(W, H, False, BG, "zw", FAR, [b], filt=1), "posed")


def test_updated_normals_and_positions(gpu):
    mesh = M.lit_textured_sphere()
    gm = _gpu_mesh(mesh)
    g = scenes.rng(5)
    moved = dict(mesh, normals=np.ascontiguousarray(mesh["normals"][::-1] * 0.8),
                 pos=mesh["pos"] + g.uniform(-0.03, 0.03, size=mesh["pos"].shape))
    gm.update_normals(moved["normals"])
    gm.update_positions(moved["pos"])
    ctx = _ctx(gpu)
    ctx.draw_mesh_lit(gm, _matrix("perspective"), None, texture=gpu.texture(P.mesh_texture(False)))
    b = M.mesh_batch(moved, _matrix("perspective"), P.mesh_texture(False), lit=True, N=None, ambient=A, lights=LIGHTS)
    _same(MR.read_frame(ctx, "zw"), M.expected_payload(W, H, False, BG, "zw", FAR, [b]), "updated")


# ---- errors and extremes --------------------------------------------------------------------------
def test_mesh_errors_and_extremes(gpu):
    R = _R()
    lib = R.lib
    mesh = M.lit_textured_sphere()
    lit, unlit = _gpu_mesh(mesh), _gpu_mesh(mesh, lit=False)
    colour = R.Mesh(mesh["pos"], mesh["idx"], colors=mesh["colors"], normals=mesh["normals"])
    textured = R.Mesh(mesh["pos"], mesh["idx"], uv=mesh["uv"])
    tex = gpu.texture(P.mesh_texture(False))
    ctx = _ctx(gpu)
    before = ctx.get_buffer_numpy()
    mats = np.ascontiguousarray(np.tile(_matrix("perspective"), (2, 1)))
    P_ = lambda a: a.ctypes.data
    nout = np.zeros(1, dtype=np.int64)
    buf = np.zeros(4 * lit.triangle_count * 18)
    unsupported = "not supported for a textured colour mesh"
    calls = {
        "lit draw without normals": (lambda: lib.DrawTexturedMeshLit(ctx._ptr, unlit._ptr, tex._ptr, None, None), "normals"),
        "lit draw of a colour mesh": (lambda: lib.DrawTexturedMeshLit(ctx._ptr, colour._ptr, tex._ptr, None, None),
                                      "not a textured colour mesh"),
        "lit draw of a textured mesh": (lambda: lib.DrawTexturedMeshLit(ctx._ptr, textured._ptr, tex._ptr, None, None),
                                        "not a textured colour mesh"),
        "NULL texture": (lambda: lib.DrawTexturedMeshLit(ctx._ptr, lit._ptr, None, None, None), "NULL texture"),
        "DrawMesh": (lambda: lib.DrawMesh(ctx._ptr, lit._ptr, None), unsupported),
        "DrawMeshLit": (lambda: lib.DrawMeshLit(ctx._ptr, lit._ptr, None, None), unsupported),
        "DrawMeshInstanced": (lambda: lib.DrawMeshInstanced(ctx._ptr, lit._ptr, P_(mats), None, 2), unsupported),
        "DrawTexturedMeshInstanced": (lambda: lib.DrawTexturedMeshInstanced(ctx._ptr, lit._ptr, tex._ptr, P_(mats), 2),
                                      unsupported),
        "DrawMeshLitInstanced": (lambda: lib.DrawMeshLitInstanced(ctx._ptr, lit._ptr, P_(mats), None, None, 2), unsupported),
        "AssembleMeshPerspective": (lambda: lib.AssembleMeshPerspective(ctx._ptr, lit._ptr, None, 4, P_(buf), P_(buf), P_(buf),
                                                                        P_(buf), P_(nout)), unsupported),
    }
    for what, (call, msg) in calls.items():
        lib.ClearLastError()
        ctx.draw_mesh(lit, _matrix("perspective"), texture=tex)   # (a draw that leaves a count behind)
        assert ctx.mesh_last_triangle_count > 0
        MR.begin_frame(ctx, "zw", MR.XFORM, CT, bg=BG, clear=FAR)
        call()
        err = (lib.GetLastErrorString() or b"").decode()
        assert msg in err, (what, err)
        assert scenes.bits_equal(ctx.get_buffer_numpy(), before), what
        if what.startswith("lit draw") or what == "NULL texture":
            assert ctx.mesh_last_triangle_count == 0, what
    lib.ClearLastError()
    with pytest.raises(ValueError):
        ctx.draw_mesh_lit(unlit, None, None, texture=tex)
    with pytest.raises(ValueError):
        ctx.draw_mesh_lit(textured, None, None, texture=tex)
    with pytest.raises(RuntimeError, match="normals"):
        ctx.assemble_textured_color_mesh(unlit, None, None, lit=True)
    lib.ClearLastError()
    # n = 0 and nv = 0 meshes draw nothing and latch nothing
    empty_idx = np.zeros((0, 3), dtype=np.uint32)
    for m0 in (R.Mesh(mesh["pos"], empty_idx, colors=mesh["colors"], uv=mesh["uv"], normals=mesh["normals"]),
               R.Mesh(np.zeros((0, 3)), empty_idx, colors=np.zeros((0, 4)), uv=np.zeros((0, 2)), normals=np.zeros((0, 3)))):
        ctx.draw_mesh(m0, None, texture=tex)
        ctx.draw_mesh_lit(m0, None, None, texture=tex)
        assert ctx.mesh_last_triangle_count == 0
        assert [a.shape[0] for a in ctx.assemble_textured_color_mesh(m0)] == [0, 0, 0, 0]
        assert scenes.bits_equal(ctx.get_buffer_numpy(), before)
    assert not lib.GetLastErrorString()
    ctx.draw_mesh_lit(lit, _matrix("perspective"), ROT, texture=tex)   # and the context still draws
    _same(MR.read_frame(ctx, "zw"), _want("perspective", 0.0, 0, True, 0, False, True)[0], "after the errors")

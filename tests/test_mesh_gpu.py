"""Indexed meshes on the GPU, bit for bit: the vertex stage and the assembly
(assemble_mesh) against the numpy reference (tests/mesh_ref.py), and draw_mesh
(f64 framebuffer, u32 depth) against the CPU oracle's DrawTriangles of the
reference's soup -- both rasters, every attribute kind, vertices behind the
eye, the lifetime of the per-draw staging, update_positions and the error
cases.  The scenes' own conditions are checked on the CPU in
tests/test_mesh_ref.py."""
import functools

import numpy as np
import pytest

import mesh_ref as MR
import scenes
import textured_ref as T

pytestmark = pytest.mark.gpu

W, H = 130, 97             # 3 x 4 tiles, partial right and bottom tiles
ONE = (1.0, 1.0, 1.0, 1.0)
CT = (0.9, 0.8, 0.7, 1.0)


def _R():
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    return R


def _gpu_mesh(mesh):
    R = _R()
    if "uv" in mesh:
        return R.Mesh(mesh["pos"], mesh["idx"], uv=mesh["uv"])
    return R.Mesh(mesh["pos"], mesh["idx"], colors=mesh["colors"], gouraud=mesh["gouraud"])


def _same(got, want, what):
    assert scenes.bits_equal(got[0], want[0]), (what, scenes.first_mismatch(got[0], want[0]))
    if want[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "depth", scenes.first_mismatch(got[1], want[1]))


def _ctx(gpu, mode, alpha=False, ct=ONE, clear=MR.CLEAR, w=W, h=H):
    ctx = gpu.context(w, h, alpha)
    MR.begin_frame(ctx, mode, MR.XFORM, ct, clear=clear)
    return ctx


@functools.lru_cache(maxsize=None)
def _persp():
    M = MR.perspective(W, H)
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def _want(kind, mode, alpha):
    """Oracle frames of the colour scenes under the perspective matrix."""
    mesh = {"gouraud": MR.sphere3d(), "flat": MR.sphere3d(gouraud=False),
            "blended": MR.sphere3d(alpha=(0.2, 0.9))}[kind]
    want = MR.oracle_frame(W, H, alpha, mode, [(mesh, _persp())], ct=CT)
    for a in want:
        if a is not None:
            a.setflags(write=False)
    return mesh, want


# ---- vertex stage and assembly ----------------------------------------------
@pytest.mark.parametrize("nv", [3, 64, 65, 1000])
def test_assemble_matches_the_reference(gpu, nv):
    ctx = gpu.context(8, 8, False)
    mats = {"perspective": MR.perspective(W, H, d=0.9), "affine": MR.affine(W, H), "identity": None}
    for n in (1, 63, 64, 65, 85, 86, 191, 193, 257, 3000):   # (3n crosses 256 between 85 and 86)
        mesh = MR.random_mesh(nv, n, seed=1000 * nv + n)
        gm = _gpu_mesh(mesh)
        assert (gm.vertex_count, gm.triangle_count) == (nv, n)
        for name, M in mats.items():
            xy, z = ctx.assemble_mesh(gm, M)
            wxy, wz, _ = MR.expand(mesh, M)
            if name == "perspective" and nv > 3 and n >= 63:   # (the eye at 0.9 from the origin: some vertices behind it)
                assert np.isnan(wxy).any() and np.isfinite(wxy).any()
            assert np.array_equal(xy, wxy, equal_nan=True), (name, nv, n)
            assert np.array_equal(z, wz, equal_nan=True), (name, nv, n)
            if name != "perspective":   # cw == 1: no NaN, and bitwise the linear expression
                assert scenes.bits_equal(xy, wxy) and scenes.bits_equal(z, wz)


def test_assemble_of_a_textured_mesh(gpu):
    mesh = MR.sphere3d(uv_size=(37, 23))
    xy, z = gpu.context(8, 8, False).assemble_mesh(_gpu_mesh(mesh), _persp())
    wxy, wz, _ = MR.expand(mesh, _persp())
    assert scenes.bits_equal(xy, wxy) and scenes.bits_equal(z, wz)


# ---- draw parity against the oracle -----------------------------------------
@pytest.mark.parametrize("alpha", [False, True])
def test_gouraud_opaque_depth_write(gpu, alpha):
    mesh, want = _want("gouraud", "zw", alpha)
    ctx = _ctx(gpu, "zw", alpha, CT)
    ctx.draw_mesh(_gpu_mesh(mesh), _persp())
    assert ctx.last_raster_path() == "order-free"
    _same(MR.read_frame(ctx, "zw"), want, f"gouraud alpha={alpha}")


def test_flat_takes_the_first_index_colour(gpu):
    mesh, want = _want("flat", "zw", False)
    ctx = _ctx(gpu, "zw", False, CT)
    ctx.draw_mesh(_gpu_mesh(mesh), _persp())
    assert ctx.last_raster_path() == "order-free"
    _same(MR.read_frame(ctx, "zw"), want, "flat")
    assert not scenes.bits_equal(want[0], _want("gouraud", "zw", False)[1][0])


@pytest.mark.parametrize("mode", ["zt", "nz"])
def test_translucent_vertices_take_the_ordered_raster(gpu, mode):
    mesh, want = _want("blended", mode, True)
    ctx = _ctx(gpu, mode, True, CT)
    ctx.draw_mesh(_gpu_mesh(mesh), _persp())
    assert ctx.last_raster_path() == "ordered"
    _same(MR.read_frame(ctx, mode), want, f"blended {mode}")


def test_forced_ordered_raster_gives_the_same_frame(gpu):
    mesh, want = _want("gouraud", "zw", False)
    ctx = _ctx(gpu, "zw", False, CT)
    ctx.set_force_ordered_raster(True)
    ctx.draw_mesh(_gpu_mesh(mesh), _persp())
    assert ctx.last_raster_path() == "ordered"
    _same(MR.read_frame(ctx, "zw"), want, "forced ordered")


@pytest.mark.parametrize("channels", [3, 4])
def test_textured_mesh(gpu, channels):
    tex = T.texture_rgb() if channels == 3 else T.texture_rgba(w=37, h=23)
    mesh = MR.sphere3d(uv_size=(37, 23))
    batch = MR.textured_batch(mesh, _persp(), tex, ct=CT)
    expected = T.expected_payload if channels == 3 else T.expected_loop
    info = {}
    want = expected(W, H, False, MR.BG, "zw", MR.CLEAR, [batch], info)
    assert info["covered"].mean() > 0.2 and len(info["texels"]) >= 100
    ctx = _ctx(gpu, "zw", False, CT)
    ctx.draw_mesh(_gpu_mesh(mesh), _persp(), texture=gpu.texture(tex))
    assert ctx.last_raster_path() == ("order-free" if channels == 3 else "ordered")
    _same(MR.read_frame(ctx, "zw"), want, f"textured, {channels} channels")


# ---- identity and affine matrices: the GPU's own soup draw -------------------
def test_identity_and_affine_equal_the_soup_draw(gpu):
    mesh = MR.sphere3d()
    A = MR.affine(W, H)
    screen = dict(mesh, pos=np.stack(MR.vertex_stage(mesh["pos"], A), axis=-1))   # already projected
    xy, z, c = MR.expand(mesh, A)
    ref = _ctx(gpu, "zw", False, CT)
    ref.draw_triangles(xy, c, z=z, gouraud=True)
    want = MR.read_frame(ref, "zw")
    _same(want, MR.oracle_frame(W, H, False, "zw", [(mesh, A)], ct=CT), "the soup itself")
    for what, m, M in (("affine", mesh, A), ("identity", screen, None), ("identity matrix", screen, MR.IDENT16)):
        ctx = _ctx(gpu, "zw", False, CT)
        ctx.draw_mesh(_gpu_mesh(m), M)
        _same(MR.read_frame(ctx, "zw"), want, what)


# ---- behind the eye -----------------------------------------------------------
def test_vertices_behind_the_eye_drop_their_triangles(gpu):
    mesh, M = MR.behind_eye_mesh(), MR.behind_eye(W, H)
    xy, z, _ = MR.expand(mesh, M)
    keep = MR.kept(xy, MR.XFORM)
    assert 0.1 <= 1 - keep.mean() <= 0.9, keep.mean()
    assert (np.abs(MR.xform(MR.XFORM, xy[keep])) > 1e7).any()   # the huge-coordinate rule runs
    want = MR.oracle_frame(W, H, False, "zw", [(mesh, M)], ct=CT, clear=0xFFFFFFFF)
    assert (want[1] != 0xFFFFFFFF).mean() > 0.1
    gm = _gpu_mesh(mesh)
    for force in (False, True):
        ctx = _ctx(gpu, "zw", False, CT, clear=0xFFFFFFFF)
        ctx.set_force_ordered_raster(force)
        ctx.draw_mesh(gm, M)
        _same(MR.read_frame(ctx, "zw"), want, f"behind the eye, force={force}")
    gxy, gz = ctx.assemble_mesh(gm, M)
    assert np.array_equal(gxy, xy, equal_nan=True) and np.array_equal(gz, z, equal_nan=True)


# ---- lifetime of the per-draw staging -----------------------------------------
def _second_mesh():
    """More triangles than sphere3d() (the staging is regrown), smaller and off
    to one side, so that both meshes show."""
    mesh = MR.sphere3d(rows=13, cols=21, seed=8)
    mesh["pos"] = mesh["pos"] * 0.6 + np.array([0.0, 0.3, -0.8])
    return mesh


M_SECOND = dict(d=3.0, ax=-0.4, ay=1.1)


def test_two_meshes_back_to_back(gpu):
    m1, m2 = MR.sphere3d(), _second_mesh()
    M1, M2 = _persp(), MR.perspective(W, H, **M_SECOND)
    want = MR.oracle_frame(W, H, False, "zw", [(m1, M1), (m2, M2)], ct=CT)
    assert not scenes.bits_equal(want[0], _want("gouraud", "zw", False)[1][0])
    ctx = _ctx(gpu, "zw", False, CT)
    ctx.draw_mesh(_gpu_mesh(m1), M1)
    ctx.draw_mesh(_gpu_mesh(m2), M2)   # (no flush between them)
    _same(MR.read_frame(ctx, "zw"), want, "two meshes")


def test_one_mesh_on_two_contexts(gpu):
    mesh = MR.sphere3d()
    M1, M2 = _persp(), MR.perspective(W, H, **M_SECOND)
    gm = _gpu_mesh(mesh)
    c1, c2 = _ctx(gpu, "zw", False, CT), _ctx(gpu, "zw", True, CT)
    c1.draw_mesh(gm, M1)
    c2.draw_mesh(gm, M2)
    c1.draw_mesh(gm, M2)
    _same(MR.read_frame(c2, "zw"), MR.oracle_frame(W, H, True, "zw", [(mesh, M2)], ct=CT), "second context")
    _same(MR.read_frame(c1, "zw"), MR.oracle_frame(W, H, False, "zw", [(mesh, M1), (mesh, M2)], ct=CT),
          "first context")


def test_three_frames_under_three_matrices(gpu):
    mesh = MR.sphere3d()
    gm = _gpu_mesh(mesh)
    ctx = gpu.context(W, H, False)
    frames = []
    for k in range(3):
        M = MR.perspective(W, H, ax=0.3 + 0.4 * k, ay=0.5 - 0.7 * k)
        MR.begin_frame(ctx, "zw", MR.XFORM, CT)
        ctx.draw_mesh(gm, M)
        frames.append(MR.read_frame(ctx, "zw"))
        _same(frames[-1], MR.oracle_frame(W, H, False, "zw", [(mesh, M)], ct=CT), f"frame {k}")
    assert not scenes.bits_equal(frames[0][0], frames[1][0]) and not scenes.bits_equal(frames[1][0], frames[2][0])


def test_overflow_rerun_reads_the_staging(gpu):
    mesh, want = _want("gouraud", "zw", False)
    ctx = _ctx(gpu, "zw", False, CT)
    ctx.set_pair_capacity_override(50)
    ctx.draw_mesh(_gpu_mesh(mesh), _persp())
    _same(MR.read_frame(ctx, "zw"), want, "overflow re-run")
    # ... and a second mesh drawn while the first batch's re-run is still due
    m2, M2 = _second_mesh(), MR.perspective(W, H, **M_SECOND)
    ctx = _ctx(gpu, "zw", False, CT)
    ctx.set_pair_capacity_override(50)
    ctx.draw_mesh(_gpu_mesh(mesh), _persp())
    ctx.draw_mesh(_gpu_mesh(m2), M2)
    _same(MR.read_frame(ctx, "zw"), MR.oracle_frame(W, H, False, "zw", [(mesh, _persp()), (m2, M2)], ct=CT),
          "overflow re-run before the next mesh")


def test_recorded_commands_run_before_the_mesh(gpu):
    mesh = MR.sphere3d()
    rect = (20.0, 15.0, 70.0, 50.0, 0.1, 0.9, 0.2, 1.0)
    want = MR.oracle_frame(W, H, False, "zw", [(mesh, _persp())], ct=CT, before=lambda c: c.draw_rect(*rect))
    rect_only = MR.oracle_frame(W, H, False, "zw", [], ct=CT, before=lambda c: c.draw_rect(*rect))
    assert not scenes.bits_equal(want[0], rect_only[0])
    assert not scenes.bits_equal(want[0], _want("gouraud", "zw", False)[1][0])   # (the rectangle shows beside the mesh)
    ctx = _ctx(gpu, "zw", False, CT)
    ctx.begin_commands()
    ctx.draw_rect(*rect)
    ctx.draw_mesh(_gpu_mesh(mesh), _persp())
    ctx.end_commands()
    _same(MR.read_frame(ctx, "zw"), want, "recorded rectangle, then the mesh")


# ---- update_positions ---------------------------------------------------------
@pytest.mark.parametrize("override", [0, 50])
def test_update_positions(gpu, override):
    mesh = MR.sphere3d()
    moved = dict(mesh, pos=mesh["pos"] * np.array([0.6, 1.1, 0.8]) + np.array([0.3, -0.1, 0.0]))
    want = MR.oracle_frame(W, H, False, "zw", [(mesh, _persp()), (moved, _persp())], ct=CT)
    assert not scenes.bits_equal(want[0], _want("gouraud", "zw", False)[1][0])
    gm = _gpu_mesh(mesh)
    ctx = _ctx(gpu, "zw", False, CT)
    ctx.set_pair_capacity_override(override)
    ctx.draw_mesh(gm, _persp())            # pending across the update: keeps the old positions
    gm.update_positions(moved["pos"])
    ctx.draw_mesh(gm, _persp())
    _same(MR.read_frame(ctx, "zw"), want, "update_positions")
    xy, z = ctx.assemble_mesh(gm, _persp())
    wxy, wz, _ = MR.expand(moved, _persp())
    assert scenes.bits_equal(xy, wxy) and scenes.bits_equal(z, wz)
    with pytest.raises(ValueError):
        gm.update_positions(moved["pos"][:-1])


# ---- errors ---------------------------------------------------------------------
def _expect_error(R, ctx, before, what, call):
    R.lib.ClearLastError()
    assert not R.lib.GetLastErrorString()
    try:
        assert not call(), what
        assert R.lib.GetLastErrorString(), what
    finally:
        R.lib.ClearLastError()
    assert scenes.bits_equal(ctx.get_buffer_numpy(), before), what


def test_creation_errors(gpu):
    R = _R()
    mesh = MR.sphere3d()
    nv = mesh["pos"].shape[0]
    ctx = _ctx(gpu, "nz")
    before = ctx.get_buffer_numpy()
    bad = mesh["idx"].copy()
    bad[7, 1] = nv                          # one past the last vertex
    pos, idx, col = (np.ascontiguousarray(a) for a in (mesh["pos"], mesh["idx"], mesh["colors"]))
    P = lambda a: a.ctypes.data
    n = idx.shape[0]
    uv = np.zeros((nv, 2))
    for what, call in {
        "index == nv": lambda: R.lib.CreateMesh(nv, P(pos), n, P(bad), P(col), True),
        "index == nv, textured": lambda: R.lib.CreateTexturedMesh(nv, P(pos), n, P(bad), P(uv)),
        "NULL rgba": lambda: R.lib.CreateMesh(nv, P(pos), n, P(idx), None, True),
        "NULL uv": lambda: R.lib.CreateTexturedMesh(nv, P(pos), n, P(idx), None),
    }.items():
        _expect_error(R, ctx, before, what, call)
    with pytest.raises(RuntimeError, match="index out of range"):
        R.Mesh(mesh["pos"], bad, colors=mesh["colors"])
    R.lib.ClearLastError()
    with pytest.raises(ValueError):
        R.Mesh(mesh["pos"], mesh["idx"])
    with pytest.raises(ValueError):
        R.Mesh(mesh["pos"], -mesh["idx"].astype(np.int64), colors=mesh["colors"])
    assert not R.lib.GetLastErrorString()


def test_wrong_draw_call_for_the_mesh_kind(gpu):
    R = _R()
    colour, textured = _gpu_mesh(MR.sphere3d()), _gpu_mesh(MR.sphere3d(uv_size=(37, 23)))
    tex = gpu.texture(T.texture_rgb())
    ctx = _ctx(gpu, "nz")
    before = ctx.get_buffer_numpy()
    for what, call in {
        "colour mesh in DrawTexturedMesh": lambda: R.lib.DrawTexturedMesh(ctx._ptr, colour._ptr, tex._ptr, None),
        "textured mesh in DrawMesh": lambda: R.lib.DrawMesh(ctx._ptr, textured._ptr, None),
        "NULL texture": lambda: R.lib.DrawTexturedMesh(ctx._ptr, textured._ptr, None, None),
        "NULL mesh": lambda: R.lib.DrawMesh(ctx._ptr, None, None),
    }.items():
        _expect_error(R, ctx, before, what, call)
    with pytest.raises(ValueError):
        ctx.draw_mesh(textured)
    with pytest.raises(ValueError):
        ctx.draw_mesh(colour, texture=tex)
    # and the context still draws
    ctx.draw_mesh(colour, _persp())
    assert not scenes.bits_equal(ctx.get_buffer_numpy(), before)
    assert not R.lib.GetLastErrorString()


def test_empty_mesh_draws_nothing(gpu):
    R = _R()
    mesh = MR.sphere3d()
    ctx = _ctx(gpu, "zw")
    before = MR.read_frame(ctx, "zw")
    for gm in (R.Mesh(mesh["pos"], np.zeros((0, 3), dtype=np.uint32), colors=mesh["colors"]),
               R.Mesh(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.uint32), colors=np.zeros((0, 4))),
               R.Mesh(mesh["pos"], np.zeros((0, 3), dtype=np.uint32), uv=np.zeros((mesh["pos"].shape[0], 2)))):
        assert gm.triangle_count == 0
        ctx.draw_mesh(gm, _persp(), texture=gpu.texture(T.texture_rgb()) if gm.textured else None)
        xy, z = ctx.assemble_mesh(gm, _persp())
        assert xy.shape == (0, 6) and z.shape == (0, 3)
    _same(MR.read_frame(ctx, "zw"), before, "empty meshes")
    assert not R.lib.GetLastErrorString()


def test_repeated_index_is_dropped(gpu):
    mesh = MR.sphere3d()
    idx = mesh["idx"].copy()
    idx[::3, 2] = idx[::3, 0]               # den == 0
    idx[1::6, 1] = idx[1::6, 2]
    bad = dict(mesh, idx=idx)
    assert (~MR.kept(MR.expand(bad, _persp())[0], MR.XFORM)).sum() >= 150
    want = MR.oracle_frame(W, H, False, "zw", [(bad, _persp())], ct=CT)
    assert not np.array_equal(want[1], _want("gouraud", "zw", False)[1][1])
    for force in (False, True):
        ctx = _ctx(gpu, "zw", False, CT)
        ctx.set_force_ordered_raster(force)
        ctx.draw_mesh(_gpu_mesh(bad), _persp())
        _same(MR.read_frame(ctx, "zw"), want, f"repeated indices, force={force}")

"""Lit mesh draws on the GPU, bit for bit (DESIGN.md §3 "Vertex lighting"): the
soups of assemble_mesh_lit and assemble_mesh_lit_instanced against the numpy
reference (tests/mesh_light_ref.py); draw_mesh_lit and draw_mesh_lit_instanced
(f64 framebuffer, u32 depth) against the CPU oracle's frame of the reference's
soups -- both rasters, Gouraud and flat, the colour transform, the clip stage,
tints, the device variant; the lifetime of the staging that holds the lit
colours; the identities with the unlit draws; the error cases and the two shape
extremes.  The scene's own conditions are checked on the CPU in
tests/test_mesh_light_ref.py."""
import ctypes
import functools

import numpy as np
import pytest

import mesh_inst_ref as MI
import mesh_light_ref as ML
import mesh_ref as MR
import scenes

pytestmark = pytest.mark.gpu

W, H = MI.W, MI.H
CT = (0.9, 0.8, 0.7, 1.0)
NEAR = MI.NEAR
FAR = 0xFFFFFFFF
A, LIGHTS = ML.AMBIENT, ML.LIGHTS
A2, LIGHTS2 = (0.4, 0.05, 0.1), np.array([[0.0, 0.6, 0.8, 0.2, 1.5, 0.7]])   # the "different lights" of the tests


def _R():
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    return R


def _gpu_mesh(mesh, lit=True):
    return _R().Mesh(mesh["pos"], mesh["idx"], colors=mesh["colors"], gouraud=mesh["gouraud"],
                     normals=mesh["normals"] if lit else None)


def _same(got, want, what):
    assert scenes.bits_equal(got[0], want[0]), (what, scenes.first_mismatch(got[0], want[0]))
    if want[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "depth", scenes.first_mismatch(got[1], want[1]))


def _soup_same(got, want, what, exact=True):
    for g, w, name in zip(got, want, ("xy", "z", "attr")):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        # positions follow the sibling tests: a division's NaN payload is not specified, the colours' bits are
        ok = scenes.bits_equal(g, w) if exact or name == "attr" else np.array_equal(g, w, equal_nan=True)
        assert ok, (what, name, scenes.first_mismatch(g, w))


def _frozen(want):
    for a in want:
        if a is not None:
            a.setflags(write=False)
    return want


def _ctx(gpu, mode, alpha=False, ct=CT, clear=MR.CLEAR, near=0.0, cull=0, force=False, ambient=A, lights=LIGHTS):
    ctx = gpu.context(W, H, alpha)
    MR.begin_frame(ctx, mode, MR.XFORM, ct, clear=clear)
    ctx.set_mesh_near_plane(near)
    ctx.set_mesh_cull(cull)
    ctx.set_force_ordered_raster(force)
    ctx.set_mesh_lights(ambient, lights)
    return ctx


def _mesh(kind):
    return {"gouraud": ML.lit_sphere3d, "flat": lambda: ML.lit_sphere3d(gouraud=False),
            "blended": lambda: ML.lit_sphere3d(alpha=(0.2, 0.9))}[kind]()


def _persp():
    return MR.perspective(W, H)


ROT = ML.rotation3()


@functools.lru_cache(maxsize=None)
def _want(kind, mode, alpha, rotated=True, near=0.0, cull=0, clear=MR.CLEAR, ct=CT, behind=False):
    """Oracle frame of one lit draw of the shared sphere under the shared lights."""
    lm = ML.lit_mesh(_mesh(kind), ROT if rotated else None, A, LIGHTS)
    M = MR.behind_eye(W, H) if behind else _persp()
    return _frozen(ML.oracle_frame(W, H, alpha, mode, [(lm, M)], near, cull, ct=ct, clear=clear))


# ---- 1. the soup of a single draw against the reference ---------------------------
@pytest.mark.parametrize("nv", [1, 3, 255, 256, 257, 1000])
def test_soup_matches_the_reference(gpu, nv):
    ctx = gpu.context(8, 8, False)
    M = MR.perspective(W, H, d=2.5)
    clamped = back = 0
    for n in sorted({1, max(1, nv // 3), 2 * nv - 1}):
        mesh = ML.random_lit_mesh(nv, n, seed=100 * nv + n)
        gms = {True: _gpu_mesh(mesh), False: _gpu_mesh(dict(mesh, gouraud=False))}
        for nl in (0, 1, 3, 8):
            amb, lights = ML.random_lights(nl, seed=nv + nl)
            ctx.set_mesh_lights(amb, lights)
            assert ctx.get_mesh_light_count() == nl
            for N in (None, ROT):
                lit = ML.lit_colors(mesh, N, amb, lights)
                clamped += int((lit[:, :3] == 1.0).sum())
                for gouraud in (True, False):
                    what = (nv, n, nl, N is not None, gouraud)
                    got = ctx.assemble_mesh_lit(gms[gouraud], M, N)
                    _soup_same(got, ML.lit_soup(dict(mesh, gouraud=gouraud), M, N, amb, lights), what, exact=False)
                    assert got[2].shape == (n, 12 if gouraud else 4)
            if nl:
                back += int((ML.lit_colors(mesh, None, (0, 0, 0), lights[:1])[:, :3] == 0).all(axis=1).sum())
    assert (back > 0 and clamped > 0) or nv < 255


def test_soup_with_nan_and_huge_normals_and_a_negative_light(gpu):
    mesh = ML.random_lit_mesh(300, 500, seed=12)
    mesh["normals"][7] = np.nan
    mesh["normals"][8] = (np.inf, 0.0, 0.0)
    mesh["normals"][9] = (1e300, -1e300, 1e300)
    mesh["normals"][10] = (1e308, 1e308, 1e308)           # the dot overflows to +inf: inf * colour, then the clamp
    mesh["colors"][11, 0] = np.nan                         # a NaN product stays NaN
    lights = LIGHTS.copy()
    lights[1, 3:] = (-0.7, -2.0, 0.3)
    want = ML.lit_soup(mesh, None, ROT, A, lights)
    lit = ML.lit_colors(mesh, ROT, A, lights)
    assert np.isfinite(lit[[7, 8]]).all() and np.isnan(lit[11, 0]) and (lit[:, :3] == 0.0).any()
    ctx = gpu.context(8, 8, False)
    ctx.set_mesh_lights(A, lights)
    for gouraud in (True, False):
        m = dict(mesh, gouraud=gouraud)
        _soup_same(ctx.assemble_mesh_lit(_gpu_mesh(m), None, ROT), ML.lit_soup(m, None, ROT, A, lights), gouraud)
    assert np.isnan(want[2]).any()


# ---- 2. the soup of an instanced draw ------------------------------------------------
def _normal_matrices(K, seed):
    g = scenes.rng(seed)
    return np.stack([ML.rotation3(g.uniform(-3, 3), g.uniform(-3, 3)) for _ in range(K)])


@pytest.mark.parametrize("nv,K", [(3, 100), (187, 7), (257, 3)])
def test_instanced_soup_matches_the_reference(gpu, nv, K):
    ctx = gpu.context(8, 8, False)
    ctx.set_mesh_lights(A, LIGHTS)
    mesh = ML.lit_sphere3d() if nv == 187 else ML.random_lit_mesh(nv, 2 * nv - 1, seed=nv)
    g = scenes.rng(K)
    mats = np.stack([MR.affine(W, H, ax=g.uniform(-1, 1), ay=g.uniform(-1, 1), scale=g.uniform(0.2, 0.5))
                     for _ in range(K)])
    normals, tint = _normal_matrices(K, nv), g.uniform(0.1, 1.0, size=(K, 4))
    n = mesh["idx"].shape[0]
    for gouraud in (True, False):
        m = dict(mesh, gouraud=gouraud)
        gm = _gpu_mesh(m)
        for nm in (None, normals):
            for t in (None, tint):
                what = (nv, K, gouraud, nm is not None, t is not None)
                got = ctx.assemble_mesh_lit_instanced(gm, mats, nm, t)
                _soup_same(got, ML.lit_instanced_soup(m, mats, nm, t, A, LIGHTS), what)
        # instance k's colours come from normal matrix k: its slice is the single draw's soup under that matrix
        attr = ctx.assemble_mesh_lit_instanced(gm, mats, normals)[2]
        for k in (0, K // 2, K - 1):
            one = ctx.assemble_mesh_lit(gm, mats[k], normals[k])[2]
            assert scenes.bits_equal(attr[k * n:(k + 1) * n], one), (nv, K, gouraud, k)
        assert not scenes.bits_equal(attr[:n], attr[n:2 * n])


# ---- 3. frames against the oracle ------------------------------------------------------
def _draw_case(gpu, kind, mode, alpha, path, what, rotated=True, **state):
    ctx = _ctx(gpu, mode, alpha, **state)
    ctx.draw_mesh_lit(_gpu_mesh(_mesh(kind)), _persp(), ROT if rotated else None)
    assert ctx.last_raster_path() == path, what
    assert ctx.mesh_last_triangle_count == 320
    got = MR.read_frame(ctx, mode)
    _same(got, _want(kind, mode, alpha, rotated, ct=state.get("ct", CT)), what)
    return got


@pytest.mark.parametrize("alpha", [False, True])
def test_gouraud_opaque_depth_write(gpu, alpha):
    got = _draw_case(gpu, "gouraud", "zw", alpha, "order-free", f"lit gouraud alpha={alpha}")
    unlit = MR.oracle_frame(W, H, alpha, "zw", [(_mesh("gouraud"), _persp())], ct=CT)
    assert not scenes.bits_equal(got[0], unlit[0]) and np.array_equal(got[1], unlit[1])
    assert not scenes.bits_equal(got[0], _want("gouraud", "zw", alpha, False)[0])     # the normal matrix shows


def test_flat_takes_the_lit_colour_of_the_first_index(gpu):
    got = _draw_case(gpu, "flat", "zw", False, "order-free", "lit flat")
    assert not scenes.bits_equal(got[0], _want("gouraud", "zw", False)[0])


@pytest.mark.parametrize("mode", ["zt", "nz"])
def test_translucent_vertex_alpha_takes_the_ordered_raster(gpu, mode):
    _draw_case(gpu, "blended", mode, True, "ordered", f"lit blended {mode}")


def test_forced_ordered_raster_gives_the_same_frame(gpu):
    _draw_case(gpu, "gouraud", "zw", False, "ordered", "forced ordered", force=True)


def test_context_colour_transform(gpu):
    ct = (0.5, 1.0, 0.25, 1.0)
    got = _draw_case(gpu, "gouraud", "zw", False, "order-free", "colour transform", ct=ct)
    assert not scenes.bits_equal(got[0], _want("gouraud", "zw", False)[0])


@pytest.mark.parametrize("near,cull", [(NEAR, 1), (NEAR, 2), (NEAR, 0), (0.0, 1)])
def test_near_plane_and_cull(gpu, near, cull):
    M = MR.behind_eye(W, H)
    for kind in ("gouraud", "flat"):
        mesh = _mesh(kind)
        gm = _gpu_mesh(mesh)
        want_soup = ML.lit_soup(mesh, M, ROT, A, LIGHTS, near, cull)
        count = want_soup[0].shape[0]
        assert 0 < count != 320
        ctx = _ctx(gpu, "zw", False, clear=FAR, near=near, cull=cull)
        _soup_same(ctx.assemble_mesh_lit(gm, M, ROT), want_soup, (kind, near, cull))
        ctx.draw_mesh_lit(gm, M, ROT)
        assert ctx.mesh_last_triangle_count == count
        _same(MR.read_frame(ctx, "zw"), _want(kind, "zw", False, True, near, cull, FAR, behind=True), (kind, near, cull))


# ---- 4. instanced frames ------------------------------------------------------------------
def _scene_normals():
    return _normal_matrices(MI.scene_matrices().shape[0], seed=21)


@functools.lru_cache(maxsize=None)
def _inst_want(kind, mode, alpha, tint=None, near=0.0, cull=0, clear=MR.CLEAR):
    mats = MI.scene_matrices()
    K = mats.shape[0]
    t = {None: None, "opaque": MI.scene_tints(K), "alpha": MI.scene_tints(K, alpha=(2, 0.5))}[tint]
    draws = ML.instance_meshes(_mesh(kind), mats, _scene_normals(), t, A, LIGHTS)
    return t, _frozen(ML.oracle_frame(W, H, alpha, mode, draws, near, cull, ct=CT, clear=clear))


@pytest.mark.parametrize("tint,path", [(None, "order-free"), ("opaque", "order-free"), ("alpha", "ordered")])
def test_instanced(gpu, tint, path):
    mats, normals = MI.scene_matrices(), _scene_normals()
    t, want = _inst_want("gouraud", "zw", True, tint)
    ctx = _ctx(gpu, "zw", True)
    ctx.draw_mesh_lit_instanced(_gpu_mesh(_mesh("gouraud")), mats, normals, t)
    assert ctx.last_raster_path() == path and ctx.mesh_last_triangle_count == mats.shape[0] * 320
    got = MR.read_frame(ctx, "zw")
    _same(got, want, f"instanced, tint={tint}")
    other = _inst_want("gouraud", "zw", True, None if tint else "opaque")[1]
    assert not scenes.bits_equal(got[0], other[0])


def test_instanced_flat_and_clipped(gpu):
    mats, normals = MI.scene_matrices(), _scene_normals()
    for kind, tint in (("flat", None), ("gouraud", "opaque"), ("flat", "opaque")):
        t, want = _inst_want(kind, "zw", False, tint, NEAR, 1, FAR)
        mesh = _mesh(kind)
        counts = []
        want_soup = ML.lit_instanced_soup(mesh, mats, normals, t, A, LIGHTS, NEAR, 1, counts=counts)
        assert 0 < sum(counts) != mats.shape[0] * 320
        ctx = _ctx(gpu, "zw", False, clear=FAR, near=NEAR, cull=1)
        gm = _gpu_mesh(mesh)
        _soup_same(ctx.assemble_mesh_lit_instanced(gm, mats, normals, t), want_soup, (kind, tint))
        ctx.draw_mesh_lit_instanced(gm, mats, normals, t)
        assert ctx.mesh_last_triangle_count == sum(counts)
        _same(MR.read_frame(ctx, "zw"), want, (kind, tint, "clipped"))
    t, want = _inst_want("flat", "zw", False)
    ctx = _ctx(gpu, "zw", False)
    ctx.draw_mesh_lit_instanced(_gpu_mesh(_mesh("flat")), mats, normals)
    _same(MR.read_frame(ctx, "zw"), want, "instanced flat")


def _device(a, dev, pad):
    """`a` inside a larger device tensor, `pad` doubles in: (the whole tensor, the view)."""
    import torch
    flat = torch.from_numpy(np.array(a, dtype=np.float64).ravel())
    big = torch.full((flat.numel() + 2 * pad + 2,), float("nan"), dtype=torch.float64, device=dev)
    view = big[pad:pad + flat.numel()]
    view.copy_(flat)
    torch.cuda.synchronize(dev)
    return big, view


@pytest.mark.parametrize("tint", [None, "opaque", "alpha"])
def test_device_pointers_at_an_offset(gpu, tint):
    mats, normals = MI.scene_matrices(), _scene_normals()
    t, want = _inst_want("gouraud", "zw", True, tint)
    ctx = _ctx(gpu, "zw", True)
    dev = f"cuda:{ctx.device}"
    keep = [_device(mats, dev, 5), _device(normals, dev, 3), (None, None) if t is None else _device(t, dev, 7)]
    ctx.draw_mesh_lit_instanced_device(_gpu_mesh(_mesh("gouraud")), keep[0][1], mats.shape[0],
                                       normal_matrices=keep[1][1], tint=keep[2][1])
    assert ctx.last_raster_path() == ("ordered" if tint == "alpha" else "order-free")
    _same(MR.read_frame(ctx, "zw"), want, f"device pointers, tint={tint}")
    # NULL normal matrices on the device path: the identity
    ctx = _ctx(gpu, "zw", True)
    ctx.draw_mesh_lit_instanced_device(_gpu_mesh(_mesh("gouraud")), keep[0][1], mats.shape[0])
    host = _ctx(gpu, "zw", True)
    host.draw_mesh_lit_instanced(_gpu_mesh(_mesh("gouraud")), mats)
    _same(MR.read_frame(ctx, "zw"), MR.read_frame(host, "zw"), "device, no normal matrices")


# ---- 5. lifetime of the staging and of the light state -----------------------------------
def _second_mesh():
    mesh = ML.lit_sphere3d(rows=13, cols=21, seed=8)
    mesh["pos"] = mesh["pos"] * 0.6 + np.array([0.0, 0.3, -0.8])
    return mesh


def test_two_lit_draws_back_to_back_under_different_lights(gpu):
    m1, m2 = _mesh("gouraud"), _second_mesh()
    M2 = MR.perspective(W, H, d=3.0, ax=-0.4, ay=1.1)
    draws = [(ML.lit_mesh(m1, ROT, A, LIGHTS), _persp()), (ML.lit_mesh(m2, None, A2, LIGHTS2), M2)]
    want = MR.oracle_frame(W, H, False, "zw", draws, ct=CT)
    wrong = MR.oracle_frame(W, H, False, "zw", [(ML.lit_mesh(m1, ROT, A2, LIGHTS2), _persp()), draws[1]], ct=CT)
    assert not scenes.bits_equal(want[0], wrong[0])
    for cap in (0, 50):                                   # 50: the first batch overflows, its re-run reads the staging
        ctx = _ctx(gpu, "zw", False)
        ctx.set_pair_capacity_override(cap)
        ctx.draw_mesh_lit(_gpu_mesh(m1), _persp(), ROT)
        ctx.set_mesh_lights(A2, LIGHTS2)                  # (no flush: the pending batch keeps the colours it was issued with)
        ctx.draw_mesh_lit(_gpu_mesh(m2), M2)              # a larger mesh: the staging is regrown
        _same(MR.read_frame(ctx, "zw"), want, f"two lit draws, capacity override {cap}")


def test_one_mesh_lit_on_two_contexts(gpu):
    gm = _gpu_mesh(_mesh("gouraud"))
    c1, c2 = _ctx(gpu, "zw", False), _ctx(gpu, "zw", False, ambient=A2, lights=LIGHTS2)
    c1.draw_mesh_lit(gm, _persp(), ROT)
    c2.draw_mesh_lit(gm, _persp(), ROT)
    want2 = MR.oracle_frame(W, H, False, "zw", [(ML.lit_mesh(_mesh("gouraud"), ROT, A2, LIGHTS2), _persp())], ct=CT)
    _same(MR.read_frame(c2, "zw"), want2, "second context")
    _same(MR.read_frame(c1, "zw"), _want("gouraud", "zw", False), "first context")
    assert not scenes.bits_equal(want2[0], _want("gouraud", "zw", False)[0])


def test_overflow_rerun_reads_the_lit_staging(gpu):
    ctx = _ctx(gpu, "zw", False)
    ctx.set_pair_capacity_override(50)
    ctx.draw_mesh_lit(_gpu_mesh(_mesh("gouraud")), _persp(), ROT)
    ctx.set_mesh_lights(None, None)
    _same(MR.read_frame(ctx, "zw"), _want("gouraud", "zw", False), "overflow re-run")
    mats, normals = MI.scene_matrices(), _scene_normals().copy()
    t, want = _inst_want("gouraud", "zw", False, "opaque")
    ctx = _ctx(gpu, "zw", False)
    ctx.set_pair_capacity_override(50)
    ctx.draw_mesh_lit_instanced(_gpu_mesh(_mesh("gouraud")), mats, normals, t)
    normals[:] = np.nan                                   # the caller's arrays are its own again
    _same(MR.read_frame(ctx, "zw"), want, "instanced overflow re-run, arrays rewritten")


def test_updated_normals_and_positions(gpu):
    mesh = _mesh("gouraud")
    gm = _gpu_mesh(mesh)
    ctx = _ctx(gpu, "zw", False)
    ctx.draw_mesh_lit(gm, _persp(), ROT)
    moved = dict(mesh, normals=np.ascontiguousarray(mesh["normals"][:, [2, 0, 1]] * np.array([1.0, -1.0, 1.0])),
                 pos=mesh["pos"] * np.array([0.8, 1.1, 0.9]))
    gm.update_normals(moved["normals"])                   # (the draw already issued keeps the old ones)
    gm.update_positions(moved["pos"])
    _same(MR.read_frame(ctx, "zw"), _want("gouraud", "zw", False), "issued before the update")
    ctx = _ctx(gpu, "zw", False)
    ctx.draw_mesh_lit(gm, _persp(), ROT)
    want = MR.oracle_frame(W, H, False, "zw", [(ML.lit_mesh(moved, ROT, A, LIGHTS), _persp())], ct=CT)
    assert not scenes.bits_equal(want[0], _want("gouraud", "zw", False)[0])
    _same(MR.read_frame(ctx, "zw"), want, "after update_normals and update_positions")
    assert gm.lit and not _gpu_mesh(mesh, lit=False).lit


def test_recorded_commands_run_before_a_lit_draw(gpu):
    rect = (20.0, 15.0, 70.0, 50.0, 0.1, 0.9, 0.2, 1.0)
    lm = ML.lit_mesh(_mesh("gouraud"), ROT, A, LIGHTS)
    want = MR.oracle_frame(W, H, False, "zw", [(lm, _persp())], ct=CT, before=lambda c: c.draw_rect(*rect))
    assert not scenes.bits_equal(want[0], _want("gouraud", "zw", False)[0])
    ctx = _ctx(gpu, "zw", False)
    ctx.begin_commands()
    ctx.draw_rect(*rect)
    ctx.draw_mesh_lit(_gpu_mesh(_mesh("gouraud")), _persp(), ROT)
    ctx.end_commands()
    _same(MR.read_frame(ctx, "zw"), want, "recorded rectangle, then the lit mesh")


# ---- 6. identities ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode,alpha", [("gouraud", "zw", False), ("flat", "zw", True), ("blended", "zt", True)])
def test_default_lights_are_draw_mesh_bit_for_bit(gpu, kind, mode, alpha):
    mesh = _mesh(kind)
    for near in (0.0, NEAR):
        M = MR.behind_eye(W, H) if near else _persp()
        lit = _ctx(gpu, mode, alpha, near=near, ambient=None, lights=None)
        assert lit.get_mesh_light_count() == 0
        lit.draw_mesh_lit(_gpu_mesh(mesh), M, ROT)
        plain = _ctx(gpu, mode, alpha, near=near)
        plain.draw_mesh(_gpu_mesh(mesh, lit=False), M)
        _same(MR.read_frame(lit, mode), MR.read_frame(plain, mode), (kind, near, "default lights"))
        assert lit.mesh_last_triangle_count == plain.mesh_last_triangle_count
        # ... and draw_mesh of the lit mesh ignores its normals and the lights
        unlit = _ctx(gpu, mode, alpha, near=near)
        unlit.draw_mesh(_gpu_mesh(mesh), M)
        _same(MR.read_frame(unlit, mode), MR.read_frame(plain, mode), (kind, near, "draw_mesh of a lit mesh"))
    mats = MI.scene_matrices()
    a, b = _ctx(gpu, mode, alpha), _ctx(gpu, mode, alpha)
    a.draw_mesh_instanced(_gpu_mesh(mesh), mats)
    b.draw_mesh_instanced(_gpu_mesh(mesh, lit=False), mats)
    _same(MR.read_frame(a, mode), MR.read_frame(b, mode), (kind, "draw_mesh_instanced of a lit mesh"))


def test_light_state_is_not_saved_or_restored(gpu):
    fresh = gpu.context(W, H, False)
    assert fresh.get_mesh_light_count() == 0
    ctx = _ctx(gpu, "zw", False, ambient=None, lights=None)
    ctx.save_state()
    ctx.set_mesh_lights(A, LIGHTS)
    ctx.restore_state()
    assert ctx.get_mesh_light_count() == 3
    ctx.draw_mesh_lit(_gpu_mesh(_mesh("gouraud")), _persp(), ROT)
    _same(MR.read_frame(ctx, "zw"), _want("gouraud", "zw", False), "lights set between save and restore")


# ---- 7. errors ---------------------------------------------------------------------------------
def _expect_error(R, ctx, before, what, call, name):
    R.lib.ClearLastError()
    assert not R.lib.GetLastErrorString()
    try:
        assert not call(), what
        assert R.lib.GetLastErrorString().decode().startswith(name + ":"), (what, R.lib.GetLastErrorString())
    finally:
        R.lib.ClearLastError()
    assert ctx.mesh_last_triangle_count == 0, what
    assert scenes.bits_equal(ctx.get_buffer_numpy(), before), what


def test_errors_draw_nothing(gpu):
    R = _R()
    mesh = _mesh("gouraud")
    lit, unlit = _gpu_mesh(mesh), _gpu_mesh(mesh, lit=False)
    tex_mesh = MR.sphere3d(uv_size=(37, 23))
    textured = R.Mesh(tex_mesh["pos"], tex_mesh["idx"], uv=tex_mesh["uv"])
    mats = np.ascontiguousarray(MI.scene_matrices())
    M = np.ascontiguousarray(mats[MI.OFFSCREEN])
    P = lambda a: a.ctypes.data
    ctx = _ctx(gpu, "nz")
    before = ctx.get_buffer_numpy()
    n_out = np.zeros(1, dtype=np.int64)
    out = np.zeros(6400 * 12)
    lib, c = R.lib, ctx._ptr
    draws = {
        "DrawMeshLit": {
            "an unlit mesh": lambda: lib.DrawMeshLit(c, unlit._ptr, P(M), None),
            "a textured mesh": lambda: lib.DrawMeshLit(c, textured._ptr, P(M), None),
            "NULL mesh": lambda: lib.DrawMeshLit(c, None, P(M), None),
        },
        "DrawMeshLitInstanced": {
            "an unlit mesh": lambda: lib.DrawMeshLitInstanced(c, unlit._ptr, P(mats), None, None, 10),
            "a textured mesh": lambda: lib.DrawMeshLitInstanced(c, textured._ptr, P(mats), None, None, 10),
            "K < 0": lambda: lib.DrawMeshLitInstanced(c, lit._ptr, P(mats), None, None, -1),
            "NULL matrices": lambda: lib.DrawMeshLitInstanced(c, lit._ptr, None, None, None, 10),
        },
        "DrawMeshLitInstancedDevice": {
            "an unlit mesh": lambda: lib.DrawMeshLitInstancedDevice(c, unlit._ptr, None, None, None, 10),
            "K < 0": lambda: lib.DrawMeshLitInstancedDevice(c, lit._ptr, None, None, None, -2),
            "NULL matrices": lambda: lib.DrawMeshLitInstancedDevice(c, lit._ptr, None, None, None, 10),
        },
    }
    for name, cases in draws.items():
        for what, call in cases.items():
            ctx.draw_mesh(lit, M)                          # (the last count is 320 before every case)
            assert ctx.mesh_last_triangle_count == 320
            _expect_error(R, ctx, before, (name, what), call, name)
    assembles = {
        "AssembleMeshLit": {
            "an unlit mesh": lambda: lib.AssembleMeshLit(c, unlit._ptr, P(M), None, 640, P(out), P(out), P(out), P(n_out)),
            "a textured mesh": lambda: lib.AssembleMeshLit(c, textured._ptr, P(M), None, 640, P(out), P(out), P(out), P(n_out)),
            "negative cap": lambda: lib.AssembleMeshLit(c, lit._ptr, P(M), None, -1, P(out), P(out), P(out), P(n_out)),
            "NULL output": lambda: lib.AssembleMeshLit(c, lit._ptr, P(M), None, 640, P(out), None, P(out), P(n_out)),
            "NULL count": lambda: lib.AssembleMeshLit(c, lit._ptr, P(M), None, 640, P(out), P(out), P(out), None),
        },
        "AssembleMeshLitInstanced": {
            "an unlit mesh": lambda: lib.AssembleMeshLitInstanced(c, unlit._ptr, P(mats), None, None, 10, 6400, P(out), P(out),
                                                                   P(out), P(n_out)),
            "negative cap": lambda: lib.AssembleMeshLitInstanced(c, lit._ptr, P(mats), None, None, 10, -1, P(out), P(out),
                                                                  P(out), P(n_out)),
            "NULL output": lambda: lib.AssembleMeshLitInstanced(c, lit._ptr, P(mats), None, None, 10, 6400, None, P(out),
                                                                 P(out), P(n_out)),
            "K < 0": lambda: lib.AssembleMeshLitInstanced(c, lit._ptr, P(mats), None, None, -1, 6400, P(out), P(out), P(out),
                                                           P(n_out)),
            "NULL matrices": lambda: lib.AssembleMeshLitInstanced(c, lit._ptr, None, None, None, 10, 6400, P(out), P(out),
                                                                   P(out), P(n_out)),
        },
    }
    for name, cases in assembles.items():
        for what, call in cases.items():
            n_out[0] = -5
            lib.ClearLastError()
            assert not call(), (name, what)
            assert lib.GetLastErrorString().decode().startswith(name + ":"), (name, what)
            assert n_out[0] == (-5 if what == "NULL count" else 0), (name, what)
            lib.ClearLastError()
    # cap 0 asks for the count alone; a smaller cap copies the first triangles only
    assert lib.AssembleMeshLit(c, lit._ptr, P(np.ascontiguousarray(_persp())), None, 0, None, None, None, P(n_out))
    assert n_out[0] == 320
    out[:] = -1.0
    assert lib.AssembleMeshLit(c, lit._ptr, P(np.ascontiguousarray(_persp())), None, 2, P(out), P(out[100:]), P(out[200:]),
                               P(n_out))
    assert n_out[0] == 320 and (out[:12] != -1).all() and (out[12:100] == -1).all() and (out[224:] == -1).all()
    # the light state: errors leave it unchanged
    ctx.set_mesh_lights(A, LIGHTS)
    amb, lt = np.array(A2), np.ascontiguousarray(np.tile(LIGHTS2, (9, 1)))
    for what, call in {"nl = -1": lambda: lib.SetMeshLights(c, P(amb), P(lt), -1),
                       "nl = 9": lambda: lib.SetMeshLights(c, P(amb), P(lt), 9),
                       "NULL lights": lambda: lib.SetMeshLights(c, P(amb), None, 2)}.items():
        lib.ClearLastError()
        assert not call(), what
        assert lib.GetLastErrorString().decode().startswith("SetMeshLights:"), what
        lib.ClearLastError()
        assert ctx.get_mesh_light_count() == 3, what
    with pytest.raises(RuntimeError):
        ctx.set_mesh_lights(A2, lt)
    lib.ClearLastError()
    want = ML.lit_soup(mesh, _persp(), ROT, A, LIGHTS)
    _soup_same(ctx.assemble_mesh_lit(lit, _persp(), ROT), want, "state unchanged after the errors")
    # creation and update
    pos, idx, col = (np.ascontiguousarray(mesh[k]) for k in ("pos", "idx", "colors"))
    assert not lib.CreateLitMesh(187, P(pos), None, 320, P(idx), P(col), True)
    assert lib.GetLastErrorString().decode().startswith("CreateLitMesh:")
    lib.ClearLastError()
    assert not lib.UpdateMeshNormals(unlit._ptr, P(pos))
    assert lib.GetLastErrorString().decode().startswith("UpdateMeshNormals:")
    lib.ClearLastError()
    assert not lib.UpdateMeshNormals(lit._ptr, None) and lib.GetLastErrorString()
    lib.ClearLastError()
    # the binding raises before the call for the wrong mesh kind
    for bad in (unlit, textured):
        with pytest.raises(ValueError):
            ctx.draw_mesh_lit(bad, M)
        with pytest.raises(ValueError):
            ctx.draw_mesh_lit_instanced(bad, mats)
        with pytest.raises(ValueError):
            ctx.assemble_mesh_lit(bad, M)
    with pytest.raises(ValueError):
        ctx.draw_mesh_lit_instanced(lit, mats, normal_matrices=np.zeros((3, 9)))
    with pytest.raises(ValueError):
        R.Mesh(tex_mesh["pos"], tex_mesh["idx"], uv=tex_mesh["uv"], normals=mesh["normals"])
    assert not lib.GetLastErrorString()
    # empty draws are no errors, and the context still draws
    ctx.draw_mesh_lit_instanced(lit, np.zeros((0, 16)))
    empty = R.Mesh(mesh["pos"], np.zeros((0, 3), dtype=np.uint32), colors=mesh["colors"], normals=mesh["normals"])
    ctx.draw_mesh_lit(empty, M)
    assert empty.lit and ctx.mesh_last_triangle_count == 0 and not lib.GetLastErrorString()
    assert scenes.bits_equal(ctx.get_buffer_numpy(), before)
    ctx.draw_mesh_lit(lit, _persp(), ROT)
    assert not scenes.bits_equal(ctx.get_buffer_numpy(), before) and not lib.GetLastErrorString()


def test_mesh_on_another_device(gpu):
    R = _R()
    if R.device_count() < 2:
        pytest.skip("one device")
    try:
        assert R.set_device(1)
        other = _gpu_mesh(_mesh("gouraud"))
    finally:
        assert R.set_device(0)
    ctx = _ctx(gpu, "zw")
    before = ctx.get_buffer_numpy()
    M = np.ascontiguousarray(_persp())
    nout = ctypes.c_long(-1)
    out = np.zeros(640 * 12)
    P = lambda a: a.ctypes.data
    for what, call in {
        "draw": lambda: R.lib.DrawMeshLit(ctx._ptr, other._ptr, P(M), None),
        "instanced": lambda: R.lib.DrawMeshLitInstanced(ctx._ptr, other._ptr, P(M), None, None, 1),
        "assemble": lambda: R.lib.AssembleMeshLit(ctx._ptr, other._ptr, P(M), None, 640, P(out), P(out), P(out),
                                                  ctypes.byref(nout)),
    }.items():
        R.lib.ClearLastError()
        try:
            assert not call(), what
            assert "another device" in R.lib.GetLastErrorString().decode(), what
        finally:
            R.lib.ClearLastError()
    assert scenes.bits_equal(ctx.get_buffer_numpy(), before) and ctx.mesh_last_triangle_count == 0


# ---- 8. one larger shape each way -----------------------------------------------------------------
def test_three_thousand_instances_of_one_triangle(gpu):
    K = 3000
    g = scenes.rng(31)
    mesh = dict(pos=np.array([[-1.0, -0.8, 0.0], [1.0, -0.6, 0.1], [0.1, 0.9, -0.1]]),
                idx=np.array([[0, 1, 2]], dtype=np.uint32), colors=g.uniform(0.3, 1, size=(3, 4)), gouraud=True,
                normals=np.array([[0.0, 0.0, -1.0], [0.6, 0.0, -0.8], [0.0, 0.8, -0.6]]))
    mesh["colors"][:, 3] = 1.0
    Pm = MR.perspective(W, H).reshape(4, 4)
    mats = np.empty((K, 16))
    for k in range(K):
        Am = MI.translate(*(g.uniform(-1, 1, size=3) * (1.7, 1.2, 1.0)))
        Am[0, 0] = Am[1, 1] = Am[2, 2] = g.uniform(0.03, 0.15)
        mats[k] = (Pm @ Am).reshape(16)
    normals = _normal_matrices(K, seed=3)
    tint = g.uniform(0.2, 1.0, size=(K, 4))
    tint[:, 3] = 1.0
    want = MR.oracle_frame(W, H, False, "zw", ML.instance_meshes(mesh, mats, normals, tint, A, LIGHTS), ct=CT)
    assert (want[1] != MR.CLEAR).mean() > 0.3
    ctx = _ctx(gpu, "zw", False)
    ctx.draw_mesh_lit_instanced(_gpu_mesh(mesh), mats, normals, tint)
    assert ctx.last_raster_path() == "order-free" and ctx.mesh_last_triangle_count == K
    _same(MR.read_frame(ctx, "zw"), want, "3000 lit instances of one triangle")


def test_two_instances_of_three_thousand_triangles(gpu):
    mesh = ML.random_lit_mesh(1000, 3000, seed=5)
    mats = np.stack([MR.perspective(W, H, d=2.5), MR.perspective(W, H, d=3.5, ax=-0.7, ay=0.2)])
    normals = _normal_matrices(2, seed=4)
    for near in (0.0, 2.0):
        draws = ML.instance_meshes(mesh, mats, normals, None, A, LIGHTS)
        want = ML.oracle_frame(W, H, True, "zt", draws, near, 0, ct=CT)
        counts = []
        ML.lit_instanced_soup(mesh, mats, normals, None, A, LIGHTS, near, 0, counts=counts)
        ctx = _ctx(gpu, "zt", True, near=near)
        ctx.draw_mesh_lit_instanced(_gpu_mesh(mesh), mats, normals)
        assert ctx.last_raster_path() == "ordered"      # (random vertex alphas)
        assert ctx.mesh_last_triangle_count == sum(counts) and (near == 0 or sum(counts) != 6000)
        _same(MR.read_frame(ctx, "zt"), want, f"two large lit instances, near={near}")

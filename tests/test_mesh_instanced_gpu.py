"""Instanced mesh draws on the GPU, bit for bit (DESIGN.md §3 "Instanced mesh
draws"): the soup of assemble_mesh_instanced against the numpy reference
(tests/mesh_inst_ref.py) and against the single-mesh entry point instance by
instance; draw_mesh_instanced (f64 framebuffer, u32 depth) against the CPU
oracle's frame of the K single draws and against K draw_mesh calls on a second
context -- both rasters, every attribute kind, tints, the clip stage, the
perspective state and the texture filter; the device variant, the lifetime of
the staging and of the caller's arrays, the empty and error cases, and the two
shape extremes.  The scene's own conditions are checked on the CPU in
tests/test_mesh_inst_ref.py."""
import functools

import numpy as np
import pytest

import bilinear_ref as B
import mesh_inst_ref as MI
import mesh_ref as MR
import scenes
import textured_ref as T

pytestmark = pytest.mark.gpu

W, H = MI.W, MI.H
CT = (0.9, 0.8, 0.7, 1.0)
NEAR = MI.NEAR
FAR = 0xFFFFFFFF
I32 = 2 ** 31 - 1


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


def _frozen(want):
    for a in want:
        if a is not None:
            a.setflags(write=False)
    return want


def _ctx(gpu, mode, alpha=False, ct=CT, clear=MR.CLEAR, near=0.0, cull=0, persp=False, filt=0, force=False):
    ctx = gpu.context(W, H, alpha)
    MR.begin_frame(ctx, mode, MR.XFORM, ct, clear=clear)
    ctx.set_mesh_near_plane(near)
    ctx.set_mesh_cull(cull)
    ctx.set_mesh_perspective(persp)
    ctx.set_triangle_texture_filter(filt)
    ctx.set_force_ordered_raster(force)
    return ctx


def _mesh(kind):
    return {"gouraud": MR.sphere3d, "flat": lambda: MR.sphere3d(gouraud=False),
            "blended": lambda: MR.sphere3d(alpha=(0.2, 0.9)),
            "textured": lambda: MR.sphere3d(uv_size=(37, 23))}[kind]()


def _tint(name):
    """None, every alpha 1, or one instance (a random one that shows) at alpha 0.5."""
    K = MI.scene_matrices().shape[0]
    return {None: None, "opaque": MI.scene_tints(K), "alpha": MI.scene_tints(K, alpha=(2, 0.5))}[name]


@functools.lru_cache(maxsize=None)
def _want(kind, mode, alpha, tint=None, near=0.0, cull=0, clear=MR.CLEAR):
    """Oracle frame of the shared scene's K single draws."""
    return _frozen(MI.oracle_frame(W, H, alpha, mode, _mesh(kind), MI.scene_matrices(), _tint(tint), near, cull,
                                   ct=CT, clear=clear))


def _single_draws(gpu, mode, alpha, mesh, mats, tint=None, texture=None, **state):
    """The frame of K draw_mesh calls, one by one, on a context of its own."""
    ctx = _ctx(gpu, mode, alpha, **state)
    for m, M in MI.instance_meshes(mesh, mats, tint):
        ctx.draw_mesh(_gpu_mesh(m), M, texture=texture)
    return MR.read_frame(ctx, mode)


def _colour_case(gpu, kind, mode, alpha, path, tint=None, what="", **state):
    mesh, mats, t = _mesh(kind), MI.scene_matrices(), _tint(tint)
    ctx = _ctx(gpu, mode, alpha, **state)
    ctx.draw_mesh_instanced(_gpu_mesh(mesh), mats, tint=t)
    assert ctx.last_raster_path() == path, what
    assert ctx.mesh_last_triangle_count == mats.shape[0] * 320
    got = MR.read_frame(ctx, mode)
    _same(got, _want(kind, mode, alpha, tint), what + ": oracle")
    _same(got, _single_draws(gpu, mode, alpha, mesh, mats, t, **state), what + ": K draw_mesh calls")
    return got


# ---- 1. the soup against the reference -------------------------------------------
def _families(K, seed):
    g = scenes.rng(seed)
    persp = np.stack([MR.perspective(W, H, d=0.9 + 0.3 * g.uniform(), ax=g.uniform(-1, 1), ay=g.uniform(-1, 1))
                      for _ in range(K)])
    affine = np.stack([MR.affine(W, H, ax=g.uniform(-1, 1), ay=g.uniform(-1, 1), scale=g.uniform(0.2, 0.5))
                       for _ in range(K)])
    nan = persp.copy()
    nan[K // 2, 4:8] = np.nan            # row 1 of one instance: its y is NaN, the others' bits are untouched
    return {"perspective": persp, "affine": affine, "nan": nan}


def _eq(a, b, exact):
    return scenes.bits_equal(a, b) if exact else (a.shape == b.shape and np.array_equal(a, b, equal_nan=True))


@pytest.mark.parametrize("nv", [3, 64, 65, 300])
def test_soup_matches_the_reference(gpu, nv):
    ctx = gpu.context(8, 8, False)
    some_nan = False
    for n in (1, 85, 86, 257):           # (3n crosses 256 between 85 and 86)
        g = MR.random_mesh(nv, n, seed=1000 * nv + n)
        tex = dict(pos=g["pos"], idx=g["idx"], uv=scenes.rng(nv + n).uniform(-3, 40, size=(nv, 2)))
        kinds = {"gouraud": g, "flat": dict(g, gouraud=False), "textured": tex}
        gms = {k: _gpu_mesh(m) for k, m in kinds.items()}
        for K in (1, 2, 5, 64, 65):
            tint = scenes.rng(K).uniform(0.1, 1.0, size=(K, 4))
            for name, mats in _families(K, 7 * nv + n + K).items():
                exact = name == "affine"
                for kind, mesh in kinds.items():
                    variants = [(None, False), (None, True)] if kind == "textured" else [(None, False), (tint, False)]
                    for t, persp in variants:
                        what = (kind, nv, n, K, name, t is not None, persp)
                        ctx.set_mesh_perspective(persp)
                        xy, z, attr, q = ctx.assemble_mesh_instanced(gms[kind], mats, tint=t)
                        wxy, wz, wattr, wq = MI.instanced_soup(mesh, mats, t, persp=persp)
                        assert xy.shape == (K * n, 6), what
                        assert _eq(xy, wxy, exact) and _eq(z, wz, exact), what
                        assert scenes.bits_equal(attr, wattr), what
                        assert (q is None) == (wq is None) and (q is None or _eq(q, wq, exact)), what
                        some_nan = some_nan or bool(np.isnan(wxy).any())
                ctx.set_mesh_perspective(False)
                xy, z, _, _ = ctx.assemble_mesh_instanced(gms["gouraud"], mats)
                for k in range(K):       # instance k's slice is the single-mesh entry point's soup
                    sxy, sz = ctx.assemble_mesh(gms["gouraud"], mats[k])
                    assert _eq(xy[k * n:(k + 1) * n], sxy, exact) and _eq(z[k * n:(k + 1) * n], sz, exact), (nv, n, K, k)
    assert some_nan


# ---- 2. frames against the oracle and against K single draws ------------------------
@pytest.mark.parametrize("alpha", [False, True])
def test_gouraud_opaque_depth_write(gpu, alpha):
    _colour_case(gpu, "gouraud", "zw", alpha, "order-free", what=f"gouraud alpha={alpha}")


def test_flat_opaque_depth_write(gpu):
    got = _colour_case(gpu, "flat", "zw", False, "order-free", what="flat")
    assert not scenes.bits_equal(got[0], _want("gouraud", "zw", False)[0])


@pytest.mark.parametrize("mode", ["zt", "nz"])
def test_blended_vertex_alpha_takes_the_ordered_raster(gpu, mode):
    _colour_case(gpu, "blended", mode, True, "ordered", what=f"blended {mode}")


def test_forced_ordered_raster(gpu):
    _colour_case(gpu, "gouraud", "zw", False, "ordered", what="forced ordered", force=True)


def test_one_tint_alpha_below_one_takes_the_ordered_raster(gpu):
    got = _colour_case(gpu, "gouraud", "zw", True, "ordered", tint="alpha", what="tint alpha 0.5")
    assert not scenes.bits_equal(got[0], _want("gouraud", "zw", True, "opaque")[0])


@pytest.mark.parametrize("kind", ["gouraud", "flat"])
def test_tints_of_alpha_one_stay_order_free(gpu, kind):
    got = _colour_case(gpu, kind, "zw", False, "order-free", tint="opaque", what=f"opaque tint, {kind}")
    assert not scenes.bits_equal(got[0], _want(kind, "zw", False)[0])


@functools.lru_cache(maxsize=None)
def _textured_want(channels, filt, persp, near=0.0, cull=0, clear=MR.CLEAR):
    tex = T.texture_rgb() if channels == 3 else T.texture_rgba(w=37, h=23)
    batch = MI.textured_batch(_mesh("textured"), MI.scene_matrices(), tex, near, cull, persp, ct=CT)
    expected = B.expected_payload if channels == 3 else B.expected_loop
    info = {}
    want = expected(W, H, False, MR.BG, "zw", clear, [batch], info, filt=filt)
    assert info["covered"].mean() > 0.2
    return tex, _frozen(want)


@pytest.mark.parametrize("persp", [False, True])
@pytest.mark.parametrize("filt", [0, 1])
@pytest.mark.parametrize("channels", [3, 4])
def test_textured_mesh(gpu, channels, filt, persp):
    tex, want = _textured_want(channels, filt, persp)
    mesh, mats = _mesh("textured"), MI.scene_matrices()
    gtex = gpu.texture(tex)
    ctx = _ctx(gpu, "zw", False, persp=persp, filt=filt)
    ctx.draw_mesh_instanced(_gpu_mesh(mesh), mats, texture=gtex)
    assert ctx.last_raster_path() == ("order-free" if channels == 3 else "ordered")
    got = MR.read_frame(ctx, "zw")
    what = f"textured, {channels} channels, filter {filt}, perspective {persp}"
    _same(got, want, what + ": oracle")
    _same(got, _single_draws(gpu, "zw", False, mesh, mats, texture=gtex, persp=persp, filt=filt), what + ": K draw_mesh calls")
    if channels == 3:
        other = _textured_want(3, 1 - filt, persp)[1], _textured_want(3, filt, not persp)[1]
        assert not scenes.bits_equal(want[0], other[0][0]) and not scenes.bits_equal(want[0], other[1][0])


# ---- 3. the clip stage -----------------------------------------------------------------
@pytest.mark.parametrize("near,cull", [(NEAR, 0), (NEAR, 1), (NEAR, 2), (0.0, 1), (0.0, 2)])
def test_clip_stage(gpu, near, cull):
    mats = MI.scene_matrices()
    K = mats.shape[0]
    for kind, tint in (("gouraud", "opaque"), ("flat", None), ("textured", None)):
        mesh, t = _mesh(kind), _tint(tint)
        gm = _gpu_mesh(mesh)
        what = (kind, near, cull)
        counts = []
        wxy, wz, wattr, _ = MI.instanced_soup(mesh, mats, t, near, cull, counts=counts)
        assert 0 < sum(counts) != K * 320
        ctx = _ctx(gpu, "zw", False, clear=FAR, near=near, cull=cull)
        xy, z, attr, q = ctx.assemble_mesh_instanced(gm, mats, tint=t)
        assert q is None and xy.shape[0] == sum(counts), what
        assert scenes.bits_equal(xy, wxy) and scenes.bits_equal(z, wz) and scenes.bits_equal(attr, wattr), what
        if kind == "textured":
            tex = T.texture_rgb()
            want = B.expected_payload(W, H, False, MR.BG, "zw", FAR,
                                      [MI.textured_batch(mesh, mats, tex, near, cull, False, ct=CT)], filt=0)
            ctx.draw_mesh_instanced(gm, mats, texture=gpu.texture(tex))
        else:
            want = _want(kind, "zw", False, tint, near, cull, FAR)
            ctx.draw_mesh_instanced(gm, mats, tint=t)
        assert ctx.mesh_last_triangle_count == sum(counts), what
        _same(MR.read_frame(ctx, "zw"), want, what)
        if kind == "gouraud" and near > 0:   # the cut vertices interpolate tinted colours
            assert not scenes.bits_equal(want[0], _want(kind, "zw", False, None, near, cull, FAR)[0])


def test_clip_stage_with_the_perspective_state(gpu):
    mesh, mats = _mesh("textured"), MI.scene_matrices()
    ctx = _ctx(gpu, "zw", False, clear=FAR, near=NEAR, cull=1, persp=True)
    xy, z, uv, q = ctx.assemble_mesh_instanced(_gpu_mesh(mesh), mats)
    wxy, wz, wuv, wq = MI.instanced_soup(mesh, mats, None, NEAR, 1, persp=True)
    assert scenes.bits_equal(xy, wxy) and scenes.bits_equal(z, wz) and scenes.bits_equal(uv, wuv)
    assert scenes.bits_equal(q, wq) and (q != 1.0).any()
    tex = T.texture_rgb()
    want = B.expected_payload(W, H, False, MR.BG, "zw", FAR, [MI.textured_batch(mesh, mats, tex, NEAR, 1, True, ct=CT)], filt=0)
    ctx.draw_mesh_instanced(_gpu_mesh(mesh), mats, texture=gpu.texture(tex))
    _same(MR.read_frame(ctx, "zw"), want, "clipped, perspective")


# ---- 4. the device variant ---------------------------------------------------------------
def _device(a, dev, off=0):
    """`a` as a device tensor, `off` doubles past a 16-byte boundary."""
    import torch
    flat = torch.from_numpy(np.array(a, dtype=np.float64).ravel())
    t = torch.zeros(flat.numel() + 2, dtype=torch.float64, device=dev)[off:off + flat.numel()]
    t.copy_(flat)
    assert t.data_ptr() % 16 == 8 * off
    torch.cuda.synchronize(dev)
    return t


@pytest.mark.parametrize("tint,path,off", [(None, "order-free", 0), ("opaque", "order-free", 1), ("alpha", "ordered", 0)])
def test_device_matrices_and_tint(gpu, tint, path, off):
    import torch
    mesh, mats, t = _mesh("gouraud"), MI.scene_matrices(), _tint(tint)
    K = mats.shape[0]
    ctx = _ctx(gpu, "zw", True)
    dev = f"cuda:{ctx.device}"
    dm, dt = _device(mats, dev, off), (None if t is None else _device(t, dev, off))
    ctx.draw_mesh_instanced_device(_gpu_mesh(mesh), dm, K, tint=dt)
    assert ctx.last_raster_path() == path     # (a device tint: the batch's opacity comes from the device scan)
    got = MR.read_frame(ctx, "zw")
    host = _ctx(gpu, "zw", True)
    host.draw_mesh_instanced(_gpu_mesh(mesh), mats, tint=t)
    _same(got, MR.read_frame(host, "zw"), f"device, tint={tint}")
    _same(got, _want("gouraud", "zw", True, tint), f"device, tint={tint}: oracle")
    # the batch read the context's staging: the tensors are the caller's again once it has synchronised
    ctx2 = _ctx(gpu, "zw", True)
    ctx2.set_pair_capacity_override(50)
    ctx2.draw_mesh_instanced_device(_gpu_mesh(mesh), dm, K, tint=dt)
    torch.cuda.synchronize(dev)
    dm.fill_(float("nan"))
    if dt is not None:
        dt.fill_(0.0)
    torch.cuda.synchronize(dev)
    _same(MR.read_frame(ctx2, "zw"), _want("gouraud", "zw", True, tint), "device arrays rewritten before the re-run")


def test_device_textured(gpu):
    tex, want = _textured_want(3, 0, True)
    mesh, mats = _mesh("textured"), MI.scene_matrices()
    ctx = _ctx(gpu, "zw", False, persp=True)
    dm = _device(mats, f"cuda:{ctx.device}")
    ctx.draw_mesh_instanced_device(_gpu_mesh(mesh), dm, mats.shape[0], texture=gpu.texture(tex))
    _same(MR.read_frame(ctx, "zw"), want, "device, textured")


# ---- 5. lifetime of the staging and of the caller's arrays -------------------------------
def _second_mesh():
    mesh = MR.sphere3d(rows=13, cols=21, seed=8)
    mesh["pos"] = mesh["pos"] * 0.6 + np.array([0.0, 0.3, -0.8])
    return mesh


def test_two_instanced_draws_back_to_back(gpu):
    m1, m2 = _mesh("gouraud"), _second_mesh()
    mats = MI.scene_matrices()
    few, t = mats[:3], MI.scene_tints(3, seed=5)
    want = MR.oracle_frame(W, H, False, "zw", MI.instance_meshes(m1, few, t) + MI.instance_meshes(m2, mats), ct=CT)
    ctx = _ctx(gpu, "zw", False)
    ctx.draw_mesh_instanced(_gpu_mesh(m1), few, tint=t)
    ctx.draw_mesh_instanced(_gpu_mesh(m2), mats)      # (no flush; more instances of a larger mesh: the staging is regrown)
    _same(MR.read_frame(ctx, "zw"), want, "two instanced draws")


@pytest.mark.parametrize("first", ["instanced", "single"])
def test_an_instanced_draw_beside_a_plain_draw(gpu, first):
    m1, m2 = _mesh("gouraud"), _second_mesh()
    mats, M2 = MI.scene_matrices(), MR.perspective(W, H, d=3.0, ax=-0.4, ay=1.1)
    inst, single = MI.instance_meshes(m1, mats), [(m2, M2)]
    want = MR.oracle_frame(W, H, False, "zw", inst + single if first == "instanced" else single + inst, ct=CT)
    ctx = _ctx(gpu, "zw", False)
    g1, g2 = _gpu_mesh(m1), _gpu_mesh(m2)
    if first == "instanced":
        ctx.draw_mesh_instanced(g1, mats)
        ctx.draw_mesh(g2, M2)
    else:
        ctx.draw_mesh(g2, M2)
        ctx.draw_mesh_instanced(g1, mats)
    _same(MR.read_frame(ctx, "zw"), want, f"{first} first")


def test_overflow_rerun_and_rewritten_host_arrays(gpu):
    mesh = _mesh("gouraud")
    mats, tint = MI.scene_matrices().copy(), _tint("opaque").copy()
    ctx = _ctx(gpu, "zw", False)
    ctx.set_pair_capacity_override(50)                # the batch overflows: re-run from the staging after the call
    ctx.draw_mesh_instanced(_gpu_mesh(mesh), mats, tint=tint)
    mats[:] = np.nan                                  # the caller's arrays are its own again
    tint[:] = -7.0
    _same(MR.read_frame(ctx, "zw"), _want("gouraud", "zw", False, "opaque"), "overflow re-run, arrays rewritten")
    # ... and a second instanced draw while the first batch's re-run is still due
    mats = MI.scene_matrices()
    ctx = _ctx(gpu, "zw", False)
    ctx.set_pair_capacity_override(50)
    ctx.draw_mesh_instanced(_gpu_mesh(mesh), mats[:4])
    ctx.draw_mesh_instanced(_gpu_mesh(mesh), mats[4:])
    _same(MR.read_frame(ctx, "zw"), _want("gouraud", "zw", False), "re-run before the next instanced draw")


# ---- 6. empty and error cases ----------------------------------------------------------------
def _expect_error(R, ctx, before, what, call):
    R.lib.ClearLastError()
    assert not R.lib.GetLastErrorString()
    try:
        assert not call(), what
        assert R.lib.GetLastErrorString(), what
    finally:
        R.lib.ClearLastError()
    assert ctx.mesh_last_triangle_count == 0, what
    assert scenes.bits_equal(ctx.get_buffer_numpy(), before), what


def test_no_instances_draw_nothing(gpu):
    R = _R()
    R.lib.ClearLastError()
    ctx = _ctx(gpu, "zw")
    before = MR.read_frame(ctx, "zw")
    colour, textured = _gpu_mesh(_mesh("gouraud")), _gpu_mesh(_mesh("textured"))
    empty = R.Mesh(_mesh("gouraud")["pos"], np.zeros((0, 3), dtype=np.uint32), colors=_mesh("gouraud")["colors"])
    ctx.draw_mesh(colour, MI.scene_matrices()[0])
    assert ctx.mesh_last_triangle_count == 320
    ctx = _ctx(gpu, "zw")
    ctx.draw_mesh_instanced(colour, np.zeros((0, 16)))
    ctx.draw_mesh_instanced(colour, np.zeros((0, 16)), tint=np.zeros((0, 4)))
    ctx.draw_mesh_instanced(textured, np.zeros((0, 4, 4)), texture=gpu.texture(T.texture_rgb()))
    ctx.draw_mesh_instanced(empty, MI.scene_matrices())
    R.lib.DrawMeshInstanced(ctx._ptr, colour._ptr, None, None, 0)
    assert ctx.mesh_last_triangle_count == 0
    xy, z, attr, q = ctx.assemble_mesh_instanced(colour, np.zeros((0, 16)))
    assert xy.shape == (0, 6) and z.shape == (0, 3) and attr.shape == (0, 12) and q is None
    _same(MR.read_frame(ctx, "zw"), before, "no instances")
    assert not R.lib.GetLastErrorString()


def test_errors_draw_nothing(gpu):
    R = _R()
    colour, textured = _gpu_mesh(_mesh("gouraud")), _gpu_mesh(_mesh("textured"))
    one = _gpu_mesh(MR.random_mesh(3, 1, seed=2))
    tex = gpu.texture(T.texture_rgb())
    mats = np.ascontiguousarray(MI.scene_matrices())
    tint = MI.scene_tints(mats.shape[0])
    P = lambda a: a.ctypes.data
    ctx = _ctx(gpu, "nz")
    before = ctx.get_buffer_numpy()
    n_out = np.zeros(1, dtype=np.int64)
    out = np.zeros(6400 * 12)
    lib, c = R.lib, ctx._ptr
    cases = {
        "K < 0": lambda: lib.DrawMeshInstanced(c, colour._ptr, P(mats), None, -1),
        "K < 0, textured": lambda: lib.DrawTexturedMeshInstanced(c, textured._ptr, tex._ptr, P(mats), -3),
        "K < 0, device": lambda: lib.DrawMeshInstancedDevice(c, colour._ptr, None, None, -1),
        "NULL matrices": lambda: lib.DrawMeshInstanced(c, colour._ptr, None, None, 10),
        "NULL matrices, textured device": lambda: lib.DrawTexturedMeshInstancedDevice(c, textured._ptr, tex._ptr, None, 2),
        "a tint on a textured mesh": lambda: lib.AssembleMeshInstanced(c, textured._ptr, P(mats), P(tint), 10, 6400, P(out),
                                                                       P(out), P(out), None, P(n_out)),
        "textured mesh in DrawMeshInstanced": lambda: lib.DrawMeshInstanced(c, textured._ptr, P(mats), None, 10),
        "colour mesh in DrawTexturedMeshInstanced": lambda: lib.DrawTexturedMeshInstanced(c, colour._ptr, tex._ptr, P(mats), 10),
        "NULL texture": lambda: lib.DrawTexturedMeshInstanced(c, textured._ptr, None, P(mats), 10),
        "NULL mesh": lambda: lib.DrawMeshInstancedDevice(c, None, P(mats), None, 10),
        # the limits, against a 1-triangle mesh: the check comes before any allocation and before the arrays are read
        "K * n > 2^31 - 1": lambda: lib.DrawMeshInstanced(c, one._ptr, P(mats), None, I32 + 1),
        "K * nv > 2^31 - 1": lambda: lib.DrawMeshInstanced(c, one._ptr, P(mats), P(tint), I32 // 3 + 1),
        "K * nv > 2^31 - 1, device": lambda: lib.DrawMeshInstancedDevice(c, one._ptr, P(mats), None, I32 // 3 + 1),
        "K * nv > 2^31 - 1, assemble": lambda: lib.AssembleMeshInstanced(c, one._ptr, P(mats), None, I32 // 3 + 1, 0, None,
                                                                        None, None, None, P(n_out)),
    }
    for what, call in cases.items():
        ctx.draw_mesh(colour, mats[MI.OFFSCREEN])     # (the last count is 320 before every case)
        assert ctx.mesh_last_triangle_count == 320
        if "assemble" in what or "tint on" in what:
            R.lib.ClearLastError()
            assert not call() and R.lib.GetLastErrorString() and n_out[0] == 0, what
            R.lib.ClearLastError()
            continue
        _expect_error(R, ctx, before, what, call)
    with pytest.raises(ValueError):
        ctx.draw_mesh_instanced(textured, mats)
    with pytest.raises(ValueError):
        ctx.draw_mesh_instanced(colour, mats, texture=tex)
    with pytest.raises(ValueError):
        ctx.draw_mesh_instanced(textured, mats, texture=tex, tint=tint)
    with pytest.raises(ValueError):
        ctx.draw_mesh_instanced(colour, mats, tint=tint[:-1])
    with pytest.raises(ValueError):
        ctx.draw_mesh_instanced_device(textured, 0, 1, texture=tex, tint=0)
    assert not R.lib.GetLastErrorString()
    # and the context still draws
    ctx.draw_mesh_instanced(colour, mats, tint=tint)
    assert not scenes.bits_equal(ctx.get_buffer_numpy(), before)
    assert not R.lib.GetLastErrorString()


# ---- 7. shape extremes ----------------------------------------------------------------------
def test_three_thousand_instances_of_one_triangle(gpu):
    K = 3000
    g = scenes.rng(31)
    mesh = dict(pos=np.array([[-1.0, -0.8, 0.0], [1.0, -0.6, 0.1], [0.1, 0.9, -0.1]]),
                idx=np.array([[0, 1, 2]], dtype=np.uint32), colors=g.uniform(0, 1, size=(3, 4)), gouraud=True)
    mesh["colors"][:, 3] = 1.0
    Pm = MR.perspective(W, H).reshape(4, 4)
    mats = np.empty((K, 16))
    for k in range(K):
        A = MI.translate(*(g.uniform(-1, 1, size=3) * (1.7, 1.2, 1.0)))
        A[0, 0] = A[1, 1] = A[2, 2] = g.uniform(0.03, 0.15)
        mats[k] = (Pm @ A).reshape(16)
    tint = g.uniform(0.2, 1.0, size=(K, 4))
    tint[:, 3] = 1.0
    want = MI.oracle_frame(W, H, False, "zw", mesh, mats, tint, ct=CT)
    assert (want[1] != MR.CLEAR).mean() > 0.3
    ctx = _ctx(gpu, "zw", False)
    ctx.draw_mesh_instanced(_gpu_mesh(mesh), mats, tint=tint)
    assert ctx.last_raster_path() == "order-free" and ctx.mesh_last_triangle_count == K
    _same(MR.read_frame(ctx, "zw"), want, "3000 instances of one triangle")


def test_two_instances_of_three_thousand_triangles(gpu):
    mesh = MR.random_mesh(1000, 3000, seed=5)
    mats = np.stack([MR.perspective(W, H, d=2.5), MR.perspective(W, H, d=3.5, ax=-0.7, ay=0.2)])
    for near in (0.0, 2.0):
        want = MI.oracle_frame(W, H, True, "zt", mesh, mats, w_near=near, ct=CT)
        ctx = _ctx(gpu, "zt", True, near=near)
        ctx.draw_mesh_instanced(_gpu_mesh(mesh), mats)
        assert ctx.last_raster_path() == "ordered"      # (random vertex alphas)
        counts = []
        MI.instanced_soup(mesh, mats, w_near=near, counts=counts)
        assert ctx.mesh_last_triangle_count == sum(counts) and (near == 0 or sum(counts) != 6000)
        _same(MR.read_frame(ctx, "zt"), want, f"two large instances, near={near}")

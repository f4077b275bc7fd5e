"""Perspective-correct texture mapping on the GPU, bit for bit (f64 framebuffer,
u32 depth, u8 where read) against tests/persp_ref.py: soups with a 1/w per corner
on both rasters and through the k_vis variants, the identity and degenerate q,
the entry points' rejections, and textured meshes under SetMeshPerspective --
their soup (q included) and their frames under the clip states, with the
state's invariants and one case each of the neighbouring features."""
import functools

import numpy as np
import pytest

import mesh_ref as MR
import persp_ref as P
import scenes
import textured_ref as T

pytestmark = pytest.mark.gpu

W, H = P.W, P.H
BG, CLEAR, FAR, CT = P.BG, P.CLEAR, P.FAR, P.CT
MATRICES = ("perspective", "behind_eye", "affine")


def _R():
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    return R


@pytest.fixture(autouse=True)
def _fresh_error_latch():
    _R().lib.ClearLastError()


def _same(got, want, what):
    assert scenes.bits_equal(got[0], want[0]), (what, scenes.first_mismatch(got[0], want[0]))
    if want[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "depth", scenes.first_mismatch(got[1], want[1]))


def _differs(a, b):
    return not scenes.bits_equal(a[0], b[0])


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def _frozen(want):
    for a in want:
        if a is not None:
            a.setflags(write=False)
    return want


# ---- soups ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _expected(kind, mode, alpha):
    bs = P.soup_batches(kind)
    fn = P.expected_payload if kind == "opaque" else P.expected_loop
    info = {}
    want = fn(W, H, alpha, BG, mode, CLEAR, bs, info)
    assert info["covered"].mean() >= 0.5 and len(info["texels"]) >= 100
    return _frozen(want)


@pytest.mark.parametrize("alpha", [False, True])
@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("kind", P.KINDS)
def test_soup_parity(gpu, kind, mode, alpha):
    want = _expected(kind, mode, alpha)
    ctx = gpu.context(W, H, alpha)
    got = P.draw_gpu(ctx, gpu, mode, CLEAR, BG, P.soup_batches(kind))
    assert ctx.last_raster_path() == ("order-free" if kind == "opaque" else "ordered")
    _same(got, want, f"{kind} {mode} alpha={alpha}")
    if kind == "opaque":   # the result does not depend on the raster
        ctx = gpu.context(W, H, alpha)
        ctx.set_force_ordered_raster(True)
        got = P.draw_gpu(ctx, gpu, mode, CLEAR, BG, P.soup_batches(kind))
        assert ctx.last_raster_path() == "ordered"
        _same(got, want, f"{kind} {mode} alpha={alpha} forced ordered")
        # and it is not the affine frame
        actx = gpu.context(W, H, alpha)
        assert _differs(T.draw_gpu(actx, gpu, mode, CLEAR, BG, P.soup_batches(kind)), want)


@pytest.mark.parametrize("coop", [1, 2])
def test_coop_raster_variants(gpu, coop):
    for mode in T.MODES:
        ctx = gpu.context(W, H, False)
        ctx.set_coop_raster(coop)
        _same(P.draw_gpu(ctx, gpu, mode, CLEAR, BG, P.soup_batches("opaque")), _expected("opaque", mode, False),
              f"coop {coop} {mode}")


def test_large_triangles_take_the_flattened_variant(gpu):
    bs = [P.soup(W, H, 30, 21, T.texture_rgb(), spread=60.0, m=T.XFORM, ct=CT)]
    for mode in T.MODES:
        for alpha in (False, True):
            want = P.expected_payload(W, H, alpha, BG, mode, CLEAR, bs)
            ctx = gpu.context(W, H, alpha)
            got = P.draw_gpu(ctx, gpu, mode, CLEAR, BG, bs)   # (no history: the flattened raster)
            assert ctx.last_raster_path() == "order-free"
            _same(got, want, f"large {mode} alpha={alpha}")


@functools.lru_cache(maxsize=None)
def _dense():
    DW, DH = 256, 160
    bs = [P.soup(DW, DH, 20000, 31, T.texture_rgb(), spread=3.0, ct=CT, zrange=(0.0, 1.0))]
    wants = {(mode, alpha): P.expected_payload(DW, DH, alpha, BG, mode, FAR, bs)
             for mode in T.MODES for alpha in (False, True)}
    return DW, DH, bs, wants


@pytest.mark.parametrize("limits", [(64, 64), (200, 96)])
def test_split_dense_tiles(gpu, limits):
    DW, DH, bs, wants = _dense()
    tex = gpu.texture(bs[0]["tex"])
    for (mode, alpha), want in wants.items():
        ctx = gpu.context(DW, DH, alpha)
        ctx.set_split_limits(*limits)
        _same(P.draw_gpu(ctx, gpu, mode, FAR, BG, bs, [tex]), want, f"split {limits} {mode} alpha={alpha}")


def _one_batch_ctx(gpu, b, mode="zw"):
    ctx = gpu.context(W, H, False)
    MR.begin_frame(ctx, mode, b["m"], b["ct"], bg=BG, clear=CLEAR)
    return ctx


def test_pair_capacity_overflow_rerun(gpu):
    b = P.soup_batches("opaque")[0]
    want = P.expected_payload(W, H, False, BG, "zw", CLEAR, [b])
    ctx = _one_batch_ctx(gpu, b)
    ctx.set_pair_capacity_override(50)
    ctx.draw_textured_triangles(gpu.texture(b["tex"]), b["xy"], b["uv"], z=b["z"], q=b["q"])
    _same(MR.read_frame(ctx, "zw"), want, "overflow re-run")


def test_device_pointers(gpu):
    import torch
    b = P.soup_batches("opaque")[0]
    n = b["xy"].shape[0]
    want = P.expected_payload(W, H, False, BG, "zw", CLEAR, [b])
    tex = gpu.texture(b["tex"])
    dev = torch.device("cuda", gpu.context(8, 8, False).device)
    txy, tuv, tz, tq = (torch.from_numpy(np.ascontiguousarray(b[k])).to(dev) for k in ("xy", "uv", "z", "q"))
    torch.cuda.synchronize(dev)
    for off in (0, 1):   # (1: xy / uv that are not 16-byte aligned are re-staged; q is read as single doubles)
        if off:
            pad = lambda t: torch.cat([torch.zeros(1, dtype=t.dtype, device=dev), t.reshape(-1)])[1:]
            txy, tuv, tq = pad(txy), pad(tuv), pad(tq)
            torch.cuda.synchronize(dev)
            assert txy.data_ptr() % 16 == 8
        ctx = _one_batch_ctx(gpu, b)
        ctx.draw_textured_triangles_device(tex, txy, tuv, n, z=tz, q=tq)
        assert ctx.last_raster_path() == "order-free"
        _same(MR.read_frame(ctx, "zw"), want, f"device pointers +{off}")


@pytest.mark.parametrize("force", [False, True])
def test_fragment_count_equals_the_affine_draws(gpu, force):
    b = P.soup_batches("opaque")[0]
    tex = gpu.texture(b["tex"])
    counts = []
    for q in (b["q"], None):
        ctx = _one_batch_ctx(gpu, b)
        ctx.set_force_ordered_raster(force)
        ctx.set_fragment_counting(True)
        ctx.draw_textured_triangles(tex, b["xy"], b["uv"], z=b["z"], q=q)
        if q is not None:
            _same(MR.read_frame(ctx, "zw"), P.expected_payload(W, H, False, BG, "zw", CLEAR, [b]), "counting frame")
        counts.append(ctx.get_fragment_count())
    assert counts[0] == counts[1] > 1000, counts


# ---- identity, degenerate q, rejections ------------------------------------------------------
@pytest.mark.parametrize("kind", ["opaque", "rgba_texture"])
def test_unit_q_is_the_affine_draw(gpu, kind):
    bs = [dict(b, q=np.ones_like(b["q"])) for b in P.soup_batches(kind)]
    tfn = T.expected_payload if kind == "opaque" else T.expected_loop
    for mode in T.MODES:
        want = tfn(W, H, False, BG, mode, CLEAR, bs)
        for force in ((False, True) if kind == "opaque" else (False,)):
            ctx = gpu.context(W, H, False)
            ctx.set_force_ordered_raster(force)
            got = P.draw_gpu(ctx, gpu, mode, CLEAR, BG, bs)
            _same(got, want, f"q == 1 against the oracle's frame, {kind} {mode} force={force}")
            actx = gpu.context(W, H, False)
            actx.set_force_ordered_raster(force)
            _same(got, T.draw_gpu(actx, gpu, mode, CLEAR, BG, bs), f"q == 1 against draw_textured_triangles, {kind} {mode}")


def test_degenerate_q(gpu):
    """q is not validated: every value gives the texel the expressions give."""
    R = _R()
    b = P.soup(W, H, 60, 41, T.texture_rgb(), spread=40.0, ct=CT)
    odd = [0.0, -1.0, np.inf, -np.inf, np.nan, 1e300, 1e-300]
    g = scenes.rng(5)
    q = b["q"].copy()
    for t in range(0, 60, 2):           # every other triangle: one, two or three odd corners
        for c in g.choice(3, size=1 + t // 2 % 3, replace=False):
            q[t, c] = odd[int(g.integers(len(odd)))]
    for k, v in enumerate(odd):         # and each odd value on every corner of some triangle
        q[2 * k + 1] = v
    b["q"] = q
    for mode in ("zw", "nz"):
        info = {}
        want = P.expected_payload(W, H, False, BG, mode, CLEAR, [b], info)
        assert info["covered"].mean() > 0.5
        for force in (False, True):
            ctx = gpu.context(W, H, False)
            ctx.set_force_ordered_raster(force)
            _same(P.draw_gpu(ctx, gpu, mode, CLEAR, BG, [b]), want, f"degenerate q {mode} force={force}")
            assert not R.lib.GetLastErrorString()
    b4 = dict(b, tex=T.texture_rgba(), ct=P.CT_BLEND)
    ctx = gpu.context(W, H, True)
    _same(P.draw_gpu(ctx, gpu, "zw", CLEAR, BG, [b4]), P.expected_loop(W, H, True, BG, "zw", CLEAR, [b4]),
          "degenerate q, blended")
    assert not R.lib.GetLastErrorString()


def test_rejected_draws_latch_an_error_and_draw_nothing(gpu):
    import torch
    R = _R()
    b = P.soup(64, 40, 10, 5, T.texture_rgb(), spread=25.0)
    ctx = gpu.context(64, 40, False)
    ctx.set_color(*BG)
    before = ctx.get_buffer_numpy()
    good = gpu.texture(b["tex"])
    xy, uv, q = (np.ascontiguousarray(b[k]) for k in ("xy", "uv", "q"))
    A = lambda a: a.ctypes.data
    dev = torch.device("cuda", ctx.device)
    dxy, duv, dq = (torch.from_numpy(a).to(dev) for a in (xy, uv, q))
    torch.cuda.synchronize(dev)
    D = lambda t: t.data_ptr()
    calls = {
        "NULL q": lambda: R.lib.DrawTexturedTrianglesPerspective(ctx._ptr, good._ptr, A(xy), None, A(uv), None, 10),
        "NULL q, device": lambda: R.lib.DrawTexturedTrianglesPerspectiveDevice(ctx._ptr, good._ptr, D(dxy), None, D(duv),
                                                                               None, 10),
        "NULL texture": lambda: R.lib.DrawTexturedTrianglesPerspective(ctx._ptr, None, A(xy), None, A(uv), A(q), 10),
        "NULL texture, device": lambda: R.lib.DrawTexturedTrianglesPerspectiveDevice(ctx._ptr, None, D(dxy), None, D(duv),
                                                                                     D(dq), 10),
        "1x5 texture": lambda: ctx.draw_textured_triangles(gpu.texture(np.ones((5, 1, 3))), xy, uv, q=q),
    }
    if R.device_count() >= 2:
        try:
            assert R.set_device(1)
            other = gpu.texture(b["tex"])
        finally:
            R.set_device(0)
        calls["texture on another device"] = lambda: ctx.draw_textured_triangles(other, xy, uv, q=q)
    try:
        for what, call in calls.items():
            R.lib.ClearLastError()
            call()
            assert R.lib.GetLastErrorString(), what
            assert scenes.bits_equal(ctx.get_buffer_numpy(), before), what
    finally:
        R.lib.ClearLastError()
    ctx.draw_textured_triangles(good, xy, uv, q=q)   # and the context still draws
    want = P.expected_payload(64, 40, False, BG, "nz", 0, [dict(b, z=None, ct=(1.0, 1.0, 1.0, 1.0))])[0]
    assert scenes.bits_equal(ctx.get_buffer_numpy(), want)
    assert not R.lib.GetLastErrorString()


# ---- meshes -----------------------------------------------------------------------------------
def _gpu_mesh(mesh):
    R = _R()
    if "uv" in mesh:
        return R.Mesh(mesh["pos"], mesh["idx"], uv=mesh["uv"])
    return R.Mesh(mesh["pos"], mesh["idx"], colors=mesh["colors"], gouraud=mesh["gouraud"])


def _mesh_ctx(gpu, mode, alpha=False, near=0.0, cull=0, persp=True, ct=CT):
    ctx = gpu.context(W, H, alpha)
    MR.begin_frame(ctx, mode, MR.XFORM, ct, clear=FAR)
    ctx.set_mesh_near_plane(near)
    ctx.set_mesh_cull(cull)
    ctx.set_mesh_perspective(persp)
    return ctx


@functools.lru_cache(maxsize=None)
def _matrix(name):
    M = P.mesh_matrix(name)
    M.setflags(write=False)
    return M


@pytest.mark.parametrize("fine", [False, True])
@pytest.mark.parametrize("name", MATRICES)
def test_mesh_soup_bits(gpu, name, fine):
    """(fine: mesh_ref's 320-triangle sphere, more than one block of every mesh kernel's grid)"""
    mesh = MR.sphere3d(uv_size=(37, 23)) if fine else P.mesh_scene()
    gm = _gpu_mesh(mesh)
    M = _matrix(name)
    ctx = _mesh_ctx(gpu, "zw")
    for near, cull in P.MESH_STATES:
        ctx.set_mesh_near_plane(near)
        ctx.set_mesh_cull(cull)
        for persp in (True, False):
            ctx.set_mesh_perspective(persp)
            xy, z, uv, q = ctx.assemble_mesh_perspective(gm, M)
            if near > 0 or cull:
                wxy, wz, wuv, wq, _ = P.clip_soup_q(mesh, M, near, cull, persp)
            else:
                wxy, wz, wuv, wq = P.expand_q(mesh, M)
                if not persp:
                    wq = np.ones_like(wq)
            what = f"{name} near={near} cull={cull} persp={persp}"
            assert xy.shape[0] == wxy.shape[0], what
            assert _bits(xy, wxy) and _bits(z, wz) and _bits(uv, wuv), what
            assert _bits(q, wq), (what, scenes.first_mismatch(q, wq))
    if name == "affine":
        assert np.array_equal(q, np.ones_like(q))


@functools.lru_cache(maxsize=None)
def _mesh_want(name, near, cull, mode, rgba, persp=True):
    tex = P.mesh_texture(rgba)
    b = P.mesh_batch(P.mesh_scene(), _matrix(name), tex, near, cull, persp, ct=CT)
    fn = P.expected_loop if rgba else P.expected_payload
    if b["xy"].shape[0] == 0:
        b = dict(b, z=None)
    return _frozen(fn(W, H, rgba, BG, mode, FAR, [b]))


@pytest.mark.parametrize("state", P.MESH_STATES)
@pytest.mark.parametrize("name", MATRICES)
def test_mesh_frames(gpu, name, state):
    near, cull = state
    gm = _gpu_mesh(P.mesh_scene())
    for rgba in (False, True):
        tex = gpu.texture(P.mesh_texture(rgba))
        for mode in T.MODES:
            ctx = _mesh_ctx(gpu, mode, rgba, near, cull)
            ctx.draw_mesh(gm, _matrix(name), texture=tex)
            assert ctx.last_raster_path() == ("ordered" if rgba else "order-free")
            what = f"{name} near={near} cull={cull} {mode} rgba={rgba}"
            _same(MR.read_frame(ctx, mode), _mesh_want(name, near, cull, mode, rgba), what)
    if name != "affine" and (name, near, cull) not in P.MESH_EMPTY:
        assert _differs(_mesh_want(name, near, cull, "zw", False), _mesh_want(name, near, cull, "zw", False, False))


def test_affine_matrix_equals_the_state_off_frame(gpu):
    gm = _gpu_mesh(P.mesh_scene())
    tex = gpu.texture(P.mesh_texture())
    for near, cull in ((0.0, 0), (P.NEAR, 1)):
        frames = []
        for persp in (True, False):
            ctx = _mesh_ctx(gpu, "zw", False, near, cull, persp)
            ctx.draw_mesh(gm, _matrix("affine"), texture=tex)
            frames.append(MR.read_frame(ctx, "zw"))
        _same(frames[0], frames[1], f"affine matrix, near={near} cull={cull}")
        _same(frames[0], _mesh_want("affine", near, cull, "zw", False, False), "affine matrix against the affine reference")


def test_colour_mesh_ignores_the_state(gpu):
    mesh = MR.sphere3d(rows=4, cols=6)
    gm = _gpu_mesh(mesh)
    frames = []
    for persp in (True, False):
        ctx = _mesh_ctx(gpu, "zw", persp=persp, ct=(1.0, 1.0, 1.0, 1.0))
        ctx.draw_mesh(gm, _matrix("perspective"))
        frames.append(MR.read_frame(ctx, "zw"))
    _same(frames[0], frames[1], "colour mesh")
    _same(frames[0], MR.oracle_frame(W, H, False, "zw", [(mesh, _matrix("perspective"))], clear=FAR), "colour mesh, oracle")


def test_state_round_trip_save_restore_and_recording(gpu):
    ctx = gpu.context(W, H, False)
    assert ctx.mesh_perspective() is False            # off by default
    ctx.set_mesh_perspective(True)
    assert ctx.mesh_perspective() is True
    ctx.save_state()
    ctx.set_mesh_perspective(False)
    ctx.restore_state()
    assert ctx.mesh_perspective() is False            # not part of the stack: the last set stands
    ctx.save_state()
    ctx.set_mesh_perspective(True)
    ctx.restore_state()
    assert ctx.mesh_perspective() is True
    ctx.set_mesh_perspective(False)
    # a command list does not capture it: a set while recording holds at once, and nothing is queued for it
    ctx.begin_commands()
    ctx.draw_rect(20.0, 15.0, 70.0, 50.0, 0.1, 0.9, 0.2, 1.0)
    ctx.set_mesh_perspective(True)
    assert ctx.mesh_perspective() is True and ctx.command_list_length() == 1
    ctx.end_commands()
    assert ctx.mesh_perspective() is True
    assert gpu.context(W, H, False).mesh_perspective() is False   # per context


def test_recorded_rectangle_then_a_perspective_mesh(gpu):
    """The state set before a recording applies to the mesh drawn within it
    (mesh draws are never recorded: the queued rectangle runs first, and the
    opaque mesh, seen from inside under this clip state, hides all of it)."""
    rect = (20.0, 15.0, 70.0, 50.0, 0.1, 0.9, 0.2, 1.0)
    gm = _gpu_mesh(P.mesh_scene())
    tex = gpu.texture(P.mesh_texture())
    ctx = _mesh_ctx(gpu, "zw", near=P.NEAR, cull=2)
    ctx.begin_commands()
    ctx.draw_rect(*rect)
    ctx.draw_mesh(gm, _matrix("behind_eye"), texture=tex)
    ctx.end_commands()
    want = _mesh_want("behind_eye", P.NEAR, 2, "zw", False)
    octx = scenes.OracleFactory().context(W, H, False)    # the rectangle's footprint: every pixel of it is covered
    MR.begin_frame(octx, "zw", MR.XFORM, CT, clear=FAR)
    octx.draw_rect(*rect)
    bg = np.array(BG[:3])
    foot = (octx.get_buffer_numpy() != bg).any(axis=-1)
    assert foot.sum() > 1000 and (want[0] != bg).any(axis=-1)[foot].all()
    _same(MR.read_frame(ctx, "zw"), want, "rectangle under the mesh")


# ---- cross-feature, one case each -----------------------------------------------------------------
def test_yuv420p_frame_output(gpu):
    gm = _gpu_mesh(P.mesh_scene())
    tex = gpu.texture(P.mesh_texture())
    ctx = gpu.context(W - 2, H - 1, False)            # (even sizes: 4:2:0 planes)
    WW, HH = W - 2, H - 1
    ctx.set_frame_format("yuv420p")
    ctx.set_color(*BG)
    ctx.gather_frame_u8()    # the frame output is produced by the rasters from now on
    MR.begin_frame(ctx, "zw", MR.XFORM, CT, clear=FAR)
    ctx.set_mesh_perspective(True)
    ctx.draw_mesh(gm, _matrix("behind_eye"), texture=tex)
    ctx.gather_frame_u8()
    frame = ctx.get_frame_u8()
    b = P.mesh_batch(P.mesh_scene(), _matrix("behind_eye"), P.mesh_texture(), ct=CT)
    _same(MR.read_frame(ctx, "zw"), P.expected_payload(WW, HH, False, BG, "zw", FAR, [b]), "yuv frame")
    assert np.array_equal(frame, scenes.yuv420p(ctx.get_buffer_as_uint8_numpy()))


def test_two_shards_assemble_the_unsharded_frame(gpu):
    from libnativecpurenderer_amd import sharding
    gm = _gpu_mesh(P.mesh_scene())
    pat = sharding.band_pattern(2, None)
    for rgba in (False, True):
        tex = gpu.texture(P.mesh_texture(rgba))
        want = _mesh_want("behind_eye", P.NEAR, 2, "zw", rgba)
        seen = np.zeros(H, dtype=bool)
        for s in range(2):
            ctx = _mesh_ctx(gpu, "zw", rgba, P.NEAR, 2)
            ctx.set_shard(2, s)
            ctx.draw_mesh(gm, _matrix("behind_eye"), texture=tex)
            got = MR.read_frame(ctx, "zw")
            rows = [y for y in range(H) if pat[(y // 32) % len(pat)] == s]
            assert len(rows) >= 32
            seen[rows] = True
            _same((got[0][rows], got[1][rows]), (want[0][rows], want[1][rows]), f"shard {s} rgba={rgba}")
        assert seen.all()


def test_self_aliasing_texture_is_a_snapshot(gpu):
    base = P.soup(64, 40, 25, 5, T.texture_rgb(), spread=25.0, ct=CT)
    over = P.soup(64, 40, 25, 6, np.zeros((40, 64, 3)), spread=25.0, ct=CT)
    for force in (False, True):
        outs = []
        for shared in (True, False):
            ctx = gpu.context(64, 40, False)
            ctx.set_color(*BG)
            ctx.set_depth_state(False, False)
            ctx.set_force_ordered_raster(force)
            ctx.set_color_transform(*CT)
            ctx.draw_textured_triangles(gpu.texture(base["tex"]), base["xy"], base["uv"], q=base["q"])
            snap = ctx.as_texture_shared() if shared else ctx.as_texure()
            ctx.draw_textured_triangles(snap, over["xy"], over["uv"], q=over["q"])
            outs.append(ctx.get_buffer_numpy())
            if not shared:
                first = P.expected_payload(64, 40, False, BG, "nz", 0, [base])[0]
                want = P.expected_payload(64, 40, False, BG, "nz", 0, [base, dict(over, tex=first)])[0]
                assert scenes.bits_equal(outs[-1], want), scenes.first_mismatch(outs[-1], want)
        assert scenes.bits_equal(outs[0], outs[1]), scenes.first_mismatch(outs[0], outs[1])


def test_update_positions_between_two_perspective_draws(gpu):
    mesh = P.mesh_scene()
    moved = dict(mesh, pos=mesh["pos"] * np.array([0.6, 1.1, 0.8]) + np.array([0.3, -0.1, 0.0]))
    tex = P.mesh_texture()
    M = _matrix("perspective")
    want = P.expected_payload(W, H, False, BG, "zw", FAR,
                              [P.mesh_batch(mesh, M, tex, ct=CT), P.mesh_batch(moved, M, tex, ct=CT)])
    gm = _gpu_mesh(mesh)
    gtex = gpu.texture(tex)
    ctx = _mesh_ctx(gpu, "zw")
    ctx.draw_mesh(gm, M, texture=gtex)      # pending across the update: keeps the old positions
    gm.update_positions(moved["pos"])
    ctx.draw_mesh(gm, M, texture=gtex)
    _same(MR.read_frame(ctx, "zw"), want, "update_positions")
    xy, z, uv, q = ctx.assemble_mesh_perspective(gm, M)
    wxy, wz, wuv, wq = P.expand_q(moved, M)
    assert _bits(xy, wxy) and _bits(z, wz) and _bits(uv, wuv) and _bits(q, wq)

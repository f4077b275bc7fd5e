"""Texture wrap addressing on the GPU (SetTriangleTextureWrap), bit for bit (f64
framebuffer, u32 depth) against tests/wrap_ref.py: affine, perspective and
modulated soups on both rasters under every wrap state and both filters, the
2 x 2 texture, non-finite and huge coordinates, unstaged winners (pass 3b), the
identities I1 and I2, the state's rules, a textured TriangleBuffer across its
cached frames, and the three textured mesh draws."""
import functools

import numpy as np
import pytest

import bilinear_ref as BL
import mesh_inst_ref as MI
import mesh_light_ref as ML
import mesh_ref as MR
import modulate_ref as M
import persp_ref as P
import scenes
import wrap_ref as WR

pytestmark = pytest.mark.gpu

W, H = WR.W, WR.H
BG, CLEAR, FAR, CT = WR.BG, WR.CLEAR, WR.FAR, WR.CT
ALL_WRAPS = WR.WRAPS


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


def _frozen(want):
    for a in want:
        if a is not None:
            a.setflags(write=False)
    return want


def _discriminates(want, clamp, info, tex, wrap, what):
    """The condition on a wrap scene (tests/test_wrap_ref.py asserts it on wrap_ref's scenes; the scenes formed here
    assert it themselves): at least 40 % of the covered pixels sample outside [0, n-1) on each wrapped axis, and
    the expected frame differs from the clamp expected frame on at least 40 % of them."""
    cov = info["covered"]
    assert cov.mean() > 0.1, what
    h, w, _ = tex.shape
    if wrap[0]:
        assert WR.outside(info["u"][cov], w).mean() >= 0.4, (what, "u")
    if wrap[1]:
        assert WR.outside(info["v"][cov], h).mean() >= 0.4, (what, "v")
    assert (want[0][cov] != clamp[0][cov]).any(axis=-1).mean() >= 0.4, (what, "differs from the clamp frame")


# ---- soups -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _expected(case):
    return _frozen(WR.expected(*case))


@pytest.mark.parametrize("case", WR.soup_cases(), ids=lambda c: "-".join(map(str, c)))
def test_soup_parity(gpu, case):
    kind, form, wrap, filt, mode, alpha = case
    want = _expected(case)
    bs = WR.soup_batches(kind, form)
    ctx = gpu.context(W, H, alpha)
    got = WR.draw_gpu(ctx, gpu, mode, CLEAR, BG, bs, filt=filt, wrap=wrap)
    assert ctx.get_triangle_texture_wrap() == wrap
    assert ctx.last_raster_path() == ("order-free" if kind == "opaque" else "ordered")
    _same(got, want, f"{case}")
    if kind == "opaque":   # the result does not depend on the raster
        ctx = gpu.context(W, H, alpha)
        ctx.set_force_ordered_raster(True)
        got = WR.draw_gpu(ctx, gpu, mode, CLEAR, BG, bs, filt=filt, wrap=wrap)
        assert ctx.last_raster_path() == "ordered"
        _same(got, want, f"{case} forced ordered")


# ---- edge scenes -----------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [0, 1])
@pytest.mark.parametrize("wrap", ALL_WRAPS)
def test_two_by_two_texture(gpu, wrap, filt):
    b = WR.tiny_texture_batch()
    want = WR.expected_payload(W, H, False, BG, "zw", CLEAR, [b], filt=filt, wrap=wrap)
    for force in (False, True):
        ctx = gpu.context(W, H, False)
        ctx.set_force_ordered_raster(force)
        _same(WR.draw_gpu(ctx, gpu, "zw", CLEAR, BG, [b], filt=filt, wrap=wrap), want, f"2x2 {wrap} {filt} force={force}")
    b4 = WR.tiny_texture_batch(True)
    ctx = gpu.context(W, H, True)
    _same(WR.draw_gpu(ctx, gpu, "zw", CLEAR, BG, [b4], filt=filt, wrap=wrap),
          WR.expected_loop(W, H, True, BG, "zw", CLEAR, [b4], filt=filt, wrap=wrap), f"2x2 rgba {wrap} {filt}")


@pytest.mark.parametrize("persp", [False, True])
@pytest.mark.parametrize("wrap", [(1, 1), (2, 2)])
def test_odd_coordinates_and_degenerate_q(gpu, wrap, persp):
    """NaN, +-inf and huge (u, v), and q of 0, negative, inf, NaN: every value
    gives an in-range texel, the one the rule gives, and nothing is latched.
    (bilinear_ref's coordinates as they are: this scene is about the odd values, and
    most of its ordinary ones lie inside the texture -- the 40 % condition of the wrap
    scenes is not asked of it; the frame must differ from the clamp frame.)"""
    R = _R()
    b = BL.odd_uv_batch(persp)
    for filt in (0, 1):
        info = {}
        want = WR.expected_payload(W, H, False, BG, "zw", CLEAR, [b], info, filt=filt, wrap=wrap)
        assert info["covered"].mean() > 0.5
        assert not scenes.bits_equal(want[0], WR.expected_payload(W, H, False, BG, "zw", CLEAR, [b], filt=filt)[0])
        for force in (False, True):
            ctx = gpu.context(W, H, False)
            ctx.set_force_ordered_raster(force)
            _same(WR.draw_gpu(ctx, gpu, "zw", CLEAR, BG, [b], filt=filt, wrap=wrap), want,
                  f"odd uv {wrap} filt={filt} force={force} persp={persp}")
            assert not R.lib.GetLastErrorString()


@pytest.mark.parametrize("filt", [0, 1])
def test_unstaged_winners_sample_wrapped(gpu, filt):
    """More distinct winners in a tile than the staged records hold: pass 3b."""
    b = WR.dense_batch()
    for wrap in ((1, 1), (2, 1)):
        want = WR.expected_payload(W, H, False, BG, "zw", FAR, [b], filt=filt, wrap=wrap)
        ctx = gpu.context(W, H, False)
        got = WR.draw_gpu(ctx, gpu, "zw", FAR, BG, [b], filt=filt, wrap=wrap)
        assert ctx.last_raster_path() == "order-free"
        _same(got, want, f"dense {wrap} filt={filt}")


def test_pair_capacity_overflow_rerun_keeps_the_state(gpu):
    """The re-run in settle takes the batch's snapshot: the wrap state it was
    issued with, though the state is (0, 0) by then."""
    b = WR.soup_batches("opaque", "persp")[0]
    want = WR.expected_payload(W, H, False, BG, "zw", CLEAR, [b], filt=1, wrap=(1, 2))
    ctx = gpu.context(W, H, False)
    MR.begin_frame(ctx, "zw", b["m"], b["ct"], bg=BG, clear=CLEAR)
    ctx.set_triangle_texture_filter(1)
    ctx.set_triangle_texture_wrap(1, 2)
    ctx.set_pair_capacity_override(50)
    ctx.draw_textured_triangles(gpu.texture(b["tex"]), b["xy"], b["uv"], z=b["z"], q=b["q"])
    ctx.set_triangle_texture_wrap(0)
    _same(MR.read_frame(ctx, "zw"), want, "overflow re-run")


# ---- identities ------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [0, 1])
def test_i1_inside_the_texture_every_state_gives_the_clamp_frame(gpu, filt):
    for form in ("affine", "persp"):
        bs = WR.inside_batches(form)
        want = BL.expected_payload(W, H, False, BG, "zw", CLEAR, bs, filt=filt)
        for force in (False, True):
            frames = []
            for wrap in ((0, 0), (1, 1), (2, 2)):
                ctx = gpu.context(W, H, False)
                ctx.set_force_ordered_raster(force)
                frames.append(WR.draw_gpu(ctx, gpu, "zw", CLEAR, BG, bs, filt=filt, wrap=wrap))
            for f, wrap in zip(frames, ("clamp", "repeat", "mirror")):
                _same(f, want, f"inside {form} filt={filt} force={force} {wrap}")


@pytest.mark.parametrize("kind", WR.KINDS)
def test_i2_wrap_zero_is_the_frame_without_the_call(gpu, kind):
    R = _R()
    bs = BL.soup_batches(kind, True)
    fn = BL.expected_payload if kind == "opaque" else BL.expected_loop
    want = fn(W, H, False, BG, "zw", CLEAR, bs, filt=1)
    plain = gpu.context(W, H, False)
    _same(BL.draw_gpu(plain, gpu, "zw", CLEAR, BG, bs), want, f"{kind}: no call")
    ctx = gpu.context(W, H, False)
    assert R.lib.SetTriangleTextureWrap(ctx._ptr, 0, 0) is True
    _same(BL.draw_gpu(ctx, gpu, "zw", CLEAR, BG, bs), want, f"{kind}: wrap (0, 0)")


# ---- the state -------------------------------------------------------------------------------
def test_state_default_rejection_and_save_restore(gpu):
    R = _R()
    ctx = gpu.context(W, H, False)
    assert ctx.get_triangle_texture_wrap() == (0, 0)
    ctx.set_triangle_texture_wrap(2)
    assert ctx.get_triangle_texture_wrap() == (2, 2)         # v=None: v = u
    ctx.set_triangle_texture_wrap(1, 2)
    assert ctx.get_triangle_texture_wrap() == (1, 2)
    for bad in ((3, 0), (0, 3), (-1, 1), (1, -1), (1 << 40, 0), (2, 1 << 40)):
        R.lib.ClearLastError()
        with pytest.raises(RuntimeError):
            ctx.set_triangle_texture_wrap(*bad)
        assert "SetTriangleTextureWrap" in R.lib.GetLastErrorString().decode()
        assert ctx.get_triangle_texture_wrap() == (1, 2)     # both axes are kept
        assert R.lib.SetTriangleTextureWrap(ctx._ptr, *bad) is False
    R.lib.ClearLastError()
    ctx.save_state()
    ctx.set_triangle_texture_wrap(2, 0)
    ctx.restore_state()
    assert ctx.get_triangle_texture_wrap() == (2, 0)         # not part of the stack: the last set stands
    ctx.begin_commands()
    ctx.draw_rect(20.0, 15.0, 70.0, 50.0, 0.1, 0.9, 0.2, 1.0)
    ctx.set_triangle_texture_wrap(1, 1)
    assert ctx.get_triangle_texture_wrap() == (1, 1) and ctx.command_list_length() == 1   # not recorded
    ctx.end_commands()
    assert gpu.context(W, H, False).get_triangle_texture_wrap() == (0, 0)   # per context
    assert ctx.get_triangle_texture_filter() == 0                            # and apart from the filter
    assert not R.lib.GetLastErrorString()


@pytest.mark.parametrize("force", [False, True])
def test_pending_batch_keeps_the_state_it_was_issued_with(gpu, force):
    """Draw under (1, 1), set (0, 0), draw a second batch, then read: the first
    batch is wrapped and the second clamped."""
    bs = WR.soup_batches("opaque", "persp")
    states = [(1, 1), (0, 0)]
    for filt in (0, 1):
        info = {}
        want = WR.expected_payload(W, H, False, BG, "zw", CLEAR, bs, info, filt=filt, wrap=states)
        assert min((info["batch"] == k).mean() for k in (0, 1)) > 0.1      # both batches show
        first = info["batch"] == 0                                         # the wrapped batch's pixels discriminate
        clamp = WR.expected_payload(W, H, False, BG, "zw", CLEAR, bs, filt=filt)
        _discriminates(want, clamp, dict(info, covered=first), bs[0]["tex"], (1, 1), f"pending, filt={filt}")
        for other in ((1, 1), (0, 0)):
            assert not scenes.bits_equal(want[0], WR.expected_payload(W, H, False, BG, "zw", CLEAR, bs, filt=filt, wrap=other)[0])
        ctx = gpu.context(W, H, False)
        ctx.set_force_ordered_raster(force)
        _same(WR.draw_gpu(ctx, gpu, "zw", CLEAR, BG, bs, filt=filt, wrap=states), want, f"pending, filt={filt}, force={force}")
        assert ctx.get_triangle_texture_wrap() == (0, 0)


# ---- TriangleBuffer: the cached paths know nothing of colour -----------------------------------
@pytest.mark.parametrize("path", ["key cache", "visible list", "no list reuse"])
def test_triangle_buffer_frames_change_the_state(gpu, path):
    R = _R()
    b = WR.soup_batches("opaque", "affine")[0]
    tex = gpu.texture(b["tex"])
    buf = R.TriangleBuffer(b["xy"], uv=b["uv"], z=b["z"])
    ctx = gpu.context(W, H, False)
    ctx.set_warm_binning(1)
    if path == "visible list":
        ctx.set_key_cache(2)
    elif path == "no list reuse":
        ctx.set_list_reuse(2)
    ctx.set_transform(*b["m"])
    ctx.set_color_transform(*b["ct"])
    plan = [((0, 0), 0)] * 4 + [((1, 1), 0), ((2, 0), 0), ((1, 1), 1), ((2, 0), 1), ((0, 0), 0)]   # (wrap, filter) per frame
    wants, cached, pruned, warm = {}, [], [], []
    for k, (wrap, filt) in enumerate(plan):
        if (wrap, filt) not in wants:
            wants[(wrap, filt)] = WR.expected_payload(W, H, False, BG, "zw", FAR, [b], filt=filt, wrap=wrap)
        ctx.set_color(*BG)
        ctx.set_depth_state(True, True)
        ctx.clear_depth(FAR)
        ctx.set_triangle_texture_filter(filt)
        ctx.set_triangle_texture_wrap(*wrap)
        ctx.draw_triangle_buffer(buf, tex)
        assert ctx.last_raster_path() == "order-free"
        _same((ctx.get_buffer_numpy(), ctx.get_depth_buffer()), wants[(wrap, filt)], f"{path}: frame {k} wrap={wrap} filter={filt}")
        cached.append(ctx.key_cached_batch_count())
        pruned.append(ctx.pruned_batch_count())
        warm.append(ctx.warm_batch_count())
    info = {}
    WR.expected_payload(W, H, False, BG, "zw", FAR, [b], info)
    for wrap, filt in ((w, f) for w, f in wants if w != (0, 0)):
        _discriminates(wants[(wrap, filt)], wants[((0, 0), 0)] if filt == 0 else
                       WR.expected_payload(W, H, False, BG, "zw", FAR, [b], filt=1), info, b["tex"], wrap, f"{path} {wrap} {filt}")
    assert not scenes.bits_equal(wants[((2, 0), 0)][0], wants[((1, 1), 0)][0])
    assert ctx.warm_failure_count() == 0
    assert warm[-1] > 0, warm                                # warm binning, through every change of the state
    if path == "key cache":
        assert cached[4] == 0 and cached[5:] == [1, 2, 3, 4], cached   # the wrapped frames were shaded from the cached keys
    elif path == "visible list":
        assert cached[-1] == 0 and pruned == [0, 0, 0, 1, 2, 3, 4, 5, 6], (cached, pruned)
    else:
        assert cached[-1] == 0 and pruned[-1] == 0 and ctx.reused_batch_count() == 0, (cached, pruned)


# ---- meshes: the front end passes the state through --------------------------------------------
NEAR = P.NEAR
MESH_WRAP = (1, 2)
MTEX = (7, 6)


def _tiled_mesh(mesh):
    """The mesh's uv (over the persp_ref texture's size) rescaled to run over [-2n, 3n) of the 7 x 6 texture."""
    s = np.array([5.0 * MTEX[0] / P.MESH_TEX[0], 5.0 * MTEX[1] / P.MESH_TEX[1]])
    return dict(mesh, uv=np.ascontiguousarray(mesh["uv"] * s - np.array([2.0 * MTEX[0], 2.0 * MTEX[1]])))


def _mesh_ctx(gpu, lights=False):
    ctx = gpu.context(W, H, False)
    MR.begin_frame(ctx, "zw", MR.XFORM, CT, bg=BG, clear=FAR)
    ctx.set_mesh_near_plane(NEAR)
    ctx.set_mesh_cull(0)
    ctx.set_mesh_perspective(True)
    ctx.set_triangle_texture_filter(1)
    ctx.set_triangle_texture_wrap(*MESH_WRAP)
    if lights:
        ctx.set_mesh_lights(ML.AMBIENT, ML.LIGHTS)
    return ctx


def _mesh_check(ctx, batch, what):
    assert batch["xy"].shape[0] > 0
    info = {}
    want = WR.expected_payload(W, H, False, BG, "zw", FAR, [batch], info, filt=1, wrap=MESH_WRAP)
    clamp = WR.expected_payload(W, H, False, BG, "zw", FAR, [batch], filt=1)
    _discriminates(want, clamp, info, batch["tex"], MESH_WRAP, what)
    assert ctx.last_raster_path() == "order-free"
    _same(MR.read_frame(ctx, "zw"), want, what)


def test_textured_mesh(gpu):
    R = _R()
    mesh = _tiled_mesh(P.mesh_scene())
    gm = R.Mesh(mesh["pos"], mesh["idx"], uv=mesh["uv"])
    tex = WR.texture(*MTEX)
    Mx = P.mesh_matrix("behind_eye")
    ctx = _mesh_ctx(gpu)
    ctx.draw_mesh(gm, Mx, texture=gpu.texture(tex))
    xy, z, uv, q = ctx.assemble_mesh_perspective(gm, Mx)
    _mesh_check(ctx, dict(xy=xy, z=z, uv=uv, q=q, tex=tex, ct=CT, m=MR.XFORM), "DrawTexturedMesh")


def test_textured_mesh_instanced(gpu):
    R = _R()
    mesh = _tiled_mesh(MR.sphere3d(uv_size=P.MESH_TEX))
    gm = R.Mesh(mesh["pos"], mesh["idx"], uv=mesh["uv"])
    tex = WR.texture(*MTEX)
    mats = np.asarray(MI.scene_matrices())[[0, 1, 7]]          # two placements and the one partly behind the eye: K = 3
    ctx = _mesh_ctx(gpu)
    ctx.draw_mesh_instanced(gm, mats, texture=gpu.texture(tex))
    xy, z, uv, q = ctx.assemble_mesh_instanced(gm, mats)
    _mesh_check(ctx, dict(xy=xy, z=z, uv=uv, q=q, tex=tex, ct=CT, m=MR.XFORM), "DrawTexturedMeshInstanced")


def test_textured_mesh_lit(gpu):
    R = _R()
    mesh = _tiled_mesh(M.lit_textured_sphere())
    gm = R.Mesh(mesh["pos"], mesh["idx"], colors=mesh["colors"], uv=mesh["uv"], normals=mesh["normals"])
    tex = WR.texture(*MTEX)
    Mx, N = P.mesh_matrix("behind_eye"), ML.rotation3()
    ctx = _mesh_ctx(gpu, lights=True)
    ctx.draw_mesh_lit(gm, Mx, N, texture=gpu.texture(tex))
    xy, z, uvc, q = ctx.assemble_textured_color_mesh(gm, Mx, N, lit=True)
    a = uvc.reshape(-1, 3, 6)
    n = xy.shape[0]
    batch = dict(xy=xy, z=z, q=q, uv=np.ascontiguousarray(a[:, :, 0:2].reshape(n, 6)),
                 rgba=np.ascontiguousarray(a[:, :, 2:6].reshape(n, 12)), tex=tex, ct=CT, m=MR.XFORM)
    assert M.is_opaque(batch)
    _mesh_check(ctx, batch, "DrawTexturedMeshLit")

"""Bilinear texture filtering on the GPU (SetTriangleTextureFilter), bit for bit
(f64 framebuffer, u32 depth, u8 and frame output where read) against
tests/bilinear_ref.py: affine and perspective soups on both rasters and through
the k_vis variants, the filter's fixed points and degenerate inputs, a textured
TriangleBuffer across its warm frames with the filter and the texture toggled,
textured meshes under the clip and perspective states, the state's rules, and
one case each of the neighbouring features."""
import functools

import numpy as np
import pytest

import bilinear_ref as B
import mesh_ref as MR
import persp_ref as P
import scenes
import textured_ref as T

pytestmark = pytest.mark.gpu

W, H = B.W, B.H
BG, CLEAR, FAR, CT = B.BG, B.CLEAR, B.FAR, B.CT
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


def _frozen(want):
    for a in want:
        if a is not None:
            a.setflags(write=False)
    return want


# ---- soups ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _expected(kind, mode, alpha, persp, filt=1):
    bs = B.soup_batches(kind, persp)
    fn = B.expected_payload if kind == "opaque" else B.expected_loop
    info = {}
    want = fn(W, H, alpha, BG, mode, CLEAR, bs, info, filt=filt)
    assert info["covered"].mean() >= 0.5
    return _frozen(want)


@pytest.mark.parametrize("persp", [False, True])
@pytest.mark.parametrize("alpha", [False, True])
@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("kind", B.KINDS)
def test_soup_parity(gpu, kind, mode, alpha, persp):
    want = _expected(kind, mode, alpha, persp)
    bs = B.soup_batches(kind, persp)
    ctx = gpu.context(W, H, alpha)
    got = B.draw_gpu(ctx, gpu, mode, CLEAR, BG, bs)
    assert ctx.last_raster_path() == ("order-free" if kind == "opaque" else "ordered")
    _same(got, want, f"{kind} {mode} alpha={alpha} persp={persp}")
    if kind == "opaque":   # the result does not depend on the raster
        ctx = gpu.context(W, H, alpha)
        ctx.set_force_ordered_raster(True)
        got = B.draw_gpu(ctx, gpu, mode, CLEAR, BG, bs)
        assert ctx.last_raster_path() == "ordered"
        _same(got, want, f"{kind} {mode} alpha={alpha} persp={persp} forced ordered")
        # and it is not the nearest frame
        nctx = gpu.context(W, H, alpha)
        assert _differs(B.draw_gpu(nctx, gpu, mode, CLEAR, BG, bs, filt=0), want)


@pytest.mark.parametrize("persp", [False, True])
@pytest.mark.parametrize("coop", [1, 2])
def test_coop_raster_variants(gpu, coop, persp):
    for mode in T.MODES:
        ctx = gpu.context(W, H, False)
        ctx.set_coop_raster(coop)
        _same(B.draw_gpu(ctx, gpu, mode, CLEAR, BG, B.soup_batches("opaque", persp)),
              _expected("opaque", mode, False, persp), f"coop {coop} {mode} persp={persp}")


def _large(persp):
    b = P.soup(W, H, 30, 21, T.texture_rgb(), spread=60.0, m=T.XFORM, ct=CT)
    if not persp:
        del b["q"]
    return [b]


@pytest.mark.parametrize("persp", [False, True])
def test_large_triangles_take_the_flattened_variant(gpu, persp):
    bs = _large(persp)
    for mode in T.MODES:
        want = B.expected_payload(W, H, False, BG, mode, CLEAR, bs)
        ctx = gpu.context(W, H, False)
        got = B.draw_gpu(ctx, gpu, mode, CLEAR, BG, bs)   # (no history: the flattened raster)
        assert ctx.last_raster_path() == "order-free"
        _same(got, want, f"large {mode} persp={persp}")


@functools.lru_cache(maxsize=None)
def _dense(persp):
    """104 small triangles whose centroids lie within one tile: a tile list
    longer than the split limits below."""
    b = P.soup(W, H, 104, 31, T.texture_rgb(), spread=9.0, ct=CT, zrange=(0.0, 0.99))
    xy = b["xy"].reshape(104, 3, 2)
    c = xy.mean(axis=1, keepdims=True)
    g = scenes.rng(32)
    centre = np.stack([g.uniform(70, 120, 104), g.uniform(36, 60, 104)], axis=1)[:, None, :]
    b["xy"] = np.ascontiguousarray((xy - c + centre).reshape(104, 6))
    if not persp:
        del b["q"]
    wants = {mode: _frozen(B.expected_payload(W, H, False, BG, mode, FAR, [b])) for mode in T.MODES}
    return b, wants


@pytest.mark.parametrize("persp", [False, True])
@pytest.mark.parametrize("limits", [(64, 64), (200, 96)])
def test_split_dense_tiles(gpu, limits, persp):
    b, wants = _dense(persp)
    tex = gpu.texture(b["tex"])
    for mode, want in wants.items():
        ctx = gpu.context(W, H, False)
        ctx.set_split_limits(*limits)
        _same(B.draw_gpu(ctx, gpu, mode, FAR, BG, [b], [tex]), want, f"split {limits} {mode} persp={persp}")


def _one_batch_ctx(gpu, b, mode="zw", filt=1, clear=CLEAR, alpha=False):
    ctx = gpu.context(W, H, alpha)
    MR.begin_frame(ctx, mode, b["m"], b["ct"], bg=BG, clear=clear)
    ctx.set_triangle_texture_filter(filt)
    return ctx


@pytest.mark.parametrize("persp", [False, True])
def test_pair_capacity_overflow_rerun_keeps_the_filter(gpu, persp):
    """The re-run in settle takes the batch's snapshot: the filter it was issued
    with, though the state is 0 by then."""
    b = B.soup_batches("opaque", persp)[0]
    want = B.expected_payload(W, H, False, BG, "zw", CLEAR, [b])
    ctx = _one_batch_ctx(gpu, b)
    ctx.set_pair_capacity_override(50)
    ctx.draw_textured_triangles(gpu.texture(b["tex"]), b["xy"], b["uv"], z=b["z"], q=b.get("q"))
    ctx.set_triangle_texture_filter(0)
    _same(MR.read_frame(ctx, "zw"), want, "overflow re-run")


@pytest.mark.parametrize("force", [False, True])
def test_fragment_count_equals_the_nearest_draws(gpu, force):
    for persp in (False, True):
        b = B.soup_batches("opaque", persp)[0]
        tex = gpu.texture(b["tex"])
        counts = []
        for filt in (1, 0):
            ctx = _one_batch_ctx(gpu, b, filt=filt)
            ctx.set_force_ordered_raster(force)
            ctx.set_fragment_counting(True)
            ctx.draw_textured_triangles(tex, b["xy"], b["uv"], z=b["z"], q=b.get("q"))
            if filt:
                _same(MR.read_frame(ctx, "zw"), B.expected_payload(W, H, False, BG, "zw", CLEAR, [b]), "counting frame")
            counts.append(ctx.get_fragment_count())
        assert counts[0] == counts[1] > 1000, counts


# ---- fixed points and degenerate inputs ---------------------------------------------------
def test_integer_uv_gives_the_nearest_frame(gpu):
    bs = B.integer_uv_batches()
    for mode in T.MODES:
        want = T.expected_payload(W, H, False, BG, mode, CLEAR, bs)
        for force in (False, True):
            frames = []
            for filt in (1, 0):
                ctx = gpu.context(W, H, False)
                ctx.set_force_ordered_raster(force)
                frames.append(B.draw_gpu(ctx, gpu, mode, CLEAR, BG, bs, filt=filt))
            _same(frames[0], frames[1], f"integer uv {mode} force={force}: filtered against nearest")
            _same(frames[0], want, f"integer uv {mode} force={force}: against the oracle's nearest frame")


@pytest.mark.parametrize("persp", [False, True])
def test_odd_coordinates_and_degenerate_q(gpu, persp):
    """NaN, +-inf and huge (u, v), and q of 0, negative, inf, NaN: every value
    gives the colour the expressions give, and nothing is latched."""
    R = _R()
    b = B.odd_uv_batch(persp)
    for mode in ("zw", "nz"):
        info = {}
        want = B.expected_payload(W, H, False, BG, mode, CLEAR, [b], info)
        assert info["covered"].mean() > 0.5
        for force in (False, True):
            ctx = gpu.context(W, H, False)
            ctx.set_force_ordered_raster(force)
            _same(B.draw_gpu(ctx, gpu, mode, CLEAR, BG, [b]), want, f"odd uv {mode} force={force} persp={persp}")
            assert not R.lib.GetLastErrorString()
    b4 = dict(b, tex=T.texture_rgba(), ct=B.CT_BLEND)
    ctx = gpu.context(W, H, True)
    _same(B.draw_gpu(ctx, gpu, "zw", CLEAR, BG, [b4]), B.expected_loop(W, H, True, BG, "zw", CLEAR, [b4]),
          f"odd uv, blended, persp={persp}")
    assert not R.lib.GetLastErrorString()


@pytest.mark.parametrize("channels", [3, 4])
def test_two_by_two_texture(gpu, channels):
    b = B.tiny_texture_batch(channels == 4)
    fn = B.expected_loop if channels == 4 else B.expected_payload
    for mode in ("zw", "nz"):
        for alpha in (False, True):
            want = fn(W, H, alpha, BG, mode, CLEAR, [b])
            for force in ((False, True) if channels == 3 else (False,)):
                ctx = gpu.context(W, H, alpha)
                ctx.set_force_ordered_raster(force)
                _same(B.draw_gpu(ctx, gpu, mode, CLEAR, BG, [b]), want, f"2x2 x{channels} {mode} alpha={alpha} force={force}")


# ---- TriangleBuffer: warm binning, list reuse, the visible-triangle path ---------------------
def test_triangle_buffer_frames_toggle_filter_and_texture(gpu):
    R = _R()
    b = B.soup_batches("opaque", False)[0]
    texs = [T.texture_rgb(), T.texture_rgb(seed=8, w=11, h=7)]
    gtex = [gpu.texture(t) for t in texs]
    buf = R.TriangleBuffer(b["xy"], uv=b["uv"], z=b["z"])
    ctx = gpu.context(W, H, False)
    ctx.set_warm_binning(1)
    ctx.set_transform(*b["m"])
    ctx.set_color_transform(*b["ct"])
    # (filter, texture) per frame: on from the start, then both toggled on the pruned path
    plan = [(1, 0), (1, 0), (1, 0), (1, 0), (0, 0), (1, 1), (0, 1), (1, 0), (1, 0)]
    wants, pruned = {}, []
    for k, (filt, ti) in enumerate(plan):
        if (filt, ti) not in wants:
            wants[(filt, ti)] = B.expected_payload(W, H, False, BG, "zw", FAR, [dict(b, tex=texs[ti])], filt=filt)
        ctx.set_color(*BG)
        ctx.set_depth_state(True, True)
        ctx.clear_depth(FAR)
        ctx.set_triangle_texture_filter(filt)
        ctx.draw_triangle_buffer(buf, gtex[ti])
        assert ctx.last_raster_path() == "order-free"
        _same((ctx.get_buffer_numpy(), ctx.get_depth_buffer()), wants[(filt, ti)], f"frame {k} filter={filt} texture={ti}")
        pruned.append(ctx.pruned_batch_count())
    assert _differs(wants[(1, 0)], wants[(0, 0)]) and _differs(wants[(1, 1)], wants[(0, 1)])
    # warm from frame 1, list reuse from frame 2, the visible-triangle path from frame 3 on -- through every toggle
    assert pruned == [0, 0, 0, 1, 2, 3, 4, 5, 6], pruned
    assert ctx.warm_failure_count() == 0
    assert 0 < ctx.visible_pair_count() < ctx.schedule_totals()["pairs"]


def test_device_pointers_toggle_filter_and_texture(gpu):
    import torch
    b = B.soup_batches("opaque", True)[0]
    n = b["xy"].shape[0]
    texs = [T.texture_rgb(), T.texture_rgb(seed=8, w=11, h=7)]
    gtex = [gpu.texture(t) for t in texs]
    dev = torch.device("cuda", gpu.context(8, 8, False).device)
    txy, tuv, tz, tq = (torch.from_numpy(np.ascontiguousarray(b[k])).to(dev) for k in ("xy", "uv", "z", "q"))
    torch.cuda.synchronize(dev)
    for off in (0, 1):   # (1: xy / uv that are not 16-byte aligned are re-staged)
        if off:
            pad = lambda t: torch.cat([torch.zeros(1, dtype=t.dtype, device=dev), t.reshape(-1)])[1:]
            txy, tuv, tq = pad(txy), pad(tuv), pad(tq)
            torch.cuda.synchronize(dev)
            assert txy.data_ptr() % 16 == 8
        ctx = gpu.context(W, H, False)
        ctx.set_transform(*b["m"])
        ctx.set_color_transform(*b["ct"])
        for filt, ti, q in ((1, 0, tq), (0, 0, tq), (1, 1, tq), (1, 0, None)):
            bb = dict(b, tex=texs[ti])
            if q is None:
                del bb["q"]
            want = B.expected_payload(W, H, False, BG, "zw", FAR, [bb], filt=filt)
            ctx.set_color(*BG)
            ctx.set_depth_state(True, True)
            ctx.clear_depth(FAR)
            ctx.set_triangle_texture_filter(filt)
            ctx.draw_textured_triangles_device(gtex[ti], txy, tuv, n, z=tz, q=q)
            assert ctx.last_raster_path() == "order-free"
            _same(MR.read_frame(ctx, "zw"), want, f"device +{off} filter={filt} texture={ti} q={q is not None}")


# ---- meshes -----------------------------------------------------------------------------------
def _gpu_mesh(mesh):
    R = _R()
    if "uv" in mesh:
        return R.Mesh(mesh["pos"], mesh["idx"], uv=mesh["uv"])
    return R.Mesh(mesh["pos"], mesh["idx"], colors=mesh["colors"], gouraud=mesh["gouraud"])


def _mesh_ctx(gpu, mode, alpha=False, near=0.0, cull=0, persp=True, ct=CT, filt=1):
    ctx = gpu.context(W, H, alpha)
    MR.begin_frame(ctx, mode, MR.XFORM, ct, clear=FAR)
    ctx.set_mesh_near_plane(near)
    ctx.set_mesh_cull(cull)
    ctx.set_mesh_perspective(persp)
    ctx.set_triangle_texture_filter(filt)
    return ctx


@functools.lru_cache(maxsize=None)
def _matrix(name):
    M = P.mesh_matrix(name)
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def _mesh_want(name, near, cull, mode, rgba, persp, filt=1):
    tex = P.mesh_texture(rgba)
    b = P.mesh_batch(P.mesh_scene(), _matrix(name), tex, near, cull, persp, ct=CT)
    fn = B.expected_loop if rgba else B.expected_payload
    if b["xy"].shape[0] == 0:
        b = dict(b, z=None)
    return _frozen(fn(W, H, rgba, BG, mode, FAR, [b], filt=filt))


@pytest.mark.parametrize("persp", [False, True])
@pytest.mark.parametrize("state", P.MESH_STATES)
@pytest.mark.parametrize("name", MATRICES)
def test_mesh_frames(gpu, name, state, persp):
    near, cull = state
    gm = _gpu_mesh(P.mesh_scene())
    for rgba, modes in ((False, T.MODES), (True, ("zw",))):
        tex = gpu.texture(P.mesh_texture(rgba))
        for mode in modes:
            ctx = _mesh_ctx(gpu, mode, rgba, near, cull, persp)
            ctx.draw_mesh(gm, _matrix(name), texture=tex)
            assert ctx.last_raster_path() == ("ordered" if rgba else "order-free")
            what = f"{name} near={near} cull={cull} persp={persp} {mode} rgba={rgba}"
            _same(MR.read_frame(ctx, mode), _mesh_want(name, near, cull, mode, rgba, persp), what)
    if (name, near, cull) not in P.MESH_EMPTY:
        assert _differs(_mesh_want(name, near, cull, "zw", False, persp), _mesh_want(name, near, cull, "zw", False, persp, 0))


# ---- the state ----------------------------------------------------------------------------------
def test_state_default_rejection_save_restore_and_recording(gpu):
    R = _R()
    ctx = gpu.context(W, H, False)
    assert ctx.get_triangle_texture_filter() == 0            # nearest by default
    ctx.set_triangle_texture_filter(1)
    assert ctx.get_triangle_texture_filter() == 1
    for bad in (2, -1, 1 << 40):
        R.lib.ClearLastError()
        with pytest.raises(RuntimeError):
            ctx.set_triangle_texture_filter(bad)
        assert "SetTriangleTextureFilter" in R.lib.GetLastErrorString().decode()
        assert ctx.get_triangle_texture_filter() == 1        # the state is kept
        assert R.lib.SetTriangleTextureFilter(ctx._ptr, bad) is False
    R.lib.ClearLastError()
    ctx.save_state()
    ctx.set_triangle_texture_filter(0)
    ctx.restore_state()
    assert ctx.get_triangle_texture_filter() == 0            # not part of the stack: the last set stands
    ctx.save_state()
    ctx.set_triangle_texture_filter(1)
    ctx.restore_state()
    assert ctx.get_triangle_texture_filter() == 1
    ctx.set_triangle_texture_filter(0)
    # a command list does not capture it: a set while recording holds at once, and nothing is queued for it
    ctx.begin_commands()
    ctx.draw_rect(20.0, 15.0, 70.0, 50.0, 0.1, 0.9, 0.2, 1.0)
    ctx.set_triangle_texture_filter(1)
    assert ctx.get_triangle_texture_filter() == 1 and ctx.command_list_length() == 1
    ctx.end_commands()
    assert ctx.get_triangle_texture_filter() == 1
    assert gpu.context(W, H, False).get_triangle_texture_filter() == 0   # per context
    assert not R.lib.GetLastErrorString()


def test_other_draws_ignore_the_filter(gpu):
    """A colour batch, a colour mesh and draw_texture (which stays nearest)."""
    g = scenes.rng(50)
    b = T.soup(W, H, 60, 51, T.texture_rgb(), spread=40.0)
    rgba = g.uniform(0, 1, size=(60, 12))
    rgba[:, 3::4] = 1.0
    mesh = MR.sphere3d(rows=4, cols=6)
    gm = _gpu_mesh(mesh)
    img = T.texture_rgb(seed=52, w=12, h=10)
    frames = []
    for filt in (1, 0):
        out = []
        ctx = _one_batch_ctx(gpu, dict(b, ct=(1.0, 1.0, 1.0, 1.0)), filt=filt)
        ctx.draw_triangles(b["xy"], rgba, z=b["z"], gouraud=True)
        out.append(MR.read_frame(ctx, "zw"))
        ctx = _mesh_ctx(gpu, "zw", ct=(1.0, 1.0, 1.0, 1.0), filt=filt)
        ctx.draw_mesh(gm, _matrix("perspective"))
        out.append(MR.read_frame(ctx, "zw"))
        ctx = gpu.context(W, H, False)
        ctx.set_triangle_texture_filter(filt)
        ctx.set_color(*BG)
        ctx.draw_texture(gpu.texture(img), 7.5, 5.25, 100.0, 80.0)   # magnified: a filter would show
        out.append((ctx.get_buffer_numpy(), None))
        frames.append(out)
    for k, what in enumerate(("colour batch", "colour mesh", "draw_texture")):
        _same(frames[0][k], frames[1][k], what)
    ora = scenes.OracleFactory()
    octx = ora.context(W, H, False)
    octx.set_color(*BG)
    octx.draw_texture(ora.texture(img), 7.5, 5.25, 100.0, 80.0)
    _same(frames[0][2], (octx.get_buffer_numpy(), None), "draw_texture against the oracle")


@pytest.mark.parametrize("force", [False, True])
def test_pending_batch_keeps_the_filter_it_was_issued_with(gpu, force):
    for persp in (False, True):
        b = B.soup_batches("opaque", persp)[0]
        tex = gpu.texture(b["tex"])
        for first in (1, 0):
            ctx = _one_batch_ctx(gpu, b, filt=first)
            ctx.set_force_ordered_raster(force)
            ctx.draw_textured_triangles(tex, b["xy"], b["uv"], z=b["z"], q=b.get("q"))
            ctx.set_triangle_texture_filter(1 - first)      # before the first readback
            want = B.expected_payload(W, H, False, BG, "zw", CLEAR, [b], filt=first)
            _same(MR.read_frame(ctx, "zw"), want, f"issued with {first}, persp={persp}, force={force}")


# ---- cross-feature, one case each -----------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb", "yuv420p"])
def test_frame_output(gpu, fmt):
    """The rasters' fused frame output (a pending clear: written by the
    raster's own write-back) equals the u8 readback, or its YUV420P planes."""
    WW, HH = W - 2, H - 1            # (even sizes: 4:2:0 planes)
    for kind in ("opaque", "ct_alpha"):
        bs = B.soup_batches(kind, True)
        fn = B.expected_payload if kind == "opaque" else B.expected_loop
        ctx = gpu.context(WW, HH, False)
        ctx.set_frame_format(fmt)
        ctx.set_color(*BG)
        ctx.gather_frame_u8()    # the frame output is produced by the rasters from now on
        got = B.draw_gpu(ctx, gpu, "zw", CLEAR, BG, bs)
        ctx.gather_frame_u8()
        frame = ctx.get_frame_u8()
        _same(got, fn(WW, HH, False, BG, "zw", CLEAR, bs), f"frame output {kind}")
        u8 = ctx.get_buffer_as_uint8_numpy()
        assert np.array_equal(frame, scenes.yuv420p(u8) if fmt == "yuv420p" else u8), kind


def test_two_shards_assemble_the_unsharded_frame(gpu):
    from libnativecpurenderer_amd import sharding
    pat = sharding.band_pattern(2, None)
    for kind in ("opaque", "rgba_texture"):
        want = _expected(kind, "zw", False, True)
        seen = np.zeros(H, dtype=bool)
        for s in range(2):
            ctx = gpu.context(W, H, False)
            ctx.set_shard(2, s)
            got = B.draw_gpu(ctx, gpu, "zw", CLEAR, BG, B.soup_batches(kind, True))
            rows = [y for y in range(H) if pat[(y // 32) % len(pat)] == s]
            assert len(rows) >= 32
            seen[rows] = True
            _same((got[0][rows], got[1][rows]), (want[0][rows], want[1][rows]), f"shard {s} {kind}")
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
            ctx.set_triangle_texture_filter(1)
            ctx.draw_textured_triangles(gpu.texture(base["tex"]), base["xy"], base["uv"], q=base["q"])
            snap = ctx.as_texture_shared() if shared else ctx.as_texure()
            ctx.draw_textured_triangles(snap, over["xy"], over["uv"], q=over["q"])
            outs.append(ctx.get_buffer_numpy())
            if not shared:
                first = B.expected_payload(64, 40, False, BG, "nz", 0, [base])[0]
                want = B.expected_payload(64, 40, False, BG, "nz", 0, [base, dict(over, tex=first)])[0]
                assert scenes.bits_equal(outs[-1], want), scenes.first_mismatch(outs[-1], want)
        assert scenes.bits_equal(outs[0], outs[1]), scenes.first_mismatch(outs[0], outs[1])

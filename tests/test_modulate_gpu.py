"""Modulated textured triangle soups on the GPU (DrawTexturedTrianglesModulated
and its Device form: texel times interpolated vertex colour), bit for bit (f64
framebuffer, u32 depth) against tests/modulate_ref.py: both rasters, both
filters, the dense tile whose winners overflow the staged records, the two
identities, the device entry, the overflow re-run, fragment counting and the
latched errors."""
import functools

import numpy as np
import pytest

import bilinear_ref as BL
import mesh_ref as MR
import modulate_ref as M
import scenes
import textured_ref as T

pytestmark = pytest.mark.gpu

W, H, BG, CLEAR, FAR = M.W, M.H, M.BG, M.CLEAR, M.FAR


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


@functools.lru_cache(maxsize=None)
def _expected(kind, mode, alpha, persp, filt):
    bs = M.soup_batches(kind, persp)
    fn = M.expected_payload if kind == "opaque" else M.expected_loop
    info = {}
    want = fn(W, H, alpha, BG, mode, CLEAR, bs, info, filt=filt)
    assert info["covered"].mean() >= 0.5
    return _frozen(want)


# ---- soups: order-free and ordered raster, depth modes, filters, q spread and q == 1 ------------
@pytest.mark.parametrize("persp", [False, True])
@pytest.mark.parametrize("filt", [0, 1])
@pytest.mark.parametrize("mode", T.MODES)
def test_opaque_soups_on_both_rasters(gpu, mode, filt, persp):
    bs = M.soup_batches("opaque", persp)
    for alpha in (False, True):
        want = _expected("opaque", mode, alpha, persp, filt)
        for force in (False, True):
            ctx = gpu.context(W, H, alpha)
            ctx.set_force_ordered_raster(force)
            got = M.draw_gpu(ctx, gpu, mode, CLEAR, BG, bs, filt=filt)
            assert ctx.last_raster_path() == ("ordered" if force else "order-free")
            _same(got, want, f"opaque {mode} filter={filt} persp={persp} alpha={alpha} force={force}")


@pytest.mark.parametrize("filt", [0, 1])
@pytest.mark.parametrize("mode", T.MODES)
def test_blended_soups(gpu, mode, filt):
    bs = M.soup_batches("blended")
    for alpha in (False, True):
        ctx = gpu.context(W, H, alpha)
        got = M.draw_gpu(ctx, gpu, mode, CLEAR, BG, bs, filt=filt)
        assert ctx.last_raster_path() == "ordered"
        _same(got, _expected("blended", mode, alpha, True, filt), f"blended {mode} filter={filt} alpha={alpha}")


@pytest.mark.parametrize("kind", M.KINDS)
def test_small_frame(gpu, kind):
    bs = M.small_batches(kind)
    fn = M.expected_payload if kind == "opaque" else M.expected_loop
    for mode in T.MODES:
        for filt in (0, 1):
            want = fn(M.W2, M.H2, False, BG, mode, CLEAR, bs, filt=filt)
            ctx = gpu.context(M.W2, M.H2, False)
            got = M.draw_gpu(ctx, gpu, mode, CLEAR, BG, bs, filt=filt)
            assert ctx.last_raster_path() == ("order-free" if kind == "opaque" else "ordered")
            _same(got, want, f"small {kind} {mode} filter={filt}")


@pytest.mark.parametrize("filt", [0, 1])
def test_dense_tile_overflows_the_staged_records(gpu, filt):
    """More distinct winners in one tile than records are staged: the rest are loaded directly."""
    b = M.dense_batch()
    tex = gpu.texture(b["tex"])
    for mode in T.MODES:
        want = M.expected_payload(W, H, False, BG, mode, FAR, [b], filt=filt)
        for coop in (0, 1, 2):
            ctx = gpu.context(W, H, False)
            ctx.set_coop_raster(coop)
            got = M.draw_gpu(ctx, gpu, mode, FAR, BG, [b], [tex], filt=filt)
            assert ctx.last_raster_path() == "order-free"
            _same(got, want, f"dense {mode} filter={filt} coop={coop}")
    ctx = gpu.context(W, H, False)
    ctx.set_force_ordered_raster(True)
    _same(M.draw_gpu(ctx, gpu, "zw", FAR, BG, [b], [tex], filt=filt),
          M.expected_payload(W, H, False, BG, "zw", FAR, [b], filt=filt), f"dense ordered filter={filt}")


def test_path_follows_the_opacity_rule(gpu):
    """Order-free exactly when: no texture alpha, every corner alpha 1, ct[3] == 1, ordered not forced."""
    b = M.soup_batches("opaque")[0]
    one_alpha = b["rgba"].copy()
    one_alpha[-1, 11] = 0.5
    cases = [
        ("opaque", b, "order-free"),
        ("one corner alpha", dict(b, rgba=one_alpha), "ordered"),
        ("texture alpha", dict(b, tex=T.texture_rgba()), "ordered"),
        ("ct alpha", dict(b, ct=M.CT_BLEND), "ordered"),
    ]
    for what, bb, path in cases:
        ctx = gpu.context(W, H, False)
        got = M.draw_gpu(ctx, gpu, "zw", CLEAR, BG, [bb])
        assert ctx.last_raster_path() == path, what
        fn = M.expected_payload if path == "order-free" else M.expected_loop
        _same(got, fn(W, H, False, BG, "zw", CLEAR, [bb]), what)


# ---- identities ---------------------------------------------------------------------------
@pytest.mark.parametrize("force", [False, True])
@pytest.mark.parametrize("filt", [0, 1])
def test_unit_colours_give_the_perspective_draws_frame(gpu, filt, force):
    """I1: against the library's own DrawTexturedTrianglesPerspective with the same q."""
    for persp in (False, True):
        bs = [M.ones_colours(b) for b in M.soup_batches("opaque", persp)]
        frames = []
        for draw in (M.draw_gpu, BL.draw_gpu):
            ctx = gpu.context(W, H, True)
            ctx.set_force_ordered_raster(force)
            frames.append(draw(ctx, gpu, "zw", CLEAR, BG, bs, filt=filt))
        _same(frames[0], frames[1], f"I1 filter={filt} force={force} persp={persp}")
        _same(frames[0], BL.expected_payload(W, H, True, BG, "zw", CLEAR, bs, filt=filt), "I1 against the reference")


@pytest.mark.parametrize("force", [False, True])
def test_unit_texture_gives_the_oracles_gouraud_frame(gpu, force):
    """I2, nearest filter: against the oracle's own Gouraud DrawTriangles."""
    for kind in M.KINDS:
        bs = [M.ones_texture(b) for b in M.soup_batches(kind)]
        for mode in T.MODES:
            ctx = gpu.context(W, H, True)
            ctx.set_force_ordered_raster(force)
            got = M.draw_gpu(ctx, gpu, mode, CLEAR, BG, bs, filt=0)
            _same(got, M.expected_gouraud(W, H, True, BG, mode, CLEAR, bs), f"I2 {kind} {mode} force={force}")


# ---- the device entry ------------------------------------------------------------------------
def _device_arrays(dev, b, n, off):
    import torch
    arrs = [np.ascontiguousarray(b["xy"][:n]), M.uvc(b)[:n], np.ascontiguousarray(b["z"][:n]),
            np.ascontiguousarray(b["q"][:n])]
    out = []
    for a in arrs:
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev).reshape(-1)
        if off:
            t = torch.cat([torch.zeros(1, dtype=t.dtype, device=dev), t])[1:]
        out.append(t)
    torch.cuda.synchronize(dev)
    return out


@pytest.mark.parametrize("off", [0, 1])
def test_device_entry(gpu, off):
    import torch
    dev = torch.device("cuda", gpu.context(8, 8, False).device)
    b257 = M.with_colours(M.P.soup(W, H, 257, 91, T.texture_rgb(), spread=30.0, ct=M.CT), 92)
    b90 = M.soup_batches("opaque")[0]
    blended = b90["rgba"].copy()
    blended[89, 11] = 0.5   # one alpha != 1, in the last triangle: found by the device scan
    cases = [("n=257", b257, 257, "order-free"), ("n=1", b257, 1, "order-free"), ("n=90", b90, 90, "order-free"),
             ("last alpha", dict(b90, rgba=blended), 90, "ordered")]
    for what, b, n, path in cases:
        sub = dict(b, xy=b["xy"][:n], uv=b["uv"][:n], z=b["z"][:n], q=b["q"][:n], rgba=b["rgba"][:n])
        fn = M.expected_payload if path == "order-free" else M.expected_loop
        txy, tuvc, tz, tq = _device_arrays(dev, sub, n, off)
        assert txy.data_ptr() % 16 == (8 if off else 0) and tuvc.data_ptr() % 16 == (8 if off else 0)
        for filt in (0, 1):
            if path == "ordered" and filt:
                continue
            want = fn(W, H, False, BG, "zw", CLEAR, [sub], filt=filt)
            ctx = gpu.context(W, H, False)
            MR.begin_frame(ctx, "zw", sub["m"], sub["ct"], bg=BG, clear=CLEAR)
            ctx.set_triangle_texture_filter(filt)
            ctx.draw_textured_triangles_device(gpu.texture(sub["tex"]), txy, tuvc, n, z=tz, q=tq, colors=True)
            assert ctx.last_raster_path() == path, what
            _same(MR.read_frame(ctx, "zw"), want, f"device +{off} {what} filter={filt}")


# ---- a pending batch's re-run, fragment counting ---------------------------------------------
@pytest.mark.parametrize("filt", [0, 1])
def test_pair_capacity_overflow_rerun_stays_exact(gpu, filt):
    b = M.soup_batches("opaque")[0]
    want = M.expected_payload(W, H, False, BG, "zw", CLEAR, [b], filt=filt)
    ctx = gpu.context(W, H, False)
    MR.begin_frame(ctx, "zw", b["m"], b["ct"], bg=BG, clear=CLEAR)
    ctx.set_triangle_texture_filter(filt)
    ctx.set_pair_capacity_override(50)
    ctx.draw_textured_triangles(gpu.texture(b["tex"]), b["xy"], b["uv"], z=b["z"], q=b["q"], colors=b["rgba"])
    ctx.set_triangle_texture_filter(1 - filt)   # (the re-run keeps the snapshot's mode)
    _same(MR.read_frame(ctx, "zw"), want, "overflow re-run")


@pytest.mark.parametrize("force", [False, True])
def test_fragment_count_equals_the_gouraud_draws(gpu, force):
    b = M.soup_batches("opaque")[0]
    counts = []
    for modulated in (True, False):
        ctx = gpu.context(W, H, False)
        MR.begin_frame(ctx, "zw", b["m"], b["ct"], bg=BG, clear=CLEAR)
        ctx.set_force_ordered_raster(force)
        ctx.set_fragment_counting(True)
        if modulated:
            ctx.draw_textured_triangles(gpu.texture(b["tex"]), b["xy"], b["uv"], z=b["z"], q=b["q"], colors=b["rgba"])
            _same(MR.read_frame(ctx, "zw"), M.expected_payload(W, H, False, BG, "zw", CLEAR, [b]), "counting frame")
        else:
            ctx.draw_triangles(b["xy"], b["rgba"], z=b["z"], gouraud=True)
        counts.append(ctx.get_fragment_count())
    assert counts[0] == counts[1] > 1000, counts


# ---- errors -----------------------------------------------------------------------------------
def test_soup_errors_latch_and_draw_nothing(gpu):
    R = _R()
    b = M.soup_batches("opaque")[0]
    n = 10
    xy, uvc, q = np.ascontiguousarray(b["xy"][:n]), M.uvc(b)[:n].copy(), np.ascontiguousarray(b["q"][:n])
    A = lambda a: a.ctypes.data
    ctx = gpu.context(W, H, False)
    ctx.set_color(*BG)
    before = ctx.get_buffer_numpy()
    good = gpu.texture(b["tex"])
    thin = gpu.texture(np.ones((5, 1, 3)))
    name = "DrawTexturedTrianglesModulated"
    cases = {
        "NULL uvc": (lambda: R.lib.DrawTexturedTrianglesModulated(ctx._ptr, good._ptr, A(xy), None, None, A(q), n),
                     name + ": NULL uvc"),
        "NULL q": (lambda: R.lib.DrawTexturedTrianglesModulated(ctx._ptr, good._ptr, A(xy), None, A(uvc), None, n),
                   name + ": NULL q"),
        "NULL texture": (lambda: R.lib.DrawTexturedTrianglesModulated(ctx._ptr, None, A(xy), None, A(uvc), A(q), n),
                         name + ": NULL texture"),
        "thin texture": (lambda: R.lib.DrawTexturedTrianglesModulated(ctx._ptr, thin._ptr, A(xy), None, A(uvc), A(q), n),
                         name + ": texture narrower or lower than 2 texels"),
        "NULL uvc, device": (lambda: R.lib.DrawTexturedTrianglesModulatedDevice(ctx._ptr, good._ptr, None, None, None, None, n),
                             name + "Device: NULL uvc"),
    }
    for what, (call, msg) in cases.items():
        R.lib.ClearLastError()
        call()
        err = R.lib.GetLastErrorString()
        err = err.decode() if isinstance(err, bytes) else err
        assert err == msg, (what, err)
        assert scenes.bits_equal(ctx.get_buffer_numpy(), before), what

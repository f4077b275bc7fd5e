"""Textured triangles on the GPU, bit for bit (f64 framebuffer, u32 depth, u8
readback) against frames derived from the oracle (tests/textured_ref.py: the
oracle's own DrawTriangles and ApplyPixel plus the numpy sampler): both
rasters, every depth mode, RGB / RGBA textures and contexts, the k_vis
variants (flattened, split tiles, 512 threads by way of shards, overflow
re-run), TriangleBuffers and warm binning, the edge cases of the sampler and
of the entry points, frame outputs and shards."""
import functools

import numpy as np
import pytest

import scenes
import textured_ref as T

pytestmark = pytest.mark.gpu

W, H = 200, 140            # 4 x 5 tiles, partial right and bottom tiles
BG = (0.25, 0.25, 0.25, 0.25)
CLEAR = 0x90000000         # z in (0.05, 0.99): both outcomes of the LESS test
CT = (0.9, 0.8, 0.7, 1.0)
CT_BLEND = (0.9, 0.8, 0.7, 0.5)
KINDS = ("opaque", "ct_alpha", "rgba_texture")


def _same(got, want, what):
    assert scenes.bits_equal(got[0], want[0]), (what, scenes.first_mismatch(got[0], want[0]))
    if want[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "depth", scenes.first_mismatch(got[1], want[1]))


def _batches(kind, const_uv=False, n=(240, 80)):
    """Two overlapping batches: the first under a scale + rotate + translate
    transform, the second (another texture size) drawn over it."""
    if kind == "rgba_texture":
        t1, t2 = T.texture_rgba(), T.texture_rgba(seed=9, w=12, h=10)
    else:
        t1, t2 = T.texture_rgb(), T.texture_rgb(seed=8, w=11, h=7)
    ct = CT_BLEND if kind == "ct_alpha" else CT
    return [T.soup(W, H, n[0], 11, t1, m=T.XFORM, ct=ct, const_uv=const_uv),
            T.soup(W, H, n[1], 12, t2, ct=ct, const_uv=const_uv)]


@functools.lru_cache(maxsize=None)
def _expected(kind, mode, alpha):
    bs = _batches(kind)
    info = {}
    if kind == "opaque":
        want = T.expected_payload(W, H, alpha, BG, mode, CLEAR, bs, info)
        if mode != "nz":   # both depth outcomes: pixels some fragment covers, where none / one passes
            every = {}
            T.expected_payload(W, H, alpha, BG, "nz", CLEAR, bs, every)
            info["zpass"] = int(info["covered"].sum())
            info["zfail"] = int((every["covered"] & ~info["covered"]).sum())
    else:
        want = T.expected_loop(W, H, alpha, BG, mode, CLEAR, bs, info)
    # the expected frame itself exercises what the test is about
    assert info["covered"].mean() >= 0.5, info["covered"].mean()
    assert len(info["texels"]) >= 100, len(info["texels"])
    if mode != "nz":
        assert info["zpass"] > 0 and info["zfail"] > 0, (info["zpass"], info["zfail"])
    for a in want:
        if a is not None:
            a.setflags(write=False)
    return want


@pytest.mark.parametrize("alpha", [False, True])
@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_parity_across_modes(gpu, kind, mode, alpha):
    want = _expected(kind, mode, alpha)
    ctx = gpu.context(W, H, alpha)
    got = T.draw_gpu(ctx, gpu, mode, CLEAR, BG, _batches(kind))
    assert ctx.last_raster_path() == ("order-free" if kind == "opaque" else "ordered")
    _same(got, want, f"{kind} {mode} alpha={alpha}")
    if kind == "opaque":   # results must not depend on the path
        ctx = gpu.context(W, H, alpha)
        ctx.set_force_ordered_raster(True)
        got = T.draw_gpu(ctx, gpu, mode, CLEAR, BG, _batches(kind))
        assert ctx.last_raster_path() == "ordered"
        _same(got, want, f"{kind} {mode} alpha={alpha} forced ordered")


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_constant_uv_equals_flat_colour(gpu, kind, mode):
    """One (u, v) per triangle: the oracle's own flat DrawTriangles is the
    expected frame; through both rasters, which must also agree."""
    bs = _batches(kind, const_uv=True)
    for alpha in (False, True):
        want = T.expected_flat(W, H, alpha, BG, mode, CLEAR, bs)
        outs = []
        for force in (False, True):
            ctx = gpu.context(W, H, alpha)
            ctx.set_force_ordered_raster(force)
            outs.append(T.draw_gpu(ctx, gpu, mode, CLEAR, BG, bs))
            assert ctx.last_raster_path() == ("order-free" if kind == "opaque" and not force else "ordered")
            _same(outs[-1], want, f"{kind} {mode} alpha={alpha} force={force}")
        _same(outs[0], outs[1], f"{kind} {mode} alpha={alpha}: free vs ordered")


@pytest.mark.parametrize("coop", [1, 2])
def test_coop_raster_variants(gpu, coop):
    for mode in T.MODES:
        ctx = gpu.context(W, H, False)
        ctx.set_coop_raster(coop)
        _same(T.draw_gpu(ctx, gpu, mode, CLEAR, BG, _batches("opaque")), _expected("opaque", mode, False),
              f"coop {coop} {mode}")


def test_large_triangles_take_the_flattened_variant(gpu):
    tex = T.texture_rgb()
    bs = [T.soup(W, H, 30, 21, tex, spread=60.0, m=T.XFORM, ct=CT)]
    for mode in T.MODES:
        for alpha in (False, True):
            want = T.expected_payload(W, H, alpha, BG, mode, CLEAR, bs)
            ctx = gpu.context(W, H, alpha)
            got = T.draw_gpu(ctx, gpu, mode, CLEAR, BG, bs)   # (no history: the flattened raster)
            assert ctx.last_raster_path() == "order-free"
            _same(got, want, f"large {mode} alpha={alpha}")


@functools.lru_cache(maxsize=None)
def _dense():
    DW, DH = 256, 160
    tex = T.texture_rgb()
    bs = [T.soup(DW, DH, 20000, 31, tex, spread=3.0, ct=CT, zrange=(0.0, 1.0))]
    wants = {(mode, alpha): T.expected_payload(DW, DH, alpha, BG, mode, 0xFFFFFFFF, bs)
             for mode in T.MODES for alpha in (False, True)}
    return DW, DH, bs, wants


@pytest.mark.parametrize("limits", [(64, 64), (200, 96)])
def test_split_dense_tiles(gpu, limits):
    DW, DH, bs, wants = _dense()
    tex = gpu.texture(bs[0]["tex"])
    for (mode, alpha), want in wants.items():
        ctx = gpu.context(DW, DH, alpha)
        ctx.set_split_limits(*limits)
        _same(T.draw_gpu(ctx, gpu, mode, 0xFFFFFFFF, BG, bs, [tex]), want, f"split {limits} {mode} alpha={alpha}")


def test_pair_capacity_overflow_rerun(gpu):
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    b = _batches("opaque")[0]
    tex = gpu.texture(b["tex"])
    want = T.expected_payload(W, H, False, BG, "zw", CLEAR, [b])
    for use_buffer in (False, True):
        ctx = gpu.context(W, H, False)
        ctx.set_pair_capacity_override(50)
        ctx.set_color(*BG)
        ctx.set_depth_state(True, True)
        ctx.clear_depth(CLEAR)
        ctx.set_transform(*b["m"])
        ctx.set_color_transform(*b["ct"])
        if use_buffer:
            ctx.draw_triangle_buffer(R.TriangleBuffer(b["xy"], uv=b["uv"], z=b["z"]), tex)
        else:
            ctx.draw_textured_triangles(tex, b["xy"], b["uv"], z=b["z"])
        _same((ctx.get_buffer_numpy(), ctx.get_depth_buffer()), want, f"overflow re-run buffer={use_buffer}")


def test_triangle_buffer_warm_frames_and_device_pointers(gpu):
    import torch
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    b = _batches("opaque")[0]
    tex_a, tex_b = T.texture_rgb(), T.texture_rgb(seed=8, w=11, h=7)
    ga, gb = gpu.texture(tex_a), gpu.texture(tex_b)
    buf = R.TriangleBuffer(b["xy"], uv=b["uv"], z=b["z"])
    assert buf.textured and buf.n == 240
    ctx = gpu.context(W, H, False)
    ctx.set_depth_state(True, True)
    ctx.set_color_transform(*CT)
    m2 = (1.0, 0.0, 0.0, 1.0, 3.0, -2.0)
    wants = {}
    for frame in range(5):
        tex, gtex = (tex_b, gb) if frame == 3 else (tex_a, ga)
        m = m2 if frame == 4 else b["m"]
        key = (frame == 3, frame == 4)
        if key not in wants:
            wants[key] = T.expected_payload(W, H, False, BG, "zw", CLEAR, [dict(b, tex=tex, m=m)])
        ctx.set_color(*BG)
        ctx.clear_depth(CLEAR)
        ctx.set_transform(*m)
        warm = ctx.warm_batch_count()
        ctx.draw_triangle_buffer(buf, gtex)
        assert ctx.last_raster_path() == "order-free"
        if frame == 3:   # a repeat draw with another texture stays warm (binning reads only xy)
            assert ctx.warm_batch_count() == warm + 1
        _same((ctx.get_buffer_numpy(), ctx.get_depth_buffer()), wants[key], f"frame {frame}")
    assert ctx.warm_batch_count() >= 2
    assert ctx.warm_failure_count() == 0
    # the device-pointer entry point on torch tensors: the same frame
    dev = torch.device("cuda", ctx.device)
    txy = torch.from_numpy(b["xy"]).to(dev)
    tuv = torch.from_numpy(b["uv"]).to(dev)
    tz = torch.from_numpy(b["z"]).to(dev)
    torch.cuda.synchronize(dev)
    for off in (0, 1):   # (1: arrays that are not 16-byte aligned are re-staged)
        if off:
            pad = lambda t: torch.cat([torch.zeros(1, dtype=t.dtype, device=dev), t.reshape(-1)])[1:]
            txy, tuv = pad(txy), pad(tuv)
            torch.cuda.synchronize(dev)
            assert txy.data_ptr() % 16 == 8
        c2 = gpu.context(W, H, False)
        c2.set_depth_state(True, True)
        c2.set_color_transform(*CT)
        c2.set_color(*BG)
        c2.clear_depth(CLEAR)
        c2.set_transform(*b["m"])
        c2.draw_textured_triangles_device(ga, txy, tuv, 240, z=tz)
        _same((c2.get_buffer_numpy(), c2.get_depth_buffer()), wants[(False, False)], f"device pointers +{off}")


def _edge_ctx(gpu, alpha=False):
    ctx = gpu.context(64, 40, alpha)
    ctx.set_color(*BG)
    ctx.set_depth_state(False, False)
    return ctx


def test_nan_and_huge_coordinates(gpu):
    """A NaN coordinate is defined as coordinate 0; +-1e300 clamps."""
    tex = T.texture_rgb()
    xy = np.array([[2.0, 2.0, 60.0, 4.0, 30.0, 38.0]] * 3) + np.array([[0.0], [1.5], [3.0]])
    uv = np.array([[np.nan, 5.0, 10.0, 5.0, 20.0, 9.0],          # u NaN everywhere: column 0, v varies
                   [1e300, 3.0, 1e300, 8.0, 1e300, 20.0],        # u clamps to w-2
                   [-1e300, -1e300, 5.0, 1e300, 30.0, 4.0]])     # mixed huge values: inf - inf -> NaN inside
    for force in (False, True):
        for k in range(3):
            b = dict(xy=xy[k:k + 1], uv=uv[k:k + 1], z=None, tex=tex, ct=CT, m=T.IDENT)
            want = T.expected_payload(64, 40, False, BG, "nz", 0, [b])
            ctx = _edge_ctx(gpu)
            ctx.set_force_ordered_raster(force)
            _same(T.draw_gpu(ctx, gpu, "nz", 0, BG, [b]), want, f"edge uv {k} force={force}")
            if k == 0:   # pinned: every covered pixel samples column 0
                cov = want[0][..., 0] != BG[0]
                assert cov.sum() > 200
                col0 = {tuple(tex[r, 0] * np.array(CT[:3])) for r in range(tex.shape[0])}
                assert {tuple(p) for p in want[0][cov]} <= col0


@pytest.mark.parametrize("channels", [3, 4])
def test_two_by_two_texture_samples_texel_zero(gpu, channels):
    """Clamp bounds w-2 = h-2 = 0: every sample is texel (0, 0) -- an RGB
    texture through k_vis (and the ordered raster when forced), an RGBA one
    through the ordered raster."""
    tex = scenes.rng(3).uniform(0, 1, size=(2, 2, channels))
    b = T.soup(64, 40, 20, 7, tex, spread=25.0, ct=(1.0, 1.0, 1.0, 1.0))
    flat = dict(b, uv=np.zeros_like(b["uv"]))
    want = T.expected_flat(64, 40, True, BG, "nz", 0, [flat])
    for force in (False, True):
        ctx = _edge_ctx(gpu, True)
        ctx.set_force_ordered_raster(force)
        _same(T.draw_gpu(ctx, gpu, "nz", 0, BG, [b]), want, f"2x2 texture, {channels} channels, force={force}")
        assert ctx.last_raster_path() == ("order-free" if channels == 3 and not force else "ordered")


def test_self_aliasing_texture_is_a_snapshot(gpu):
    """as_texture_shared() of the target: sampled as it was before the draw,
    the same result as a copied texture (as_texure)."""
    base = T.soup(64, 40, 25, 5, T.texture_rgb(), spread=25.0, ct=CT)
    over = T.soup(64, 40, 25, 6, np.zeros((40, 64, 3)), spread=25.0, ct=CT)
    for force in (False, True):
        outs = []
        for shared in (True, False):
            ctx = _edge_ctx(gpu)
            ctx.set_force_ordered_raster(force)
            ctx.set_color_transform(*CT)
            ctx.draw_textured_triangles(gpu.texture(base["tex"]), base["xy"], base["uv"])
            snap = ctx.as_texture_shared() if shared else ctx.as_texure()
            ctx.draw_textured_triangles(snap, over["xy"], over["uv"])
            outs.append(ctx.get_buffer_numpy())
            if not shared:
                first = T.expected_payload(64, 40, False, BG, "nz", 0, [base])[0]
                want = T.expected_payload(64, 40, False, BG, "nz", 0, [base, dict(over, tex=first)])[0]
                assert scenes.bits_equal(outs[-1], want), scenes.first_mismatch(outs[-1], want)
        assert scenes.bits_equal(outs[0], outs[1]), scenes.first_mismatch(outs[0], outs[1])


def test_rejected_draws_latch_an_error_and_draw_nothing(gpu):
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    b = T.soup(64, 40, 10, 5, T.texture_rgb(), spread=25.0)
    ctx = _edge_ctx(gpu)
    before = ctx.get_buffer_numpy()
    good = gpu.texture(b["tex"])
    thin = gpu.texture(np.ones((5, 1, 3)))                      # 1 x 5
    tbuf = R.TriangleBuffer(b["xy"], uv=b["uv"])
    cbuf = R.TriangleBuffer(b["xy"], np.ones((10, 4)))
    xy = np.ascontiguousarray(b["xy"]); uv = np.ascontiguousarray(b["uv"])
    P = lambda a: a.ctypes.data
    calls = {
        "1x5 texture": lambda: ctx.draw_textured_triangles(thin, b["xy"], b["uv"]),
        "1x5 texture, buffer": lambda: ctx.draw_triangle_buffer(tbuf, thin),
        "NULL texture": lambda: R.lib.DrawTexturedTriangles(ctx._ptr, None, P(xy), None, P(uv), 10),
        "NULL texture, buffer": lambda: R.lib.DrawTexturedTriangleBuffer(ctx._ptr, tbuf._ptr, None),
        "textured buffer in DrawTriangleBuffer": lambda: R.lib.DrawTriangleBuffer(ctx._ptr, tbuf._ptr),
        "colour buffer in DrawTexturedTriangleBuffer":
            lambda: R.lib.DrawTexturedTriangleBuffer(ctx._ptr, cbuf._ptr, good._ptr),
    }
    try:
        for what, call in calls.items():
            R.lib.ClearLastError()
            assert not R.lib.GetLastErrorString()
            call()
            assert R.lib.GetLastErrorString(), what
            after = ctx.get_buffer_numpy()
            assert scenes.bits_equal(after, before), what
    finally:
        R.lib.ClearLastError()
    with pytest.raises(ValueError):
        ctx.draw_triangle_buffer(tbuf)
    with pytest.raises(ValueError):
        ctx.draw_triangle_buffer(cbuf, good)
    # and the context still draws
    ctx.draw_triangle_buffer(tbuf, good)
    want = T.expected_payload(64, 40, False, BG, "nz", 0, [dict(b, z=None, ct=(1.0, 1.0, 1.0, 1.0))])[0]
    assert scenes.bits_equal(ctx.get_buffer_numpy(), want)
    assert not R.lib.GetLastErrorString()


@pytest.mark.parametrize("fmt", ["rgb", "yuv420p"])
def test_frame_output(gpu, fmt):
    """The rasters' fused frame output (a pending clear: written by the
    raster's own write-back) equals the u8 readback, or its YUV420P planes."""
    for kind in ("opaque", "ct_alpha"):
        ctx = gpu.context(W, H, False)
        ctx.set_frame_format(fmt)
        ctx.set_color(*BG)
        ctx.gather_frame_u8()    # the frame output is produced by the rasters from now on
        got = T.draw_gpu(ctx, gpu, "zw", CLEAR, BG, _batches(kind))
        ctx.gather_frame_u8()
        frame = ctx.get_frame_u8()
        _same(got, _expected(kind, "zw", False), f"frame output {kind}")
        u8 = ctx.get_buffer_as_uint8_numpy()
        if fmt == "rgb":
            assert np.array_equal(frame, u8), kind
            assert np.array_equal(ctx.get_frame_yuv420p(), scenes.yuv420p(u8)), kind
        else:
            assert np.array_equal(frame, scenes.yuv420p(u8)), kind


def test_shards_own_their_bands(gpu):
    from libnativecpurenderer_amd import sharding
    for kind in ("opaque", "rgba_texture"):
        want = _expected(kind, "zw", False)
        pat = sharding.band_pattern(2, None)
        for s in range(2):
            ctx = gpu.context(W, H, False)
            ctx.set_shard(2, s)
            got = T.draw_gpu(ctx, gpu, "zw", CLEAR, BG, _batches(kind))
            rows = [y for y in range(H) if pat[(y // 32) % len(pat)] == s]
            assert len(rows) > 32
            _same((got[0][rows], got[1][rows]), (want[0][rows], want[1][rows]), f"shard {s} {kind}")

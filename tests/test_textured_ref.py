"""CPU checks for textured triangles: the expected-frame helper
(tests/textured_ref.py) against the oracle itself, and the new entry points'
presence in the header, the ctypes table, the built library and the binding.
No GPU call is made here."""
import os
import re
import subprocess

import numpy as np
import pytest

import scenes
import textured_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["DrawTexturedTriangles", "DrawTexturedTrianglesDevice", "CreateTexturedTriangleBuffer",
               "DrawTexturedTriangleBuffer"]
W, H = 96, 70
BG = (0.2, 0.3, 0.4, 0.5)


def _same(a, b, what):
    assert scenes.bits_equal(a[0], b[0]), (what, scenes.first_mismatch(a[0], b[0]))
    if a[1] is None:
        assert b[1] is None
    else:
        assert np.array_equal(a[1], b[1]), (what, scenes.first_mismatch(a[1], b[1]))


@pytest.mark.parametrize("mode", T.MODES)
def test_payload_and_loop_derivations_agree(mode):
    """Opaque scene, two overlapping batches (the second under another
    transform and texture): both derivations give the same frame and depth."""
    rgb = T.texture_rgb()
    b1 = T.soup(W, H, 60, 3, rgb, spread=30.0)
    b2 = T.soup(W, H, 40, 4, T.texture_rgb(seed=8, w=11, h=7), spread=30.0, m=T.XFORM, ct=(1.0, 0.5, 0.25, 1.0))
    for alpha in (False, True):
        a = T.expected_payload(W, H, alpha, BG, mode, 0x90000000, [b1, b2])
        info = {}
        b = T.expected_loop(W, H, alpha, BG, mode, 0x90000000, [b1, b2], info)
        _same(a, b, f"{mode} alpha={alpha}")
        assert info["covered"].mean() > 0.3
        if mode != "nz":
            assert info["zpass"] > 0 and info["zfail"] > 0


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("kind", ["opaque", "rgba_texture", "ct_alpha"])
def test_constant_uv_equals_oracle_flat_triangles(mode, kind):
    """Three vertices sharing one (u, v): every fragment samples one texel, so
    the frame must be the oracle's own flat DrawTriangles with that texel as
    the colour -- the helper's expected frame checked against the oracle alone."""
    tex = T.texture_rgba() if kind == "rgba_texture" else T.texture_rgb()
    ct = (0.9, 0.8, 0.7, 0.5) if kind == "ct_alpha" else (0.9, 0.8, 0.7, 1.0)
    b1 = T.soup(W, H, 60, 5, tex, spread=30.0, ct=ct, const_uv=True)
    b2 = T.soup(W, H, 40, 6, tex, spread=30.0, ct=ct, m=T.XFORM, const_uv=True)
    for alpha in (False, True):
        want = T.expected_flat(W, H, alpha, BG, mode, 0x90000000, [b1, b2])
        _same(T.expected_loop(W, H, alpha, BG, mode, 0x90000000, [b1, b2]), want, f"loop {mode} {kind} {alpha}")
        if kind == "opaque":
            _same(T.expected_payload(W, H, alpha, BG, mode, 0x90000000, [b1, b2]), want,
                  f"payload {mode} {alpha}")


def test_sampler_clamps_truncation_and_nan():
    tex = np.arange(5 * 7 * 3, dtype=np.float64).reshape(5, 7, 3)
    u = np.array([-1.0, 0.0, 0.99, 5.0, 5.99, 6.0, 1e300, -1e300, np.nan, np.inf, -np.inf, 2.5])
    v = np.array([np.nan, -0.0, 3.0, 3.99, 4.0, 1e300, 0.5, 2.0, 1.0, -np.inf, np.inf, -3.0])
    t, idx = T.sample(tex, u, v)
    xs = [0, 0, 0, 5, 5, 5, 5, 0, 0, 5, 0, 2]
    ys = [0, 0, 3, 3, 3, 3, 0, 2, 1, 0, 3, 0]
    assert idx.tolist() == [y * 7 + x for x, y in zip(xs, ys)]
    assert np.array_equal(t[:, :3], tex[ys, xs]) and np.all(t[:, 3] == 1.0)
    two, idx2 = T.sample(np.ones((2, 2, 4)) * 0.25, u, v)
    assert np.all(idx2 == 0) and np.all(two == 0.25)


# ---- ABI -------------------------------------------------------------------
def test_new_symbols_in_header_and_table():
    from libnativecpurenderer_amd import _abi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "libNativeCPURenderer.h")).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _abi.HIP_LIBRARY_ABI and s in _abi.DEVICE_ABI, s
        assert s not in _abi.TRIANGLE_ABI and s not in _abi.ORACLE_ABI, s


def test_new_symbols_exported_unmangled():
    from libnativecpurenderer_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for s in NEW_SYMBOLS:
        assert s in defined, s


def test_binding_has_the_textured_methods():
    import inspect
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    assert callable(R.RenderContext.draw_textured_triangles)
    assert callable(R.RenderContext.draw_textured_triangles_device)
    assert "texture" in inspect.signature(R.RenderContext.draw_triangle_buffer).parameters
    assert "uv" in inspect.signature(R.TriangleBuffer.__init__).parameters
    with pytest.raises(ValueError):
        R.TriangleBuffer(np.zeros((1, 6)))                                   # neither rgba nor uv
    with pytest.raises(ValueError):
        R.TriangleBuffer(np.zeros((1, 6)), np.zeros((1, 4)), uv=np.zeros((1, 6)))   # both

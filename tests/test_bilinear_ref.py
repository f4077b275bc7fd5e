"""The bilinear reference itself (tests/bilinear_ref.py), on the CPU: the numpy
sampler against a scalar transcription of the filter, the kernels' clamp form
against the literal one, the filter's algebraic properties, the agreement of
the two frame derivations, and that the scenes the GPU tests draw can tell a
bilinear frame from a nearest one and reach every branch of the clamps."""
import functools
import math

import numpy as np
import pytest

import bilinear_ref as B
import persp_ref as P
import scenes
import textured_ref as T

W, H = B.W, B.H


def _scalar(tex, x, y):
    """One sample in Python floats, statement by statement as the reference's
    sampler body states the filter (its clamps, then the commented-out part)."""
    h, w, c = tex.shape
    alpha = c == 4
    if math.isnan(x):        # (the project's rule: a NaN coordinate is 0)
        x = 0.0
    if math.isnan(y):
        y = 0.0
    if x < 0:
        x = 0.0
    if x >= w - 1:
        x = float(w - 2)
    if y < 0:
        y = 0.0
    if y >= h - 1:
        y = float(h - 2)
    ix = int(x)
    iy = int(y)
    nx = ix + 1
    ny = iy + 1
    flat = tex.reshape(-1).tolist()
    ipp = 4 if alpha else 3
    index0 = iy * w * ipp + ix * ipp
    index1 = iy * w * ipp + nx * ipp
    index2 = ny * w * ipp + ix * ipp
    index3 = ny * w * ipp + nx * ipp
    u = x - ix
    v = y - iy
    out = []
    for k in range(3):
        c0, c1, c2, c3 = flat[index0 + k], flat[index1 + k], flat[index2 + k], flat[index3 + k]
        out.append(c0 * (1 - u) * (1 - v) + c1 * u * (1 - v) + c2 * (1 - u) * v + c3 * u * v)
    if alpha:
        a0, a1, a2, a3 = flat[index0 + 3], flat[index1 + 3], flat[index2 + 3], flat[index3 + 3]
        out.append(a0 * (1 - u) * (1 - v) + a1 * u * (1 - v) + a2 * (1 - u) * v + a3 * u * v)
    else:
        out.append(1.0)
    return out


def _edge_values(n):
    """Coordinates around every branch of the clamps of an axis of n texels."""
    return [0.0, -0.0, -1e-300, -0.5, -7.0, 0.25, 0.5, 1.0 - 2.0 ** -53, float(n - 2), n - 2 + 0.375,
            np.nextafter(float(n - 1), 0.0), float(n - 1), np.nextafter(float(n - 1), np.inf), n + 3.5, 1e19, 2.0 ** 31,
            2.0 ** 63, 1e300, -1e300, np.inf, -np.inf, np.nan]


TEXTURES = [("2x2 rgb", lambda: scenes.rng(1).uniform(0, 1, size=(2, 2, 3))),
            ("2x2 rgba", lambda: scenes.rng(2).uniform(0, 1, size=(2, 2, 4))),
            ("37x23 rgb", T.texture_rgb),
            ("16x9 rgba", T.texture_rgba),
            ("11x7 rgb", lambda: T.texture_rgb(seed=8, w=11, h=7))]


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("name,make", TEXTURES)
def test_sampler_equals_the_scalar_transcription(name, make):
    tex = make()
    h, w, _ = tex.shape
    us, vs = _edge_values(w), _edge_values(h)
    g = scenes.rng(3)
    us += g.uniform(-2, w + 2, size=40).tolist()
    vs += g.uniform(-2, h + 2, size=40).tolist()
    uu, vv = np.meshgrid(np.array(us), np.array(vs), indexing="ij")
    got = B.sample_bilinear(tex, uu.ravel(), vv.ravel())
    want = np.array([_scalar(tex, float(x), float(y)) for x, y in zip(uu.ravel(), vv.ravel())])
    assert _bits(got, want), (name, scenes.first_mismatch(got, want))
    assert np.isfinite(got).all()


@pytest.mark.parametrize("n", [2, 3, 7, 37, 149, 1024, (1 << 29) - 1])
def test_kernel_clamp_form_equals_the_literal_one(n):
    """nr_tri.h tex_bilinear's fmax / fmin / `f < 1 ? f : 0` against the
    reference's two clamps: the same texel index and the same fraction (as
    values: a -0.0 coordinate, kept by the literal `x < 0`, has the fraction
    -0.0 there and may have +0.0 in the kernel form -- equal, and the same
    colour for every texture that holds no -0.0 texel)."""
    g = scenes.rng(n)
    x = np.concatenate([np.array(_edge_values(n)),
                        g.uniform(-3.0, n + 3.0, size=60000),
                        g.uniform(n - 2.5, n - 0.5, size=30000),          # around the discontinuity at n-1
                        np.floor(g.uniform(-2, n + 2, size=5000)),        # integers
                        np.nextafter(np.floor(g.uniform(0, n, size=5000)), -np.inf)])
    assert x.size > 100000
    i0, f0 = B.footprint(x, n)
    i1, f1 = B.footprint_kernel(x, n)
    assert np.array_equal(i0, i1)
    assert np.array_equal(f0, f1)
    nz = x != 0
    assert _bits(f0[nz], f1[nz])
    assert i0.min() >= 0 and i0.max() <= n - 2 and (f0 >= 0).all() and (f0 < 1).all()
    # the literal consequences: the band [n-2, n-1) keeps its fraction, n-1 and beyond snap to n-2 with fraction 0
    band = (x >= n - 2) & (x < n - 1)
    assert band.any() and (i0[band] == n - 2).all() and np.array_equal(f0[band], x[band] - (n - 2))
    past = x >= n - 1
    assert past.any() and (i0[past] == n - 2).all() and (f0[past] == 0).all()


@pytest.mark.parametrize("name,make", TEXTURES)
def test_kernel_form_samples_equal_the_literal_samples(name, make):
    tex = make()
    h, w, _ = tex.shape
    g = scenes.rng(4)
    u = np.concatenate([np.array(_edge_values(w)), g.uniform(-3, w + 3, size=20000)])
    v = np.concatenate([g.uniform(-3, h + 3, size=20000), np.array(_edge_values(h))])
    g.shuffle(v)
    assert _bits(B.sample_bilinear(tex, u, v), B.sample_bilinear(tex, u, v, footprint=B.footprint_kernel))


@pytest.mark.parametrize("name,make", TEXTURES)
def test_integer_coordinates_return_the_nearest_texel(name, make):
    tex = make()
    h, w, _ = tex.shape
    uu, vv = np.meshgrid(np.arange(w - 1, dtype=np.float64), np.arange(h - 1, dtype=np.float64), indexing="ij")
    got = B.sample_bilinear(tex, uu.ravel(), vv.ravel())
    want = T.sample(tex, uu.ravel(), vv.ravel())[0]
    assert _bits(got, want), name


def test_rgb_alpha_is_the_literal_one():
    tex = T.texture_rgb()
    g = scenes.rng(5)
    t = B.sample_bilinear(tex, g.uniform(-3, 40, size=5000), g.uniform(-3, 26, size=5000))
    assert _bits(t[:, 3], np.ones(5000))
    # ... which the filtered sum of ones is not, for some fractions
    fu, fv = g.uniform(0, 1, size=5000), g.uniform(0, 1, size=5000)
    s = (1 - fu) * (1 - fv) + fu * (1 - fv) + (1 - fu) * fv + fu * fv
    assert (s != 1.0).any()


def test_ramp_texture_is_reproduced():
    """t(x, y) = a + b x + c y: the sample is a + b u + c v to 32 ulp of the
    largest texel magnitude (four terms of three roundings and three additions
    bound the error by 15 ulp; the factor 2 is slack)."""
    w, h = 37, 23
    coef = np.array([[0.3, 0.011, 0.017], [5.0, -0.07, 0.09], [-2.0, 0.05, -0.03], [0.1, 0.02, 0.004]])
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    tex = np.stack([a + b * xs + c * ys for a, b, c in coef], axis=-1)
    g = scenes.rng(6)
    u, v = g.uniform(0, w - 1, size=20000), g.uniform(0, h - 1, size=20000)
    u[-1], v[-1] = np.nextafter(w - 1.0, 0), np.nextafter(h - 1.0, 0)
    got = B.sample_bilinear(tex, u, v)
    for k, (a, b, c) in enumerate(coef):
        want = a + b * u + c * v
        tol = 32 * np.spacing(np.abs(tex[..., k]).max())
        assert np.abs(got[:, k] - want).max() <= tol, (k, np.abs(got[:, k] - want).max(), tol)


@functools.lru_cache(maxsize=None)
def _opaque(persp, mode, filt):
    info = {}
    want = B.expected_payload(W, H, False, B.BG, mode, B.CLEAR, B.soup_batches("opaque", persp), info, filt=filt)
    return want, info


@pytest.mark.parametrize("persp", [False, True])
@pytest.mark.parametrize("mode", T.MODES)
def test_payload_and_loop_derivations_agree(persp, mode):
    bs = B.soup_batches("opaque", persp)
    want = _opaque(persp, mode, 1)[0]
    for alpha in (False, True):
        a = want if not alpha else B.expected_payload(W, H, True, B.BG, mode, B.CLEAR, bs)
        b = B.expected_loop(W, H, alpha, B.BG, mode, B.CLEAR, bs)
        assert scenes.bits_equal(a[0], b[0]), scenes.first_mismatch(a[0], b[0])
        assert (a[1] is None and b[1] is None) or np.array_equal(a[1], b[1])


def test_nearest_through_this_module_is_the_existing_reference():
    """filt=0 reproduces persp_ref / textured_ref: the derivations differ from
    theirs in the sampler only."""
    for mode in T.MODES:
        a = _opaque(True, mode, 0)[0]
        b = P.expected_payload(W, H, False, B.BG, mode, B.CLEAR, P.soup_batches("opaque"))
        assert scenes.bits_equal(a[0], b[0]) and (a[1] is None or np.array_equal(a[1], b[1]))
        a = _opaque(False, mode, 0)[0]
        b = T.expected_payload(W, H, False, B.BG, mode, B.CLEAR, B.soup_batches("opaque", False))
        assert scenes.bits_equal(a[0], b[0]) and (a[1] is None or np.array_equal(a[1], b[1]))


@pytest.mark.parametrize("persp", [False, True])
@pytest.mark.parametrize("mode", T.MODES)
def test_scenes_discriminate(persp, mode):
    """Per batch at least 90 % of the covered pixels get a bilinear colour that
    differs from the nearest one; per depth mode some covered pixel has u < 0,
    some u in [w-2, w-1) and some u >= w-1."""
    (bil, _), info = _opaque(persp, mode, 1)
    (near, _), _ = _opaque(persp, mode, 0)
    cov, which, u = info["covered"], info["batch"], info["u"]
    differs = (bil != near).any(axis=-1)
    assert not differs[~cov].any()
    below = band = past = 0
    for k, b in enumerate(B.soup_batches("opaque", persp)):
        sel = cov & (which == k)
        assert sel.sum() > 500, (k, int(sel.sum()))
        share = differs[sel].mean()
        print(f"persp={persp} {mode} batch {k}: {int(sel.sum())} pixels, differing share {share:.4f}")
        assert share >= 0.9, (k, share)
        w = b["tex"].shape[1]
        below += int((u[sel] < 0).sum())
        band += int(((u[sel] >= w - 2) & (u[sel] < w - 1)).sum())
        past += int((u[sel] >= w - 1).sum())
    assert below > 0 and band > 0 and past > 0, (below, band, past)


def test_special_scenes_reach_what_they_are_for():
    # integer UVs: the filtered frame is the nearest frame
    bs = B.integer_uv_batches()
    a = B.expected_payload(W, H, False, B.BG, "zw", B.CLEAR, bs, filt=1)
    b = B.expected_payload(W, H, False, B.BG, "zw", B.CLEAR, bs, filt=0)
    assert scenes.bits_equal(a[0], b[0])
    # the 2x2 texture: coordinates on both sides of [0, 1) on covered pixels, and most pixels blend
    for alpha in (False, True):
        t = B.tiny_texture_batch(alpha)
        assert t["tex"].shape[:2] == (2, 2) and t["uv"].min() < -0.9 and t["uv"].max() > 1.9
    info = {}
    t = B.tiny_texture_batch(False)
    a = B.expected_payload(W, H, False, B.BG, "zw", B.CLEAR, [t], info, filt=1)
    b = B.expected_payload(W, H, False, B.BG, "zw", B.CLEAR, [t], filt=0)
    u = info["u"][info["covered"]]
    assert (u < 0).any() and ((u >= 0) & (u < 1)).any() and (u >= 1).any()
    assert (a[0] != b[0]).any(axis=-1)[info["covered"]].mean() > 0.2
    # odd coordinates: non-finite and huge (u, v) on covered pixels, and a finite frame
    for persp in (False, True):
        info = {}
        o = B.odd_uv_batch(persp)
        f = B.expected_payload(W, H, False, B.BG, "nz", B.CLEAR, [o], info)[0]
        u = info["u"][info["covered"]]
        assert np.isnan(u).any() and (np.isinf(u).any() or (np.abs(u) > 1e18).any())
        assert np.isfinite(f).all()

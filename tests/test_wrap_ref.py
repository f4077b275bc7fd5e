"""tests/wrap_ref.py against itself and the CPU oracle (no GPU): the fold against a
scalar transcription on edge and random values, every index in range, the
kernels' form against the literal one, the identities I1 and I3 on the sampler,
the two derivations against each other, and that the scenes the GPU tests draw
discriminate a wrapped sampler from the clamped one."""
import functools

import numpy as np
import pytest

import bilinear_ref as BL
import scenes
import wrap_ref as WR

W, H = WR.W, WR.H
SIDES = (2, 3, 5, 6, 7, 16, 37, 2 ** 29 - 1)


def _edges(n):
    na = np.nextafter
    v = [-0.0, 0.0, -1e-300, -1e-17, 1e-17, 0.5, n - 1.0, na(n - 1.0, 0), float(n), na(float(n), 0), na(float(n), np.inf),
         2.0 * n - 1, na(2.0 * n - 1, 0), 2.0 * n, na(2.0 * n, 0), na(2.0 * n, np.inf), -1.0, -0.5, -float(n),
         na(-float(n), 0), na(-float(n), -np.inf), 2.0 ** 31, -(2.0 ** 31), 2.0 ** 63, -(2.0 ** 63), 1e19, -1e19, 1e300,
         -1e300, np.inf, -np.inf, np.nan]
    for k in (-7, -3, -2, -1, 1, 2, 3, 4, 9, 1000, -1000):
        v += [float(k * n), na(float(k * n), np.inf), na(float(k * n), -np.inf), k * n - 1.0, k * n + 0.75]
    return np.array(v)


def _same_fold(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and scenes.bits_equal(a[2], b[2])


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_fold_equals_the_scalar_transcription_on_edge_values(mode):
    for n in SIDES:
        x = _edges(n)
        got = WR.fold(x, n, mode)
        want = [WR.fold_scalar(v, n, mode) for v in x.tolist()]
        for k, (j0, j1, f) in enumerate(want):
            assert (int(got[0][k]), int(got[1][k])) == (j0, j1), (n, mode, x[k])
            assert scenes.bits_equal(np.float64(got[2][k]), np.float64(f)), (n, mode, x[k])
            assert 0 <= j0 < n and 0 <= j1 < n and 0.0 <= f < 1.0, (n, mode, x[k])


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_fold_equals_the_scalar_transcription_on_random_values(mode):
    g = scenes.rng(800 + mode)
    for n, count in ((5, 40000), (3, 20000), (7, 20000), (16, 10000), (2, 10000)):   # 10^5 per mode
        x = np.concatenate([g.uniform(-4.0 * n, 5.0 * n, count // 2), g.normal(0, 1e6, count // 4),
                            g.integers(-50, 50, count // 4) * float(n) + g.choice([0.0, -2.0 ** -40, 2.0 ** -40], count // 4)])
        got = WR.fold(x, n, mode)
        want = [WR.fold_scalar(v, n, mode) for v in x.tolist()]
        assert np.array_equal(got[0], np.array([w[0] for w in want]))
        assert np.array_equal(got[1], np.array([w[1] for w in want]))
        assert scenes.bits_equal(got[2], np.array([w[2] for w in want]))
        for j in got[:2]:
            assert j.min() >= 0 and j.max() < n
        assert got[2].min() >= 0.0 and got[2].max() < 1.0


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_the_kernel_form_equals_the_literal_form(mode):
    for p in list(range(2, 300)) + [2 ** k + d for k in range(2, 30) for d in (-1, 0, 1) if 2 <= 2 ** k + d < 2 ** 30]:
        assert WR.period_kernel(p) == float(p)
    g = scenes.rng(810 + mode)
    for n in SIDES:
        x = np.concatenate([_edges(n), g.uniform(-4.0 * n, 5.0 * n, 20000), g.normal(0, 1e9, 2000)])
        if mode == 0:   # (the clamp axis is bilinear_ref's pair of forms; at -0.0 they give a zero fraction of either sign)
            x = x[~((x == 0) & np.signbit(x))]
        assert _same_fold(WR.fold_kernel(x, n, mode), WR.fold(x, n, mode)), (n, mode)


@pytest.mark.parametrize("filt", [0, 1])
def test_i1_inside_the_texture_every_mode_is_the_clamp_sampler(filt):
    g = scenes.rng(820)
    for w, h, c in ((5, 3, 3), (7, 6, 3), (6, 5, 4), (2, 2, 3), (16, 16, 3)):
        tex = WR.texture(w, h, c)
        u = np.concatenate([g.uniform(0, w - 1, 5000), [0.0, np.nextafter(w - 1.0, 0), 0.5]])
        v = np.concatenate([g.uniform(0, h - 1, 5000), [0.0, np.nextafter(h - 1.0, 0), 0.5]])
        want = BL._sample(tex, u, v, filt)
        for wrap in ((0, 0),) + WR.WRAPS:
            assert scenes.bits_equal(WR.sample(tex, u, v, filt, wrap), want), (w, h, wrap)
            assert scenes.bits_equal(WR.sample(tex, u, v, filt, wrap, WR.fold_kernel), want), (w, h, wrap)
    for n in SIDES:   # the footprint itself: k = 0 and t = x
        x = np.concatenate([g.uniform(0, n - 1, 5000), [0.0, np.nextafter(n - 1.0, 0)]])
        for mode in (1, 2):
            assert _same_fold(WR.fold(x, n, mode), WR.fold(x, n, 0)), (n, mode)


def test_i3_the_mirror_seam_is_flat():
    g = scenes.rng(830)
    for n in SIDES:
        for lo in (n - 1.0, 2.0 * n - 1):
            for k in (-3, -1, 0, 1, 4):
                x = lo + k * 2.0 * n + np.concatenate([g.uniform(0, 1, 500), [0.0]])
                x = x[(x >= lo + k * 2.0 * n) & (x < lo + k * 2.0 * n + 1)]
                j0, j1, f = WR.fold(x, n, 2)
                assert np.array_equal(j0, j1), (n, lo, k)
                assert np.all(j0 == (n - 1 if lo == n - 1.0 else 0)), (n, lo, k)
    tex = WR.texture(5, 3)
    u = 4.0 + g.uniform(0, 1, 200)
    v = g.uniform(0, 2, 200)
    # on the sampler: both columns of the footprint are the last texel column
    got = WR.sample(tex, u, v, 1, (2, 0))[:, 0:3]
    j0 = v.astype(np.int64)
    fu, fv = (u - 4.0)[:, None], (v - j0)[:, None]
    a, b = tex[j0, 4], tex[j0 + 1, 4]
    assert scenes.bits_equal(got, a * (1 - fu) * (1 - fv) + a * fu * (1 - fv) + b * (1 - fu) * fv + b * fu * fv)


# ---- the scenes ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(case):
    info = {}
    want = WR.expected(*case, info=info)
    return want, info


def _coords(case, info):
    """Per batch (tex, u, v) of the sampled coordinates of a case's scene."""
    kind, form = case[0], case[1]
    bs = WR.soup_batches(kind, form)
    if kind == "opaque":
        cov = info["covered"]
        return [(b["tex"], info["u"][cov & (info["batch"] == k)], info["v"][cov & (info["batch"] == k)])
                for k, b in enumerate(bs)]
    return [(b["tex"], *info["frags"][k]) for k, b in enumerate(bs)]


@pytest.mark.parametrize("case", WR.soup_cases(), ids=lambda c: "-".join(map(str, c)))
def test_the_soup_scenes_discriminate(case):
    kind, form, wrap, filt, mode, alpha = case
    want, info = _case(case)
    assert info["covered"].mean() >= 0.5
    out_u = np.concatenate([WR.outside(u, t.shape[1]) for t, u, v in _coords(case, info)])
    out_v = np.concatenate([WR.outside(v, t.shape[0]) for t, u, v in _coords(case, info)])
    print(f"{case}: outside u {out_u.mean():.3f}, outside v {out_v.mean():.3f}")
    if wrap[0]:
        assert out_u.mean() >= 0.4, out_u.mean()
    if wrap[1]:
        assert out_v.mean() >= 0.4, out_v.mean()
    clamp = _case((kind, form, (0, 0), filt, mode, alpha))[0]
    cov = info["covered"]
    differ = (want[0][cov] != clamp[0][cov]).any(axis=-1).mean()
    print(f"{case}: differs from the clamp frame on {differ:.3f} of the covered pixels")
    assert differ >= 0.4, differ


@pytest.mark.parametrize("form", WR.FORMS)
def test_payload_equals_loop_on_the_opaque_scenes(form):
    bs = WR.soup_batches("opaque", form)
    for wrap, filt, mode, alpha in (((1, 1), 1, "zw", False), ((2, 1), 0, "zt", True), ((0, 2), 1, "nz", False)):
        a = WR.expected_payload(W, H, alpha, WR.BG, mode, WR.CLEAR, bs, filt=filt, wrap=wrap)
        b = WR.expected_loop(W, H, alpha, WR.BG, mode, WR.CLEAR, bs, filt=filt, wrap=wrap)
        assert scenes.bits_equal(a[0], b[0]), (form, wrap, scenes.first_mismatch(a[0], b[0]))
        assert (a[1] is None and b[1] is None) or np.array_equal(a[1], b[1])


def test_wrap_zero_is_the_clamped_references():
    """(0, 0) restates bilinear_ref / modulate_ref: the parent's expected frames."""
    import modulate_ref as M
    bs = WR.soup_batches("opaque", "persp")
    for filt in (0, 1):
        a = WR.expected_payload(W, H, False, WR.BG, "zw", WR.CLEAR, bs, filt=filt)
        b = BL.expected_payload(W, H, False, WR.BG, "zw", WR.CLEAR, bs, filt=filt)
        assert scenes.bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    bs = WR.soup_batches("ct_alpha", "mod")
    a = WR.expected_loop(W, H, True, WR.BG, "zw", WR.CLEAR, bs, filt=1)
    b = M.expected_loop(W, H, True, WR.BG, "zw", WR.CLEAR, bs, filt=1)
    assert scenes.bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_inside_scene_stays_inside():
    for form in ("affine", "persp"):
        info = {}
        WR.expected_payload(W, H, False, WR.BG, "zw", WR.CLEAR, WR.inside_batches(form), info)
        cov = info["covered"]
        assert cov.mean() >= 0.5
        for k, b in enumerate(WR.inside_batches(form)):
            sel = cov & (info["batch"] == k)
            h, w, _ = b["tex"].shape
            assert not WR.outside(info["u"][sel], w).any() and not WR.outside(info["v"][sel], h).any()


def test_the_edge_scenes_discriminate():
    for b in (WR.tiny_texture_batch(), WR.dense_batch()):
        info = {}
        clamp = WR.expected_payload(W, H, False, WR.BG, "zw", WR.FAR, [b], info)
        cov = info["covered"]
        h, w, _ = b["tex"].shape
        assert WR.outside(info["u"][cov], w).mean() >= 0.4 and WR.outside(info["v"][cov], h).mean() >= 0.4
        for wrap in ((1, 1), (2, 2)):
            want = WR.expected_payload(W, H, False, WR.BG, "zw", WR.FAR, [b], filt=1, wrap=wrap)
            c1 = WR.expected_payload(W, H, False, WR.BG, "zw", WR.FAR, [b], filt=1)
            assert (want[0][cov] != c1[0][cov]).any(axis=-1).mean() >= 0.4
    import modulate_ref as M
    idx = M.P._oracle_pass(W, H, "zw", WR.FAR, [WR.dense_batch()], True)[0][..., 0]
    assert M.tile_winners(idx, 1, 1) > M.GOURAUD_RT

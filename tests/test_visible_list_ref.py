"""The argument behind the visible list, pinned on the CPU oracle: a triangle
that wins no pixel of a frame can be left out of the batch without changing
the frame.

For each depth mode and for the flat and the Gouraud sphere scene, the oracle's
frame of the whole soup equals, bit for bit (f64 framebuffer, u32 depth), its
frame of the soup filtered to the triangles that win a pixel, submission order
kept.  For LESS + write the winners found over a depth cleared to 0xFFFFFFFF
also serve over a depth buffer another soup has written: a triangle left out
lost every pixel to a kept one's smaller (depth, index) key, and goes on losing
under any initial depth, which can only be lower.

The share of (tile, triangle) pairs the winners keep is checked here against
the bound the GPU test asserts of GetVisiblePairCount (0.75 for the two-faced
spheres: at least the back faces go)."""
import numpy as np
import pytest

import scenes
import visible_ref as V

W, H = 640, 400
SMALL, BIG = (60, 200), (250, 700)
CLEAR = (0.1, 0.2, 0.3, 0.1)
DEPTHS = {"less_write": (True, True), "no_test": (False, False), "less_nowrite": (True, False)}

_MESH, _WIN = {}, {}


def _mesh(name, gouraud=True):
    if name not in _MESH:
        _MESH[name] = scenes.sphere_mesh(W, H, *name)
    xy, z, c = _MESH[name]
    return xy, z, (c if gouraud else np.ascontiguousarray(c[:, :4]))


def _winners(name, depth, shard=None):
    if (name, depth, shard) not in _WIN:
        xy, z, _ = _mesh(name)
        _WIN[(name, depth, shard)] = V.winners(xy, z, (W, H), depth, shard=shard)
    return _WIN[(name, depth, shard)]


def _frame(xy, z, c, depth, pre=None):
    ctx = scenes.OracleFactory().context(W, H, False)
    ctx.set_color(*CLEAR)
    V.set_depth(ctx, depth)
    if pre is not None:
        ctx.draw_triangles(pre[0], pre[2], z=pre[1])
    ctx.draw_triangles(xy, c, z=z)
    return ctx.get_buffer_numpy(), ctx.get_depth_buffer()


def _same(a, b, what):
    assert scenes.bits_equal(a[0], b[0]), (what, scenes.first_mismatch(a[0], b[0]))
    assert np.array_equal(a[1], b[1]), (what, "depth")


@pytest.mark.parametrize("gouraud", [False, True], ids=["flat", "gouraud"])
@pytest.mark.parametrize("depth", list(DEPTHS))
def test_filtered_soup_gives_the_same_frame(oracle, depth, gouraud):
    xy, z, c = _mesh(SMALL, gouraud)
    w = _winners(SMALL, DEPTHS[depth])
    assert 0 < len(w) < len(xy)
    _same(_frame(xy[w], z[w], c[w], DEPTHS[depth]), _frame(xy, z, c, DEPTHS[depth]), depth)


def test_filtered_big_sphere(oracle):
    xy, z, c = _mesh(BIG)
    w = _winners(BIG, (True, True))
    _same(_frame(xy[w], z[w], c[w], (True, True)), _frame(xy, z, c, (True, True)), "big")


@pytest.mark.parametrize("gouraud", [False, True], ids=["flat", "gouraud"])
def test_less_write_winners_serve_over_a_written_depth(oracle, gouraud):
    """The winners over a cleared depth, used over the depth (and colours)
    another soup left: LESS + write."""
    xy, z, c = _mesh(SMALL, gouraud)
    w = _winners(SMALL, (True, True))
    pre = scenes.triangle_soup(3000, W, H, 12, seed=3, gouraud=True)
    whole = _frame(xy, z, c, (True, True), pre)
    assert (whole[1] != _frame(xy, z, c, (True, True))[1]).any()   # the other soup does show
    _same(_frame(xy[w], z[w], c[w], (True, True), pre), whole, "over a written depth")


@pytest.mark.parametrize("mesh", [SMALL, BIG])
@pytest.mark.parametrize("shard", [None, (2, 0), (2, 1), (8, 3)])
def test_winners_keep_at_most_three_quarters_of_the_pairs(oracle, mesh, shard):
    xy, _, _ = _mesh(mesh)
    pairs = V.tile_pairs(xy, (W, H), shard)
    kept = pairs[_winners(mesh, (True, True), shard)].sum()   # (a rank marks the winners of its own tile rows)
    assert 0 < kept <= 0.75 * pairs.sum(), (kept, pairs.sum())

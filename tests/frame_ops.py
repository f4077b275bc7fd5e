"""Whole frames as plain data: one operation vocabulary for every draw kind of
the library, one interpreter (run) that executes a frame on a factory
(scenes.GpuFactory or scenes.OracleFactory), and the hypothesis strategies
that generate frames (tests/test_frame_ops.py checks what they generate,
tests/test_fuzz_mixed_gpu.py runs them on the GPU against the oracle).

A frame is (W, H, alpha, knobs, resources, ops).

knobs       dict, GPU only, applied right after the context is created:
            ordered (set_force_ordered_raster), coop (set_coop_raster),
            paircap (set_pair_capacity_override), split (set_split_limits
            arguments or None), warm (set_warm_binning), record (recording
            from creation on), fmt (None, "rgb" or "yuv420p": the frame format;
            run then ends with gather_frame_u8 and returns the frame output).
resources   dict made before the first operation:
            texs    [(w, h, channels, "u8" | "f64", seed, (rw, rh) | None)]
            bufs    [("c", n, seed, spread, gouraud, blended) |
                     ("t", n, seed, spread, "const" | "tiled" | "free")]   TriangleBuffers
            meshes  [("c", space, rows, cols, seed, gouraud, blended) |
                     ("l", space, rows, cols, seed, gouraud, blended) |
                     ("tu", space, n, seed, spread) | ("ts", space, rows, cols, seed)]
                    "l": a lit colour mesh, positions and colours as "c",
                    normals mesh_light_ref.sphere_normals plus a seeded
                    perturbation (not renormalised).
                    space "screen" (positions are pixels and depths; drawn
                    under None / IDENT16) or "model" (positions in [-1, 1]^3;
                    drawn under mesh_ref.affine / perspective / behind_eye).
ops         list of tuples, see OPS below.  A texture reference is
            ("res", i) a resource texture, ("tiny", seed, channels) a 2x2
            texture, or ("snap", "main" | "aux", shared): the snapshot of the
            frame (or of the auxiliary context) in that slot, taken at its
            first use and again by every ("snap", ...) operation.

How the oracle, which has no textured draw, no mesh, no buffer and no
recording, runs each operation:

  colour soup ("tri": draw_triangles / draw_triangles_device on torch tensors,
      aligned or offset by 8 bytes; "buf" on a colour TriangleBuffer)
          -> draw_triangles of the same arrays
  textured soup, one (u, v) per triangle ("ttri" / "buf" with uv "const", or
      "tiled": the same over [-2w, 3w) x [-2h, 3h), wrap_ref.tiled_uv's range)
          -> flat draw_triangles with textured_ref.flat_colours(texels, uv)
  textured soup, free UVs on a 2x2 texture (uv "free": every sample is texel
      (0, 0))     -> flat draw_triangles with that texel
  colour mesh ("mesh" / "mesh2": draw, update_positions, draw)
          -> draw_triangles of mesh_ref.expand(mesh, M)
  textured mesh: "tu" unshared vertices, one UV per triangle; "ts" shared
      vertices on a 2x2 texture
          -> as the textured soups, from mesh_ref.expand
  draw_texture / draw_splitted_texture of the frame's own shared snapshot
      (the library samples a copy taken before the draw; the reference reads
      the framebuffer while writing it, an order-dependent result)
          -> the same call with a fresh as_texure() copy
  primitives, pixels, other snapshots, state, probes -> the same calls
  begin / end / flush (command recording), gather (gather_frame_u8), knobs
          -> nothing

The six sticky states of the mesh and textured draws -- near plane, cull mode,
mesh perspective, triangle texture filter, lights, texture wrap -- are tracked
by the interpreter itself (near, cull, persp, filt, ambient, lights, wrap),
identically on both sides; the lowerings read that tracked state and never ask
the library.  The wrap is tracked, set and checked here; the lowerings that
sample under a wrap other than clamp, and the modulated, posed and morphed
draws, are tests/frame_anim.py's, which extends this interpreter (this module
never imports it: see _stable_seed).
A state operation calls the setter on the GPU and nothing on the oracle, and a
GPU run ends by asserting that the six getters return the tracked state: no
resize, save / restore, set_color, recording or draw between may have touched
them (DESIGN.md documents no operation that resets one).  Operation by
operation, all bit-exact:

  "mesh" / "mesh2" of a colour (or lit, drawn unlit) mesh
          -> draw_triangles of mesh_clip_ref.clip_soup(mesh, M, near, cull)
             (mesh_ref.expand with both off)
  "meshi" (draw_mesh_instanced, host or device matrices and tints)
          -> draw_triangles of mesh_inst_ref.instanced_soup(mesh, mats, tint,
             near, cull); a textured mesh as the textured meshes below, from
             the same soup
  "lmesh" / "lmesh2" (draw_mesh_lit; draw, update_normals and
      update_positions, draw)
          -> draw_triangles of mesh_light_ref.lit_soup(mesh, M, N, ambient,
             lights, near, cull)
  "lmeshi" (draw_mesh_lit_instanced and its device form)
          -> draw_triangles of mesh_light_ref.lit_instanced_soup(...)
  an empty soup draws nothing on either side
  textured draws with one (u, v) per triangle under the bilinear filter
          -> flat draw_triangles coloured bilinear_ref.sample_bilinear(texels,
             u, v): a0 + (a1-a0)*w1 + (a2-a0)*w2 returns a constant exactly,
             at a cut vertex too (a + (a-a)*t)
  "ptri" (a textured soup with q: one UV and one q in {0.25, 0.5, 1, 2, 4} per
      triangle; u*q, 1/q and (u*q)*(1/q) are exact)
          -> the affine lowering of its (u, v), nearest or bilinear
  textured meshes with the mesh perspective on, under None / the identity / an
      affine matrix (cw and q exactly 1)
          -> the affine lowering
  the 2x2 "ts" mesh under the nearest filter, any matrix, perspective on or off
          -> texel (0, 0), as before

The one substitution rule.  No exact lowering exists for free UVs under the
bilinear filter or under a wrap other than clamp (uv "free" soups and buffers,
the "ts" mesh: under repeat the 2x2 texture no longer always yields texel
(0, 0)) nor for a "tu" mesh with the mesh perspective on under a perspective or
behind-eye matrix (an instanced draw: under any such matrix).  For such a draw
the interpreter switches the offending state off on the GPU side
(set_triangle_texture_filter(0), set_triangle_texture_wrap(0, 0) or
set_mesh_perspective(False)), draws, and switches it back; the tracked
state is unchanged and the lowering uses the state as drawn.

Rules of the interpreter, the same on both sides: a draw whose texture is
narrower or lower than 2 texels (the snapshot of a 1-pixel-wide frame) is left
out -- the library rejects a textured batch from it
(tests/test_textured_gpu.py covers the rejection), and the reference's
sampler, whose clamp to w - 2 is then -1, reads before the texture; resize drops the shared snapshots of the resized
context, whose framebuffer they alias; every texture, buffer, mesh and device
array lives until the frame's last readback.

What this leaves to the dedicated tests: per-pixel sampling with varying UVs
on real textures (test_textured_gpu.py, test_persp_gpu.py,
test_bilinear_gpu.py), shards and RCCL, warm fault injection.
"""
from __future__ import annotations

import random

import numpy as np
from hypothesis import HealthCheck, given, settings, strategies as st

import bilinear_ref as B
import mesh_clip_ref as MC
import mesh_inst_ref as MI
import mesh_light_ref as ML
import mesh_ref as MR
import scenes
import textured_ref as T

TW, TH = 64, 32                     # the rasters' tile
ZRANGE = (-0.1, 1.1)
AUX_W, AUX_H = 24, 18               # the auxiliary context
NOMINAL_UV = (37, 23)               # UV range of textured buffers (their texture is chosen per draw)
DEPTH_VALUES = (0xFFFFFFFF, 0x90000000, 0x7FFFFFFF, 12345, 0)
KNOBS_OFF = dict(ordered=False, coop=0, paircap=0, split=None, warm=0, record=False, fmt=None)
KNOB_VALUES = dict(ordered=(False, True), coop=(0, 1, 2), paircap=(0, 50), split=(None, (64, 64)),
                   warm=(0, 1, 2), record=(False, True), fmt=(None, "rgb", "yuv420p"))

NEAR_VALUES = (0.0, 0.5, MI.NEAR)
Q_VALUES = (0.25, 0.5, 1.0, 2.0, 4.0)

BATCH_OPS = ("tri", "ttri", "buf", "buf2", "mesh", "mesh2", "meshi", "lmesh", "lmesh2", "lmeshi", "ptri")
STATE5_OPS = ("near", "cull", "mpersp", "filter", "lights")
OPS = """
("tri", src, n, seed, spread, gouraud, blended)       colour soup; src "host" | "dev" | "dev8"
("ttri", src, n, seed, spread, uvkind, texref)        textured soup; uvkind "const" | "tiled" | "free" (texref then "tiny")
("buf", i, texref)                                    resource buffer i (texref: textured buffers, uv "const" / "tiled")
("buf2", i, texref, dx)                               the same twice, translate(dx, 0) between (0: the second is warm)
("mesh", i, mat, texref)                              resource mesh i; mat indexes the matrices of its space
("mesh2", i, mat, texref, seed)                       draw, update_positions(seed), draw
("meshi", i, K, seed, tint, src)                      draw_mesh_instanced of resource mesh i under K seeded matrices of its
                                                      space; tint None | "opaque" | "alpha" (None for textured meshes);
                                                      src "host" | "dev" | "dev8" (matrices and tint); a "tu" mesh
                                                      samples the resource texture ("res", seed)
("lmesh", i, mat, nseed)                              draw_mesh_lit of the i-th lit mesh; nseed: a seeded rotation3 or None
("lmesh2", i, mat, nseed, seed)                       draw, update_normals(seed) and update_positions(seed), draw
("lmeshi", i, K, seed, tint, src)                     draw_mesh_lit_instanced (seeded normal matrices, None for seed % 3 == 0)
("ptri", src, n, seed, spread, texref)                textured soup with q: one UV and one q of Q_VALUES per triangle
("near", w) ("cull", mode) ("mpersp", on) ("filter", mode)   the sticky states: w in NEAR_VALUES, mode 0 | 1 | 2, 0 | 1
("lights", seed, nl)                                  set_mesh_lights(*mesh_light_ref.random_lights(nl, seed)), nl in 0..8;
                                                      seed None: (None, None), the default lights
("wrap", u, v)                                        the sixth state, set_triangle_texture_wrap(u, v), u and v in 0..2
                                                      (generated by tests/frame_anim.py, whose OPS table lists the
                                                      modulated, posed and morphed draws)
("fill", c) ("rect", c, g) ("line", c, g) ("circle", c, g) ("grd", c, g)
("tex", texref, g) ("stex", texref, g, uv4) ("setpx", x, y, c) ("applypx", x, y, c)
("snap", which, shared)                               take the snapshot of that slot (again)
("aux", kind, c, g)                                   draw into the auxiliary context: "rect" | "circle" | "clear" | "tri"
("translate", v) ("rotate", v) ("scale", v) ("ct", v) ("save", v) ("restore", v) ("clear", v)
("transform", m6)                                     set_transform (the fixed sequences; not generated)
("cleardepth", value) ("depthstate", test, write) ("resize", w, h)
("getcolor", x, y) ("readf64",) ("readdepth",)        probes
("begin",) ("end",) ("flush",) ("gather",)            GPU only
"""


# ---------------------------------------------------------------------------
# inputs from the specs
# ---------------------------------------------------------------------------
def texture_array(spec):
    w, h, ch, dtype, seed, _ = spec
    g = scenes.rng(seed)
    if dtype == "u8":
        return g.integers(0, 256, size=(h, w, ch), dtype=np.uint8)
    return g.uniform(-0.2, 1.3, size=(h, w, ch))


def tiny_array(seed, ch):
    return scenes.rng(seed).uniform(0, 1, size=(2, 2, ch))


def colour_soup(n, W, H, seed, spread, gouraud, blended):
    return scenes.triangle_soup(n, W, H, spread, seed=seed, gouraud=gouraud,
                                alpha=(0.1, 0.9) if blended else None, zrange=ZRANGE)


def textured_soup(n, W, H, seed, spread, uvkind, size):
    """(xy, z, uv): uv "const": one (u, v) per triangle, uniform in
    [-3, w+3] x [-3, h+3] of `size`; "tiled": the same over [-2w, 3w) x
    [-2h, 3h); "free": any UVs per vertex."""
    xy, z, _ = scenes.triangle_soup(n, W, H, spread, seed=seed, zrange=ZRANGE)
    g = scenes.rng(seed + 1)
    w, h = size
    if uvkind == "const":
        uv = np.stack([g.uniform(-3, w + 3, n), g.uniform(-3, h + 3, n)], axis=1)
        uv = np.repeat(uv[:, None, :], 3, axis=1)
    elif uvkind == "tiled":         # (wrap_ref.tiled_uv's range, one (u, v) per triangle)
        uv = np.stack([g.uniform(-2.0 * w, 3.0 * w, n), g.uniform(-2.0 * h, 3.0 * h, n)], axis=1)
        uv = np.repeat(uv[:, None, :], 3, axis=1)
    else:
        uv = g.uniform(-3, 5, size=(n, 3, 2))
    return xy, z, np.ascontiguousarray(uv.reshape(n, 6))


def oracle_texels(tex):
    """The texels of an oracle texture as they are now, (h, w, 3|4) f64."""
    out = np.empty((tex.height, tex.width, 4 if tex.enableAlpha else 3), dtype=np.float64)
    tex.lib.OracleGetTextureBuffer(tex._ptr, scenes._vp(out))
    return out


def _to_space(space, p, W, H):
    """Unit-box positions p (in about [-1.2, 1.2]^3) in the mesh's space."""
    if space == "model":
        return np.ascontiguousarray(p)
    return np.ascontiguousarray(np.stack([W / 2 + 0.45 * W * p[:, 0], H / 2 - 0.45 * H * p[:, 1],
                                          0.5 + 0.5 * p[:, 2]], axis=1))


def mesh_positions(spec, W, H, seed):
    """The positions of a resource mesh for `seed` (the spec's own at
    creation, another for update_positions)."""
    kind, space = spec[0], spec[1]
    g = scenes.rng(seed)
    if kind == "tu":
        n, spread = spec[2], spec[4]
        c = g.uniform(-1, 1, size=(n, 1, 3))
        p = (c + g.uniform(-spread, spread, size=(n, 3, 3))).reshape(3 * n, 3)
        return p, g
    rows, cols = spec[2], spec[3]
    p = MR.sphere3d(rows, cols)["pos"]
    return p + g.uniform(-0.04, 0.04, size=p.shape), g


def mesh_dict(spec, W, H):
    """The mesh of a spec as mesh_ref's dict (pos, idx, colors + gouraud | uv)."""
    kind, space = spec[0], spec[1]
    if kind in ("c", "l"):
        _, _, rows, cols, seed, gouraud, blended = spec
        p, g = mesh_positions(spec, W, H, seed)
        col = g.uniform(0, 1, size=(p.shape[0], 4))
        col[:, 3] = g.uniform(0.1, 0.9, size=p.shape[0]) if blended else 1.0
        mesh = dict(pos=_to_space(space, p, W, H), idx=MR.grid_indices(rows, cols), colors=col, gouraud=gouraud)
        if kind == "l":
            mesh["normals"] = mesh_normals(spec, seed)
        return mesh
    if kind == "ts":
        _, _, rows, cols, seed = spec
        p, g = mesh_positions(spec, W, H, seed)
        return dict(pos=_to_space(space, p, W, H), idx=MR.grid_indices(rows, cols),
                    uv=g.uniform(-3, 5, size=(p.shape[0], 2)))
    _, _, n, seed, spread = spec
    p, g = mesh_positions(spec, W, H, seed)
    uv = np.repeat(np.stack([g.uniform(-3, NOMINAL_UV[0] + 3, n), g.uniform(-3, NOMINAL_UV[1] + 3, n)], 1), 3, axis=0)
    perm = g.permutation(3 * n)          # vertex k of the soup is stored at perm[k]
    pos, puv = np.empty((3 * n, 3)), np.empty((3 * n, 2))
    pos[perm], puv[perm] = _to_space(space, p, W, H), uv
    return dict(pos=pos, idx=perm.reshape(n, 3).astype(np.uint32), uv=puv)


def mesh_soup(spec, W, H):
    """The soup an unshared-vertex mesh ("tu") is built from: xy, z, uv."""
    _, space, n, seed, _ = spec
    p, g = mesh_positions(spec, W, H, seed)
    p = _to_space(space, p, W, H)
    uv = np.repeat(np.stack([g.uniform(-3, NOMINAL_UV[0] + 3, n), g.uniform(-3, NOMINAL_UV[1] + 3, n)], 1), 3, axis=0)
    return p[:, :2].reshape(n, 6), p[:, 2].reshape(n, 3), uv.reshape(n, 6)


def mesh_matrix(space, mat, W, H):
    """(label, matrix) of a mesh draw."""
    if space == "screen":
        return (("none", None), ("ident", MR.IDENT16))[mat % 2]
    return (("affine", MR.affine(W, H)), ("perspective", MR.perspective(W, H)),
            ("perspective", MR.behind_eye(W, H)), ("affine", MR.affine(W, H, ax=1.1, ay=-0.7, scale=0.3)))[mat % 4]


def mesh_normals(spec, seed):
    """The normals of a lit mesh for `seed`: the sphere's analytic ones plus a
    perturbation (their lengths are then not 1: nothing renormalises them)."""
    n = ML.sphere_normals(spec[2], spec[3])
    return np.ascontiguousarray(n + scenes.rng(seed + 3).uniform(-0.15, 0.15, size=n.shape))


def moved_mesh(spec, mesh, W, H, seed):
    """`mesh` with the positions (a lit mesh: and the normals) of `seed`."""
    p, _ = mesh_positions(spec, W, H, seed)
    p = _to_space(spec[1], p, W, H)
    if spec[0] == "tu":           # (stored through the permutation, as at creation)
        pos = np.empty_like(p)
        pos[mesh["idx"].reshape(-1).astype(np.int64)] = p
        p = pos
    out = dict(mesh, pos=p)
    if spec[0] == "l":
        out["normals"] = mesh_normals(spec, seed)
    return out


_INSTANCE_MATS = (0, 1, 2, 2, 2, 3)       # (perspective and behind-eye at least as often as the affine ones)


def instance_matrices(space, K, seed, W, H):
    """(labels, (K, 16)): K matrices of the mesh's space, each one of
    mesh_matrix's set times a seeded placement (a uniform scale and an offset)."""
    g = scenes.rng(seed)
    labels, mats = [], []
    for _ in range(K):
        s = g.uniform(0.3, 0.8)
        A = np.eye(4)
        if space == "screen":
            A[0, 0] = A[1, 1] = s
            A[:3, 3] = (W / 2 * (1 - s) + g.uniform(-0.3, 0.3) * W, H / 2 * (1 - s) + g.uniform(-0.3, 0.3) * H,
                        g.uniform(-0.2, 0.2))
            label, M = "ident", A
        else:
            A[0, 0] = A[1, 1] = A[2, 2] = s
            A[:3, 3] = g.uniform(-0.7, 0.7, size=3)
            label, M = mesh_matrix(space, _INSTANCE_MATS[int(g.integers(len(_INSTANCE_MATS)))], W, H)
            M = M.reshape(4, 4) @ A
            if label == "affine":
                M[3] = (0.0, 0.0, 0.0, 1.0)
        labels.append(label)
        mats.append(M.reshape(16))
    return labels, np.ascontiguousarray(np.stack(mats))


def instance_tint(kind, K, seed):
    """(K, 4) colour factors in [0.3, 1]: "opaque" alpha 1, "alpha" alpha in
    [0.2, 0.9] for about half of the instances, the first included; None."""
    if kind is None:
        return None
    g = scenes.rng(seed + 11)
    t = g.uniform(0.3, 1.0, size=(K, 4))
    t[:, 3] = 1.0
    if kind == "alpha":
        sel = g.random(K) < 0.5
        sel[0] = True
        t[sel, 3] = g.uniform(0.2, 0.9, size=int(sel.sum()))
    return np.ascontiguousarray(t)


def normal_matrix(nseed):
    """A seeded mesh_light_ref.rotation3, or None."""
    if nseed is None:
        return None
    ax, ay = scenes.rng(nseed + 17).uniform(-np.pi, np.pi, size=2)
    return ML.rotation3(ax, ay)


def instance_normals(K, seed):
    """(K, 9) seeded rotations; None (the identity) for seed % 3 == 0."""
    if seed % 3 == 0:
        return None
    return np.ascontiguousarray(np.stack([normal_matrix(seed + 31 * k) for k in range(K)]))


def light_state(seed, nl):
    """(ambient, lights) of a ("lights", seed, nl) operation."""
    if seed is None:
        return None, None
    return ML.random_lights(nl, seed)


def mesh_draw_soup(mesh, M, near, cull):
    """(xy, z, attr) of a single unlit mesh draw under the clip state."""
    if near > 0 or cull != 0:
        return MC.clip_soup(mesh, M, near, cull)[:3]
    return MR.expand(mesh, M)


def textured_colours(texels, uv, filt):
    """The flat colours (n, 4) of triangles with one (u, v) each, uv (n, >= 2)."""
    if filt:
        return np.ascontiguousarray(B.sample_bilinear(texels, uv[:, 0], uv[:, 1]))
    return T.flat_colours(texels, uv[:, :2])


def perspective_soup(n, W, H, seed, spread, size):
    """textured_soup with uv "const" plus q (n, 3): one of Q_VALUES per triangle."""
    xy, z, uv = textured_soup(n, W, H, seed, spread, "const", size)
    q = np.asarray(Q_VALUES)[scenes.rng(seed + 2).integers(0, len(Q_VALUES), size=n)]
    return xy, z, uv, np.ascontiguousarray(np.repeat(q[:, None], 3, axis=1))


def tile_pairs(xy, m, W, H):
    """(tile, triangle) pairs of a soup by bounding boxes, under transform m."""
    if xy.shape[0] == 0 or W <= 0 or H <= 0:
        return 0
    s = MR.xform(m, xy)
    keep = MR.kept(xy, m)
    with np.errstate(all="ignore"):
        x0, x1 = np.floor(s[..., 0].min(axis=1)), np.ceil(s[..., 0].max(axis=1))
        y0, y1 = np.floor(s[..., 1].min(axis=1)), np.ceil(s[..., 1].max(axis=1))
    keep &= (x1 >= 0) & (x0 <= W - 1) & (y1 >= 0) & (y0 <= H - 1)
    if not keep.any():
        return 0
    x0, x1 = np.clip(x0[keep], 0, W - 1) // TW, np.clip(x1[keep], 0, W - 1) // TW
    y0, y1 = np.clip(y0[keep], 0, H - 1) // TH, np.clip(y1[keep], 0, H - 1) // TH
    return int(((x1 - x0 + 1) * (y1 - y0 + 1)).sum())


# ---------------------------------------------------------------------------
# the interpreter
# ---------------------------------------------------------------------------
class _Run:
    batch_ops = BATCH_OPS

    def __init__(self, fac, frame, triangles=True):
        self.fac = fac
        self.gpu = fac.name != "oracle"
        self.W, self.H, self.alpha, self.knobs, self.res, self.ops = frame
        self.W0, self.H0 = self.W, self.H       # (matrices and inputs follow the frame's first size)
        self.triangles = triangles
        self.keep = []                          # everything the library may still read
        self.probes = []
        self.batches = []                       # (kind, raster path or None, tile pairs)
        self.snaps = {}
        self.aux = None
        # the five sticky states, tracked here and never read back from the library before the run's end
        self.near, self.cull, self.persp, self.filt = 0.0, 0, False, 0
        self.ambient = self.lights = None
        self.wrap = self.wrap_drawn = (0, 0)    # the sixth: the texture wrap, and the wrap the current draw is issued under
        self.counts = []                        # (full, rasterised) triangle counts of the mesh draws
        self.over_cap = False                   # a batch of more than 50 tile pairs since the last synchronisation
        self.changed_over_cap = 0               # changes of the six states while such a batch may be pending
        if self.gpu:
            from libnativecpurenderer_amd import libNativeCPURendererPybind as R
            self.R = R

    # ---- contexts, resources ------------------------------------------------
    def context(self, w, h, alpha, fmt=None):
        ctx = self.fac.context(w, h, alpha)
        if self.gpu:
            k = self.knobs
            ctx.set_force_ordered_raster(bool(k["ordered"]))
            ctx.set_coop_raster(k["coop"])
            ctx.set_pair_capacity_override(k["paircap"])
            if k["split"]:
                ctx.set_split_limits(*k["split"])
            ctx.set_warm_binning(k["warm"])
            if fmt:
                ctx.set_frame_format(fmt)
            if k["record"]:
                ctx.begin_commands()
        return ctx

    def aux_ctx(self):
        if self.aux is None:
            self.aux = self.context(AUX_W, AUX_H, self.alpha)
            self.aux.set_color(0.6, 0.3, 0.1, 1.0)
        return self.aux

    def make_resources(self):
        W, H = self.W, self.H
        self.texs = []
        for spec in self.res.get("texs", []):
            t = self.fac.texture(texture_array(spec))
            self.keep.append(t)
            if spec[5]:
                t = t.resample(*spec[5])
                self.keep.append(t)
            self.texs.append(t)
        self.bufs = []
        for spec in self.res.get("bufs", []):
            if spec[0] == "c":
                arrays = colour_soup(spec[1], W, H, *spec[2:])
            else:
                arrays = textured_soup(spec[1], W, H, spec[2], spec[3], spec[4], NOMINAL_UV)
            gbuf = None
            if self.gpu and self.triangles:
                xy, z, a = arrays
                gbuf = (self.R.TriangleBuffer(xy, a, z=z, gouraud=spec[4]) if spec[0] == "c"
                        else self.R.TriangleBuffer(xy, uv=a, z=z))
            self.bufs.append((spec, arrays, gbuf))
        self.meshes = []
        for spec in self.res.get("meshes", []):
            mesh = self.mesh_dict(spec)
            gm = None
            if self.gpu and self.triangles:
                gm = (self.R.Mesh(mesh["pos"], mesh["idx"], uv=mesh["uv"], colors=mesh.get("colors"),
                                  normals=mesh.get("normals")) if "uv" in mesh else
                      self.R.Mesh(mesh["pos"], mesh["idx"], colors=mesh["colors"], gouraud=mesh["gouraud"],
                                  normals=mesh.get("normals")))
            self.meshes.append([spec, mesh, gm])
        self.lit = [e for e in self.meshes if e[0][0] == "l"]

    def mesh_dict(self, spec):
        return mesh_dict(spec, self.W, self.H)

    def flat(self, texels, uv, filt):
        """The flat colours of a constant-UV draw issued under wrap_drawn."""
        assert self.wrap_drawn == (0, 0), "the wrapped lowering is frame_anim's"
        return textured_colours(texels, uv, filt)

    def texture(self, ref, prim=False):
        if prim and not self.gpu and ref[0] == "snap" and ref[1] == "main" and ref[2]:
            self.texture(ref)                 # (the slot is taken as on the GPU side)
            t = self.ctx.as_texure()
            self.keep.append(t)
            return t
        if ref[0] == "res":
            return self.texs[ref[1] % len(self.texs)] if self.texs else self.texture(("tiny", ref[1], 3))
        if ref[0] == "tiny":
            t = self.fac.texture(tiny_array(ref[1], ref[2]))
            self.keep.append(t)
            return t
        key = (ref[1], bool(ref[2]))
        if key not in self.snaps:
            self.snap(*key)
        return self.snaps[key]

    def snap(self, which, shared):
        src = self.ctx if which == "main" else self.aux_ctx()
        t = src.as_texture_shared() if shared else src.as_texure()
        self.keep.append(t)
        self.snaps[(which, bool(shared))] = t

    def texels(self, tex):
        return oracle_texels(tex)

    # ---- triangle batches -----------------------------------------------------
    def _note(self, kind, xy, ctx=None):
        ctx = ctx or self.ctx
        if xy.shape[0] == 0:
            return
        path = ctx.last_raster_path() if self.gpu else None
        self.batches.append((kind, path, tile_pairs(xy, ctx.get_transform(), ctx.width, ctx.height)))
        self.over_cap |= ctx is self.ctx and self.batches[-1][2] > 50

    def _device(self, arrays, offset):
        import torch
        dev = torch.device("cuda", self.ctx.device)
        out = []
        for a in arrays:
            t = torch.from_numpy(np.ascontiguousarray(a)).to(dev).reshape(-1)
            if offset:
                t = torch.cat([torch.zeros(1, dtype=t.dtype, device=dev), t])[1:]
                assert t.data_ptr() % 16 == 8
            out.append(t)
        torch.cuda.synchronize(dev)
        self.keep.append(out)
        return out

    def colour_batch(self, xy, z, c, gouraud, src="host", gbuf=None, ctx=None):
        ctx = ctx or self.ctx
        if not self.triangles:
            return
        if not self.gpu or src == "host":
            ctx.draw_triangles(xy, c, z=z, gouraud=gouraud)
        elif src == "buf":
            ctx.draw_triangle_buffer(gbuf)
        else:
            txy, tc = self._device((xy, c), src == "dev8")
            tz, = self._device((z,), False)
            ctx.draw_triangles_device(txy, tc, xy.shape[0], z=tz, gouraud=gouraud)
        self._note("colour", xy, ctx)

    def _nearest_for(self, free):
        """The substitution rule for free UVs: the filter as drawn (the wrap as
        drawn goes to wrap_drawn), and a function that restores what the GPU
        side switched off: the bilinear filter, a wrap other than clamp."""
        filt_off, wrap_off = bool(free and self.filt), free and self.wrap != (0, 0)
        self.wrap_drawn = (0, 0) if wrap_off else self.wrap
        if self.gpu and filt_off:
            self.ctx.set_triangle_texture_filter(0)
        if self.gpu and wrap_off:
            self.ctx.set_triangle_texture_wrap(0, 0)

        def restore():
            if self.gpu and filt_off:
                self.ctx.set_triangle_texture_filter(1)
            if self.gpu and wrap_off:
                self.ctx.set_triangle_texture_wrap(*self.wrap)
        return (0 if filt_off else self.filt), restore

    def textured_batch(self, tex, xy, z, uv, uvkind, src="host", gbuf=None, q=None):
        if not self.triangles or tex.width < 2 or tex.height < 2:
            return
        assert uvkind != "free" or (tex.width, tex.height) == (2, 2), "free UVs are lowered on 2x2 textures only"
        filt, restore = self._nearest_for(uvkind == "free")
        if not self.gpu:
            flat = self.flat(self.texels(tex), uv, filt)
            self.ctx.draw_triangles(xy, flat, z=z, gouraud=False)
        elif src == "host":
            self.ctx.draw_textured_triangles(tex, xy, uv, z=z, q=q)
        elif src == "buf":
            self.ctx.draw_triangle_buffer(gbuf, tex)
        else:
            txy, tuv = self._device((xy, uv), src == "dev8")
            tz, = self._device((z,), False)
            tq = None if q is None else self._device((q,), src == "dev8")[0]
            self.ctx.draw_textured_triangles_device(tex, txy, tuv, xy.shape[0], z=tz, q=tq)
        restore()
        self._note("textured", xy)

    def draw_buffer(self, i, texref):
        if not self.bufs:
            return
        spec, arrays, gbuf = self.bufs[i % len(self.bufs)]
        xy, z, a = arrays
        if spec[0] == "c":
            self.colour_batch(xy, z, a, spec[4], "buf", gbuf)
        else:
            ref = texref if spec[4] != "free" else ("tiny", spec[2], 3 + spec[2] % 2)
            self.textured_batch(self.texture(ref), xy, z, a, spec[4], "buf", gbuf)

    def _mesh_texture(self, spec, texref):
        """The texture of a mesh draw (None: a colour mesh), and whether the draw is left out."""
        if spec[0] not in ("tu", "ts"):
            return None, False
        tex = self.texture(texref if spec[0] == "tu" else ("tiny", spec[4], 3 + spec[4] % 2))
        return tex, tex.width < 2 or tex.height < 2

    def _textured_mesh_states(self, spec, labels):
        """The substitution rule for a textured mesh draw under matrices of
        `labels`: the filter as drawn, and a function that restores what the
        GPU side switched off."""
        filt, back = self._nearest_for(spec[0] == "ts")
        off = self.gpu and self.persp and spec[0] == "tu" and "perspective" in labels
        if off:
            self.ctx.set_mesh_perspective(False)

        def restore():
            back()
            if off:
                self.ctx.set_mesh_perspective(True)
        return filt, restore

    def _oracle_soup(self, mesh, soup, tex, filt):
        xy, z, attr = soup
        if xy.shape[0] == 0:
            return
        if tex is None:
            self.ctx.draw_triangles(xy, attr, z=z, gouraud=bool(mesh["gouraud"]))
        else:
            self.ctx.draw_triangles(xy, self.flat(self.texels(tex), attr, filt), z=z, gouraud=False)

    def _note_mesh(self, kind, full, xy):
        self.counts.append((full, xy.shape[0]))
        with np.errstate(all="ignore"):
            self._note(kind, xy)

    def draw_mesh(self, i, mat, texref):
        if not self.meshes or not self.triangles:
            return
        spec, mesh, gm = self.meshes[i % len(self.meshes)]
        label, M = mesh_matrix(spec[1], mat, self.W0, self.H0)
        tex, skip = self._mesh_texture(spec, texref)
        if skip:
            return
        soup = mesh_draw_soup(mesh, M, self.near, self.cull)
        filt, restore = self._textured_mesh_states(spec, (label,))
        if self.gpu:
            self.ctx.draw_mesh(gm, M, texture=tex)
        else:
            self._oracle_soup(mesh, soup, tex, filt)
        restore()
        self._note_mesh("mesh", mesh["idx"].shape[0], soup[0])

    def move_mesh(self, entry, seed):
        entry[1] = moved_mesh(entry[0], entry[1], self.W0, self.H0, seed)
        if entry[2] is not None:
            if entry[0][0] == "l":
                entry[2].update_normals(entry[1]["normals"])
            entry[2].update_positions(entry[1]["pos"])

    def _instances(self, spec, K, seed, tint, src, normals=False):
        """labels, the host arrays (matrices, normal matrices, tint) and what the GPU call takes for them."""
        labels, mats = instance_matrices(spec[1], K, seed, self.W0, self.H0)
        host = [mats, instance_normals(K, seed) if normals else None,
                instance_tint(None if spec[0] in ("tu", "ts") else tint, K, seed)]
        args = host
        if self.gpu and src != "host":
            args = [None if a is None else self._device((a,), src == "dev8")[0] for a in host]
        return labels, host, args

    def draw_mesh_instanced(self, i, K, seed, tint, src):
        if not self.meshes or not self.triangles:
            return
        spec, mesh, gm = self.meshes[i % len(self.meshes)]
        tex, skip = self._mesh_texture(spec, ("res", seed))     # (a "tu" mesh: the resource texture its seed names)
        if skip:
            return
        labels, (mats, _, tn), (gmats, _, gtn) = self._instances(spec, K, seed, tint, src)
        soup = MI.instanced_soup(mesh, mats, tn, self.near, self.cull)[:3]
        filt, restore = self._textured_mesh_states(spec, labels)
        if not self.gpu:
            self._oracle_soup(mesh, soup, tex, filt)
        elif src == "host":
            self.ctx.draw_mesh_instanced(gm, gmats, texture=tex, tint=gtn)
        else:
            self.ctx.draw_mesh_instanced_device(gm, gmats, K, texture=tex, tint=gtn)
        restore()
        self._note_mesh("instanced", K * mesh["idx"].shape[0], soup[0])

    def draw_mesh_lit(self, i, mat, nseed):
        if not self.lit or not self.triangles:
            return
        spec, mesh, gm = self.lit[i % len(self.lit)]
        _, M = mesh_matrix(spec[1], mat, self.W0, self.H0)
        N = normal_matrix(nseed)
        soup = ML.lit_soup(mesh, M, N, self.ambient, self.lights, self.near, self.cull)
        if self.gpu:
            self.ctx.draw_mesh_lit(gm, M, N)
        else:
            self._oracle_soup(mesh, soup, None, 0)
        self._note_mesh("lit", mesh["idx"].shape[0], soup[0])

    def draw_mesh_lit_instanced(self, i, K, seed, tint, src):
        if not self.lit or not self.triangles:
            return
        spec, mesh, gm = self.lit[i % len(self.lit)]
        _, (mats, nm, tn), (gmats, gnm, gtn) = self._instances(spec, K, seed, tint, src, normals=True)
        soup = ML.lit_instanced_soup(mesh, mats, nm, tn, self.ambient, self.lights, self.near, self.cull)
        if not self.gpu:
            self._oracle_soup(mesh, soup, None, 0)
        elif src == "host":
            self.ctx.draw_mesh_lit_instanced(gm, gmats, gnm, gtn)
        else:
            self.ctx.draw_mesh_lit_instanced_device(gm, gmats, K, gnm, gtn)
        self._note_mesh("lit", K * mesh["idx"].shape[0], soup[0])

    def set_state(self, k, op):
        ctx, before = self.ctx, (self.near, self.cull, self.persp, self.filt, self.ambient, self.lights, self.wrap)
        if k == "near":
            self.near = float(op[1])
            if self.gpu:
                ctx.set_mesh_near_plane(self.near)
        elif k == "cull":
            self.cull = int(op[1])
            if self.gpu:
                ctx.set_mesh_cull(self.cull)
        elif k == "mpersp":
            self.persp = bool(op[1])
            if self.gpu:
                ctx.set_mesh_perspective(self.persp)
        elif k == "filter":
            self.filt = int(op[1])
            if self.gpu:
                ctx.set_triangle_texture_filter(self.filt)
        elif k == "wrap":
            self.wrap = (int(op[1]), int(op[2]))
            if self.gpu:
                ctx.set_triangle_texture_wrap(*self.wrap)
        else:
            self.ambient, self.lights = light_state(op[1], op[2])
            if self.gpu:
                ctx.set_mesh_lights(self.ambient, self.lights)
        after = (self.near, self.cull, self.persp, self.filt, self.ambient, self.lights, self.wrap)
        self.changed_over_cap += self.over_cap and repr(before) != repr(after)

    def check_states(self):
        """The six getters against the tracked state (GPU side)."""
        ctx = self.ctx
        got = (ctx.get_mesh_near_plane(), ctx.get_mesh_cull(), ctx.mesh_perspective(), ctx.get_triangle_texture_filter(),
               ctx.get_mesh_light_count(), tuple(ctx.get_triangle_texture_wrap()))
        want = (self.near, self.cull, self.persp, self.filt, 0 if self.lights is None else len(self.lights), self.wrap)
        assert got == want, f"sticky states {got} != tracked {want}"

    # ---- one operation --------------------------------------------------------
    def op(self, op):
        ctx, k = self.ctx, op[0]
        W0, H0 = self.W0, self.H0
        if k == "tri":
            _, src, n, seed, spread, gouraud, blended = op
            xy, z, c = colour_soup(n, W0, H0, seed, spread, gouraud, blended)
            self.colour_batch(xy, z, c, gouraud, src)
        elif k == "ttri":
            _, src, n, seed, spread, uvkind, texref = op
            tex = self.texture(texref)
            xy, z, uv = textured_soup(n, W0, H0, seed, spread, uvkind, (tex.width, tex.height))
            self.textured_batch(tex, xy, z, uv, uvkind, src)
        elif k == "buf":
            self.draw_buffer(op[1], op[2])
        elif k == "buf2":
            self.draw_buffer(op[1], op[2])
            if op[3]:
                ctx.translate(op[3], 0.0)
            self.draw_buffer(op[1], op[2])
        elif k == "mesh":
            self.draw_mesh(op[1], op[2], op[3])
        elif k == "mesh2":
            self.draw_mesh(op[1], op[2], op[3])
            if self.meshes:
                self.move_mesh(self.meshes[op[1] % len(self.meshes)], op[4])
            self.draw_mesh(op[1], op[2], op[3])
        elif k == "meshi":
            self.draw_mesh_instanced(op[1], op[2], op[3], op[4], op[5])
        elif k == "lmesh":
            self.draw_mesh_lit(op[1], op[2], op[3])
        elif k == "lmesh2":
            self.draw_mesh_lit(op[1], op[2], op[3])
            if self.lit:
                self.move_mesh(self.lit[op[1] % len(self.lit)], op[4])
            self.draw_mesh_lit(op[1], op[2], op[3])
        elif k == "lmeshi":
            self.draw_mesh_lit_instanced(op[1], op[2], op[3], op[4], op[5])
        elif k == "ptri":
            _, src, n, seed, spread, texref = op
            tex = self.texture(texref)
            xy, z, uv, q = perspective_soup(n, W0, H0, seed, spread, (tex.width, tex.height))
            self.textured_batch(tex, xy, z, uv, "const", src, q=q)
        elif k in STATE5_OPS or k == "wrap":
            self.set_state(k, op)
        elif k == "fill":
            ctx.fill_color(*op[1])
        elif k == "rect":
            g = op[2]
            ctx.draw_rect(g[0], g[1], g[2], g[3], *op[1])
        elif k == "line":
            g = op[2]
            ctx.draw_line(g[0], g[1], g[2], g[3], 1.0 + abs(g[0]) % 7, *op[1])
        elif k == "circle":
            g = op[2]
            ctx.draw_circle(g[0], g[1], abs(g[2]) % 50, *op[1])
        elif k == "grd":
            g, c = op[2], op[1]
            ctx.draw_vertical_grd(g[0], g[1], g[2], g[3], c[0], c[1], c[2], c[3], c[3], c[2], c[1], c[0])
        elif k in ("tex", "stex"):
            g, tex = op[2], self.texture(op[1], True)
            if tex.width < 2 or tex.height < 2:
                pass
            elif k == "tex":
                ctx.draw_texture(tex, g[0], g[1], g[2], g[3])
            else:
                u = op[3]
                ctx.draw_splitted_texture(tex, g[0], g[1], g[2], g[3], u[0], u[1], u[2], u[3])
        elif k == "setpx":
            ctx.set_pixel(op[1], op[2], *op[3])
        elif k == "applypx":
            ctx.apply_pixel(op[1], op[2], *op[3])
        elif k == "snap":
            self.snap(op[1], op[2])
        elif k == "aux":
            aux, c, g = self.aux_ctx(), op[2], op[3]
            if op[1] == "rect":
                aux.draw_rect(g[0] % AUX_W, g[1] % AUX_H, 2 + g[2] % AUX_W, 2 + g[3] % AUX_H, *c)
            elif op[1] == "circle":
                aux.draw_circle(g[0] % AUX_W, g[1] % AUX_H, 1 + g[2] % 12, *c)
            elif op[1] == "clear":
                aux.set_color(*c)
            else:
                xy, z, col = colour_soup(12, AUX_W, AUX_H, int(abs(g[0]) * 1000), 8.0, True, c[3] < 0.5)
                self.colour_batch(xy, z, col, True, "host", ctx=aux)
        elif k == "transform":
            ctx.set_transform(*op[1])
        elif k == "translate":
            ctx.translate(op[1][0] * 10, op[1][1] * 10)
        elif k == "rotate":
            ctx.rotate(op[1][0])
        elif k == "scale":
            ctx.scale(0.5 + abs(op[1][0]) / 3, 0.5 + abs(op[1][1]) / 3)
        elif k == "ct":
            ctx.set_color_transform(*[abs(v) / 3 for v in op[1]])
        elif k == "save":
            ctx.save_state()
        elif k == "restore":
            ctx.restore_state()
        elif k == "clear":
            ctx.set_color(*[abs(v) / 3 for v in op[1]])
        elif k == "cleardepth":
            ctx.clear_depth(op[1])
        elif k == "depthstate":
            ctx.set_depth_state(op[1], op[2])
        elif k == "resize":
            ctx.resize(op[1], op[2])
            self.W, self.H = op[1], op[2]
            self.snaps.pop(("main", True), None)
        elif k == "getcolor":
            self.over_cap = False
            self.probes.append(np.array(ctx.get_color(op[1], op[2])[:4 if self.alpha else 3], dtype=np.float64))
        elif k == "readf64":
            self.over_cap = False
            self.probes.append(ctx.get_buffer_numpy())
        elif k == "readdepth":
            self.over_cap = False
            self.probes.append(ctx.get_depth_buffer())
        elif k in ("begin", "end", "flush", "gather"):
            self.over_cap &= k in ("begin", "end")
            if self.gpu:
                {"begin": ctx.begin_commands, "end": ctx.end_commands, "flush": ctx.flush_commands,
                 "gather": ctx.gather_frame_u8}[k]()
        else:
            raise ValueError(f"unknown operation {op!r}")

    def run(self):
        fmt = self.knobs["fmt"]
        self.ctx = self.context(self.W, self.H, self.alpha, fmt)
        self.make_resources()
        ctx = self.ctx
        ctx.set_color(0.25, 0.5, 0.75, 1.0)
        ctx.set_depth_state(True, True)
        ctx.clear_depth()
        for op in self.ops:
            if op[0] in self.batch_ops and not self.triangles:
                continue
            self.op(op)
        out = {}
        if self.gpu:
            self.check_states()
        if fmt and self.gpu:
            ctx.gather_frame_u8()
            out["frame"] = ctx.get_frame_u8()
        out.update(f64=ctx.get_buffer_numpy(), depth=ctx.get_depth_buffer(), u8=ctx.get_buffer_as_uint8_numpy())
        if fmt and not self.gpu:
            out["frame"] = out["u8"] if fmt == "rgb" else scenes.yuv420p(out["u8"])
        out["probes"] = self.probes
        out["batches"] = self.batches
        out["warm"] = ctx.warm_batch_count() if self.gpu else 0
        out["counts"] = self.counts
        out["changed_over_cap"] = self.changed_over_cap
        self.keep.clear()
        return out


def run(fac, frame, triangles=True):
    """Executes `frame` on `fac`: dict f64, depth, u8, frame (with a frame
    format), probes (list of arrays), batches [(kind, raster path, tile
    pairs)] (kind colour, textured, mesh, instanced or lit), warm, counts
    [(full, rasterised triangles)] of the mesh draws, changed_over_cap (how
    often one of the six states changed after a batch of more than 50 tile
    pairs and before the next flush, gather or probe).  triangles=False leaves
    the triangle operations out."""
    return _Run(fac, frame, triangles).run()


ARRAYS = ("frame", "f64", "depth", "u8")


def mismatches(got, want):
    """[(what, scenes.first_mismatch)] over the arrays and probes of two runs."""
    bad = []
    for k in ARRAYS:
        if k in want and not scenes.bits_equal(got[k], want[k]):
            bad.append((k, scenes.first_mismatch(got[k], want[k])))
    if len(got["probes"]) != len(want["probes"]):
        bad.append(("probes", f"{len(got['probes'])} != {len(want['probes'])}"))
    for i, (a, b) in enumerate(zip(got["probes"], want["probes"])):
        if not scenes.bits_equal(a, b):
            bad.append((f"probe {i}", scenes.first_mismatch(a, b)))
    return bad


# ---------------------------------------------------------------------------
# what a frame holds (for the generator's own test and the GPU counters)
# ---------------------------------------------------------------------------
def kinds(frame):
    """The operation kinds of the vocabulary's table that `frame` uses."""
    W, H, alpha, knobs, res, ops = frame
    out = set()
    texs, bufs, meshes = res.get("texs", []), res.get("bufs", []), res.get("meshes", [])

    def texref(ref, user):
        if ref[0] == "res" and texs:
            w, h, ch, dtype, _, rs = texs[ref[1] % len(texs)]
            out.update({"texture:" + dtype, "texture:rgba" if ch == 4 else "texture:rgb"})
            if rs:
                out.add("texture:resampled")
        elif ref[0] == "snap":
            out.update({"snapshot:" + ref[1], "snapshot:shared" if ref[2] else "snapshot:as_texure",
                        "snapshot->" + user})

    def buffer(i, ref):
        if bufs:
            spec = bufs[i % len(bufs)]
            if spec[0] == "c":
                out.add("colour:buffer")
            else:
                out.update({"textured:buffer", "uv:" + spec[4]})
                if spec[4] == "const":
                    texref(ref, "soup")

    def mesh(i, mat, ref):
        if meshes:
            spec = meshes[i % len(meshes)]
            out.add({"c": "mesh:colour", "l": "mesh:colour", "tu": "mesh:textured-unshared",
                     "ts": "mesh:textured-2x2"}[spec[0]])
            out.add("matrix:" + mesh_matrix(spec[1], mat, 8, 8)[0])
            if spec[0] == "tu":
                texref(ref, "soup")

    # the mesh draws under the tracked clip state: the triangle counts of their reference soups
    near, cull, nl = 0.0, 0, 0
    dicts = {}
    lit = [i for i, spec in enumerate(meshes) if spec[0] == "l"]

    def clipped(i, mats):
        """Notes whether the near plane or the cull changed the draw's triangle count."""
        if i not in dicts:
            dicts[i] = mesh_dict(meshes[i], W, H)
        if near > 0 or cull:
            for M in mats:
                n0 = dicts[i]["idx"].shape[0]
                n1 = int(MC.clip_soup(dicts[i], M, near, 0)[3].sum()) if near > 0 else n0
                n2 = int(MC.clip_soup(dicts[i], M, near, cull)[3].sum()) if cull else n1
                if n1 != n0:
                    out.add("clip:cut")
                if n2 < n1:
                    out.add("cull:dropped")

    def move(i, seed):
        clipped(i, ())
        dicts[i] = moved_mesh(meshes[i], dicts[i], W, H, seed)

    for op in ops:
        k = op[0]
        if k in ("mesh", "mesh2") and meshes:
            i = op[1] % len(meshes)
            clipped(i, [mesh_matrix(meshes[i][1], op[2], W, H)[1]])
            if k == "mesh2":
                move(i, op[4])
                clipped(i, [mesh_matrix(meshes[i][1], op[2], W, H)[1]])
        elif k in ("lmesh", "lmesh2") and lit:
            i = lit[op[1] % len(lit)]
            out.update({k, "lights:0"} if nl == 0 else {k, "lights:8"} if nl == 8 else {k})
            clipped(i, [mesh_matrix(meshes[i][1], op[2], W, H)[1]])
            if k == "lmesh2":
                move(i, op[4])
                clipped(i, [mesh_matrix(meshes[i][1], op[2], W, H)[1]])
        elif (k == "meshi" and meshes) or (k == "lmeshi" and lit):
            i = op[1] % len(meshes) if k == "meshi" else lit[op[1] % len(lit)]
            out.add(k)
            if k == "lmeshi" and nl in (0, 8):
                out.add(f"lights:{nl}")
            if op[4] == "alpha" and meshes[i][0] in ("c", "l"):
                out.add("tint:alpha")
            clipped(i, instance_matrices(meshes[i][1], op[2], op[3], W, H)[1])
        elif k == "near":
            near = float(op[1])
        elif k == "cull":
            cull = int(op[1])
        elif k == "lights":
            nl = 0 if op[1] is None else op[2]
        if k == "tri":
            out.add("colour:" + {"host": "host", "dev": "device", "dev8": "device"}[op[1]])
        elif k == "ttri":
            out.update({"textured:" + {"host": "host", "dev": "device", "dev8": "device"}[op[1]], "uv:" + op[5]})
            texref(op[6], "soup")
        elif k in ("buf", "buf2"):
            buffer(op[1], op[2])
            if k == "buf2" and bufs:
                out.add("buffer:again")
        elif k in ("mesh", "mesh2"):
            mesh(op[1], op[2], op[3])
            if k == "mesh2" and meshes:
                out.add("mesh:update_positions")
        elif k in ("meshi", "lmesh", "lmesh2", "lmeshi"):
            pass                                   # (noted above, where the mesh exists)
        elif k == "ptri":
            out.add("ptri")
            texref(op[5], "soup")
        elif k in ("tex", "stex"):
            out.add(k)
            texref(op[1], "draw_texture")
        elif k == "snap":
            out.update({"snapshot:" + op[1], "snapshot:shared" if op[2] else "snapshot:as_texure"})
        elif k == "aux":
            out.add("aux:draw")
        elif k == "cleardepth":
            out.add("cleardepth" if op[1] == 0xFFFFFFFF else "cleardepth:value")
        else:
            out.add(k)
    return out


BASE_KINDS = (
    "colour:host", "colour:buffer", "colour:device",
    "textured:host", "textured:buffer", "textured:device", "uv:const", "uv:free",
    "mesh:colour", "mesh:textured-unshared", "mesh:textured-2x2", "mesh:update_positions", "buffer:again",
    "matrix:none", "matrix:ident", "matrix:affine", "matrix:perspective",
    "fill", "rect", "line", "circle", "grd", "tex", "stex", "setpx", "applypx",
    "texture:u8", "texture:f64", "texture:rgb", "texture:rgba", "texture:resampled",
    "snapshot:main", "snapshot:aux", "snapshot:as_texure", "snapshot:shared",
    "snapshot->draw_texture", "snapshot->soup", "aux:draw",
    "translate", "rotate", "scale", "ct", "save", "restore", "clear", "cleardepth", "cleardepth:value",
    "depthstate", "resize",
    "getcolor", "readf64", "readdepth",
    "begin", "end", "flush", "gather",
)
# the state frames add the five states, the draws that read them and what those draws must reach
STATE_KINDS = ("near", "cull", "mpersp", "filter", "lights", "meshi", "lmesh", "lmesh2", "lmeshi", "ptri",
               "clip:cut", "cull:dropped", "tint:alpha", "lights:0", "lights:8")
ALL_KINDS = BASE_KINDS + STATE_KINDS


def batch_kinds(frame):
    """[set of triangle kinds per depth-buffer epoch], total batch count: the
    triangle kinds (colour, textured, mesh) that meet in one depth buffer
    with no clear_depth (or resize) between them."""
    W, H, alpha, knobs, res, ops = frame
    bufs, meshes = res.get("bufs", []), res.get("meshes", [])
    epochs, count = [set()], 0
    for op in ops:
        k = op[0]
        if k in ("cleardepth", "resize"):
            epochs.append(set())
        elif k == "tri":
            epochs[-1].add("colour"); count += 1
        elif k == "ttri":
            epochs[-1].add("textured"); count += 1
        elif k in ("buf", "buf2") and bufs:
            epochs[-1].add("colour" if bufs[op[1] % len(bufs)][0] == "c" else "textured")
            count += 2 if k == "buf2" else 1
        elif k in ("mesh", "mesh2") and meshes:
            epochs[-1].add("mesh")
            count += 2 if k == "mesh2" else 1
        elif k == "ptri":
            epochs[-1].add("textured"); count += 1
        elif k == "meshi" and meshes:
            epochs[-1].add("instanced"); count += 1
        elif k in ("lmesh", "lmesh2", "lmeshi") and any(spec[0] == "l" for spec in meshes):
            epochs[-1].add("lit")
            count += 2 if k == "lmesh2" else 1
    return epochs, count


_DEFAULT5 = dict(near=0.0, cull=0, mpersp=False, filter=0, lights=(None, 0))


def state_stats(frame):
    """What a frame does with the five sticky states: dict of three flags.
    two_states      a mesh draw is issued with at least two of the five at a
                    non-default value
    changed_between one of the five changes value between two mesh or textured
                    batches with no flush, gather or probe between them
    meets_others    a lit or instanced draw shares a depth-buffer epoch with a
                    colour, textured or (single, unlit) mesh batch"""
    W, H, alpha, knobs, res, ops = frame
    bufs, meshes = res.get("bufs", []), res.get("meshes", [])
    has_lit = any(spec[0] == "l" for spec in meshes)
    state = dict(_DEFAULT5)
    two = between = False
    pending = changed = False            # a mesh or textured batch issued; a state changed since
    for op in ops:
        k = op[0]
        mesh_draw = (k in ("mesh", "mesh2", "meshi") and meshes) or (k in ("lmesh", "lmesh2", "lmeshi") and has_lit)
        textured = k in ("ttri", "ptri") or (k in ("buf", "buf2") and bufs and bufs[op[1] % len(bufs)][0] == "t")
        if k in STATE5_OPS:
            new = (op[1], 0 if op[1] is None else op[2]) if k == "lights" else type(_DEFAULT5[k])(op[1])
            changed |= pending and new != state[k]
            state[k] = new
        elif mesh_draw or textured:
            two |= bool(mesh_draw) and sum(state[n] != _DEFAULT5[n] for n in state) >= 2
            between |= changed
            pending, changed = True, False
        elif k in ("flush", "gather", "getcolor", "readf64", "readdepth"):
            pending = changed = False
    meets = any(e & {"lit", "instanced"} and e & {"colour", "textured", "mesh"} for e in batch_kinds(frame)[0])
    return dict(two_states=two, changed_between=between, meets_others=meets)


# ---------------------------------------------------------------------------
# strategies
# ---------------------------------------------------------------------------
# hypothesis draws two seeds, the pixel format, the frame format and a cap on
# the operation count; the rest of the frame follows from them
# (random.Random), operation by operation, so a frame cut to k operations is
# the prefix of the uncut one (what shrinking needs) and the generator's
# distribution is the one written below, not hypothesis's (which draws a
# frame side of 1 in a third of its examples).

_SPREADS = (1.5, 6.0, 40.0, 40.0, 300.0)
_WEIGHTED_DEPTHS = DEPTH_VALUES[:1] * 7 + DEPTH_VALUES[1:4] * 2 + DEPTH_VALUES[4:]
# budget: the bounding boxes of a large frame's batch cover at most so many
# pixels (the oracle's cost), so the largest counts go with the small spreads
SMALL = dict(maxn=120, maxmesh=200, resize=True, budget=None, again=3)
LARGE = dict(maxn=4000, maxmesh=4000, resize=False, budget=1.5e6, again=8)   # (few frames: more repeated buffers)


class _Gen:
    def __init__(self, r, W, H, limits):
        self.r = r
        self.W, self.H, self.lim = W, H, limits

    def seed(self):
        return self.r.randrange(2**31 - 1)

    def count(self, maxn, lo=1, spread=None):
        """Batch sizes: mostly a good part of the maximum."""
        if self.lim["budget"]:
            area = min((2 * spread + 3) ** 2, float(self.W * self.H))
            maxn = max(lo, 1, min(maxn, int(self.lim["budget"] // area)))
        return self.r.choice([self.r.randint(lo, maxn), self.r.randint(max(lo, maxn // 4), maxn), maxn])

    def col(self):
        return [self.r.random() for _ in range(4)]

    def g4(self):
        return [self.r.uniform(-20.0, 140.0) for _ in range(4)]

    def v4(self):
        return [self.r.uniform(-3.0, 3.0) for _ in range(4)]

    def knobs(self, fmt):
        k = {name: self.r.choice(values) for name, values in KNOB_VALUES.items()}
        k["fmt"] = fmt
        return k

    def resources(self):
        r, lim = self.r, self.lim
        texs = []
        for _ in range(r.choice([1, 2, 3, 3, 3])):
            rs = (r.randint(2, 24), r.randint(2, 24)) if r.random() < 0.4 else None
            texs.append((r.randint(2, 40), r.randint(2, 30), r.choice([3, 4]), r.choice(["u8", "f64"]), self.seed(), rs))
        bufs = []
        for k in range(r.choice([0, 1, 2, 2, 2, 2])):
            spread = r.choice(_SPREADS)
            n = self.count(lim["maxn"], 1, spread)
            textured = r.random() < 0.5 if k == 0 else bufs[0][0] == "c"      # (two buffers: one of each kind)
            if textured:
                bufs.append(("t", n, self.seed(), spread, r.choice(["const", "const", "free"])))
            else:
                bufs.append(("c", n, self.seed(), spread, r.random() < 0.5, r.random() < 0.4))
        meshes = []
        for _ in range(r.choice([0, 1, 2, 2, 2, 2])):
            kind = r.choice(["c", "c", "c", "tu", "tu", "ts", "ts"])
            space = r.choice(["screen", "model"])
            if kind == "tu":
                s = r.choice([0.05, 0.3, 1.0])
                meshes.append(("tu", space, self.count(lim["maxmesh"], 1, 0.45 * max(self.W, self.H) * s), self.seed(), s))
                continue
            rows = r.randint(1, 10 if lim["maxmesh"] <= 200 else 40)
            cols = r.randint(1, max(1, min(50, lim["maxmesh"] // (2 * rows))))
            meshes.append(("ts", space, rows, cols, self.seed()) if kind == "ts" else
                          ("c", space, rows, cols, self.seed(), r.random() < 0.6, r.random() < 0.35))
        self.res = dict(texs=texs, bufs=bufs, meshes=meshes)
        return self.res

    def texref(self):
        r = self.r
        x = r.random()
        if x < 0.55:
            return ("res", r.randrange(len(self.res["texs"])))
        if x < 0.65:
            return self.tiny()
        return ("snap", r.choice(["main", "aux"]), r.random() < 0.5)

    def tiny(self):
        return ("tiny", self.seed(), self.r.choice([3, 4]))

    def src(self):
        return self.r.choice(["host", "host", "dev", "dev8"])

    def batch_op(self):
        r, lim, res = self.r, self.lim, self.res
        kind = r.choice(["tri"] * 4 + ["ttri"] * 6 + (["buf"] * 2 + ["buf2"] * lim["again"]) * bool(res["bufs"])
                        + (["mesh"] * 7 + ["mesh2"] * 4) * bool(res["meshes"]))
        if kind == "tri":
            src, spread = self.src(), r.choice(_SPREADS)
            return ("tri", src, self.count(lim["maxn"], 0 if src == "host" else 1, spread), self.seed(), spread,
                    r.random() < 0.5, r.random() < 0.4)
        if kind == "ttri":
            src, spread = self.src(), r.choice(_SPREADS)
            uvkind = r.choice(["const", "const", "free"])
            return ("ttri", src, self.count(lim["maxn"], 0 if src == "host" else 1, spread), self.seed(), spread,
                    uvkind, self.texref() if uvkind == "const" else self.tiny())
        if kind == "buf":
            return ("buf", r.randrange(len(res["bufs"])), self.texref())
        if kind == "buf2":
            return ("buf2", r.randrange(len(res["bufs"])), self.texref(), r.choice([0.0, 0.0, 1.5, 33.0]))
        if kind == "mesh":
            return ("mesh", r.randrange(len(res["meshes"])), r.randrange(4), self.texref())
        return ("mesh2", r.randrange(len(res["meshes"])), r.randrange(4), self.texref(), self.seed())

    def prim_op(self):
        r = self.r
        kind = r.choice(["fill", "rect", "line", "circle", "grd", "tex", "tex", "stex", "stex", "setpx", "applypx"])
        if kind == "fill":
            return ("fill", self.col())
        if kind == "tex":
            return ("tex", self.texref(), self.g4())
        if kind == "stex":
            return ("stex", self.texref(), self.g4(), self.col())
        if kind in ("setpx", "applypx"):
            return (kind, r.randint(-2, self.W + 1), r.randint(-2, self.H + 1), self.col())
        return (kind, self.col(), self.g4())

    def state_op(self, late=False):
        """late: without the operations that wipe the frame (set_color, resize)."""
        r = self.r
        kind = r.choice(["translate", "rotate", "scale", "ct", "save", "restore", "cleardepth", "cleardepth", "cleardepth",
                         "depthstate", "depthstate"] + (["clear", "clear", "clear"] + ["resize", "resize", "resize"] * self.lim["resize"]) * (not late))
        if kind == "cleardepth":
            return ("cleardepth", r.choice(_WEIGHTED_DEPTHS))
        if kind == "depthstate":
            return ("depthstate", r.random() < 0.6, r.random() < 0.6)
        if kind == "resize":
            return ("resize", r.randint(1, 140), r.randint(1, 110))
        return (kind, self.v4())

    def other_op(self):
        r = self.r
        kind = r.choice(["getcolor", "readf64", "readdepth", "begin", "end", "flush", "gather", "snap", "aux"])
        if kind == "getcolor":
            return ("getcolor", r.uniform(-5.0, self.W + 5.0), r.uniform(-5.0, self.H + 5.0))
        if kind == "snap":
            return ("snap", r.choice(["main", "aux"]), r.random() < 0.5)
        if kind == "aux":
            return ("aux", r.choice(["rect", "circle", "clear", "tri"]), self.col(), self.g4())
        return (kind,)

    def op(self, late=False):
        x = self.r.random()
        return (self.batch_op() if x < 0.28 else self.prim_op() if x < 0.52 else
                self.state_op(late) if x < 0.80 else self.other_op())


class _StateGen(_Gen):
    """The generator of the state frames: _Gen's vocabulary plus the five
    sticky states and the draws that read them, on a random stream of its own
    (make_small_state_frame / make_large_state_frame; the streams of the
    "small" and "large" examples are not touched)."""

    def resources(self):
        """_Gen's textures and buffers; one to three meshes, a lit one first."""
        r, lim = self.r, self.lim
        res = super().resources()
        meshes = []
        for k in range(r.choice([2, 2, 3, 3])):
            kind = "l" if k == 0 else r.choice(["c", "tu", "tu", "ts", "ts"])
            space = r.choice(["screen", "model"] + ["model"] * (kind == "l"))
            if kind == "tu":
                s = r.choice([0.05, 0.3, 1.0])
                meshes.append(("tu", space, self.count(lim["maxmesh"], 1, 0.45 * max(self.W, self.H) * s), self.seed(), s))
                continue
            rows = r.randint(1, 10 if lim["maxmesh"] <= 200 else 40)
            cols = r.randint(1, max(1, min(50, lim["maxmesh"] // (2 * rows))))
            meshes.append(("ts", space, rows, cols, self.seed()) if kind == "ts" else
                          (kind, space, rows, cols, self.seed(), r.random() < 0.6, r.random() < 0.3))
        r.shuffle(meshes)
        res["meshes"] = meshes
        return res

    def mesh_triangles(self, i):
        spec = self.res["meshes"][i]
        return spec[2] if spec[0] == "tu" else 2 * spec[2] * spec[3]

    def instances(self, i):
        """K of an instanced draw of mesh i: small frames 1..6 and at most 600
        triangles; large frames at most 40, 4000 triangles and the
        bounding-box budget, which an instance of mean scale 0.55 enters with
        the frame's area (both faces of the sphere, boxes twice their triangles)."""
        n = max(1, self.mesh_triangles(i))
        if not self.lim["budget"]:
            return self.r.randint(1, max(1, min(6, 600 // n)))
        top = min(40, 4000 // n, int(self.lim["budget"] // (1.2 * self.W * self.H)))
        return self.r.randint(1, max(1, top))

    def lit_index(self):
        lit = [i for i, spec in enumerate(self.res["meshes"]) if spec[0] == "l"]
        k = self.r.randrange(len(lit))
        return k, lit[k]

    def batch_op(self):
        r = self.r
        kind = r.choice(["old"] * 14 + ["meshi"] * 4 + ["lmesh"] * 3 + ["lmesh2"] * 2 + ["lmeshi"] * 3 + ["ptri"] * 2)
        if kind == "old":
            return super().batch_op()
        if kind == "ptri":
            src, spread = self.src(), r.choice(_SPREADS)
            return ("ptri", src, self.count(self.lim["maxn"], 1, spread), self.seed(), spread, self.texref())
        if kind == "meshi":
            i = r.randrange(len(self.res["meshes"]))
            return ("meshi", i, self.instances(i), self.seed(), r.choice([None, "opaque", "alpha"]), self.src())
        k, i = self.lit_index()
        if kind == "lmeshi":
            return ("lmeshi", k, self.instances(i), self.seed(), r.choice([None, "opaque", "alpha"]), self.src())
        nseed = self.seed() if r.random() < 0.7 else None
        if kind == "lmesh":
            return ("lmesh", k, r.choice(_INSTANCE_MATS), nseed)
        return ("lmesh2", k, r.choice(_INSTANCE_MATS), nseed, self.seed())

    def five_op(self):
        r = self.r
        kind = r.choice(STATE5_OPS + ("lights", "near"))
        if kind == "near":
            return ("near", r.choice(NEAR_VALUES + NEAR_VALUES[1:]))
        if kind == "cull":
            return ("cull", r.choice([0, 1, 2, 1, 2]))
        if kind == "mpersp":
            return ("mpersp", r.random() < 0.7)
        if kind == "filter":
            return ("filter", int(r.random() < 0.7))
        x = r.random()
        return ("lights", None, 0) if x < 0.1 else ("lights", self.seed(), 0 if x < 0.3 else 8 if x < 0.7 else r.randint(1, 7))

    def op(self, late=False):
        x = self.r.random()
        return (self.batch_op() if x < 0.34 else self.prim_op() if x < 0.47 else self.state_op(late) if x < 0.64 else
                self.five_op() if x < 0.85 else self.other_op())


def _even(fmt, v):
    return v + (v & 1) if fmt == "yuv420p" else v


def _size(r, lo, hi):
    """A frame side: now and then the smallest sides and the largest one."""
    x = r.random()
    return r.randint(lo, min(lo + 2, hi)) if x < 0.08 else hi if x < 0.12 else r.randint(lo, hi)


def _rng(seed, salt, alpha, fmt):
    return random.Random(f"{seed}/{salt}/{alpha}/{fmt}")


def make_small_frame(seed, salt, alpha, fmt, keep):
    r = _rng(seed, salt, alpha, fmt)
    W, H = _even(fmt, _size(r, 1, 140)), _even(fmt, _size(r, 1, 110))
    g = _Gen(r, W, H, SMALL)
    knobs, res = g.knobs(fmt), g.resources()
    planned = r.choice(_NOPS)
    ops = [g.op(late=k >= planned // 2) for k in range(min(keep, planned))]
    ops = [("resize", _even(fmt, op[1]), _even(fmt, op[2])) if op[0] == "resize" else op for op in ops]
    return (W, H, alpha, knobs, res, ops)


def make_large_frame(seed, salt, alpha, fmt, keep):
    r = _rng(seed, salt, alpha, fmt)
    W, H = _even(fmt, _size(r, 64, 700)), _even(fmt, _size(r, 32, 420))
    g = _Gen(r, W, H, LARGE)
    knobs, res = g.knobs(fmt), g.resources()
    ops = []
    for _ in range(min(keep, r.randint(1, 4))):
        ops.append(g.batch_op())
        if r.random() < 0.5:
            ops.append(r.choice([g.prim_op, g.state_op, g.other_op])())
    return (W, H, alpha, knobs, res, ops)


def make_small_state_frame(seed, salt, alpha, fmt, keep):
    r = _rng(seed, f"state/{salt}", alpha, fmt)
    W, H = _even(fmt, _size(r, 1, 140)), _even(fmt, _size(r, 1, 110))
    g = _StateGen(r, W, H, SMALL)
    knobs, res = g.knobs(fmt), g.resources()
    planned = r.choice(_STATE_NOPS)
    ops = [g.op(late=k >= planned // 2) for k in range(min(keep, planned))]
    ops = [("resize", _even(fmt, op[1]), _even(fmt, op[2])) if op[0] == "resize" else op for op in ops]
    return (W, H, alpha, knobs, res, ops)


def make_large_state_frame(seed, salt, alpha, fmt, keep):
    r = _rng(seed, f"state/{salt}", alpha, fmt)
    W, H = _even(fmt, _size(r, 64, 700)), _even(fmt, _size(r, 32, 420))
    g = _StateGen(r, W, H, LARGE)
    knobs, res = g.knobs(fmt), g.resources()
    ops = []
    for _ in range(min(keep, r.randint(1, 4))):
        for _ in range(r.randint(0, 3)):
            ops.append(g.five_op())
        ops.append(g.batch_op())
        if r.random() < 0.5:
            ops.append(r.choice([g.prim_op, g.state_op, g.other_op])())
    return (W, H, alpha, knobs, res, ops)


_NOPS = (8, 9, 10, 10, 10, 10, 10, 10)
_STATE_NOPS = (16, 17, 18, 18, 18, 18, 18, 18)
_seed = st.integers(0, 2**31 - 1)
_fmt = st.sampled_from(KNOB_VALUES["fmt"])
_keep = st.sampled_from([10] * 20 + [5, 2, 1])     # (shrinking cuts a frame's tail)
_state_keep = st.sampled_from([18] * 20 + [9, 4, 2])
# hypothesis mixes integer constants (|v| >= 100) from the source of every project module the process has imported
# into what st.integers draws, so the examples that come from _seed depend on the process's imports (the library
# binding, say, which a GPU run imports and a CPU run of this file alone does not).  The "small" and "large" examples
# keep _seed: they are what they are.  The state frames draw their seeds as five digits below 64, which no such
# constant fits, and are the same examples in every process (tests/test_frame_ops.py checks both statements).
_digit = st.integers(0, 63)
_stable_seed = st.builds(lambda a, b, c, d, e: (((a * 64 + b) * 64 + c) * 64 + d) * 64 + e,
                         _digit, _digit, _digit, _digit, _digit)


def small_frames():
    """W in [1, 140], H in [1, 110], 1-10 operations, at most 120 triangles
    per batch, meshes of at most 200 triangles."""
    return st.builds(make_small_frame, _seed, _seed, st.booleans(), _fmt, _keep)


def large_frames():
    """W in [64, 700], H in [32, 420], 1-4 triangle operations of up to 4000
    triangles of any kind and source, primitives and state between them."""
    return st.builds(make_large_frame, _seed, _seed, st.booleans(), _fmt, _keep)


def small_state_frames():
    """small_frames' sizes with 1-18 operations: the five sticky states, the
    instanced, lit and perspective draws that read them (K in 1..6, at most 600
    triangles per instanced draw) and everything small_frames holds."""
    return st.builds(make_small_state_frame, _stable_seed, _stable_seed, st.booleans(), _fmt, _state_keep)


def large_state_frames():
    """large_frames' sizes and budget (which counts the instances: K at most 40
    and at most 4000 triangles per instanced draw), state changes before each
    of the 1-4 triangle operations."""
    return st.builds(make_large_state_frame, _stable_seed, _stable_seed, st.booleans(), _fmt, _state_keep)


SMALL_EXAMPLES = 200
LARGE_EXAMPLES = 50


def for_each_frame(size, visit):
    """Calls visit(frame) for the examples of the "small", "large",
    "small-state" or "large-state" frames:
    one inner @given function with fixed settings and derandomize=True, so
    that every caller (the generator's own CPU test and the GPU test) draws
    the same examples -- the state frames in every process, the "small" and
    "large" ones in processes that have imported the same project modules
    (see _stable_seed)."""
    strategy, n = {"small": (small_frames(), SMALL_EXAMPLES), "large": (large_frames(), LARGE_EXAMPLES),
                   "small-state": (small_state_frames(), SMALL_EXAMPLES),
                   "large-state": (large_state_frames(), LARGE_EXAMPLES)}[size]

    @settings(max_examples=n, deadline=None, derandomize=True, database=None,
              suppress_health_check=list(HealthCheck))
    @given(strategy)
    def examples(fr):
        visit(fr)

    examples()

"""The mixed-frame vocabulary of tests/frame_ops.py extended by the features
merged after it: the texture wrap state, modulated textured soups, textured
colour meshes (unlit and lit), skinned and morphed meshes.  This module
imports frame_ops and frame_ops never imports it: hypothesis mixes the integer
constants of every imported project module into st.integers, and the pinned
"small" and "large" example streams are drawn in an interpreter that imports
frame_ops alone (tests/test_frame_ops.py).  frame_ops itself only gained
hooks: the tracked wrap with its setter, getter check and substitution rule,
the "tiled" UV kind, and the methods this interpreter overrides.

A frame is frame_ops' (W, H, alpha, knobs, resources, ops) with

resources   meshes  also ("tc" | "tl", space, n, seed, spread): a textured
                    colour mesh ("tl": with normals) of n triangles with
                    unshared vertices behind a permutation, like "tu"; one
                    "tiled" (u, v) per triangle and a colour per vertex (alpha
                    in (0.1, 0.9) on every vertex for seed % 3 == 0, else 1).
                    It samples its own texture ("pow2", seed, 3 + seed % 2).
            bufs    textured buffers also with uv "tiled"
            rigs    [(mesh index, bone count, seed, with normals, variant)]
                    mesh_skin_ref.random_rig over the mesh's created positions
                    (and normals: the bind pose); variant: MeshSkin.set_variant
            morphs  [(mesh index, T, seed, with normals)]
                    mesh_morph_ref.random_morph over the created mesh (the
                    deltas of a screen-space mesh times (40, 40, 0.5))
texture references   also ("pow2", seed, channels): an f64 texture with sides
            in 2..9 whose every texel channel, alpha included, is 0.25, 0.5 or 1

OPS, beside frame_ops.OPS:

("wrap", u, v)                                        the sixth sticky state, set_triangle_texture_wrap; u, v in 0..2
("ttri", src, n, seed, spread, "tiled", texref)       one (u, v) per triangle over [-2w, 3w) x [-2h, 3h)
("mtri", src, n, seed, spread, colkind, blended, qkind, texref)
                                                      modulated soup, "tiled" UVs; colkind "flat" | "gouraud" (texref then
                                                      "pow2"); vertex alpha 1 or in (0.1, 0.9); qkind None | "pow2" (one of
                                                      Q_VALUES per triangle)
("mesh", i, mat, texref) of a "tc" / "tl" mesh        draw_mesh(gm, M, texture=) (texref ignored: the mesh's own texture)
("lmesh", i, mat, nseed), ("lmesh2", ...)             i indexes the lit meshes, "l" and "tl"; a "tl" mesh is drawn by
                                                      draw_mesh_lit(gm, M, N, texture=)
("meshi", ...), ("lmeshi", ...)                       index the meshes (the lit meshes) that are not "tc" / "tl": the
                                                      library has no instanced draw of a textured colour mesh
("pose", i, pseed, src, where)                        pose_mesh of rig i's mesh; src "host" | "dev"; where "main" | "aux":
                                                      the context that issues the call
("morph", i, wseed, active, src, where)               morph_mesh of morph i's mesh under scattered_weights(T, active, wseed)
("posemorph", i, pseed, wseed, active, src, where)    pose_mesh_morphed: rig i and the first morph of the same mesh (none:
                                                      the operation is a "pose")
("variant", i, v)                                     MeshSkin.set_variant(v) of rig i

Lowerings (tests/test_frame_ops.py proves each on the CPU), all bit-exact:

  every constant-UV textured draw -> flat draw_triangles of wrap_ref.sample(texels, u, v, filter, wrap); under wrap
      (0, 0) these are textured_colours' bits
  "mtri", colkind "flat" (one colour on the three corners: I(c) == c) -> Gouraud draw_triangles of c * T on every
      corner, T = wrap_ref.sample at the triangle's (u, v): any texture, filter and wrap
  "mtri", colkind "gouraud" on a "pow2" texture under the nearest filter -> Gouraud draw_triangles of c_k * T: a
      power-of-two factor commutes with every rounded operation of I(c)
  "tc" / "tl" meshes -> modulate_ref.mesh_soup under the tracked near plane, cull mode and lights, then the
      "gouraud" lowering; a cut vertex keeps a constant UV exactly and its colour scales exactly
  posed and morphed meshes -> the interpreter replaces the mesh's dict by mesh_skin_ref.posed, mesh_morph_ref.morphed
      or mesh_morph_ref.morph_posed, computed from the rig's bind pose or the morph's base (kept apart from the
      current positions, which update_positions may have changed); every later mesh operation draws that dict.  A
      GPU run ends by comparing positions() (lit meshes: normals() too) of every posed mesh with the dict
      (mesh_skin_ref.same_bits), so a mismatch there names the pose kernel, not a draw.

The substitution rule, extended: a free-UV draw under a wrap other than clamp is issued with the wrap switched to
(0, 0) on the GPU side (frame_ops._nearest_for); a "gouraud" mtri and a "tc" / "tl" mesh under the bilinear filter with
the filter switched off; a "tc" / "tl" mesh under a perspective matrix with the mesh perspective on with the
perspective switched off.  Each is switched back after the draw; the tracked state does not change.
"""
from __future__ import annotations

import numpy as np
from hypothesis import HealthCheck, given, settings, strategies as st

import frame_ops as F
import mesh_morph_ref as MM
import mesh_skin_ref as MS
import modulate_ref as MD
import scenes
import wrap_ref as WR

POW2_VALUES = (0.25, 0.5, 1.0)
BONE_COUNTS = (1, 3, 5, 129)
TARGET_COUNTS = (1, 2, 5, 9)
TEXC = ("tc", "tl")
POSE_OPS = ("pose", "morph", "posemorph", "variant")
BATCH_OPS = F.BATCH_OPS + ("mtri",) + POSE_OPS          # (what a run with triangles=False leaves out)
SYNC_OPS = ("flush", "gather", "getcolor", "readf64", "readdepth")


# ---------------------------------------------------------------------------
# inputs from the specs
# ---------------------------------------------------------------------------
def pow2_array(seed, ch):
    g = scenes.rng(seed)
    w, h = int(g.integers(2, 10)), int(g.integers(2, 10))
    return np.ascontiguousarray(np.asarray(POW2_VALUES)[g.integers(0, 3, size=(h, w, ch))])


def modulated_soup(n, W, H, seed, spread, colkind, blended, qkind, size):
    """(xy, z, uv (n, 6), rgba (n, 12), q (n, 3) or None) of an "mtri"."""
    xy, z, uv = F.textured_soup(n, W, H, seed, spread, "tiled", size)
    g = scenes.rng(seed + 4)
    c = g.uniform(0, 1, size=(n, 3, 4))
    c[..., 3] = g.uniform(0.1, 0.9, size=(n, 3)) if blended else 1.0
    if colkind == "flat":
        c = np.repeat(c[:, :1], 3, axis=1)
    q = None
    if qkind is not None:
        q = np.asarray(F.Q_VALUES)[g.integers(0, len(F.Q_VALUES), size=n)]
        q = np.ascontiguousarray(np.repeat(q[:, None], 3, axis=1))
    return xy, z, uv, np.ascontiguousarray(c.reshape(n, 12)), q


def modulated_colours(texels, uv, rgba, filt, wrap):
    """The Gouraud colours (n, 12) both "mtri" lowerings draw: corner colour
    times the texel at the triangle's (u, v)."""
    n = uv.shape[0]
    t = WR.sample(texels, uv[:, 0], uv[:, 1], filt, wrap)
    return np.ascontiguousarray((np.asarray(rgba).reshape(n, 3, 4) * t[:, None, :]).reshape(n, 12))


def wrapped_colours(texels, uv, filt, wrap):
    """frame_ops.textured_colours under a wrap state."""
    return np.ascontiguousarray(WR.sample(texels, uv[:, 0], uv[:, 1], filt, wrap))


def texc_normals(spec, seed):
    g = scenes.rng(seed + 3)
    v = g.normal(size=(3 * spec[2], 3))
    return np.ascontiguousarray(v / np.sqrt((v * v).sum(axis=1))[:, None] * g.uniform(0.8, 1.2, size=(3 * spec[2], 1)))


def texc_dict(spec, W, H):
    """A "tc" / "tl" mesh as modulate_ref's dict: pos, idx, colors, uv, gouraud (and normals)."""
    kind, space, n, seed, _ = spec
    p, g = F.mesh_positions(("tu",) + tuple(spec[1:]), W, H, seed)
    th, tw = pow2_array(seed, 3).shape[:2]
    uv = np.repeat(np.stack([g.uniform(-2.0 * tw, 3.0 * tw, n), g.uniform(-2.0 * th, 3.0 * th, n)], 1), 3, axis=0)
    col = g.uniform(0, 1, size=(3 * n, 4))
    col[:, 3] = g.uniform(0.1, 0.9, size=3 * n) if seed % 3 == 0 else 1.0
    perm = g.permutation(3 * n)          # vertex k of the soup is stored at perm[k]
    pos, puv, pcol = np.empty((3 * n, 3)), np.empty((3 * n, 2)), np.empty((3 * n, 4))
    pos[perm], puv[perm], pcol[perm] = F._to_space(space, p, W, H), uv, col
    mesh = dict(pos=pos, idx=perm.reshape(n, 3).astype(np.uint32), colors=pcol, uv=puv, gouraud=True)
    if kind == "tl":
        mesh["normals"] = texc_normals(spec, seed)
    return mesh


def any_mesh_dict(spec, W, H):
    return texc_dict(spec, W, H) if spec[0] in TEXC else F.mesh_dict(spec, W, H)


def moved_texc(spec, mesh, W, H, seed):
    p, _ = F.mesh_positions(("tu",) + tuple(spec[1:]), W, H, seed)
    pos = np.empty_like(p)
    pos[mesh["idx"].reshape(-1).astype(np.int64)] = F._to_space(spec[1], p, W, H)
    out = dict(mesh, pos=pos)
    if spec[0] == "tl":
        out["normals"] = texc_normals(spec, seed)
    return out


def texc_texref(spec):
    return ("pow2", spec[3], 3 + spec[3] % 2)


def palette(space, nb, pseed, W, H):
    """(nb, 12): mesh_skin_ref.random_palette for a model-space mesh; for a
    screen-space one translations only (a tenth of the frame, 0.05 in depth):
    a rotation about the pixel origin would carry the mesh out of the frame."""
    if space == "model":
        return MS.random_palette(nb, pseed)
    g = scenes.rng(pseed + 31)
    return np.ascontiguousarray(np.stack([MS.bone(0.0, 0.0, (g.uniform(-0.1, 0.1) * W, g.uniform(-0.1, 0.1) * H,
                                                             g.uniform(-0.05, 0.05))) for _ in range(nb)]))


def rig_arrays(mesh, nb, seed):
    return MS.random_rig(np.asarray(mesh["pos"]).shape[0], nb, seed)


def morph_arrays(spec, mesh, T, seed, withn):
    mo = MM.random_morph(mesh, T, seed, normals=bool(withn))
    if spec[1] == "screen":
        mo["dP"] = np.ascontiguousarray(mo["dP"] * np.array([40.0, 40.0, 0.5]))
    return mo


def posed_dict(mesh, bind, rig, use_normals, pal):
    """`mesh` after pose_mesh: from the bind pose, never from the current positions."""
    src = dict(mesh, pos=bind[0])
    if use_normals:
        src["normals"] = bind[1]
    return MS.posed(src, rig, pal, normals=use_normals)


# ---------------------------------------------------------------------------
# the interpreter
# ---------------------------------------------------------------------------
class _AnimRun(F._Run):
    batch_ops = BATCH_OPS

    def __init__(self, fac, frame, triangles=True):
        super().__init__(fac, frame, triangles)
        self.wrap_over_cap = 0          # wrap changes while a batch of more than 50 pairs may be pending
        self.posed_between = 0          # poses between two unsynchronised draws of their mesh
        self.posed_over_cap = 0         # ... issued while a batch of more than 50 pairs may be pending
        self.wrapped = [0, 0]           # constant-UV triangles sampled under a non-clamp wrap: all, outside on a wrapped axis
        self._drawn, self._posed, self._touched = set(), {}, {}
        self._cur = None
        self.posed_paths = set()        # the raster paths of the draws of posed or morphed meshes

    # ---- resources ------------------------------------------------------------
    def mesh_dict(self, spec):
        return any_mesh_dict(spec, self.W, self.H)

    def make_resources(self):
        super().make_resources()
        self.lit_plain = self.lit
        self.lit = [e for e in self.meshes if e[0][0] in ("l", "tl")]
        self.plain = [e for e in self.meshes if e[0][0] not in TEXC]
        self.bind = {id(e): (e[1]["pos"], e[1].get("normals")) for e in self.meshes}
        self.rigs, self.morphs = [], []
        if not self.meshes:
            return
        for mi, nb, seed, withn, variant in self.res.get("rigs", []):
            e = self.meshes[mi % len(self.meshes)]
            rig = rig_arrays(e[1], nb, seed)
            use = bool(withn) and "normals" in e[1]
            skin = None
            if e[2] is not None:
                skin = self.R.MeshSkin(e[1]["pos"], rig["joints"], rig["weights"], nb,
                                       bind_normals=e[1]["normals"] if use else None)
                skin.set_variant(variant)
            self.rigs.append(dict(entry=e, rig=rig, normals=use, skin=skin))
        for mi, T, seed, withn in self.res.get("morphs", []):
            e = self.meshes[mi % len(self.meshes)]
            mo = morph_arrays(e[0], e[1], T, seed, withn)
            gmo = None
            if e[2] is not None:
                gmo = self.R.MeshMorph(mo["pos"], mo["dP"], base_normals=mo.get("normals"), delta_normals=mo.get("dN"))
            self.morphs.append(dict(entry=e, mo=mo, T=T, gmo=gmo))

    def texture(self, ref, prim=False):
        if ref[0] == "pow2":
            t = self.fac.texture(pow2_array(ref[1], ref[2]))
            self.keep.append(t)
            return t
        return super().texture(ref, prim)

    # ---- sampling ---------------------------------------------------------------
    def _count_wrapped(self, texels, u, v):
        wrap = self.wrap_drawn
        if wrap != (0, 0):
            h, w, _ = texels.shape
            out = (WR.outside(u, w) & (wrap[0] != 0)) | (WR.outside(v, h) & (wrap[1] != 0))
            self.wrapped[0] += int(out.size)
            self.wrapped[1] += int(out.sum())

    def flat(self, texels, uv, filt):
        self._count_wrapped(texels, uv[:, 0], uv[:, 1])
        return wrapped_colours(texels, uv, filt, self.wrap_drawn)

    # ---- modulated soups ----------------------------------------------------------
    def modulated_batch(self, tex, xy, z, uv, rgba, q, colkind, src):
        if not self.triangles or tex.width < 2 or tex.height < 2:
            return
        filt_off = colkind == "gouraud" and self.filt
        filt = 0 if filt_off else self.filt
        self.wrap_drawn = self.wrap
        n = xy.shape[0]
        if self.gpu and filt_off:
            self.ctx.set_triangle_texture_filter(0)
        if not self.gpu:
            texels = self.texels(tex)
            self._count_wrapped(texels, uv[:, 0], uv[:, 1])
            self.ctx.draw_triangles(xy, modulated_colours(texels, uv, rgba, filt, self.wrap), z=z, gouraud=True)
        elif src == "host":
            self.ctx.draw_textured_triangles(tex, xy, uv, z=z, q=q, colors=rgba)
        else:
            txy, tuvc = self._device((xy, self.R.interleave_uv_colors(uv, rgba)), src == "dev8")
            tz, tq = self._device((z, np.ones((n, 3)) if q is None else q), False)
            self.ctx.draw_textured_triangles_device(tex, txy, tuvc, n, z=tz, q=tq, colors=True)
        if self.gpu and filt_off:
            self.ctx.set_triangle_texture_filter(1)
        self._note("modulated", xy)

    # ---- meshes -----------------------------------------------------------------
    def _note_mesh(self, kind, full, xy):
        eid = self._cur
        if eid is not None:
            if eid in self._posed:
                self.posed_between += 1
                self.posed_over_cap += bool(self._posed.pop(eid))
            self._drawn.add(eid)
        before = len(self.batches)
        super()._note_mesh(kind, full, xy)
        if eid in self._touched and len(self.batches) > before:
            self.posed_paths.add(self.batches[-1][1])

    def _draw_texc(self, entry, mat, lit, nseed):
        """A draw of a "tc" / "tl" mesh, unlit (draw_mesh) or lit (draw_mesh_lit)."""
        spec, mesh, gm = entry
        label, M = F.mesh_matrix(spec[1], mat, self.W0, self.H0)
        N = F.normal_matrix(nseed) if lit else None
        tex = self.texture(texc_texref(spec))
        filt_off, persp_off = bool(self.filt), self.persp and label == "perspective"
        self.wrap_drawn = self.wrap
        xy, z, uvc, _ = MD.mesh_soup(mesh, M, lit=lit, N=N, ambient=self.ambient, lights=self.lights,
                                     w_near=self.near, cull=self.cull, persp=False)
        if self.gpu:
            if filt_off:
                self.ctx.set_triangle_texture_filter(0)
            if persp_off:
                self.ctx.set_mesh_perspective(False)
            if lit:
                self.ctx.draw_mesh_lit(gm, M, N, texture=tex)
            else:
                self.ctx.draw_mesh(gm, M, texture=tex)
            if persp_off:
                self.ctx.set_mesh_perspective(True)
            if filt_off:
                self.ctx.set_triangle_texture_filter(1)
        elif xy.shape[0]:
            a = uvc.reshape(-1, 3, 6)
            texels = self.texels(tex)
            self._count_wrapped(texels, a[:, 0, 0], a[:, 0, 1])
            col = modulated_colours(texels, a[:, 0, 0:2], a[:, :, 2:6], 0, self.wrap)
            self.ctx.draw_triangles(xy, col, z=z, gouraud=True)
        self._note_mesh("modulated", mesh["idx"].shape[0], xy)

    def draw_mesh(self, i, mat, texref):
        if not self.meshes or not self.triangles:
            return
        entry = self.meshes[i % len(self.meshes)]
        self._cur = id(entry)
        if entry[0][0] in TEXC:
            self._draw_texc(entry, mat, False, None)
        else:
            super().draw_mesh(i, mat, texref)

    def draw_mesh_lit(self, i, mat, nseed):
        if not self.lit or not self.triangles:
            return
        entry = self.lit[i % len(self.lit)]
        self._cur = id(entry)
        if entry[0][0] == "tl":
            self._draw_texc(entry, mat, True, nseed)
        else:
            super().draw_mesh_lit(i, mat, nseed)

    def draw_mesh_instanced(self, i, K, seed, tint, src):
        if not self.plain or not self.triangles:
            return
        self._cur = id(self.plain[i % len(self.plain)])
        every, self.meshes = self.meshes, self.plain
        try:
            super().draw_mesh_instanced(i, K, seed, tint, src)
        finally:
            self.meshes = every

    def draw_mesh_lit_instanced(self, i, K, seed, tint, src):
        if not self.lit_plain or not self.triangles:
            return
        self._cur = id(self.lit_plain[i % len(self.lit_plain)])
        lit, self.lit = self.lit, self.lit_plain
        try:
            super().draw_mesh_lit_instanced(i, K, seed, tint, src)
        finally:
            self.lit = lit

    def move_mesh(self, entry, seed):
        if entry[0][0] not in TEXC:
            return super().move_mesh(entry, seed)
        entry[1] = moved_texc(entry[0], entry[1], self.W0, self.H0, seed)
        if entry[2] is not None:
            if entry[0][0] == "tl":
                entry[2].update_normals(entry[1]["normals"])
            entry[2].update_positions(entry[1]["pos"])

    # ---- poses --------------------------------------------------------------------
    def pose(self, op):
        k = op[0]
        if k == "morph":
            if not self.morphs:
                return
            _, i, wseed, active, src, where = op
            rig, mo = None, self.morphs[i % len(self.morphs)]
            entry = mo["entry"]
        else:
            if not self.rigs:
                return
            rig = self.rigs[op[1] % len(self.rigs)]
            entry, mo = rig["entry"], None
            if k == "variant":
                if rig["skin"] is not None:
                    rig["skin"].set_variant(op[2])
                return
            if k == "pose":
                _, i, pseed, src, where = op
            else:
                _, i, pseed, wseed, active, src, where = op
                mo = next((m for m in self.morphs if m["entry"] is entry), None)
        spec, mesh, gm = entry
        pal = None if rig is None else palette(spec[1], rig["rig"]["nb"], pseed, self.W0, self.H0)
        w = None if mo is None else MM.scattered_weights(mo["T"], active, wseed)
        if mo is None:
            entry[1] = posed_dict(mesh, self.bind[id(entry)], rig["rig"], rig["normals"], pal)
        elif rig is None:
            entry[1] = MM.morphed(mesh, mo["mo"], w)
        else:
            entry[1] = MM.morph_posed(mesh, mo["mo"], w, rig["rig"], pal)
        if self.gpu:
            ctx = self.ctx if where == "main" else self.aux_ctx()
            args = [a for a in (pal, w) if a is not None]
            if src != "host":
                args = self._device(args, False)
                assert all(t.data_ptr() % 16 == 0 for t in args)
            dev = "" if src == "host" else "_device"
            if mo is None:
                getattr(ctx, "pose_mesh" + dev)(gm, rig["skin"], args[0])
            elif rig is None:
                getattr(ctx, "morph_mesh" + dev)(gm, mo["gmo"], args[0])
            else:
                getattr(ctx, "pose_mesh_morphed" + dev)(gm, rig["skin"], args[0], mo["gmo"], args[1])
        eid = id(entry)
        if eid in self._drawn:
            self._posed[eid] = self._posed.get(eid, False) or self.over_cap
        self._touched[eid] = entry

    def check_poses(self):
        """The arrays the pose kernels left in every posed mesh (GPU side)."""
        for spec, mesh, gm in self._touched.values():
            got = gm.positions()
            assert MS.same_bits(got, mesh["pos"]), ("posed positions", spec, scenes.first_mismatch(got, mesh["pos"]))
            if "normals" in mesh:
                got = gm.normals()
                assert MS.same_bits(got, mesh["normals"]), ("posed normals", spec, scenes.first_mismatch(got, mesh["normals"]))

    # ---- one operation --------------------------------------------------------------
    def set_state(self, k, op):
        before = self.wrap
        super().set_state(k, op)
        self.wrap_over_cap += bool(self.over_cap and self.wrap != before)

    def op(self, op):
        k = op[0]
        self._cur = None
        if k == "mtri":
            _, src, n, seed, spread, colkind, blended, qkind, texref = op
            if colkind == "gouraud" and texref[0] != "pow2":
                texref = ("pow2", seed, 3 + seed % 2)
            tex = self.texture(texref)
            xy, z, uv, rgba, q = modulated_soup(n, self.W0, self.H0, seed, spread, colkind, blended, qkind,
                                                (tex.width, tex.height))
            self.modulated_batch(tex, xy, z, uv, rgba, q, colkind, src)
        elif k in POSE_OPS:
            self.pose(op)
        else:
            super().op(op)
            if k in SYNC_OPS:
                self._drawn.clear()
                self._posed.clear()

    def run(self):
        out = super().run()
        if self.gpu:
            self.check_poses()
        out.update(wrap_over_cap=self.wrap_over_cap, posed_between=self.posed_between,
                   posed_over_cap=self.posed_over_cap, wrapped=tuple(self.wrapped), posed=len(self._touched),
                   posed_paths=self.posed_paths)
        return out


def run(fac, frame, triangles=True):
    """frame_ops.run for the extended vocabulary.  Modulated batches ("mtri",
    "tc" and "tl" meshes) are reported as kind "modulated"; the dict also holds
    wrap_over_cap and posed_over_cap (wrap changes, and poses between two draws
    of their mesh, while a batch of more than 50 tile pairs may be pending),
    posed_between, posed (meshes posed or morphed), posed_paths (the raster
    paths their draws took) and wrapped (constant-UV
    triangles sampled under a non-clamp wrap: all, and those whose (u, v) lies
    outside [0, n-1) on a wrapped axis; oracle side)."""
    return _AnimRun(fac, frame, triangles).run()


mismatches = F.mismatches


# ---------------------------------------------------------------------------
# what a frame holds
# ---------------------------------------------------------------------------
def _lists(meshes):
    """The index lists of the mesh operations: lit ("l", "tl"), plain lit ("l"), not "tc" / "tl"."""
    lit = [i for i, s in enumerate(meshes) if s[0] in ("l", "tl")]
    return lit, [i for i in lit if meshes[i][0] == "l"], [i for i, s in enumerate(meshes) if s[0] not in TEXC]


def mesh_of(frame, op):
    """The index in resources["meshes"] of the mesh an operation draws or poses, or None."""
    res = frame[4]
    meshes = res.get("meshes", [])
    if not meshes:
        return None
    lit, lit_plain, plain = _lists(meshes)
    k = op[0]
    if k in ("mesh", "mesh2"):
        return op[1] % len(meshes)
    if k in ("lmesh", "lmesh2"):
        return lit[op[1] % len(lit)] if lit else None
    if k == "meshi":
        return plain[op[1] % len(plain)] if plain else None
    if k == "lmeshi":
        return lit_plain[op[1] % len(lit_plain)] if lit_plain else None
    if k in ("pose", "posemorph", "variant"):
        rigs = res.get("rigs", [])
        return rigs[op[1] % len(rigs)][0] % len(meshes) if rigs else None
    if k == "morph":
        morphs = res.get("morphs", [])
        return morphs[op[1] % len(morphs)][0] % len(meshes) if morphs else None
    return None


def _old_frame(frame):
    """`frame` in frame_ops' own vocabulary, for its kinds() and state_stats():
    without the new operations and the draws of "tc" / "tl" meshes (which stay
    in the list, as "tu" specs, so that the indices hold), and with the
    instanced and lit draws indexed as frame_ops indexes them."""
    W, H, alpha, knobs, res, ops = frame
    meshes = res.get("meshes", [])
    lit, lit_plain, plain = _lists(meshes)
    out = []
    for op in ops:
        k = op[0]
        if k in ("mtri", "wrap") or k in POSE_OPS:
            continue
        i = mesh_of(frame, op)
        if i is not None and meshes[i][0] in TEXC:
            continue
        if k in ("lmesh", "lmesh2", "lmeshi"):
            if i is None:
                continue
            op = (k, lit_plain.index(i)) + tuple(op[2:])
        elif k == "meshi":
            if i is None:
                continue
            op = (k, i) + tuple(op[2:])
        elif k == "ttri" and op[5] == "tiled":
            op = op[:5] + ("const",) + tuple(op[6:])
        out.append(op)
    old = dict(res, meshes=[("tu",) + tuple(s[1:]) if s[0] in TEXC else s for s in meshes],
               bufs=[s[:4] + ("const",) if s[0] == "t" and s[4] == "tiled" else s for s in res.get("bufs", [])])
    return (W, H, alpha, knobs, old, out)


def _textured_op(frame, op):
    """Whether the operation issues a batch that reads the wrap state."""
    res = frame[4]
    bufs, meshes = res.get("bufs", []), res.get("meshes", [])
    k = op[0]
    if k in ("ttri", "ptri", "mtri"):
        return True
    if k in ("buf", "buf2"):
        return bool(bufs) and bufs[op[1] % len(bufs)][0] == "t"
    i = mesh_of(frame, op)
    return k not in POSE_OPS and i is not None and meshes[i][0] in ("tu", "ts") + TEXC


def kinds(frame):
    """frame_ops.kinds plus the kinds of the new vocabulary (ANIM_KINDS)."""
    res, ops = frame[4], frame[5]
    meshes = res.get("meshes", [])
    out = set(F.kinds(_old_frame(frame)))

    def texref(ref):
        if ref[0] == "pow2":
            out.add("texture:pow2")

    for op in ops:
        k = op[0]
        i = mesh_of(frame, op)
        if k == "wrap":
            out.add("wrap")
        elif k == "ttri":
            texref(op[6])
            if op[5] == "tiled":
                out.add("uv:tiled")
        elif k == "mtri":
            out.update({"mtri", "mtri:" + op[5], "mtri:" + {"host": "host", "dev": "device", "dev8": "device"}[op[1]]})
            if op[6]:
                out.add("mtri:blended")
            if op[7] is not None:
                out.add("mtri:q")
            if op[5] == "gouraud":
                out.add("texture:pow2")
            else:
                texref(op[8])
        elif k in ("buf", "buf2"):
            bufs = res.get("bufs", [])
            if bufs and bufs[op[1] % len(bufs)][0] == "t" and bufs[op[1] % len(bufs)][4] == "tiled":
                out.add("uv:tiled")
                texref(op[2])
        elif k in POSE_OPS and i is not None:
            out.add(k)
            if k != "variant":
                out.update({"pose:" + op[-1], "pose:" + {"host": "host", "dev": "device"}[op[-2]]})
                if meshes[i][0] in ("l", "tl"):
                    out.add("pose:lit")
        elif i is not None and meshes[i][0] in TEXC:
            out.update({"mesh:textured-colour", "texture:pow2"})
            out.add("mesh:textured-colour-lit" if k in ("lmesh", "lmesh2") else "mesh:textured-colour-unlit")
    return out


ANIM_KINDS = ("wrap", "uv:tiled", "texture:pow2", "mtri", "mtri:flat", "mtri:gouraud", "mtri:host", "mtri:device",
              "mtri:blended", "mtri:q", "mesh:textured-colour", "mesh:textured-colour-unlit", "mesh:textured-colour-lit",
              "pose", "morph", "posemorph", "variant", "pose:main", "pose:aux", "pose:host", "pose:device", "pose:lit")
ALL_KINDS = F.ALL_KINDS + ANIM_KINDS


def batch_kinds(frame):
    """frame_ops.batch_kinds with "modulated" for the "mtri" and the draws of "tc" / "tl" meshes."""
    res, ops = frame[4], frame[5]
    bufs, meshes = res.get("bufs", []), res.get("meshes", [])
    epochs, count = [set()], 0
    for op in ops:
        k = op[0]
        i = mesh_of(frame, op)
        twice = 2 if k in ("buf2", "mesh2", "lmesh2") else 1
        if k in ("cleardepth", "resize"):
            epochs.append(set())
        elif k == "tri":
            epochs[-1].add("colour"); count += 1
        elif k in ("ttri", "ptri"):
            epochs[-1].add("textured"); count += 1
        elif k == "mtri":
            epochs[-1].add("modulated"); count += 1
        elif k in ("buf", "buf2") and bufs:
            epochs[-1].add("colour" if bufs[op[1] % len(bufs)][0] == "c" else "textured")
            count += twice
        elif k in POSE_OPS or i is None:
            continue
        elif meshes[i][0] in TEXC:
            epochs[-1].add("modulated"); count += twice
        else:
            epochs[-1].add({"mesh": "mesh", "mesh2": "mesh", "meshi": "instanced"}.get(k, "lit"))
            count += twice
    return epochs, count


def state_stats(frame):
    """frame_ops.state_stats (of the operations it knows) plus
    posed_between   a pose, morph or posemorph of a mesh is issued between two
                    draws of that mesh with no flush, gather or probe between them
    wrap_between    the wrap changes value between two batches that read it,
                    with no flush, gather or probe between them"""
    ops = frame[5]
    out = dict(F.state_stats(_old_frame(frame)))
    drawn, posed, between = set(), set(), False
    wrap, pending, changed, wrap_between = (0, 0), False, False, False
    for op in ops:
        k = op[0]
        i = mesh_of(frame, op)
        if k in SYNC_OPS:
            drawn.clear(); posed.clear()
            pending = changed = False
        elif k == "wrap":
            changed |= pending and (op[1], op[2]) != wrap
            wrap = (op[1], op[2])
        elif k in POSE_OPS:
            if k != "variant" and i in drawn:
                posed.add(i)
        elif i is not None:
            between |= i in posed
            drawn.add(i)
        if _textured_op(frame, op):
            wrap_between |= changed
            pending, changed = True, False
    out.update(posed_between=between, wrap_between=wrap_between)
    return out


# ---------------------------------------------------------------------------
# strategies
# ---------------------------------------------------------------------------
class _AnimGen(F._StateGen):
    """The generator of the anim frames: _StateGen's vocabulary plus the wrap
    state, tiled UVs, pow2 textures, modulated soups, textured colour meshes
    and poses, on a random stream of its own.  An operation may come with
    company (ops returns a list): a pose between two draws of its mesh, a wrap
    change between two textured batches."""

    def resources(self):
        r, lim = self.r, self.lim
        res = super().resources()
        meshes = res["meshes"]
        s = r.choice([0.05, 0.3, 1.0])
        texc = (r.choice(TEXC), r.choice(["screen", "model", "model"]),
                self.count(lim["maxmesh"], 1, 0.45 * max(self.W, self.H) * s), self.seed(), s)
        meshes.insert(r.randrange(len(meshes) + 1), texc)
        res["bufs"] = [b[:4] + ("tiled",) if b[0] == "t" and b[4] == "const" and r.random() < 0.5 else b for b in res["bufs"]]
        self.lit, self.lit_plain, self.plain = _lists(meshes)
        li = r.choice(self.lit)
        rigs = [(li, r.choice(BONE_COUNTS), self.seed(), r.random() < 0.7, r.choice([0, 1, 2]))]
        morphs = [(li, r.choice(TARGET_COUNTS), self.seed(), r.random() < 0.7)]
        for _ in range(r.choice([0, 1, 1, 2])):
            mi = r.randrange(len(meshes))
            if r.random() < 0.5:
                rigs.append((mi, r.choice(BONE_COUNTS), self.seed(), r.random() < 0.7, r.choice([0, 1, 2])))
            else:
                morphs.append((mi, r.choice(TARGET_COUNTS), self.seed(), r.random() < 0.7))
        res["rigs"], res["morphs"] = rigs, morphs
        return res

    def mesh_triangles(self, i):
        spec = self.res["meshes"][i]
        return spec[2] if spec[0] in ("tu",) + TEXC else 2 * spec[2] * spec[3]

    def pow2(self):
        return ("pow2", self.seed(), self.r.choice([3, 4]))

    def texref(self):
        return self.pow2() if self.r.random() < 0.25 else super().texref()

    def draw_of(self, i):
        """A draw of mesh i (an index into resources["meshes"])."""
        r = self.r
        kind = self.res["meshes"][i][0]
        nseed = self.seed() if r.random() < 0.7 else None
        choices = ["mesh"]
        if kind in ("l", "tl"):
            choices += ["lmesh", "lmesh"]
        if kind not in TEXC:
            choices += ["meshi"]
        if kind == "l":
            choices += ["lmeshi"]
        c = r.choice(choices)
        if c == "mesh":
            return ("mesh", i, r.randrange(4), self.texref())
        if c == "lmesh":
            return ("lmesh", self.lit.index(i), r.choice(F._INSTANCE_MATS), nseed)
        tint = r.choice([None, "opaque", "alpha"])
        if c == "meshi":
            return ("meshi", self.plain.index(i), self.instances(i), self.seed(), tint, self.src())
        return ("lmeshi", self.lit_plain.index(i), self.instances(i), self.seed(), tint, self.src())

    def mtri(self):
        r = self.r
        src, spread = self.src(), r.choice(F._SPREADS)
        colkind = r.choice(["flat", "gouraud"])
        return ("mtri", src, self.count(self.lim["maxn"], 1, spread), self.seed(), spread, colkind, r.random() < 0.4,
                r.choice([None, "pow2"]), self.pow2() if colkind == "gouraud" else self.texref())

    def tiled(self):
        r = self.r
        src, spread = self.src(), r.choice(F._SPREADS)
        return ("ttri", src, self.count(self.lim["maxn"], 1, spread), self.seed(), spread, "tiled", self.texref())

    def batch_op(self):
        r = self.r
        kind = r.choice(["base"] * 8 + ["tiled"] * 3 + ["mtri"] * 6 + ["texc"] * 4 + ["mesh"] * 5 + ["lmesh2", "ptri"]
                        + ["again"] * 4 * bool(self.res["bufs"]))
        if kind == "base":
            return F._Gen.batch_op(self)
        if kind == "again":                   # (a buffer drawn twice: with dx 0 the second draw is warm)
            return ("buf2", r.randrange(len(self.res["bufs"])), self.texref(), r.choice([0.0, 0.0, 0.0, 1.5]))
        if kind == "tiled":
            return self.tiled()
        if kind == "mtri":
            return self.mtri()
        if kind == "ptri":
            src, spread = self.src(), r.choice(F._SPREADS)
            return ("ptri", src, self.count(self.lim["maxn"], 1, spread), self.seed(), spread, self.texref())
        if kind == "lmesh2":
            return ("lmesh2", r.randrange(len(self.lit)), r.choice(F._INSTANCE_MATS), self.seed() if r.random() < 0.7 else None,
                    self.seed())
        meshes = self.res["meshes"]
        if kind == "texc":
            return self.draw_of(r.choice([i for i, s in enumerate(meshes) if s[0] in TEXC]))
        return self.draw_of(r.randrange(len(meshes)))

    def textured_op(self):
        r = self.r
        return r.choice([self.tiled, self.tiled, self.mtri, self.mtri,
                         lambda: self.draw_of(r.choice([i for i, s in enumerate(self.res["meshes"]) if s[0] in TEXC]))])()

    def wrap_op(self):
        return ("wrap", self.r.choice([0, 1, 1, 2, 2]), self.r.choice([0, 1, 1, 2, 2]))

    def five_op(self):
        return self.wrap_op() if self.r.random() < 0.3 else super().five_op()

    def pose_op(self):
        """(operation, the mesh it poses)."""
        r, res = self.r, self.res
        kind = r.choice(["pose"] * 4 + ["morph"] * 3 + ["posemorph"] * 4)
        src, where = r.choice(["host", "host", "dev"]), r.choice(["main", "main", "aux"])
        if kind == "morph":
            i = r.randrange(len(res["morphs"]))
            T = res["morphs"][i][1]
            return ("morph", i, self.seed(), r.choice([0, 1, T, T, None]), src, where), res["morphs"][i][0]
        i = 0 if kind == "posemorph" else r.randrange(len(res["rigs"]))     # (rig 0's mesh has a morph)
        if kind == "pose":
            return ("pose", i, self.seed(), src, where), res["rigs"][i][0]
        T = res["morphs"][0][1]
        return ("posemorph", i, self.seed(), self.seed(), r.choice([1, T, T, None]), src, where), res["rigs"][i][0]

    def ops(self, late=False):
        r = self.r
        x = r.random()
        if x < 0.24:
            return [self.batch_op()]
        if x < 0.33:
            return [self.prim_op()]
        if x < 0.44:
            return [self.state_op(late)]
        if x < 0.66:
            return [self.five_op()]
        if x < 0.83:
            if r.random() < 0.15:
                return [("variant", r.randrange(len(self.res["rigs"])), r.choice([0, 1, 2]))]
            op, i = self.pose_op()
            return [self.draw_of(i), op, self.draw_of(i)] if r.random() < 0.5 else [op]
        if x < 0.89:
            return [self.textured_op(), self.wrap_op(), self.textured_op()]
        return [self.other_op()]


def make_small_anim_frame(seed, salt, alpha, fmt, keep):
    r = F._rng(seed, f"anim/{salt}", alpha, fmt)
    W, H = F._even(fmt, F._size(r, 1, 140)), F._even(fmt, F._size(r, 1, 110))
    g = _AnimGen(r, W, H, F.SMALL)
    knobs, res = g.knobs(fmt), g.resources()
    planned = r.choice(F._STATE_NOPS)
    ops = []
    while len(ops) < min(keep, planned):
        ops.extend(g.ops(late=len(ops) >= planned // 2))
    ops = ops[:min(keep, planned)]
    ops = [("resize", F._even(fmt, op[1]), F._even(fmt, op[2])) if op[0] == "resize" else op for op in ops]
    return (W, H, alpha, knobs, res, ops)


def make_large_anim_frame(seed, salt, alpha, fmt, keep):
    r = F._rng(seed, f"anim/{salt}", alpha, fmt)
    W, H = F._even(fmt, F._size(r, 64, 700)), F._even(fmt, F._size(r, 32, 420))
    g = _AnimGen(r, W, H, F.LARGE)
    knobs, res = g.knobs(fmt), g.resources()
    ops = []
    for _ in range(min(keep, r.randint(1, 4))):
        for _ in range(r.randint(0, 3)):
            ops.append(g.five_op())
        if r.random() < 0.5:
            op, i = g.pose_op()
            ops.extend([g.draw_of(i), op, g.draw_of(i)] if r.random() < 0.5 else [op])
        ops.append(g.batch_op())
        if r.random() < 0.5:
            ops.append(r.choice([g.prim_op, g.state_op, g.other_op])())
    return (W, H, alpha, knobs, res, ops)


def small_anim_frames():
    """small_state_frames' sizes and budgets with the extended vocabulary."""
    return st.builds(make_small_anim_frame, F._stable_seed, F._stable_seed, st.booleans(), F._fmt, F._state_keep)


def large_anim_frames():
    """large_state_frames' sizes and budget with the extended vocabulary."""
    return st.builds(make_large_anim_frame, F._stable_seed, F._stable_seed, st.booleans(), F._fmt, F._state_keep)


def for_each_frame(size, visit):
    """frame_ops.for_each_frame, and the "small-anim" and "large-anim" examples
    (the same settings, derandomized; their seeds are _stable_seed's, so they
    are the same examples in every process)."""
    if not size.endswith("-anim"):
        return F.for_each_frame(size, visit)
    strategy, n = {"small-anim": (small_anim_frames(), F.SMALL_EXAMPLES),
                   "large-anim": (large_anim_frames(), F.LARGE_EXAMPLES)}[size]

    @settings(max_examples=n, deadline=None, derandomize=True, database=None,
              suppress_health_check=list(HealthCheck))
    @given(strategy)
    def examples(fr):
        visit(fr)

    examples()

"""Turning the C3 sphere under three directional lights: what lighting on the
device costs beside the unlit mesh draw, and beside the only way to light a
turning mesh without it, in one session on one GPU:

  a  tools/bench_mesh.py's line a: the C3 geometry (501 x 1001 vertices, 1M
     triangles, Gouraud, depth write, 3840x2160) as a Mesh under a new rotation
     matrix every frame, vertex colours fixed
  b  the same mesh with its analytic normals, DrawMeshLit under a new matrix and
     the matching normal matrix every frame: one more pass over the vertices
     (the light pass) and an assembly that also gathers the lit colours
  c  the host alternative: numpy lighting of the vertex colours (the reference's
     expressions) and the mesh created again with them, every frame, then a

Each line is wall-clock ms per frame (host clock around frames that end in a
flush) after a clock settle and warmup; a, b and c alternate over --rounds
rounds and the median round is reported with the spread.  The passes of a and b
are then timed by the library's kernel timing (HIP events around each launch, so
each figure includes the launch gap) and set against their bytes at 6.3 TB/s:
the light pass reads 24 + 32 B and writes 32 B per vertex (88 B against the
vertex stage's 48 B); b's assembly writes 96 B of attributes per triangle that
a's does not (a hands the mesh's own expanded attributes to the raster by
pointer) and reads the colour table through the indices.

The last timed frame of a 1/16-size version of b (960x540, 126 x 251 vertices)
is verified against the oracle's DrawTriangles of the numpy reference's lit soup
(tests/mesh_light_ref.py).  Prints one JSON line per configuration and writes
them all to --out.

    python tools/bench_mesh_lit.py --steps 50 --warmup 5 --out profiles/mesh_light/bench_mesh_lit.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_mesh as BM   # noqa: E402  (the model, the matrices and the timing loop of line a)

HBM_TBS = BM.HBM_TBS
AMBIENT = (0.15, 0.12, 0.2)
LIGHTS = np.array([[0.6, 0.64, -0.48, 1.6, 1.3, 1.0], [-0.8, 0.0, 0.6, 0.2, 0.5, 0.9], [0.0, -1.0, 0.0, 0.3, 0.3, 0.1]])


def lit_model(H, rows, cols):
    """bench_mesh.model with the sphere's analytic unit normals (its colours are normal * 0.5 + 0.5)."""
    mesh, R = BM.model(H, rows, cols)
    mesh["normals"] = np.ascontiguousarray((mesh["colors"][:, :3] - 0.5) * 2.0)
    return mesh, R


def normal_matrix(frame):
    """The rotation of bench_mesh.matrix(frame) alone: rx @ ry, row-major 3x3."""
    a, b = np.radians(1.0 + frame), np.radians(0.5 * frame)
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    ry = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
    rx = np.array([[1, 0, 0], [0, cb, -sb], [0, sb, cb]])
    return np.ascontiguousarray((rx @ ry).reshape(9))


class ConfigB:
    name = "b: lit Mesh, a new matrix and normal matrix every frame (light pass + lit assembly on the device)"

    def __init__(self, R, W, H, rows, cols):
        self.W, self.H = W, H
        self.mesh, self.radius = lit_model(H, rows, cols)
        self.ctx = R.RenderContext(W, H, False)
        self.ctx.set_mesh_lights(AMBIENT, LIGHTS)
        self.gm = R.Mesh(self.mesh["pos"], self.mesh["idx"], colors=self.mesh["colors"], gouraud=True,
                         normals=self.mesh["normals"])
        self.mats = [BM.matrix(W, H, self.radius, i) for i in range(360)]
        self.nmats = [normal_matrix(i) for i in range(360)]

    def frame(self, i):
        BM.begin(self.ctx)
        self.ctx.draw_mesh_lit(self.gm, self.mats[i % 360], self.nmats[i % 360])
        self.ctx.gather_frame_u8()


class ConfigC:
    name = "c: numpy lighting of the vertex colours on the host + the mesh created again, every frame, then DrawMesh"

    def __init__(self, R, W, H, rows, cols):
        self.R, self.W, self.H = R, W, H
        self.mesh, self.radius = lit_model(H, rows, cols)
        self.ctx = R.RenderContext(W, H, False)
        self.gm = None

    def frame(self, i):
        import mesh_light_ref as ML
        col = ML.lit_colors(self.mesh, normal_matrix(i), AMBIENT, LIGHTS)
        self.gm = self.R.Mesh(self.mesh["pos"], self.mesh["idx"], colors=col, gouraud=True)
        BM.begin(self.ctx)
        self.ctx.draw_mesh(self.gm, BM.matrix(self.W, self.H, self.radius, i))
        self.ctx.gather_frame_u8()


def kernel_times(cfg, steps, names):
    ctx = cfg.ctx
    for i in range(3):
        cfg.frame(i)
    ctx.flush()
    ctx.reset_kernel_timing()
    ctx.set_kernel_timing_filter(",".join(names))
    ctx.enable_kernel_timing(True)
    for i in range(steps):
        cfg.frame(i)
    ctx.flush()
    ctx.enable_kernel_timing(False)
    out = {}
    for name in names:
        tot, cnt = ctx.get_kernel_timing(name)
        if not cnt:
            raise SystemExit(f"bench_mesh_lit: no launch of '{name}' was timed")
        out[name] = round(tot / cnt * 1e3, 2)
    ctx.reset_kernel_timing()
    ctx.set_kernel_timing_filter("")
    return out


def verify(R, steps):
    """The last of `steps` frames of a 1/16-size version of b against the
    oracle's DrawTriangles of the reference's lit soup."""
    import mesh_light_ref as ML
    import scenes
    W, H = 960, 540
    small = ConfigB(R, W, H, 125, 250)
    for i in range(steps):
        small.frame(i)
    got = small.ctx.get_buffer_numpy(), small.ctx.get_depth_buffer()
    k = (steps - 1) % 360
    xy, z, c = ML.lit_soup(small.mesh, small.mats[k], small.nmats[k], AMBIENT, LIGHTS)
    octx = scenes.OracleFactory().context(W, H, False)
    BM.begin(octx)
    octx.draw_triangles(xy, c, z=z, gouraud=True)
    ok = scenes.bits_equal(got[0], octx.get_buffer_numpy()) and np.array_equal(got[1], octx.get_depth_buffer())
    return bool(ok and small.ctx.last_raster_path() == "order-free")


def us_at_hbm(nbytes):
    return round(nbytes / (HBM_TBS * 1e12) * 1e6, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    if R.device_count() <= 0:
        raise SystemExit("bench_mesh_lit: no HIP device")
    R.set_device(0)
    W, H, rows, cols = 3840, 2160, 500, 1000
    only = args.only.split(",")
    cfgs = {k: cls(R, W, H, rows, cols) for k, cls in (("a", BM.ConfigA), ("b", ConfigB), ("c", ConfigC)) if k in only}
    steps = {"a": args.steps, "b": args.steps, "c": max(3, args.steps // 10)}   # (c: tens of ms per frame)
    rounds = {k: [] for k in cfgs}
    for r in range(args.rounds):          # alternating: a, b, c, a, b, c, ...
        for k, cfg in cfgs.items():
            rounds[k].append(BM.run_timed(cfg, steps[k], args.warmup if k != "c" else 1))
    nv, n = (rows + 1) * (cols + 1), 2 * rows * cols
    results = {}
    for k, cfg in cfgs.items():
        results[k] = dict(config=cfg.name, W=W, H=H, triangles=n, vertices=nv, steps=steps[k],
                          ms_per_frame=round(statistics.median(rounds[k]), 4),
                          ms_per_frame_rounds=[round(v, 4) for v in rounds[k]],
                          raster_path=cfg.ctx.last_raster_path())
    if "a" in cfgs:
        results["a"]["kernels_us_event_timed"] = kernel_times(cfgs["a"], args.steps, ("mesh_vertex", "mesh_assemble"))
    if "b" in cfgs:
        kt = kernel_times(cfgs["b"], args.steps, ("mesh_vertex", "mesh_light", "mesh_assemble"))
        light_bytes, vertex_bytes = 88 * nv, 48 * nv
        results["b"].update(
            kernels_us_event_timed=kt,
            light_bytes=light_bytes, light_bound_us=us_at_hbm(light_bytes),
            light_over_bound=round(kt["mesh_light"] / us_at_hbm(light_bytes), 2),
            vertex_bytes=vertex_bytes, vertex_bound_us=us_at_hbm(vertex_bytes),
            light_over_vertex=round(kt["mesh_light"] / kt["mesh_vertex"], 2), byte_ratio=round(88 / 48, 2),
            lit_attr_bytes_written=96 * n)
        if not args.no_verify:
            results["b"]["verified"] = verify(R, args.steps)
            results["b"]["verify_note"] = ("the last timed frame of the 1/16-size scene (960x540, 62 500 triangles) "
                                           "against the oracle's frame of the reference's lit soup")
    for k in results:
        print(json.dumps(results[k]), flush=True)
    if "a" in results and "b" in results:
        ka, kb = results["a"]["kernels_us_event_timed"], results["b"]["kernels_us_event_timed"]
        results["b_minus_a_ms"] = round(results["b"]["ms_per_frame"] - results["a"]["ms_per_frame"], 4)
        results["b_minus_a_split_us"] = dict(light_pass=kb["mesh_light"],
                                             lit_attribute_gather=round(kb["mesh_assemble"] - ka["mesh_assemble"], 2))
    if "b" in results and "c" in results:
        results["c_over_b"] = round(results["c"]["ms_per_frame"] / results["b"]["ms_per_frame"], 2)
    print(json.dumps({k: v for k, v in results.items() if k not in cfgs}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

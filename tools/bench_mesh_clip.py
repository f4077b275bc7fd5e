"""The mesh clip stage on the turning C3 sphere (tools/bench_mesh.py's config a:
501 x 1001 vertices, 1M triangles, Gouraud, depth write, 3840x2160, a new
matrix every frame), in one session on one GPU:

  a   state off: the vertex stage and the assembly, as before the stage existed
  b   a near plane in front of everything (the matrix is affine, cw == 1, the
      plane at 0.5): nothing is clipped, n_out == n -- the cost of the stage
      itself (four passes instead of two, and the wait for the count)
  c1  cull mode 1 (drops area2 > 0)      c2  cull mode 2 (drops area2 < 0)
      about half of the closed mesh is dropped before binning; one of the two
      drops the faces that show
  d   the eye inside the sphere (a perspective matrix, the near plane at 0.05 of
      the radius): triangles behind the plane dropped, those across it cut

Each line is wall-clock ms per frame (host clock around frames that end in a
flush) after a clock settle and warmup; the configurations alternate over
--rounds rounds and the median round is reported with the spread.  The clip
kernels of b and d are then timed by the library's kernel timing (HIP events
around each launch: each figure includes the launch gap).

The last timed frame of a 1/16-size version of c1, c2 and d (960x540) is
verified against the oracle's DrawTriangles of the numpy reference's clipped
soup (tests/mesh_clip_ref.py), count included.

--root DIR loads the package from another tree (a build of another commit, for
an A/B of config a: `--only a --no-verify --root DIR`).

    python tools/bench_mesh_clip.py --steps 50 --warmup 5 --out profiles/mesh_clip/bench_mesh_clip.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CLIP_KERNELS = ("mesh_clip_vertex", "mesh_clip_count", "mesh_clip_scan", "mesh_clip_emit")


def inside_matrix(W, H, R, frame):
    """Frame `frame`'s eye-inside matrix: the eye 0.45 R in front of the
    sphere's centre, looking at it, the model turning as in bench_mesh.matrix;
    cw = the view-space depth in pixels, z from 0.05 at cw = 0.05 R to 0.95 at
    1.7 R (mesh_ref.behind_eye at this scale)."""
    a, b = np.radians(1.0 + frame), np.radians(0.5 * frame)
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    ry = np.array([[ca, 0, sa, 0], [0, 1, 0, 0], [-sa, 0, ca, 0], [0, 0, 0, 1.0]])
    rx = np.array([[1, 0, 0, 0], [0, cb, -sb, 0], [0, sb, cb, 0], [0, 0, 0, 1.0]])
    view = rx @ ry
    view[2, 3] = 0.45 * R
    near, far = 0.05 * R, 1.7 * R
    zb = (0.95 - 0.05) / (1 / far - 1 / near)
    za = 0.05 - zb / near
    s = 0.5 * H * 0.6
    proj = np.array([[s, 0, W / 2, 0], [0, -s, H / 2, 0], [0, 0, za, zb], [0, 0, 1.0, 0]])
    return np.ascontiguousarray((proj @ view).reshape(16))


def make_config(BM, R, key, W, H, rows, cols):
    """bench_mesh.ConfigA under the clip state of configuration `key`."""
    cfg = BM.ConfigA(R, W, H, rows, cols)
    cfg.near, cfg.cull = {"a": (0.0, 0), "b": (0.5, 0), "c1": (0.0, 1), "c2": (0.0, 2),
                          "d": (0.05 * cfg.radius, 0)}[key]
    cfg.name = {"a": "a: state off (vertex stage + assembly)",
                "b": "b: near plane in front of everything (cw == 1, plane 0.5): the cost of the stage",
                "c1": "c1: cull mode 1 (drops area2 > 0)", "c2": "c2: cull mode 2 (drops area2 < 0)",
                "d": "d: the eye inside the sphere, near plane at 0.05 R"}[key]
    if key == "d":
        cfg.mats = [inside_matrix(W, H, cfg.radius, i) for i in range(360)]
    if key != "a":   # (a also runs on a build without the state calls)
        cfg.ctx.set_mesh_near_plane(cfg.near)
        cfg.ctx.set_mesh_cull(cfg.cull)
    return cfg


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
            raise SystemExit(f"bench_mesh_clip: no launch of '{name}' was timed")
        out[name] = round(tot / cnt * 1e3, 2)
    ctx.reset_kernel_timing()
    ctx.set_kernel_timing_filter("")
    return out


def verify(BM, R, key, steps):
    """The last of `steps` frames of a 1/16-size version of `key` against the
    oracle's DrawTriangles of the reference's clipped soup."""
    import mesh_clip_ref as CR
    import scenes
    W, H = 960, 540
    small = make_config(BM, R, key, W, H, 125, 250)
    for i in range(steps):
        small.frame(i)
    got = small.ctx.get_buffer_numpy(), small.ctx.get_depth_buffer()
    xy, z, c, counts = CR.clip_soup(small.mesh, small.mats[(steps - 1) % 360], small.near, small.cull)
    octx = scenes.OracleFactory().context(W, H, False)
    BM.begin(octx)
    octx.draw_triangles(xy, c, z=z, gouraud=True)
    ok = scenes.bits_equal(got[0], octx.get_buffer_numpy()) and np.array_equal(got[1], octx.get_depth_buffer())
    return bool(ok and small.ctx.mesh_last_triangle_count == counts.sum()
                and small.ctx.last_raster_path() == "order-free")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="a,b,c1,c2,d")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--root", default=ROOT, help="tree whose libnativecpurenderer_amd package is loaded")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import bench_mesh as BM
    sys.path.insert(0, os.path.abspath(args.root))   # (after bench_mesh, which puts its own tree first)
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    if R.device_count() <= 0:
        raise SystemExit("bench_mesh_clip: no HIP device")
    R.set_device(0)
    W, H, rows, cols = 3840, 2160, 500, 1000
    only = args.only.split(",")
    cfgs = {k: make_config(BM, R, k, W, H, rows, cols) for k in ("a", "b", "c1", "c2", "d") if k in only}
    rounds = {k: [] for k in cfgs}
    for r in range(args.rounds):          # alternating: a, b, c1, c2, d, a, ...
        for k, cfg in cfgs.items():
            rounds[k].append(BM.run_timed(cfg, args.steps, args.warmup))
    results = {}
    for k, cfg in cfgs.items():
        results[k] = dict(config=cfg.name, W=W, H=H, triangles=2 * rows * cols, vertices=(rows + 1) * (cols + 1),
                          near=cfg.near, cull=cfg.cull, steps=args.steps,
                          ms_per_frame=round(statistics.median(rounds[k]), 4),
                          ms_per_frame_rounds=[round(v, 4) for v in rounds[k]],
                          raster_path=cfg.ctx.last_raster_path())
        if k != "a":
            results[k]["triangles_out_last_frame"] = cfg.ctx.mesh_last_triangle_count
            results[k]["kernels_us_event_timed"] = kernel_times(cfg, args.steps, CLIP_KERNELS)
            if not args.no_verify and k != "b":
                results[k]["verified"] = verify(BM, R, k, args.steps)
        else:
            results[k]["kernels_us_event_timed"] = kernel_times(cfg, args.steps, ("mesh_vertex", "mesh_assemble"))
    if not args.no_verify and any(k in results for k in ("c1", "c2", "d")):
        results["verify_note"] = ("the last timed frame of the 1/16-size scene (960x540, 62 500 triangles) against the "
                                  "oracle's frame of the reference's clipped soup, the count included")
    for k in results:
        print(json.dumps({k: results[k]}), flush=True)
    if "a" in results:
        for k in ("b", "c1", "c2"):
            if k in results:
                results[f"{k}_minus_a_ms"] = round(results[k]["ms_per_frame"] - results["a"]["ms_per_frame"], 4)
    print(json.dumps({k: v for k, v in results.items() if not isinstance(v, dict)}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""Turning the C3 sphere: an indexed Mesh drawn under a new 3D rotation every
frame, against the raster's floor and against the only way to turn a model
without the mesh front end, in one session on one GPU:

  a  the C3 geometry (501 x 1001 vertices, 1M triangles, Gouraud, depth write,
     3840x2160) as a Mesh under a new rotation matrix every frame: the vertex
     stage and the assembly run on the device, then the soup is binned cold
  b  the same geometry as a TriangleBuffer under a new 2D transform every frame
     (bench.py's c3_animated frame): the raster's floor
  c  the model turned on the host: numpy rotation + projection of the vertices,
     expansion through the indices, DrawTriangles of the 168 MB soup

Each line is wall-clock ms per frame (host clock around frames that end in a
flush) after a clock settle and warmup; a, b and c alternate over --rounds
rounds and the median round is reported with the spread.  a's two kernels are
then timed by the library's kernel timing (HIP events around each launch, so
each figure includes the launch gap; a rocprofv3 kernel trace gives the bare
spans) and set against their bytes: 24 nv + 12 n read, 72 n + 24 nv written.

The last timed frame of a 1/16-size version of a (960x540, 126 x 251 vertices)
is verified against the oracle's DrawTriangles of the numpy reference's soup
(tests/mesh_ref.py).  Prints one JSON line per configuration and writes them
all to --out.

    python tools/bench_mesh.py --steps 50 --warmup 5 --out profiles/mesh/bench_mesh.json
    python tools/bench_mesh.py --only a --no-verify --rounds 1      (for a profiler run)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BG = (0.0, 0.0, 0.0, 0.0)
CLOCK_SETTLE_MS = 250.0
HBM_TBS = 6.3   # achievable HBM rate the kernels' bytes are set against


def model(H, rows, cols, R_frac=0.45):
    """scenes.sphere_mesh's sphere in model space (pixels, y up, centred)."""
    import mesh_ref as MR
    R = R_frac * H
    th = np.linspace(0, np.pi, rows + 1)
    ph = np.linspace(0, 2 * np.pi, cols + 1)
    T, P = np.meshgrid(th, ph, indexing="ij")
    r = R * (1 + 0.15 * np.sin(5 * T) * np.sin(7 * P))
    pos = np.stack([r * np.sin(T) * np.cos(P), r * np.cos(T), r * np.sin(T) * np.sin(P)], -1).reshape(-1, 3)
    n = np.stack([np.sin(T) * np.cos(P), np.cos(T), np.sin(T) * np.sin(P)], -1).reshape(-1, 3)
    col = np.concatenate([n * 0.5 + 0.5, np.ones((n.shape[0], 1))], axis=1)
    return dict(pos=np.ascontiguousarray(pos), idx=MR.grid_indices(rows, cols), colors=np.ascontiguousarray(col),
                gouraud=True), R


def matrix(W, H, R, frame):
    """Frame `frame`'s matrix: one degree more about the y axis and half a
    degree about x per frame, orthographic as C3, viewport baked in (last row
    (0, 0, 0, 1): nothing is divided)."""
    a, b = np.radians(1.0 + frame), np.radians(0.5 * frame)
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    ry = np.array([[ca, 0, sa, 0], [0, 1, 0, 0], [-sa, 0, ca, 0], [0, 0, 0, 1.0]])
    rx = np.array([[1, 0, 0, 0], [0, cb, -sb, 0], [0, sb, cb, 0], [0, 0, 0, 1.0]])
    vp = np.array([[1, 0, 0, W / 2], [0, -1, 0, H / 2], [0, 0, 1 / (2.4 * R * 1.2), 0.5], [0, 0, 0, 1.0]])
    M = vp @ rx @ ry
    M[3] = (0.0, 0.0, 0.0, 1.0)
    return np.ascontiguousarray(M.reshape(16))


def begin(ctx):
    ctx.set_color(*BG)
    ctx.set_depth_state(True, True)
    ctx.clear_depth()


class ConfigA:
    name = "a: Mesh, a new 3D rotation matrix every frame (vertex stage + assembly on the device, cold binning)"

    def __init__(self, R, W, H, rows, cols):
        self.W, self.H = W, H
        self.mesh, self.radius = model(H, rows, cols)
        self.ctx = R.RenderContext(W, H, False)
        self.gm = R.Mesh(self.mesh["pos"], self.mesh["idx"], colors=self.mesh["colors"], gouraud=True)
        self.mats = [matrix(W, H, self.radius, i) for i in range(360)]

    def frame(self, i):
        begin(self.ctx)
        self.ctx.draw_mesh(self.gm, self.mats[i % 360])
        self.ctx.gather_frame_u8()


class ConfigB:
    name = "b: TriangleBuffer, a new 2D transform every frame (bench.py's c3_animated frame: the raster's floor)"

    def __init__(self, R, W, H, rows, cols):
        import mesh_ref as MR
        mesh, radius = model(H, rows, cols)
        xy, z, c = MR.expand(mesh, matrix(W, H, radius, 0))
        self.ctx = R.RenderContext(W, H, False)
        self.buf = R.TriangleBuffer(xy, c, z=z, gouraud=True)

    def frame(self, i):
        ctx = self.ctx
        begin(ctx)
        ctx.save_state()
        ctx.translate(0.005 + 0.01 * (i % 100), 0.0)
        ctx.draw_triangle_buffer(self.buf)
        ctx.restore_state()
        ctx.gather_frame_u8()


class ConfigC:
    name = "c: numpy rotation + projection on the host, DrawTriangles of the expanded soup (168 MB per frame)"

    def __init__(self, R, W, H, rows, cols):
        self.W, self.H = W, H
        self.mesh, self.radius = model(H, rows, cols)
        self.idx = self.mesh["idx"].astype(np.int64)
        self.col = np.ascontiguousarray(self.mesh["colors"][self.idx].reshape(-1, 12))
        self.ctx = R.RenderContext(W, H, False)

    def frame(self, i):
        M = matrix(self.W, self.H, self.radius, i).reshape(4, 4)
        p = self.mesh["pos"] @ M[:3, :3].T + M[:3, 3]
        tri = p[self.idx]                                  # (n, 3, 3)
        begin(self.ctx)
        self.ctx.draw_triangles(np.ascontiguousarray(tri[..., :2]).reshape(-1, 6), self.col,
                                z=np.ascontiguousarray(tri[..., 2]), gouraud=True)
        self.ctx.gather_frame_u8()


def run_timed(cfg, steps, warmup, first=0):
    """ms per frame of `steps` frames after a clock settle and `warmup` frames."""
    ctx = cfg.ctx
    ctx.flush()
    t0, k = time.perf_counter(), 0
    while (time.perf_counter() - t0) * 1e3 < CLOCK_SETTLE_MS:
        cfg.frame(k)
        k += 1
        ctx.flush()
    for i in range(warmup):
        cfg.frame(i)
    ctx.flush()
    t0 = time.perf_counter()
    for i in range(steps):
        cfg.frame(first + i)
    ctx.flush()
    return (time.perf_counter() - t0) * 1e3 / steps


def kernel_times(cfg, steps):
    ctx = cfg.ctx
    names = ("mesh_vertex", "mesh_assemble")
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
            raise SystemExit(f"bench_mesh: no launch of '{name}' was timed")
        out[name] = round(tot / cnt * 1e3, 2)
    ctx.reset_kernel_timing()
    ctx.set_kernel_timing_filter("")
    return out


def verify(R, steps):
    """The last of `steps` frames of a 1/16-size version of a against the
    oracle's DrawTriangles of the reference's soup."""
    import mesh_ref as MR
    import scenes
    W, H = 960, 540
    small = ConfigA(R, W, H, 125, 250)
    for i in range(steps):
        small.frame(i)
    got = small.ctx.get_buffer_numpy(), small.ctx.get_depth_buffer()
    xy, z, c = MR.expand(small.mesh, small.mats[(steps - 1) % 360])
    octx = scenes.OracleFactory().context(W, H, False)
    begin(octx)
    octx.draw_triangles(xy, c, z=z, gouraud=True)
    ok = scenes.bits_equal(got[0], octx.get_buffer_numpy()) and np.array_equal(got[1], octx.get_depth_buffer())
    return bool(ok and small.ctx.last_raster_path() == "order-free")


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
        raise SystemExit("bench_mesh: no HIP device")
    R.set_device(0)
    W, H, rows, cols = 3840, 2160, 500, 1000
    only = args.only.split(",")
    cfgs = {k: cls(R, W, H, rows, cols) for k, cls in (("a", ConfigA), ("b", ConfigB), ("c", ConfigC)) if k in only}
    steps = {"a": args.steps, "b": args.steps, "c": max(3, args.steps // 10)}   # (c: tens of ms per frame)
    rounds = {k: [] for k in cfgs}
    for r in range(args.rounds):          # alternating: a, b, c, a, b, c, ...
        for k, cfg in cfgs.items():
            rounds[k].append(run_timed(cfg, steps[k], args.warmup if k != "c" else 1))
    results = {}
    for k, cfg in cfgs.items():
        results[k] = dict(config=cfg.name, W=W, H=H, triangles=2 * rows * cols, vertices=(rows + 1) * (cols + 1),
                          steps=steps[k], ms_per_frame=round(statistics.median(rounds[k]), 4),
                          ms_per_frame_rounds=[round(v, 4) for v in rounds[k]],
                          raster_path=cfg.ctx.last_raster_path())
    if "a" in cfgs:
        nv, n = (rows + 1) * (cols + 1), 2 * rows * cols
        kt = kernel_times(cfgs["a"], args.steps)
        by = 24 * nv + 12 * n + 72 * n + 24 * nv
        results["a"].update(kernels_us_event_timed=kt, mesh_bytes=by,
                            mesh_bytes_bound_us=round(by / (HBM_TBS * 1e12) * 1e6, 2),
                            mesh_kernels_over_bound=round(sum(kt.values()) / (by / (HBM_TBS * 1e12) * 1e6), 2))
        if not args.no_verify:
            results["a"]["verified"] = verify(R, args.steps)
            results["a"]["verify_note"] = ("the last timed frame of the 1/16-size scene (960x540, 62 500 triangles) "
                                           "against the oracle's frame of the reference's soup")
    for k in results:
        print(json.dumps(results[k]), flush=True)
    if "a" in results and "c" in results:
        results["c_over_a"] = round(results["c"]["ms_per_frame"] / results["a"]["ms_per_frame"], 2)
    if "a" in results and "b" in results:
        results["a_minus_b_ms"] = round(results["a"]["ms_per_frame"] - results["b"]["ms_per_frame"], 4)
    print(json.dumps({k: v for k, v in results.items() if not isinstance(v, dict)}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

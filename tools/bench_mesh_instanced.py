"""Instanced mesh draws against the K single draws they stand for and against
the floor of one pre-merged mesh, in one session on one GPU, at 3840x2160 with
Gouraud colours and depth write:

Shape S, many tiny instances: a 16 x 32 sphere (561 vertices, 1024 triangles)
under new matrices every frame.
  a  one draw_mesh_instanced of K instances            (K = 64 and K = 1024)
  b  the same frame as K draw_mesh calls               (K = 64 and K = 1024)
  c  the 1024 instances pre-merged into one Mesh (574 464 vertices, 1 048 576
     triangles), one draw_mesh under a single new matrix every frame: the floor
     an instanced draw can approach -- not an equivalent frame, its instances
     cannot move independently
Shape L, few large instances: 4 instances of the C3 sphere (501 x 1001
vertices, 1M triangles) at half the linear size, one per screen quadrant.
  La one draw_mesh_instanced, K = 4        Lb four draw_mesh calls

Each line is wall-clock ms per frame (host clock around frames that end in a
flush) after a clock settle and warmup; the lines alternate over --rounds
rounds and the median round is reported with every round beside it.  The new
kernels of the a lines (and, for comparison, the single-mesh kernels of the b
lines) are then timed by the library's kernel timing -- HIP events around each
launch, so every figure includes the launch gap -- and set against their
bytes, counted twice: `unique` (every array once: positions, K matrices and
the 24 K nv vertex table for the vertex stage; indices, the table, the mesh's
attributes, the 72 K n of positions and depths and the 96 K n attribute copy
the single-mesh path does not pay for the assembly) and `issued` (the mesh's
positions, indices and attributes once per instance, as the K instances read
them: what reaches HBM when the mesh is larger than the caches, as at shape L).

The last timed frame of a 1/16-size version of a (960x540, K = 64) is verified
against the oracle's frame of the numpy reference's soup
(tests/mesh_inst_ref.py).  Prints one JSON line per configuration and writes
them all to --out.

    python tools/bench_mesh_instanced.py --out profiles/mesh_instanced/bench.json
    python tools/bench_mesh_instanced.py --only a1024 --no-verify --rounds 1      (for a profiler run)
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
HBM_TBS = 6.3    # achievable HBM rate the kernels' bytes are set against
FRAMES = 48      # distinct frames of matrices, formed before the clock starts


def small_sphere():
    """mesh_ref.sphere3d's displaced unit sphere at 16 x 32 with opaque normal colours."""
    import mesh_ref as MR
    mesh = MR.sphere3d(rows=16, cols=32)
    n = mesh["pos"] / np.linalg.norm(mesh["pos"], axis=1, keepdims=True)
    mesh["colors"] = np.ascontiguousarray(np.concatenate([n * 0.5 + 0.5, np.ones((n.shape[0], 1))], axis=1))
    return mesh


def placements(W, H, K, frames, radius_px, seed=3):
    """(frames, K, 16): instance k sits in cell k of a grid over the screen,
    turns a little more every frame and drifts inside its cell; orthographic,
    viewport baked in, last row (0, 0, 0, 1)."""
    g = np.random.default_rng(seed)
    cols = int(np.ceil(np.sqrt(K * W / H)))
    rows = int(np.ceil(K / cols))
    k = np.arange(K)
    cx, cy = (k % cols + 0.5) * W / cols, (k // cols + 0.5) * H / rows
    phase, size = g.uniform(0, 2 * np.pi, K), g.uniform(0.6, 1.0, K) * radius_px
    depth = g.uniform(0.2, 0.8, K)
    out = np.zeros((frames, K, 4, 4))
    for f in range(frames):
        a, b = phase + np.radians(3.0 * f), 0.5 * phase + np.radians(1.5 * f)
        ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
        # rx(b) @ ry(a), scaled; y down on the screen
        r = np.empty((K, 3, 3))
        r[:, 0] = np.stack([ca, np.zeros(K), sa], -1)
        r[:, 1] = np.stack([sb * sa, cb, -sb * ca], -1)
        r[:, 2] = np.stack([-cb * sa, sb, cb * ca], -1)
        out[f, :, 0, :3] = r[:, 0] * size[:, None]
        out[f, :, 1, :3] = -r[:, 1] * size[:, None]
        out[f, :, 2, :3] = r[:, 2] * (0.15 / 1.2)
        out[f, :, 0, 3] = cx + 0.3 * radius_px * np.sin(a)
        out[f, :, 1, 3] = cy + 0.3 * radius_px * np.cos(b)
        out[f, :, 2, 3] = depth
        out[f, :, 3, 3] = 1.0
    return np.ascontiguousarray(out.reshape(frames, K, 16))


def begin(ctx):
    ctx.set_color(*BG)
    ctx.set_depth_state(True, True)
    ctx.clear_depth()


class Instanced:
    def __init__(self, R, W, H, mesh, mats, what):
        self.name = f"a: one draw_mesh_instanced, K = {mats.shape[1]} ({what})"
        self.mesh, self.mats, self.K = mesh, mats, mats.shape[1]
        self.ctx = R.RenderContext(W, H, False)
        self.gm = R.Mesh(mesh["pos"], mesh["idx"], colors=mesh["colors"], gouraud=True)
        self.kernels = ("mesh_inst_vertex", "mesh_inst_assemble")

    def frame(self, i):
        begin(self.ctx)
        self.ctx.draw_mesh_instanced(self.gm, self.mats[i % self.mats.shape[0]])
        self.ctx.gather_frame_u8()


class Singles(Instanced):
    def __init__(self, R, W, H, mesh, mats, what):
        super().__init__(R, W, H, mesh, mats, what)
        self.name = f"b: the same frame as {self.K} draw_mesh calls ({what})"
        self.kernels = ("mesh_vertex", "mesh_assemble")

    def frame(self, i):
        begin(self.ctx)
        for M in self.mats[i % self.mats.shape[0]]:
            self.ctx.draw_mesh(self.gm, M)
        self.ctx.gather_frame_u8()


class Merged:
    name = "c: the 1024 instances pre-merged into one Mesh, one draw_mesh under a single new matrix every frame"

    def __init__(self, R, W, H, mesh, mats):
        K, nv = mats.shape[1], mesh["pos"].shape[0]
        M = mats[0].reshape(K, 4, 4)
        pos = np.einsum("kij,vj->kvi", M[:, :3, :3], mesh["pos"]) + M[:, None, :3, 3]
        idx = (mesh["idx"][None].astype(np.int64) + (np.arange(K) * nv)[:, None, None]).reshape(-1, 3)
        self.K = 1
        self.ctx = R.RenderContext(W, H, False)
        self.gm = R.Mesh(pos.reshape(-1, 3), idx.astype(np.uint32), colors=np.tile(mesh["colors"], (K, 1)), gouraud=True)
        self.kernels = ("mesh_vertex", "mesh_assemble")

    def frame(self, i):
        M = np.eye(4)
        M[0, 3] = 0.005 + 0.01 * (i % 100)
        begin(self.ctx)
        self.ctx.draw_mesh(self.gm, M)
        self.ctx.gather_frame_u8()


def run_timed(cfg, steps, warmup):
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
        cfg.frame(i)
    ctx.flush()
    return (time.perf_counter() - t0) * 1e3 / steps


def kernel_times(cfg, steps):
    """us per launch of cfg's mesh kernels (HIP events around each launch)."""
    ctx = cfg.ctx
    cfg.frame(0)
    ctx.flush()
    ctx.reset_kernel_timing()
    ctx.set_kernel_timing_filter(",".join(cfg.kernels))
    ctx.enable_kernel_timing(True)
    for i in range(steps):
        cfg.frame(i)
    ctx.flush()
    ctx.enable_kernel_timing(False)
    out = {}
    for name in cfg.kernels:
        tot, cnt = ctx.get_kernel_timing(name)
        if not cnt:
            raise SystemExit(f"bench_mesh_instanced: no launch of '{name}' was timed")
        out[name] = round(tot / cnt * 1e3, 2)
    ctx.reset_kernel_timing()
    ctx.set_kernel_timing_filter("")
    return out


def instanced_bytes(nv, n, K):
    """Bytes of the two kernels of an instanced Gouraud draw: every array once, and as issued (the mesh's own
    arrays read once per instance)."""
    out = {}
    for name, per in (("unique", 1), ("issued", K)):
        vertex = 24 * nv * per + 128 * K + 24 * K * nv
        assemble = (12 * n + 96 * n) * per + 24 * K * nv + 72 * K * n + 96 * K * n
        out[name] = dict(mesh_inst_vertex=vertex, mesh_inst_assemble=assemble)
    out["attribute_copy"] = 96 * n + 96 * K * n
    return out


def verify(R, steps):
    """The last of `steps` frames of a 1/16-size version of a (960x540, K = 64)
    against the oracle's DrawTriangles of the reference's soup."""
    import mesh_inst_ref as MI
    import scenes
    W, H = 960, 540
    mesh = small_sphere()
    small = Instanced(R, W, H, mesh, placements(W, H, 64, FRAMES, 45.0), "1/16 size")
    for i in range(steps):
        small.frame(i)
    got = small.ctx.get_buffer_numpy(), small.ctx.get_depth_buffer()
    xy, z, c, _ = MI.instanced_soup(mesh, small.mats[(steps - 1) % FRAMES])
    octx = scenes.OracleFactory().context(W, H, False)
    begin(octx)
    octx.draw_triangles(xy, c, z=z, gouraud=True)
    ok = scenes.bits_equal(got[0], octx.get_buffer_numpy()) and np.array_equal(got[1], octx.get_depth_buffer())
    return bool(ok and small.ctx.last_raster_path() == "order-free")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="a64,b64,a1024,b1024,c,La,Lb")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    import bench_mesh
    if R.device_count() <= 0:
        raise SystemExit("bench_mesh_instanced: no HIP device")
    R.set_device(0)
    W, H = 3840, 2160
    only = args.only.split(",")
    cfgs, steps = {}, {}
    if any(k in only for k in ("a64", "b64", "a1024", "b1024", "c")):
        mesh = small_sphere()
        mats = placements(W, H, 1024, FRAMES, 45.0)
        shape = "shape S: 1024 triangles an instance"
        for k, cls, K, st in (("a64", Instanced, 64, args.steps), ("b64", Singles, 64, args.steps),
                              ("a1024", Instanced, 1024, args.steps), ("b1024", Singles, 1024, max(3, args.steps // 10))):
            if k in only:
                # (K = 64: every 16th cell, so that the 64 instances spread over the screen as the 1024 do)
                cfgs[k], steps[k] = cls(R, W, H, mesh, np.ascontiguousarray(mats[:, ::1024 // K]), shape), st
        if "c" in only:
            cfgs["c"], steps["c"] = Merged(R, W, H, mesh, mats), args.steps
    if "La" in only or "Lb" in only:
        big, radius = bench_mesh.model(H, 500, 1000)
        lm = np.stack([np.stack([bench_mesh.matrix(W, H, radius, f + 40 * q).reshape(4, 4) for q in range(4)])
                       for f in range(FRAMES)])
        half = np.diag([0.5, 0.5, 1.0, 1.0])
        for q in range(4):   # half the linear size, centred in quadrant q
            lm[:, q] = half @ lm[:, q]
            lm[:, q, 0, 3] = W * (0.25 + 0.5 * (q % 2))
            lm[:, q, 1, 3] = H * (0.25 + 0.5 * (q // 2))
        lm = np.ascontiguousarray(lm.reshape(FRAMES, 4, 16))
        shape = "shape L: 1M triangles an instance"
        for k, cls in (("La", Instanced), ("Lb", Singles)):
            if k in only:
                cfgs[k], steps[k] = cls(R, W, H, big, lm, shape), max(3, args.steps // 3)
    rounds = {k: [] for k in cfgs}
    for r in range(args.rounds):          # alternating: a64, b64, a1024, ...
        for k, cfg in cfgs.items():
            rounds[k].append(run_timed(cfg, steps[k], args.warmup if steps[k] >= 10 else 1))
    results = {}
    for k, cfg in cfgs.items():
        nv, n = (cfg.gm.vertex_count, cfg.gm.triangle_count)
        results[k] = dict(config=cfg.name, W=W, H=H, instances=cfg.K, triangles=cfg.K * n, vertices=cfg.K * nv,
                          steps=steps[k], ms_per_frame=round(statistics.median(rounds[k]), 4),
                          ms_per_frame_rounds=[round(v, 4) for v in rounds[k]], raster_path=cfg.ctx.last_raster_path(),
                          kernels_us_event_timed=kernel_times(cfg, min(steps[k], 10)))
        if isinstance(cfg, Instanced) and not isinstance(cfg, Singles):
            by = instanced_bytes(nv, n, cfg.K)
            kt = results[k]["kernels_us_event_timed"]
            us = lambda b: b / (HBM_TBS * 1e12) * 1e6
            results[k].update(kernel_bytes=by, kernel_bytes_bound_us={
                kind: {name: round(us(by[kind][name]), 2) for name in cfg.kernels} for kind in ("unique", "issued")},
                kernels_over_bound={kind: round(sum(kt.values()) / us(sum(by[kind].values())), 2)
                                    for kind in ("unique", "issued")})
        else:
            results[k]["kernel_launches_per_frame"] = cfg.K
    if "a1024" in results and not args.no_verify:
        results["a1024"]["verified"] = verify(R, args.steps)
        results["a1024"]["verify_note"] = ("the last timed frame of the 1/16-size scene (960x540, K = 64, 65 536 "
                                           "triangles) against the oracle's frame of the reference's soup")
    for k in results:
        print(json.dumps(results[k]), flush=True)
    summary = {}
    for a, b, name in (("a64", "b64", "b_over_a_K64"), ("a1024", "b1024", "b_over_a_K1024"), ("La", "Lb", "b_over_a_L"),
                       ("c", "a1024", "a_over_c_K1024")):
        if a in results and b in results:
            summary[name] = round(results[b]["ms_per_frame"] / results[a]["ms_per_frame"], 2)
            if name.startswith("b_over_a"):
                summary[name + "_every_round"] = bool(all(x < y for x, y in zip(rounds[a], rounds[b])))
    results.update(summary)
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

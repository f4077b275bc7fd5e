"""Morph targets on the device: what the two morph kernels cost, alone and beside
their baselines, in one session on one GPU.

The small workload is skin_bench's: a UV sphere of 224 x 448 = 100 352 vertices
(199 362 triangles, Gouraud, depth write, 1920x1080) under a rig of 64 bones, here
with T = 32 morph targets; the large one is a sphere of 708 x 1416 = 1 002 528
vertices, where the launch gap no longer dominates.

  kernel   `mesh_morph` at A = 0, 1, 4, 16 active targets of 32, on both spheres:
           us per launch from the library's kernel timing (HIP events around each
           launch, so every figure includes the launch gap), A cycling inside a
           round and all rounds listed, against the time its bytes take at
           bench_mesh.HBM_TBS: 24 * (2 + A) bytes per vertex.
  fused    on the small sphere, alternating in one process: `mesh_skin` (pose_mesh),
           `mesh_morph_skin` at A = 0, `mesh_morph` at A = 4, `mesh_morph_skin` at
           A = 4; the ratios fused(0) / skin and fused(4) / (morph(4) + skin).
  frame    wall-clock ms per frame (host clock around frames that end in a flush)
           of a: update_positions with the morphed-and-posed vertices precomputed
           in numpy, then draw_mesh, and b: pose_mesh_morphed, then draw_mesh;
           alternating rounds; the last frames are compared bit for bit.

--lib PATH loads another build of the library (an A/B of a kernel variant runs the
`kernel` section once per build, in processes of their own, alternating).
Prints one JSON line per result and writes them all to --out.

    python tools/morph_bench.py --steps 200 --warmup 20 --out profiles/morph/morph_bench.json
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_mesh as BM   # noqa: E402  (the sphere, the clears and the timing loop)
import skin_bench as SB   # noqa: E402  (the rig and the palettes)

HBM_TBS = BM.HBM_TBS
W, H, NB, POSES, T = SB.W, SB.H, SB.NB, SB.POSES, 32
SMALL, LARGE = (223, 447), (707, 1415)
ACTIVE = (0, 1, 4, 16)


def weights(active, frame=0):
    """(T,): `active` non-zero weights on targets spread over 0 .. T-1, their values moving with the frame."""
    w = np.zeros(T)
    for k, t in enumerate(np.linspace(0, T - 1, active).round().astype(int) if active else ()):
        w[t] = 0.3 + 0.25 * np.sin(0.17 * frame + 0.9 * k)
    return w


def deltas(nv, radius, seed=5):
    return np.random.default_rng(seed).uniform(-0.02 * radius, 0.02 * radius, size=(T, nv, 3))


def timed_us(ctx, name, steps, call):
    """us per launch of the kernel `name` over `steps` calls of `call(i)` (event-timed)."""
    for i in range(5):
        call(i)
    ctx.flush()
    ctx.reset_kernel_timing()
    ctx.set_kernel_timing_filter(name)
    ctx.enable_kernel_timing(True)
    for i in range(steps):
        call(i)
    ctx.flush()
    ctx.enable_kernel_timing(False)
    tot, cnt = ctx.get_kernel_timing(name)
    if cnt != steps:
        raise SystemExit(f"morph_bench: {cnt} launches of {name} were timed, not {steps}")
    ctx.reset_kernel_timing()
    ctx.set_kernel_timing_filter("")
    return round(tot / cnt * 1e3, 3)


def spread(v):
    return round(max(v) - min(v), 3)


def kernel_section(R, shape, steps, rounds):
    mesh, radius = BM.model(H, *shape)
    nv = mesh["pos"].shape[0]
    ctx = R.RenderContext(64, 64, False)
    gm = R.Mesh(mesh["pos"], mesh["idx"], colors=mesh["colors"], gouraud=True)
    morph = R.MeshMorph(mesh["pos"], deltas(nv, radius))
    runs = {a: [] for a in ACTIVE}
    for _ in range(rounds):
        for a in ACTIVE:
            w = weights(a)
            runs[a].append(timed_us(ctx, "mesh_morph", steps, lambda i: ctx.morph_mesh(gm, morph, w)))
    out = dict(vertices=nv, targets=T, steps=steps)
    for a in ACTIVE:
        nbytes = 24 * (2 + a) * nv
        bound = nbytes / (HBM_TBS * 1e12) * 1e6
        med = statistics.median(runs[a])
        out[f"A{a}"] = dict(us=runs[a], median_us=med, spread_us=spread(runs[a]), bytes_per_launch=nbytes,
                            bound_us=round(bound, 3), bound_over_median=round(bound / med, 3))
    return out


class Rig:
    """The small sphere under skin_bench's coherent rig and T morph targets, on one context."""

    def __init__(self, R):
        self.mesh, self.radius = BM.model(H, *SMALL)
        self.joints, self.weights = SB.rig(self.mesh, self.radius, "coherent")
        nv = self.mesh["pos"].shape[0]
        self.dP = deltas(nv, self.radius)
        self.ctx = R.RenderContext(W, H, False)
        self.gm = R.Mesh(self.mesh["pos"], self.mesh["idx"], colors=self.mesh["colors"], gouraud=True)
        self.skin = R.MeshSkin(self.mesh["pos"], self.joints, self.weights, NB)
        self.morph = R.MeshMorph(self.mesh["pos"], self.dP)
        self.M = BM.matrix(W, H, self.radius, 20)
        self.pals = [SB.palette(i, self.radius) for i in range(POSES)]
        self.ws = [weights(4, i) for i in range(POSES)]


class Route:
    def __init__(self, rig, route):
        import mesh_morph_ref as MM
        import mesh_skin_ref as MS
        self.rig, self.route, self.ctx = rig, route, rig.ctx
        if route == "a":
            self.name = "a: update_positions with a precomputed numpy morph and pose, then draw_mesh"
            self.frames = [MS.pose(MM.morph(rig.mesh["pos"], None, rig.dP, None, rig.ws[i])[0], None, rig.joints,
                                   rig.weights, rig.pals[i])[0] for i in range(POSES)]
        else:
            self.name = "b: pose_mesh_morphed with the frame's palette and weights, then draw_mesh"

    def frame(self, i):
        r = self.rig
        BM.begin(r.ctx)
        if self.route == "a":
            r.gm.update_positions(self.frames[i % POSES])
        else:
            r.ctx.pose_mesh_morphed(r.gm, r.skin, r.pals[i % POSES], r.morph, r.ws[i % POSES])
        r.ctx.draw_mesh(r.gm, r.M)


def fused_section(rig, steps, rounds):
    ctx, gm, skin, morph = rig.ctx, rig.gm, rig.skin, rig.morph
    w0, w4, pal = weights(0), weights(4), rig.pals[3]
    calls = {
        "skin": ("mesh_skin", lambda i: ctx.pose_mesh(gm, skin, pal)),
        "fused_A0": ("mesh_morph_skin", lambda i: ctx.pose_mesh_morphed(gm, skin, pal, morph, w0)),
        "morph_A4": ("mesh_morph", lambda i: ctx.morph_mesh(gm, morph, w4)),
        "fused_A4": ("mesh_morph_skin", lambda i: ctx.pose_mesh_morphed(gm, skin, pal, morph, w4)),
    }
    runs = {k: [] for k in calls}
    for _ in range(rounds):
        for k, (name, call) in calls.items():
            runs[k].append(timed_us(ctx, name, steps, call))
    med = {k: statistics.median(v) for k, v in runs.items()}
    return dict(us=runs, median_us=med, spread_us={k: spread(v) for k, v in runs.items()},
                fused_A0_over_skin=round(med["fused_A0"] / med["skin"], 3),
                fused_A4_over_morph_plus_skin=round(med["fused_A4"] / (med["morph_A4"] + med["skin"]), 3),
                note="us per launch from HIP events around each launch (includes the launch gap); 64 bones, "
                     "skin_bench's coherent rig, positions only")


def frame_section(rig, steps, warmup, rounds):
    import scenes
    routes = {"a": Route(rig, "a"), "b": Route(rig, "b")}
    times = {k: [] for k in routes}
    for _ in range(rounds):                                 # alternating: a, b, a, b, ...
        for k, r in routes.items():
            times[k].append(BM.run_timed(r, steps, warmup))
    out = {k: dict(config=r.name, ms_per_frame=round(statistics.median(times[k]), 4),
                   ms_per_frame_rounds=[round(v, 4) for v in times[k]]) for k, r in routes.items()}
    out["a_over_b"] = round(out["a"]["ms_per_frame"] / out["b"]["ms_per_frame"], 2)
    frames = {}
    for k, r in routes.items():                             # the same pose index on both routes
        r.frame(steps - 1)
        frames[k] = (rig.ctx.get_buffer_numpy(), rig.ctx.get_depth_buffer())
    out["b_frame_equals_a_frame"] = bool(scenes.bits_equal(frames["a"][0], frames["b"][0])
                                         and np.array_equal(frames["a"][1], frames["b"][1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sections", default="kernel,fused,frame")
    ap.add_argument("--sizes", default="small,large")
    ap.add_argument("--lib", default="", help="another build of the library (a kernel variant's A/B)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from libnativecpurenderer_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    if R.device_count() <= 0:
        raise SystemExit("morph_bench: no HIP device")
    R.set_device(0)
    sections = args.sections.split(",")
    results = dict(lib=args.lib or "in-tree", hbm_tbs=HBM_TBS)
    if "kernel" in sections:
        for size in args.sizes.split(","):
            results[f"kernel_{size}"] = kernel_section(R, SMALL if size == "small" else LARGE, args.steps, args.rounds)
            print(json.dumps({f"kernel_{size}": results[f"kernel_{size}"]}), flush=True)
    if "fused" in sections or "frame" in sections:
        rig = Rig(R)
        if "fused" in sections:
            results["fused"] = fused_section(rig, args.steps, args.rounds)
            print(json.dumps({"fused": results["fused"]}), flush=True)
        if "frame" in sections:
            results["frame"] = frame_section(rig, args.steps, args.warmup, args.rounds)
            print(json.dumps({"frame": results["frame"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    t0 = time.perf_counter()
    main()
    print(f"morph_bench: {time.perf_counter() - t0:.1f} s", flush=True)

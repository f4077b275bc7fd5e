"""Deferred stores against a caller who draws over the static layer every frame:
the C3 scene (bench.py's: the 1M-triangle sphere at 3840x2160, Gouraud, LESS +
write, YUV420P frame output), where a frame is bench.py's frame -- clear colour,
clear depth, DrawTriangleBuffer -- plus, with --rect, one small draw_rect after
the buffer draw, then the frame output gathered.  The rectangle needs the
framebuffer, so a deferred frame pays a resolve: the case the adaptive rule
(csrc/nr_defer_policy.h) exists for.

Two libraries cannot share a process, so each measurement is a child process
(--child) that loads one library -- this commit's, or with --parent-lib the
parent's, built into a directory of its own (it has no SetDeferredStores: its
only behaviour is to store) -- and prints the ms per frame and the deferral
counts.  A child first settles as bench.py does, in drained groups of four
frames until the draw is shaded from its key index, so the timed frames are all
steady ones.  The driver alternates new / parent within each pair, the order
swapping from pair to pair.

    python tools/bench_defer.py --rect --mode 0 --parent-lib PATH/libNativeCPURenderer.so --pairs 5
    python tools/bench_defer.py --rect --mode 1 --pairs 3          (a resolve per frame: what the rule avoids)
    python tools/bench_defer.py --mode 2 --parent-lib PATH/... --pairs 5   (the plain frame, deferral off)
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NEW_ENTRY_POINTS = ("SetDeferredStores", "GetDeferredStoreCounts")
W, H, MESH = 3840, 2160, (500, 1000)


def child(args):
    from libnativecpurenderer_amd import _abi, _lib
    if os.environ.get("NR_LIB"):   # (tools only: the parent's build instead of the shipped library)
        _lib.LIB_PATH = os.path.abspath(os.environ["NR_LIB"])
        probe = ctypes.CDLL(_lib.LIB_PATH)
        for name in NEW_ENTRY_POINTS:
            if not hasattr(probe, name):
                _abi.HIP_LIBRARY_ABI.pop(name, None)
    import scenes
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    if R.device_count() <= 0:
        raise SystemExit("bench_defer: no HIP device")
    R.set_device(0)
    has = "SetDeferredStores" in _abi.HIP_LIBRARY_ABI
    xy, z, c = scenes.sphere_mesh(W, H, *MESH)
    ctx = R.RenderContext(W, H, False)
    buf = R.TriangleBuffer(xy, c, z=z, gouraud=True)
    ctx.set_frame_format("yuv420p")
    if has:
        ctx.set_deferred_stores(args.mode)

    def frame():
        ctx.set_color(0, 0, 0, 0)
        ctx.set_depth_state(True, True)
        ctx.clear_depth()
        ctx.draw_triangle_buffer(buf)
        if args.rect:
            ctx.draw_rect(100.0, 80.0, 64.0, 48.0, 0.9, 0.2, 0.1, 1.0)
        ctx.gather_frame_u8()

    # settle as bench.py does: drained groups of four frames, so that the host sees each stage of the schedule
    # generation complete (binned, marked, pruned, captured) and the timed frames are all steady ones
    for _ in range(64):
        for _ in range(4):
            frame()
        ctx.flush()
        if ctx.key_indexed_batch_count() >= 8:
            break
    for _ in range(args.warmup):
        frame()
    ctx.flush()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        frame()
    ctx.flush()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    out = {"ms": ms, "indexed": ctx.key_indexed_batch_count()}
    if has:
        out["counts"] = ctx.deferred_store_counts()
    print("AB_RESULT " + json.dumps(out), flush=True)


def run_child(args, lib):
    env = dict(os.environ)
    env.pop("NR_LIB", None)
    if lib:
        env["NR_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--mode", str(args.mode)] + (["--rect"] if args.rect else [])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit(f"bench_defer: a child failed ({p.returncode}); no further run\n{p.stdout}\n{p.stderr}")
    for line in p.stdout.splitlines():
        if line.startswith("AB_RESULT "):
            return json.loads(line[len("AB_RESULT "):])
    raise SystemExit("bench_defer: a child printed no result\n" + p.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--mode", type=int, default=0, choices=(0, 1, 2))
    ap.add_argument("--rect", action="store_true", help="one small draw_rect after the buffer draw")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        return child(args)
    plib = os.path.abspath(args.parent_lib) if args.parent_lib else ""
    if plib and not os.path.exists(plib):
        raise SystemExit("bench_defer: --parent-lib must name the parent commit's library")
    runs = {"new": [], "parent": []}
    for i in range(args.pairs):
        order = [("new", "")] + ([("parent", plib)] if plib else [])
        if i % 2:
            order.reverse()
        for key, lib in order:
            runs[key].append(run_child(args, lib))
    res = dict(scene=f"C3 frame{' + draw_rect' if args.rect else ''}, yuv420p frame output gathered; ms per frame, "
                     "one process per run", mode=args.mode, steps=args.steps, warmup=args.warmup, runs=runs)
    for key, v in runs.items():
        if v:
            ms = [r["ms"] for r in v]
            res[key] = dict(ms=[round(m, 4) for m in ms], median=round(statistics.median(ms), 4),
                            spread=round(max(ms) / min(ms) - 1, 4))
    if runs["parent"]:
        res["median_new_over_parent"] = round(res["new"]["median"] / res["parent"]["median"], 4)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

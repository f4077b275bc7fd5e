"""The default wrap state against the parent commit's library: tools/bench_filter.py's
scene (the turning C3 sphere, 1M triangles, 1024x1024 RGB texture, 3840x2160,
SetMeshPerspective on) under wrap (0, 0), filter off and on, this commit's
library and the parent's alternating in one session.

Two libraries cannot share a process, so each measurement is a child process
(--child) that loads one library -- this commit's, or with NR_LIB the parent's,
built into a directory of its own -- and prints the ms per frame of both filter
states.  The driver runs, per pair index, a new / parent pair and a parent /
parent pair -- the same number of both kinds, in one session -- with the order
within the pairs and the order of the two pairs alternating from index to index.
The check: the median new / parent frame ratio may not exceed the largest
parent / parent pair ratio -- the machine's own repeat spread, measured.

    python tools/ab_wrap_parent.py --parent-lib PATH/libNativeCPURenderer.so --pairs 5 \
        --out profiles/wrap/ab_parent.json
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRY_POINTS = ("SetTriangleTextureWrap", "GetTriangleTextureWrap")


def child(args):
    from libnativecpurenderer_amd import _abi, _lib
    if os.environ.get("NR_LIB"):   # (tools only: the parent's build instead of the shipped library)
        _lib.LIB_PATH = os.path.abspath(os.environ["NR_LIB"])
        probe = ctypes.CDLL(_lib.LIB_PATH)
        for name in NEW_ENTRY_POINTS:   # (the parent's library has no wrap state: its only state is the default)
            if not hasattr(probe, name):
                _abi.HIP_LIBRARY_ABI.pop(name, None)
    import bench_filter as BF
    import bench_mesh as BM
    import bench_persp as BP
    import scenes
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    if R.device_count() <= 0:
        raise SystemExit("ab_wrap_parent: no HIP device")
    R.set_device(0)
    tex = scenes.rng(79).uniform(0, 1, size=(BP.TEX, BP.TEX, 3))
    out = {}
    for filt in (0, 1):
        cfg = BF.config(R, BM, 3840, 2160, 500, 1000, tex, True, filt)
        if "SetTriangleTextureWrap" in _abi.HIP_LIBRARY_ABI:
            cfg.ctx.set_triangle_texture_wrap(0, 0)
        out[f"filter{filt}"] = BM.run_timed(cfg, args.steps, args.warmup)
        del cfg
    print("AB_RESULT " + json.dumps(out), flush=True)


def run_child(args, lib):
    env = dict(os.environ)
    env.pop("NR_LIB", None)
    if lib:
        env["NR_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps), "--warmup",
                        str(args.warmup)], env=env, capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit(f"ab_wrap_parent: a child failed ({p.returncode}); no further run\n{p.stdout}\n{p.stderr}")
    for line in p.stdout.splitlines():
        if line.startswith("AB_RESULT "):
            return json.loads(line[len("AB_RESULT "):])
    raise SystemExit("ab_wrap_parent: a child printed no result\n" + p.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit("ab_wrap_parent: --parent-lib must name the parent commit's library")
    plib = os.path.abspath(args.parent_lib)
    runs = {"new": [], "parent": [], "parent_a": [], "parent_b": []}
    for i in range(args.pairs):
        # the order within the pairs alternates (new, parent / parent, new; a, b / b, a) and so does which kind of
        # pair comes first: a run's place in the session -- clocks, thermal state -- is not tied to its library
        np_pair = [("new", ""), ("parent", plib)]
        pp_pair = [("parent_a", plib), ("parent_b", plib)]
        if i % 2:
            np_pair.reverse()
            pp_pair.reverse()
        order = np_pair + pp_pair if (i // 2) % 2 == 0 else pp_pair + np_pair
        for key, lib in order:
            runs[key].append(run_child(args, lib))
    res = dict(scene="tools/bench_filter.py's scene, mesh perspective on, wrap (0, 0); ms per frame, one process per run",
               steps=args.steps, pairs=args.pairs, runs=runs, filters={})
    ok = True
    for f in ("filter0", "filter1"):
        np_ratio = [a[f] / b[f] for a, b in zip(runs["new"], runs["parent"])]
        pp_ratio = [a[f] / b[f] for a, b in zip(runs["parent_a"], runs["parent_b"])]
        passed = statistics.median(np_ratio) <= max(pp_ratio)
        ok = ok and passed
        res["filters"][f] = dict(new_over_parent_pairs=[round(r, 4) for r in np_ratio],
                                 parent_over_parent_pairs=[round(r, 4) for r in pp_ratio],
                                 median_new_over_parent=round(statistics.median(np_ratio), 4),
                                 largest_parent_over_parent=round(max(pp_ratio), 4),
                                 median_ms=dict(new=round(statistics.median(r[f] for r in runs["new"]), 4),
                                                parent=round(statistics.median(r[f] for r in runs["parent"]), 4)),
                                 passed=passed)
    res["passed"] = ok
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

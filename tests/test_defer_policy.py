"""The rule of deferred stores (csrc/nr_defer_policy.h) on the CPU: a small
stand-alone program, compiled with the host C++ compiler from the header alone,
plays callers against nrdefer::Policy the way the host code does -- before each
cached frame it asks allows(); the frame's record then ends needed (deferred or
not, as the frame was) or superseded -- and prints, per pattern, the decision of
every frame, the resolves (needed records of deferred frames), the threshold
and the run counter at the end.

The expected lines below are worked out from the rule, not from a run: a frame
defers when the run of superseded records before it has reached the threshold
(2 at first); a needed record resets the run, and doubles the threshold (cap
1024) when its frame had deferred.

  always superseded   frames 1, 2 store (runs 0, 1), every later one defers.
  always needed       the run never leaves 0.
  every 2nd needed    the run never passes 1.
  every 3rd needed    frame 3 sees a run of 2 and defers; it is needed: one
                      resolve, threshold 4, which a run of 2 never reaches.
  every 10th needed   cycle 1 defers frames 3..10 (threshold 2), cycle 2 frames
                      5..10 (4), cycle 3 frames 9, 10 (8); each cycle's 10th is
                      needed: 3 resolves, threshold 16 > 9: none afterwards.
  burst then run      5 needed frames (nothing deferred, threshold stays 2), 40
                      superseded: the first two store, 38 defer; then 3 needed
                      -- the first had deferred: one resolve, threshold 4 --
                      then 10 superseded: four store, six defer.
  cap                 resolve after resolve, each as soon as the rule allows
                      again: 2, 4, ... 1024 and no further.

The same program built with -fsanitize=address,undefined and run on its own is
the sanitizer run of this header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libnativecpurenderer_amd", "csrc")

PROGRAM = r"""
#include "nr_defer_policy.h"

#include <cstdio>
#include <string>

using nrdefer::Policy;

struct Caller {
    Policy p;
    std::string decisions;
    int resolves = 0;
    void frame(bool needed) {
        const bool defer = p.allows();
        decisions += defer ? '1' : '0';
        if (needed) {
            p.needed(defer);
            if (defer) ++resolves;
        } else {
            p.superseded();
        }
    }
    void print(const char* name) const {
        std::printf("%s decisions=%s resolves=%d threshold=%u run=%u\n", name, decisions.c_str(), resolves, p.threshold,
                    p.run);
    }
};

int main() {
    {
        Caller c;
        for (int i = 1; i <= 8; ++i) c.frame(false);
        c.print("superseded");
    }
    {
        Caller c;
        for (int i = 1; i <= 8; ++i) c.frame(true);
        c.print("needed");
    }
    for (int N : {2, 3, 10}) {
        Caller c;
        for (int i = 1; i <= (N == 10 ? 50 : 12); ++i) c.frame(i % N == 0);
        c.print(N == 2 ? "every2" : N == 3 ? "every3" : "every10");
    }
    {
        Caller c;
        for (int i = 0; i < 5; ++i) c.frame(true);
        for (int i = 0; i < 40; ++i) c.frame(false);
        for (int i = 0; i < 3; ++i) c.frame(true);
        for (int i = 0; i < 10; ++i) c.frame(false);
        c.print("burst");
    }
    {
        Caller c;
        std::string thresholds;
        for (int round = 0; round < 12; ++round) {
            while (!c.p.allows()) c.frame(false);
            c.frame(true);
            thresholds += std::to_string(c.p.threshold) + ",";
        }
        std::printf("cap thresholds=%s resolves=%d\n", thresholds.c_str(), c.resolves);
    }
    return 0;
}
"""

EXPECTED = [
    "superseded decisions=00111111 resolves=0 threshold=2 run=8",
    "needed decisions=00000000 resolves=0 threshold=2 run=0",
    "every2 decisions=000000000000 resolves=0 threshold=2 run=0",
    "every3 decisions=001000000000 resolves=1 threshold=4 run=0",
    "every10 decisions=" + "0011111111" + "0000111111" + "0000000011" + "0000000000" * 2 + " resolves=3 threshold=16 run=0",
    "burst decisions=" + "00000" + "00" + "1" * 38 + "100" + "0000111111" + " resolves=1 threshold=4 run=10",
    "cap thresholds=4,8,16,32,64,128,256,512,1024,1024,1024,1024, resolves=12",
]


def test_the_rule_on_every_caller_pattern(tmp_path):
    cxx = os.environ.get("CXX") or "g++"          # the C++ driver of the compiler oracle/Makefile builds with
    if shutil.which(cxx) is None:
        pytest.fail(f"no host C++ compiler ({cxx})")
    src, exe = tmp_path / "defer_policy.cpp", tmp_path / "defer_policy"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == EXPECTED

"""The staging carve of the mesh front end (csrc/nr_mesh_stage.h) on the CPU: a
small stand-alone program, compiled with the host C++ compiler from the header
alone, walks the layout functions nr_mesh.hip itself calls -- every combination
of their flags, a superset of the layouts in use (unclipped plain with and
without q, lit colour, textured colour lit and unlit, the instanced forms, the
clipped soup with and without the lit tail) -- over small, odd and
more-than-one-block sizes, and checks that every region starts at an even
offset (16-byte alignment), that the regions are disjoint and in order, and
that a layout is at most one double per region larger than its contents."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libnativecpurenderer_amd", "csrc")

PROGRAM = r"""
#include "nr_mesh_stage.h"

#include <algorithm>
#include <cstdio>
#include <vector>

using namespace nrmesh;

static long checked = 0, failed = 0;

static void bad(const char* what, const char* layout, const StageNeeds& d, size_t nout) {
    if (failed++ < 20)
        std::printf("FAIL %s: %s NV=%zu N=%zu nout=%zu persp=%d lit=%d unitQ=%d ownAttr=%d stride=%zu\n", what, layout,
                    d.NV, d.N, nout, d.persp, d.lit, d.unitQ, d.ownAttr, d.stride);
}

// `expect`: the regions the layout must have, with their sizes; every other region must be absent.
static void check(const char* layout, const Stage& s, const StageNeeds& d, size_t nout, const size_t (&expect)[R_COUNT]) {
    ++checked;
    static double buffer[1];
    std::vector<Stage::Span> spans;
    size_t sum = 0;
    for (int k = 0; k < R_COUNT; ++k) {
        if (s.r[k].count != expect[k]) return bad("a region's size", layout, d, nout);
        double* p = s.at(buffer, (Region)k);
        if (expect[k] == 0) {
            if (p) return bad("an absent region resolves", layout, d, nout);
            continue;
        }
        if (p != buffer + s.r[k].at) return bad("a region's address", layout, d, nout);
        if (s.r[k].at % 2) return bad("an odd offset", layout, d, nout);
        spans.push_back(s.r[k]);
        sum += expect[k];
    }
    std::sort(spans.begin(), spans.end(), [](const Stage::Span& a, const Stage::Span& b) { return a.at < b.at; });
    size_t end = 0;
    for (const Stage::Span& g : spans) {
        if (g.at < end) return bad("overlapping regions", layout, d, nout);
        if (g.at > end + 1) return bad("a gap of more than one double", layout, d, nout);
        end = g.at + g.count;
    }
    if (s.total < end) return bad("the total ends inside a region", layout, d, nout);
    if (s.total > sum + spans.size()) return bad("more than one double per region of padding", layout, d, nout);
}

int main() {
    Carve c;   // the allocator itself
    if (c.take(3) != 0 || c.take(0) != 4 || c.take(2) != 4 || c.take(1) != 6 || c.total() != 8) {
        std::printf("FAIL Carve\n");
        return 1;
    }
    std::vector<size_t> sizes;
    for (size_t v : {1, 2, 3, 64, 65})
        for (size_t f : {1, 3}) sizes.push_back(v * f);
    const size_t strides[] = {4, 6, 12, 18};
    for (size_t nv : sizes)
        for (size_t n : sizes)
            for (size_t K : sizes)
                for (int flags = 0; flags < 16; ++flags)
                    for (size_t stride : strides) {
                        const StageNeeds d{K * nv, K * n, (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0,
                                           stride};
                        const bool q = d.persp || d.unitQ;
                        size_t un[R_COUNT] = {};
                        un[R_VXY] = d.NV * 2; un[R_VZ] = d.NV; un[R_VQ] = d.persp ? d.NV : 0;
                        un[R_TABLE] = d.lit ? d.NV * 4 : 0;
                        un[R_XY] = d.N * 6; un[R_Z] = d.N * 3; un[R_ATTR] = d.ownAttr ? d.N * stride : 0;
                        un[R_Q] = q ? d.N * 3 : 0;
                        check("unclipped", stage_unclipped(d), d, 0, un);
                        for (size_t nout : sizes) {
                            if (nout > 2 * d.N) continue;
                            size_t cl[R_COUNT] = {};
                            cl[R_XY] = nout * 6; cl[R_Z] = nout * 3; cl[R_ATTR] = nout * stride; cl[R_Q] = q ? nout * 3 : 0;
                            cl[R_TABLE] = d.lit ? d.NV * 4 : 0; cl[R_EXPANDED] = d.lit ? d.N * stride : 0;
                            check("clipped", stage_clipped(d, nout), d, nout, cl);
                        }
                    }
    std::printf("%ld layouts checked, %ld failed\n", checked, failed);
    return failed ? 1 : 0;
}
"""


def test_every_staging_layout_is_aligned_disjoint_and_tight(tmp_path):
    cxx = os.environ.get("CXX") or "g++"          # the C++ driver of the compiler oracle/Makefile builds with
    if shutil.which(cxx) is None:
        pytest.fail(f"no host C++ compiler ({cxx})")
    src, exe = tmp_path / "stage_check.cpp", tmp_path / "stage_check"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout

"""The size rules of the key records' store (csrc/nr_key_records.h) on the CPU:
a small stand-alone program, compiled with the host C++ compiler from the
header alone with -fsanitize=address,undefined, prints the store's bytes, its
allocation, the cap's verdict and the offsets of a few slot counts.

The expected lines are worked out from the rules, not from a run: 128 bytes per
record; the allocation holds one record more than the store; a store fits
when it is no larger than W * H * ipp doubles (64 x 32 x 3: 49152 bytes = 384
records exactly); offsets are the exclusive prefix sum of the counts."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libnativecpurenderer_amd", "csrc")

PROGRAM = r"""
#include "nr_key_records.h"

#include <cstdio>
#include <vector>

int main() {
    std::printf("bytes %llu %llu %llu\n", (unsigned long long)nrkrec::bytes(0), (unsigned long long)nrkrec::bytes(1),
                (unsigned long long)nrkrec::bytes(368602));
    std::printf("room %llu %llu\n", (unsigned long long)nrkrec::room_doubles(0),
                (unsigned long long)nrkrec::room_doubles(368602));
    std::printf("fits %d %d %d %d %d %d\n", nrkrec::fits(384, 64, 32, 3), nrkrec::fits(385, 64, 32, 3),
                nrkrec::fits(512, 64, 32, 4), nrkrec::fits(513, 64, 32, 4), nrkrec::fits(0, 0, 32, 3),
                nrkrec::fits(368602, 3840, 2160, 3));
    // (the largest total a u32 offset table can carry, on a frame that large)
    std::printf("large %d %llu\n", nrkrec::fits(0xFFFFFFFFull, 1 << 20, 1 << 20, 4),
                (unsigned long long)nrkrec::bytes(0xFFFFFFFFull));
    const std::vector<std::uint32_t> counts = {3, 0, 788, 1, 0, 4096};
    std::vector<std::uint32_t> roff(counts.size() + 1, 77u);
    const std::uint64_t total = nrkrec::offsets(counts.data(), counts.size(), roff.data());
    std::printf("offsets");
    for (std::uint32_t v : roff) std::printf(" %u", v);
    std::printf(" total %llu\n", (unsigned long long)total);
    std::vector<std::uint32_t> none(1, 77u);
    const std::uint64_t nothing = nrkrec::offsets(nullptr, 0, none.data());
    std::printf("empty %llu %u\n", (unsigned long long)nothing, none[0]);
    return 0;
}
"""

EXPECTED = [
    "bytes 0 128 47181056",
    "room 16 5897648",
    "fits 1 0 1 0 0 1",
    "large 1 549755813760",
    "offsets 0 3 3 791 792 792 4888 total 4888",
    "empty 0 0",
]


def test_the_size_rules_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or "g++"
    if shutil.which(cxx) is None:
        pytest.fail(f"no host C++ compiler ({cxx})")
    src, exe = tmp_path / "key_records.cpp", tmp_path / "key_records"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == EXPECTED

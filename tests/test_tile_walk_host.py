"""The XCD tile walk every MFMA kernel starts with (csrc/tile_walk.h, sq_xcd_tile), compiled for the host with the address and
undefined-behaviour sanitizers as a stand-alone program (tools/tile_walk_hostcheck.cpp) and checked as a map of blocks to
tiles: a permutation, one contiguous run of tiles per XCD, the runs in XCD order."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every grid size up to two whole rounds of 8 x 8 and a bit (n < 8: q = 0, the XCDs from n on get no tile), then two larger ones
SIZES = list(range(1, 131)) + [1000, 4097]


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    """n -> [sq_xcd_tile(b, n) for b in range(n)], as the host build of the header computes it."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++ or clang++) to build tools/tile_walk_hostcheck.cpp")
    exe = str(tmp_path_factory.mktemp("tile_walk") / "tile_walk_hostcheck")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tools", "tile_walk_hostcheck.cpp")], check=True)
    r = subprocess.run([exe] + [str(n) for n in SIZES], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        n, tiles = line.split(":")
        out[int(n)] = [int(t) for t in tiles.split()]
    assert sorted(out) == SIZES and all(len(out[n]) == n for n in SIZES)
    return out


def test_the_walk_is_a_permutation_of_the_tiles(walks):
    for n in SIZES:
        assert sorted(walks[n]) == list(range(n)), n


def test_each_xcd_walks_a_contiguous_run_and_the_runs_follow_in_xcd_order(walks):
    for n in SIZES:
        start = 0
        for x in range(8):
            run = walks[n][x::8]                  # the blocks with b % 8 == x, ascending
            assert run == list(range(start, start + len(run))), (n, x)
            start += len(run)
        assert start == n, n

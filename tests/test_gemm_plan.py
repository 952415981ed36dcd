"""Tail plan of the hand-written GEMMs (csrc/kernels/gemm_plan.h) on the CPU: the header is plain host
C++, so tests/native/gemm_plan_selftest.cpp is built with g++ (and ASan / UBSan) and asked for the plan of
pinned (kind, M, N, K, CU count) rows. The expected values were derived from the launchers' own expressions
before the plan replaced them (csrc/kernels/gemm_nt.hip, gemm_wgrad.hip); they pin the grid and the scratch
of the 7B weight gradients, the NT shapes with a split tail on either main loop, and the K = 64 shape where
the NT sizing functions used to ask for scratch that the launcher never used."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "gemm_plan_selftest.cpp")
TILE = 256 * 256

# ("kind M N K", expected fields) at cus = 256
ROWS = [
    ("wgrad 22016 4096 32768", dict(tiles=1376, kb=32, R=96, S=2, n_split=96, ws=96 * 2 * TILE, tickets=96, grid=1472)),
    ("wgrad 4096 11008 32768", dict(tiles=688, kb=32, R=176, S=1, n_split=0, ws=0, tickets=0, grid=688)),
    ("nt 4096 4352 128", dict(tiles=272, kb=64, R=16, S=2, n_split=16, ws=16 * 2 * TILE, tickets=16, grid=288)),
    # one 64-deep chunk: nothing to split
    ("nt 4096 4352 64", dict(tiles=272, kb=64, R=16, S=1, n_split=0, ws=0, tickets=0, grid=272)),
    # K % 64 == 32: the ring path, three 32-deep stages
    ("nt 2048 8448 96", dict(tiles=264, kb=32, R=8, S=2, n_split=8, ws=8 * 2 * TILE, tickets=8, grid=272)),
    # the weight gradient of the same shape at K = 64 has two stages and splits
    ("wgrad 4096 4352 64", dict(tiles=272, kb=32, R=16, S=2, n_split=16, ws=16 * 2 * TILE, tickets=16, grid=288)),
    # at most one round, and whole rounds: never split
    ("nt 4096 4096 4096", dict(tiles=256, S=1, n_split=0, ws=0, tickets=0, grid=256)),
    ("wgrad 2048 2048 32768", dict(tiles=64, S=1, n_split=0, ws=0, tickets=0, grid=64)),
    ("nt 8192 4096 4096", dict(tiles=512, R=0, S=1, n_split=0, ws=0, tickets=0, grid=512)),
    ("wgrad 4096 8192 32768", dict(tiles=512, R=0, S=1, n_split=0, ws=0, tickets=0, grid=512)),
]


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", f"-I{os.path.join(ROOT, 'csrc')}", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_gemm_plan_pinned_rows(selftest):
    lines = "".join(f"{row} 256\n" for row, _ in ROWS)
    r = subprocess.run([selftest], input=lines, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = [dict(w.split("=") for w in ln.split()) for ln in r.stdout.splitlines()]
    assert len(out) == len(ROWS)
    for (row, want), got in zip(ROWS, out):
        for key, val in want.items():
            assert got[key] == str(val), (row, key, got)


def test_gemm_plan_matches_the_launchers_it_replaced(selftest):
    """tiles 1..2048 x cus {64, 256, 304} x K {32, 64, 96, 128, 4096} x both kinds x two factorisations."""
    r = subprocess.run([selftest, "exhaustive"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.strip() == f"compared={2 * 3 * 5 * 2048 * 2}"

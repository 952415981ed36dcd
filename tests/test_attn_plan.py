"""Kernel selection of the training attention (csrc/kernels/attn_plan.h) on the CPU: the header is plain
host C++, so tests/native/attn_plan_selftest.cpp is built with g++ (and ASan / UBSan) and asked for the
plan of pinned (options, shape, window, CU count) rows. The expected values were derived from the
launch code the plan replaced (the predicates of csrc/kernels/attention.hip before the argument-block
refactor); they pin what runs for the benchmark shapes, the thresholds between kernels and the
workspace sizes, which callers allocate before they know whether a side-stream window is wanted."""
import os
import shutil
import subprocess

import pytest

from pyrecover_amd import _ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "attn_plan_selftest.cpp")

B16 = dict(B=16, S=2048, Hq=32, Hkv=32, D=128)   # 7B-class MHA
GQA = dict(B=1, S=2048, Hq=32, Hkv=8, D=128)     # Llama-3-8B at batch 1
NC = dict(B=2, S=512, Hq=4, Hkv=2, D=128, causal=0)
NRC_B16 = 16 * 32 * 2048
NRC_GQA = 32 * 2048

# (row of the selftest's input on top of the package defaults and cus=256, expected plan fields)
ROWS = [
    (dict(B16, window=1), dict(fwd_pipe=1, fwd_grp=4, fused=0, nw=8, dq_pipe=1, gq=4, win_early=0, dkdv="lds",
                               gk=4, nsplit=1, delta=0, rc=-1, part=-1, ws=3145728)),
    (dict(B16, window=0), dict(fused=0, dkdv="ring", gk=4, rc=NRC_B16, win_early=0, ws=3145728)),
    (dict(GQA, window=1), dict(dkdv="p2", nsplit=1, win_early=1, gq=4, fwd_grp=4, rc=NRC_GQA, part=-1, ws=196608)),
    (dict(GQA, window=0, dkdv_split=-1), dict(dkdv="p2", nsplit=4, part=3 * NRC_GQA, ws=16973824)),
    (dict(GQA, window=1, dkdv_split=-1), dict(dkdv="p2", nsplit=1, part=-1, ws=16973824)),
    (dict(B=16, S=2048, Hq=16, Hkv=16, D=64), dict(dkdv="p2", nw=8)),
    (dict(B=1, S=640, Hq=2, Hkv=2, D=64, dkdv_impl=0), dict(nw=4, dkdv="lds", ws=3 * 2 * 640)),
    (dict(NC), dict(fwd_pipe=0, dq_pipe=1)),
    (dict(NC, skv=500), dict(fwd_pipe=0, dq_pipe=0)),
    (dict(B16, bwd_fused=-1), dict(fused=1, rc=NRC_B16, acc=3 * NRC_B16, ws=137887744)),
    (dict(B16, B=12, bwd_fused=-1), dict(fused=0)),
    (dict(GQA, bwd_fused=-1), dict(fused=0)),
    # KREG and the ring kernel exist at D = 128 with 8-wave blocks only
    (dict(B16, dkdv_kreg=-1), dict(dkdv="kreg", rc=-1)),
    (dict(B16, dkdv_kreg=-1, window=1), dict(dkdv="lds")),
    (dict(B=2, S=384, Hq=4, Hkv=4, D=128, dkdv_kreg=2), dict(nw=4, dkdv="lds")),
    (dict(B=2, S=512, Hq=4, Hkv=4, D=64, dkdv_impl=0, dkdv_kreg=1), dict(nw=8, dkdv="lds")),
    # the other two families: one kernel each, sizes from the same function
    (dict(B=1, S=128, Hq=2, Hkv=1, D=64, fam=1), dict(delta=0, ws=3 * 2 * 128)),
    (dict(B=1, S=256, Hq=4, Hkv=2, D=128, fam=2), dict(delta=0, qend=4 * 256, ws=4 * 256 + 2)),
]


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("attn_plan") / "attn_plan_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", f"-I{os.path.join(ROOT, 'csrc')}", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _plans(exe, rows):
    lines = []
    for row in rows:
        kv = dict(_ext._ATTN_DEFAULTS, cus=256)
        kv.update(row)
        lines.append(" ".join(f"{k}={v}" for k, v in kv.items()))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = [dict(w.split("=") for w in ln.split()) for ln in r.stdout.splitlines()]
    assert len(out) == len(rows)
    return out


def test_attn_plan_pinned_rows(selftest):
    for (row, want), got in zip(ROWS, _plans(selftest, [r for r, _ in ROWS])):
        for key, val in want.items():
            assert got[key] == str(val), (row, key, got)


def test_attn_plan_workspace_ignores_window(selftest):
    """Callers size the workspace before they know the window; the kernels chosen may differ, the size not."""
    shapes = [dict(s, **o) for s in (B16, GQA, dict(B=2, S=384, Hq=8, Hkv=2, D=64))
              for o in (dict(), dict(dkdv_split=-1), dict(bwd_fused=1), dict(dkdv_kreg=-1, dkdv_impl=1))]
    a = _plans(selftest, [dict(s, window=0) for s in shapes])
    b = _plans(selftest, [dict(s, window=1) for s in shapes])
    for s, x, y in zip(shapes, a, b):
        assert x["ws"] == y["ws"] and x["fused"] == y["fused"], s

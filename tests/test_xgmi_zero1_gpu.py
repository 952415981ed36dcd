"""The sharded optimizer (ZeRO-1) and the sparse embedding-gradient exchange on the xGMI engine
(csrc/comm/xgmi.cpp, pyrecover_amd/parallel/xgmi.py), 2 ranks sharing one GPU over IPC memory and
IPC events: the engine's reduce-scatter, its parameter all-gather behind the AdamW update, the sparse
row kernels (csrc/kernels/comm.hip sparse_rows_kernel), and both modes through bench.py.

Every equality is exact by construction: the reduce-scatter chunks a bucket as the all-reduce does,
both sum in rank order in fp32 and round once, the update is elementwise, and the sparse exchange sums
the same rows in the same order (a rank that did not produce a row contributes an exact zero to the
dense sum). Nothing here measures bandwidth; nothing runs at more than 2 ranks except the sparse
kernels, where one process stands in for up to 4."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(tmp_path, test, port):
    out = tmp_path / f"{test}.pt"
    env = dict(os.environ, PYRECOVER_LOCAL_DEVICE="0", PYRECOVER_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "dist_workers", "xgmi_zero1_worker.py"), "--test", test, "--out", str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    res = torch.load(out, weights_only=False)
    assert len(res) == 2
    return res


def test_xgmi_reduce_scatter_alone(cuda, tmp_path):
    """GradReducer(backend="xgmi", shard=True) on rank-seeded random gradients: each rank's owned chunk
    of every bucket is the fp32 rank-ordered sum rounded once (error exactly 0), every other chunk still
    holds this rank's own input (no gradient all-gather follows the reduce)."""
    for res in _worker(tmp_path, "rs", 29561):
        assert res["buckets"] > 3
        assert res["owned_err"] == [0.0, 0.0], res
        assert res["other_err"] == [0.0, 0.0], res
        assert res["owned_numel"] == [res["numel"] // 2] * 2, res


def test_xgmi_zero1_equals_xgmi_allreduce(cuda, tmp_path):
    """20 steps of llama-tiny: ZeRO-1 on the engine (reduce-scatter, 1/W update, parameter pull-gather),
    with the update after the backward and overlapped with it, leaves the parameters and (after
    gather_state) both moments bit-equal to the engine's all-reduce run, and the two ranks' parameters
    equal within each arm."""
    for res in _worker(tmp_path, "zero1", 29562):
        assert res["trained"]
        for arm in ("shard", "shard_overlap"):
            assert res[arm] == {"params": True, "exp_avg": True, "exp_avg_sq": True}, (arm, res)
        assert res["ranks_equal"] == {"allreduce": True, "shard": True, "shard_overlap": True}, res
        # the sharded arms ran the engine's gather over the IPC-mapped parameter buffer
        assert res["params_mapped"] == {"allreduce": False, "shard": True, "shard_overlap": True}, res


def test_xgmi_sparse_exchange_equals_dense_allreduce(cuda, tmp_path):
    """20 steps with the embedding bucket reduced by the sparse row kernels against the engine's dense
    all-reduce of it, with one and with two accumulated micro-batches: equal parameters, and the
    reducer never allocated the vocab-sized scratch of the process-group path."""
    for res in _worker(tmp_path, "sparse", 29563):
        for arm in ("accum1", "accum2"):
            assert res[arm] == {"params": True, "scratch_none": True, "ranks_equal": True,
                                "ids_published": True}, (arm, res)


# ---------------------------------------------------------------------------------------------
def _id_lists(W, V, n, gen):
    """n sorted ids per rank. Where n allows: an id every rank holds (c), ids 0 and V - 1 and an id
    past the end (rank 0), an id only the last rank holds and a negative one (last rank), an id of its
    own per rank (disjoint), the rest random (duplicates)."""
    c, only_last = V // 3, V // 2 + 1
    lists = []
    for r in range(W):
        own = 2 + r
        if r == W - 1:
            first = [only_last, c] + ([0, V - 1, V + 5] if W == 1 else []) + [-3, own]
        elif r == 0:
            first = [0, V - 1, c, V + 5, own]
        else:
            first = [own, c]
        fill = torch.randint(0, V, (n,), generator=gen).tolist()
        fill = [i for i in fill if i != only_last and not 2 <= i < 2 + W]
        lists.append(sorted((first + fill + [c] * n)[:n]))
    return lists


def _sparse_case(cuda, W, dtype, V, D, lists, gen):
    C = __import__("pyrecover_amd._ext", fromlist=["native"]).native().xgmi
    n = len(lists[0])
    g = [torch.randn(V, D, generator=gen, device=cuda).to(dtype) for _ in range(W)]
    ids = [torch.tensor(lst, dtype=torch.int64, device=cuda) for lst in lists]
    # oracle: zero what a rank did not produce, sum densely in fp32 in rank order, round once
    produced = [sorted({i for i in lst if 0 <= i < V}) for lst in lists]
    union = sorted(set().union(*produced))
    total = torch.zeros(V, D, dtype=torch.float32, device=cuda)
    for r in range(W):
        masked = torch.zeros(V, D, dtype=dtype, device=cuda)
        masked[produced[r]] = g[r][produced[r]]
        total = total + masked.float()
    total = total.to(dtype)
    expect = []
    for r in range(W):
        e = g[r].clone()
        e[union] = total[union]
        expect.append(e)
    st = torch.cuda.current_stream(cuda).cuda_stream
    gp, ip = [t.data_ptr() for t in g], [t.data_ptr() for t in ids]
    for phase in (1, 2):
        for me in range(W):
            C.sparse_rows(phase, gp, ip, me, n, V, D, dtype, st)
    torch.cuda.synchronize()
    outside = [i for i in range(V) if i not in set(union)]
    for r in range(W):
        assert torch.equal(g[r], expect[r]), (W, dtype, V, D, n, r, (g[r].float() - expect[r].float()).abs().max().item())
        assert torch.equal(g[r][outside], expect[r][outside])  # rows outside the union: untouched
    return len(union)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_sparse_rows_kernels_one_process_for_w_ranks(cuda, W, dtype):
    """The phase-1 / phase-2 kernels through the pointer-list binding: every rank's buffer ends with
    the rank-ordered fp32 sum, rounded once, of the rows' producers in every union row and unchanged
    elsewhere (the buffers start random everywhere, so a row read from a rank that did not produce it,
    or a sum out of rank order at W >= 3, shows). Ids outside [0, V) index nothing."""
    gen = torch.Generator(device="cpu").manual_seed(1234 + W)
    ggen = torch.Generator(device=cuda).manual_seed(77 + W)
    for V, D, n in ((37, 8, 1), (37, 136, 5), (512, 256, 300)):
        lists = _id_lists(W, V, n, gen)
        nu = _sparse_case(cuda, W, dtype, V, D, lists, ggen)
        assert nu >= 1
        if n >= 5:
            assert all(V // 3 in lst for lst in lists) and V // 2 + 1 in lists[-1]
            assert 0 in lists[0] and V - 1 in lists[0] and V + 5 in lists[0]
            assert all(V // 2 + 1 not in lst for lst in lists[:-1])
            # one rank's ids all equal (rank 0, which then holds only the id every rank holds)
            _sparse_case(cuda, W, dtype, V, D, [[V // 3] * n] + lists[1:], ggen)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--shard-optimizer", "--sparse-embedding-grad", "on"]], ids=["auto", "both-on"])
def test_bench_gpus2_xgmi_runs_zero1(cuda, extra):
    """bench.py --allreduce xgmi at its defaults for a grouped-query model at batch 1 (--shard-optimizer
    auto turns ZeRO-1 on), and with both modes forced on: exits 0, runs sharded, replicas identical."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(PYRECOVER_LOCAL_DEVICE="0", PYRECOVER_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--model", "llama-tiny",
                        "--batch-per-gpu", "1", "--seq-len", "256", "--steps", "3", "--warmup", "1",
                        "--bucket-mb", "0.25", "--allreduce", "xgmi", "--full"] + extra,
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-5000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1])
    assert out["config"]["allreduce"] == "xgmi"
    assert out["config"]["shard_optimizer"] is True
    assert out["params_identical_across_ranks"] is True
    if extra:
        assert out["config"]["sparse_embedding_grad"] is True

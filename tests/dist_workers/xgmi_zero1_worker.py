"""Worker for tests/test_xgmi_zero1_gpu.py: 2 ranks (torchrun), both pinned to one GPU
(PYRECOVER_LOCAL_DEVICE=0, PYRECOVER_DIST_BACKEND=gloo). One launch runs every arm of one test, one
model and reducer after another in the same two processes, and rank 0 writes what the test asserts:

* ``rs``: the engine's reduce-scatter alone on rank-seeded random gradients;
* ``zero1``: 20 training steps on the engine: all-reduce, ZeRO-1, ZeRO-1 with the overlapped update;
* ``sparse``: 20 steps with the sparse embedding exchange against the dense all-reduce, also with two
  accumulated micro-batches."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

STEPS = 20


def _model(dev):
    from pyrecover_amd.config import get_preset
    from pyrecover_amd.models.llama import Transformer
    from pyrecover_amd.parallel.ddp import broadcast_flat

    torch.manual_seed(0)
    cfg = get_preset("llama-tiny", seq_len=256)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    with torch.device(dev):
        m = Transformer(cfg)
    torch.set_default_dtype(prev)
    flat = m.flatten_(shadows=False)  # every arm without weight shadows, as the sharded mode runs
    broadcast_flat(flat)
    return cfg, m, flat


def _reducer(flat, **kw):
    from pyrecover_amd.parallel.ddp import GradReducer

    red = GradReducer(flat, bucket_cap_mb=0.5, first_bucket_mb=0.25, backend="xgmi", **kw)
    assert red.num_buckets > 3, red.num_buckets
    return red


def _peer_copy(t, rank):
    """Rank 0's and rank 1's copies of t, on every rank."""
    parts = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, t.contiguous())
    return parts


def run_rs(dev, rank, world):
    """Reduce-scatter alone: the owned chunk is the fp32 rank-ordered sum rounded once, every other
    chunk keeps this rank's input."""
    _, _, flat = _model(dev)
    red = _reducer(flat, shard=True)
    ins = []
    for r in range(world):
        g = torch.Generator(device=dev)
        g.manual_seed(100 + r)
        ins.append(torch.randn(flat.numel, generator=g, device=dev).to(flat.grad.dtype))
    expect = ins[0].float()
    for r in range(1, world):
        expect = expect + ins[r].float()
    expect = expect.to(flat.grad.dtype)
    flat.grad.copy_(ins[rank])
    for b in range(red.num_buckets):
        red._launch(b)
    red.next_to_launch = red.num_buckets
    red.finish()
    red.reset()
    torch.cuda.synchronize()
    owned_err, other_err, owned_n = 0.0, 0.0, 0
    for b, (lo, hi) in enumerate(red.ranges):
        (a, z), = red.owned(b)
        owned_n += z - a
        owned_err = max(owned_err, (flat.grad[a:z].float() - expect[a:z].float()).abs().max().item())
        for x, y in ((lo, a), (z, hi)):
            if x < y:
                other_err = max(other_err, (flat.grad[x:y].float() - ins[rank][x:y].float()).abs().max().item())
    res = torch.tensor([owned_err, other_err, float(owned_n), float(flat.numel)], dtype=torch.float64, device=dev)
    per_rank = _peer_copy(res, rank)
    return {"owned_err": [float(p[0]) for p in per_rank], "other_err": [float(p[1]) for p in per_rank],
            "owned_numel": [int(p[2]) for p in per_rank], "numel": int(per_rank[0][3]), "buckets": red.num_buckets}


def _train(dev, rank, world, shard=False, overlap=False, sparse=False, accum=1):
    from pyrecover_amd.optim.adamw import FlatAdamW

    cfg, m, flat = _model(dev)
    red = _reducer(flat, shard=shard, sparse_slot=flat.slot(m.tok_embeddings.weight).index if sparse else None)
    opt = FlatAdamW(flat, lr=1e-3, grad_scale=1.0 / (world * accum))
    if overlap:
        opt.enable_overlap(red)
    gen = torch.Generator(device=dev)
    gen.manual_seed(123 + rank)
    for _ in range(STEPS):
        opt.zero_grad()
        for a in range(accum):
            if a:
                flat.next_micro_batch()
            red.enabled = a == accum - 1
            t = torch.randint(0, cfg.vocab_size, (2, 257), device=dev, generator=gen)
            m(t[:, :-1], labels=t[:, 1:]).backward()
        red.finish()
        opt.step()
    opt.gather_state()
    torch.cuda.synchronize()
    out = {"params": flat.data.clone(), "exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone(),
           "scratch_none": red._emb_scratch is None,
           # the engine's own paths ran: the published id list has the step's size; the parameters live
           # in the IPC-mapped buffer the peers pull from
           "ids_published": red.xgmi.ids_buf is not None and red.xgmi.ids_buf.numel() == 2 * 256 * accum,
           "params_mapped": red.xgmi.pbuf is not None and flat.data.data_ptr() == red.xgmi.pbuf.data_ptr()}
    p = _peer_copy(out["params"], rank)
    out["ranks_equal"] = bool(torch.equal(p[0], p[1]))
    return out


def _same(a, b, keys):
    return {k: bool(torch.equal(a[k], b[k])) for k in keys}


def run_zero1(dev, rank, world):
    keys = ("params", "exp_avg", "exp_avg_sq")
    ar = _train(dev, rank, world)
    zero = _train(dev, rank, world, shard=True)
    zero_ov = _train(dev, rank, world, shard=True, overlap=True)
    init = _model(dev)[2].data
    return {"shard": _same(ar, zero, keys), "shard_overlap": _same(ar, zero_ov, keys),
            "ranks_equal": {"allreduce": ar["ranks_equal"], "shard": zero["ranks_equal"],
                            "shard_overlap": zero_ov["ranks_equal"]},
            "trained": not torch.equal(init, ar["params"]),
            "params_mapped": {"allreduce": ar["params_mapped"], "shard": zero["params_mapped"],
                              "shard_overlap": zero_ov["params_mapped"]}}


def run_sparse(dev, rank, world):
    res = {}
    for name, accum in (("accum1", 1), ("accum2", 2)):
        dense = _train(dev, rank, world, accum=accum)
        sparse = _train(dev, rank, world, sparse=True, accum=accum)
        res[name] = {"params": bool(torch.equal(dense["params"], sparse["params"])),
                     "scratch_none": sparse["scratch_none"], "ranks_equal": sparse["ranks_equal"],
                     "ids_published": sparse["ids_published"] and not dense["ids_published"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--test", choices=["rs", "zero1", "sparse"], required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    from pyrecover_amd.parallel import dist as D

    lrank, world = D.maybe_init_distributed(True)
    rank = D.get_rank()
    dev = torch.device("cuda", D.gpu_index(lrank))
    res = {"rs": run_rs, "zero1": run_zero1, "sparse": run_sparse}[a.test](dev, rank, world)
    # every rank's verdict reaches rank 0: a mismatch seen only by rank 1 must fail the test too
    allres = [None] * world
    dist.all_gather_object(allres, res)
    if rank == 0:
        torch.save(allres, a.out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

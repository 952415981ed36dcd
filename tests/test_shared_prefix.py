"""Shared-prefix decode on the CPU: PagedKVCache.fork and its shared_len bookkeeping, and generate(n_samples=N)
on the torch-math path."""
import warnings

import pytest
import torch

from pyrecover_amd import inference as inf
from pyrecover_amd.config import get_preset
from pyrecover_amd.models.llama import Transformer


def _forked():
    """Rows of 150 and 128 tokens (pages of 64: one with a partial page, one without) forked three ways."""
    cfg = get_preset("llama-micro", seq_len=256)
    c = inf.PagedKVCache(cfg, 2, 200, torch.float32, "cpu", page_size=64, n_pages=9)
    c.reserve(0, 150), c.reserve(1, 128)
    return c, c.block_table.tolist()


def test_fork_bookkeeping():
    c, (r0, r1) = _forked()
    c.k[1][r0[2], :22] = 7.0
    with pytest.raises(RuntimeError, match="short by 1"):
        c.fork(6, [150, 128])  # five copies of the partial page, four pages free
    assert c.pages_in_use() == 5 and c.batch == 2
    f = c.fork(3, [150, 128])
    t = f.block_table.tolist()
    assert (f.batch, f.group_size, f.pages_in_use()) == (6, 3, 7)
    assert f.kv_len.tolist() == [150] * 3 + [128] * 3 and f.shared_len.tolist() == [128, 128]
    assert t[0] == r0 and t[3] == r1
    for i in (1, 2):  # the full pages named again, the partial page copied into a page of the copy's own
        assert t[i][:2] == r0[:2] and t[i][2] not in r0 + r1 and t[i][3] == -1
        assert (f.k[1][t[i][2], :22] == 7.0).all()
        assert t[3 + i] == r1[:2] + [-1, -1]
    assert t[1][2] != t[2][2]
    assert [f._refs[p] for p in r0[:3]] == [3, 3, 1] and [f._refs[p] for p in r1[:2]] == [3, 3]
    f.reserve(4, 200)  # a copy's growth lands on fresh pages and leaves the shared prefix alone
    assert f.block_table[4].tolist()[:2] == r1[:2] and f.pages_in_use() == 9 and f.shared_len.tolist() == [128, 128]


def test_shared_len_stays_truthful():
    c, (r0, r1) = _forked()
    f = c.fork(3, [150, 128])
    f.share_prefix(0, 2, 70)  # inside the group: row 2 now agrees with the others on one page only
    assert f.shared_len.tolist() == [64, 128] and f.block_table[2].tolist()[0] == r0[0]
    f.share_prefix(3, 1, 128)  # from another group: row 1 agrees with nothing of its own group
    assert f.shared_len.tolist() == [0, 128] and f.block_table[1].tolist()[:2] == r1[:2]
    f.release(5)
    assert f.shared_len.tolist() == [0, 0] and f._shared == [0, 0]
    assert [f._refs[p] for p in r1[:2]] == [3, 3]  # rows 3, 4 and now 1


def test_generate_n_samples_on_cpu_and_refusals():
    torch.manual_seed(0)
    cfg = get_preset("llama-micro", seq_len=128)
    m = Transformer(cfg).float().eval()
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist() for n in (3, 70, 64)]
    s1, s2 = {}, {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # the once-per-shape note of the torch-math path
        one = inf.generate(m, prompts, 10, kv_page_size=64, stats=s1)
        two = inf.generate(m, prompts, 10, kv_page_size=64, n_samples=2, stats=s2)
        inf.generate(m, [p for p in prompts for _ in range(2)], 10, kv_page_size=64, stats=s1)  # each on its own
    assert two[0] == [t for t in one[0] for _ in range(2)] and two[1] == [r for r in one[1] for _ in range(2)]
    assert s2["n_samples"] == 2 and 0 < s2["kv_cache_bytes"] < s1["kv_cache_bytes"]
    for kw in ({"n_samples": 2}, {"n_samples": 2, "kv_page_size": 64, "use_cache": False},
               {"n_samples": 0, "kv_page_size": 64}):
        with pytest.raises(ValueError, match="n_samples"):
            inf.generate(m, prompts, 4, **kw)

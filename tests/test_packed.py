"""Packed sequences on the CPU (torch oracle path): doc_start semantics of the model, the packed
dataset / collator, bit-exact resume with --pack-sequences, and the flag-off path."""
import csv

import numpy as np
import pytest
import torch

from pyrecover_amd.config import get_preset
from pyrecover_amd.data.dataset import (CollatorForCLM, CollatorForPackedCLM, PackedParquetDataset,
                                        SyntheticTokenDataset, make_synthetic_parquet)
from pyrecover_amd.data.tokenizer import ByteTokenizer
from pyrecover_amd.models.llama import Transformer


def _doc_start(lengths):
    out, p = [], 0
    for n in lengths:
        out += [p] * n
        p += n
    return torch.tensor(out, dtype=torch.int32)


# ------------------------------------------------------------------------------------------
def test_packed_row_equals_documents_run_alone():
    """fp64 llama-micro: a packed row of three documents gives, at every position, the logits of
    the same document run alone from position 0, and the packed loss is the token-weighted mean of
    the three separate losses. fp64 rounding over ~10^3-term sums stays orders of magnitude below
    the 1e-9 bound."""
    torch.manual_seed(0)
    a = get_preset("llama-micro", seq_len=96)
    m = Transformer(a).double()
    lens = [17, 48, 31]
    S = sum(lens)
    tok = torch.randint(0, a.vocab_size, (1, S))
    lab = torch.randint(0, a.vocab_size, (1, S))
    ds = _doc_start(lens).view(1, S)
    with torch.no_grad():
        packed = m(tok, doc_start=ds)
        loss_packed = m(tok, labels=lab, doc_start=ds)
        unmasked = m(tok)
        p, num = 0, 0.0
        for n in lens:
            alone = m(tok[:, p:p + n])
            assert (packed[:, p:p + n] - alone).abs().max().item() < 1e-9
            num += m(tok[:, p:p + n], labels=lab[:, p:p + n]).item() * n
            p += n
    assert abs(loss_packed.item() - num / S) < 1e-9
    # the mask matters: without it the later documents see their predecessors
    assert (unmasked[:, lens[0]:] - packed[:, lens[0]:]).abs().max().item() > 1e-3


def test_packed_gradients_equal_documents_run_alone():
    """The backward through the torch path: parameter gradients of the packed row equal the
    token-weighted sum of the documents' own gradients (fp64, same 1e-9 bound on values of O(1))."""
    torch.manual_seed(1)
    a = get_preset("llama-micro", seq_len=64)
    m = Transformer(a).double()
    lens = [5, 40, 19]
    S = sum(lens)
    tok = torch.randint(0, a.vocab_size, (1, S))
    lab = torch.randint(0, a.vocab_size, (1, S))
    m(tok, labels=lab, doc_start=_doc_start(lens).view(1, S)).backward()
    packed = {n: p.grad.clone() for n, p in m.named_parameters()}
    for p in m.parameters():
        p.grad = None
    q = 0
    for n in lens:
        (m(tok[:, q:q + n], labels=lab[:, q:q + n]) * (n / S)).backward()
        q += n
    for n, p in m.named_parameters():
        assert (packed[n] - p.grad).abs().max().item() < 1e-9, n


def test_reference_ops_with_doc_start():
    """attention_ref / attention_lse_ref / rope_inplace_2d / flash_attention (CPU: torch math) with
    doc_start: each document equals the plain causal op on its own slice."""
    from pyrecover_amd.ops import flash_attention
    from pyrecover_amd.ops import reference as R

    torch.manual_seed(0)
    B, S, Hq, Hkv, D = 1, 48, 4, 2, 16
    lens = [1, 20, 27]
    q, k, v = (torch.randn(B, S, h, D, dtype=torch.float64) for h in (Hq, Hkv, Hkv))
    ds = _doc_start(lens).view(1, S)
    o = R.attention_ref(q, k, v, True, doc_start=ds)
    o2, lse = R.attention_lse_ref(q, k, v, True, doc_start=ds)
    o3 = flash_attention(q, k, v, doc_start=ds)
    tab = R.rope_table(R.precompute_freqs_cis(D, S))
    x = torch.randn(S, Hq * D, dtype=torch.float64)
    xr = x.clone()
    R.rope_inplace_2d(xr, Hq * D, tab, D, S, doc_start=ds)
    p = 0
    for n in lens:
        sl = slice(p, p + n)
        alone, lse_alone = R.attention_lse_ref(q[:, sl], k[:, sl], v[:, sl], True)
        for got in (o, o2, o3):
            assert (got[:, sl] - alone).abs().max().item() < 1e-12
        assert (lse[:, :, sl] - lse_alone).abs().max().item() < 1e-12
        xa = x[sl].clone()
        R.rope_inplace_2d(xa, Hq * D, tab, D, n)
        assert torch.equal(xr[sl], xa)
        p += n
    back = xr.clone()
    R.rope_inplace_2d(back, Hq * D, tab, D, S, inverse=True, doc_start=ds)
    assert (back - x).abs().max().item() < 1e-6  # the table is fp32
    # garbage values are clamped into [0, i], as in the kernels
    bad = torch.tensor([[-5, 7, 1, 0, 9]], dtype=torch.int32)
    assert R.doc_positions(bad).tolist() == [[0, 0, 1, 3, 0]]


# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parquet(tmp_path_factory):
    return make_synthetic_parquet(str(tmp_path_factory.mktemp("pq") / "docs.parquet"), n_docs=12, min_words=5,
                                  max_words=120, seed=3)


def _stream(path, tok, n_tokens):
    import pyarrow.parquet as pq

    texts = pq.read_table(path).column("text")
    out, k = [], 0
    while len(out) < n_tokens:
        out += tok.encode(str(texts[k % len(texts)])) + [tok.eos_token_id]
        k += 1
    return out


def test_packed_dataset_tiles_the_stream_and_is_a_pure_function(parquet):
    tok = ByteTokenizer()
    S = 200
    n = 40  # several passes through the 12-document file
    ds = PackedParquetDataset(parquet, tok, S, n)
    assert len(ds) == n
    stream = _stream(parquet, tok, n * (S + 1))
    order = list(range(n))
    np.random.default_rng(0).shuffle(order)  # any access order, the index extends as needed
    got = {i: ds[i] for i in order}
    for i in range(n):
        assert got[i]["input_ids"] == stream[i * (S + 1):(i + 1) * (S + 1)], i
    for i in (n - 1, 7, 0):  # a fresh dataset asked for i first
        assert PackedParquetDataset(parquet, tok, S, n)[i] == got[i]
    # lazily: sample 0 tokenizes only the documents it needs
    fresh = PackedParquetDataset(parquet, tok, S, n)
    fresh[0]
    assert len(fresh._cum) - 1 < fresh.real_length


def test_packed_collator_boundaries_and_labels(parquet):
    tok = ByteTokenizer()
    S = 200
    ds = PackedParquetDataset(parquet, tok, S, 24)
    inputs, labels, doc_start = CollatorForPackedCLM(S, tok.pad_token_id)([ds[i] for i in range(24)])
    assert inputs.shape == labels.shape == doc_start.shape == (24, S)
    assert doc_start.dtype == torch.int32 and inputs.dtype == torch.int64
    i = torch.arange(S)
    assert (doc_start[:, 0] == 0).all()  # a document cut by the row boundary restarts at position 0
    assert (doc_start <= i).all() and (doc_start[:, 1:] >= doc_start[:, :-1]).all()
    assert ((doc_start == i) | (doc_start == torch.roll(doc_start, 1, dims=1)))[:, 1:].all()
    # a document's last token is the eos the dataset appended (the byte tokenizer never emits it)
    last = inputs == tok.eos_token_id
    assert last.any()
    assert torch.equal(labels == -100, last)
    assert (doc_start[:, 1:] == i[1:])[last[:, :-1]].all()  # the token after an eos opens a document
    assert (inputs != tok.pad_token_id).all()  # no pad tokens
    # the labels are the next tokens of the stream
    for r in range(24):
        full = ds[r]["input_ids"]
        keep = labels[r] != -100
        assert torch.equal(labels[r][keep], torch.tensor(full[1:])[keep])


def test_synthetic_dataset_documents():
    S = 256
    plain = SyntheticTokenDataset(512, S, 8, seed=5)
    packed = SyntheticTokenDataset(512, S, 8, seed=5, doc_len_range=(16, 128))
    again = SyntheticTokenDataset(512, S, 8, seed=5, doc_len_range=(16, 128))
    for idx in (3, 0, 7):
        assert set(plain[idx]) == {"input_ids"}  # default output unchanged
        assert packed[idx]["input_ids"] == plain[idx]["input_ids"]
        assert packed[idx] == again[idx]  # a function of (seed, idx) only
        ds = torch.tensor(packed[idx]["doc_start"])
        assert ds.shape == (S + 1,) and ds[0] == 0 and (ds <= torch.arange(S + 1)).all()
        starts = torch.nonzero(ds == torch.arange(S + 1)).flatten()
        lens = torch.diff(starts)
        assert len(starts) > 2 and lens.min() >= 16 and lens.max() <= 128
    assert packed[1]["doc_start"] != packed[2]["doc_start"]
    x, y = CollatorForCLM(S, 0)([plain[0], plain[1]])
    xp, yp, dsp = CollatorForPackedCLM(S, 0)([packed[0], packed[1]])
    assert torch.equal(x, xp) and torch.equal(y[yp != -100], yp[yp != -100])


# ------------------------------------------------------------------------------------------
def _args(ckdir, steps, extra=()):
    from pyrecover_amd.cli import get_args

    return get_args(["--model-preset", "llama-micro", "--synthetic-data", "--sequence-length", "128",
                     "--batch-size", "2", "--training-steps", str(steps), "--checkpoint-dir", str(ckdir),
                     "--checkpoint-frequency", "2", "--model-dtype", "fp32", "--num-workers", "0",
                     "--log-loss-to-csv", "--logging-frequency", "1"] + list(extra))


def _ckpt(ckdir, step):
    ck = torch.load(ckdir / "default-exp" / f"ckpt_{step}.pt", weights_only=True)
    return ck["model"], ck["optimizer"]["state"]


def _assert_same(a, b):
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    for k in a[1]:
        for f in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a[1][k][f], b[1][k][f]), (k, f)


def _losses(ckdir):
    with open(ckdir / "default-exp" / "default-exp_loss_log.csv") as f:
        return [row["Loss"] for row in csv.DictReader(f)]


def test_cli_flag_defaults_off():
    from pyrecover_amd.cli import get_args

    assert get_args([]).pack_sequences is False
    assert get_args(["--pack-sequences"]).pack_sequences is True


def test_pack_sequences_resume_is_bit_exact(tmp_path):
    from pyrecover_amd.trainer import train

    jl = tmp_path / "m.jsonl"
    train(_args(tmp_path / "straight", 4, ["--pack-sequences", "--metrics-jsonl", str(jl)]))
    # (the same --training-steps: the sampler's permutation depends on the number of samples)
    r = train(_args(tmp_path / "split", 4, ["--pack-sequences", "--stop-at-step", "2"]))
    assert r["step"] == 2 and r["stopped_early"]
    r = train(_args(tmp_path / "split", 4, ["--pack-sequences", "--resume-from-checkpoint", "latest"]))
    assert r["step"] == 4
    _assert_same(_ckpt(tmp_path / "straight", 4), _ckpt(tmp_path / "split", 4))
    # packing changes the computation (the documents no longer see each other)
    train(_args(tmp_path / "plain", 4))
    assert _losses(tmp_path / "plain") != _losses(tmp_path / "straight")
    import json

    recs = [json.loads(line) for line in open(jl)]
    assert all(r["docs_per_row"] > 1 and r["nonpad_fraction"] == 1.0 for r in recs)


def test_flag_off_equals_single_document_through_the_torch_path(tmp_path, monkeypatch):
    """Without --pack-sequences nothing changes: the run's losses, parameters and moments are bit-equal
    to a run whose loader hands every batch over as one document per row (doc_start all zeros), which
    takes the doc_start route through the trainer, the model and the torch ops."""
    from pyrecover_amd import trainer

    trainer.train(_args(tmp_path / "off", 4))

    class OneDocCollator(CollatorForCLM):
        def __call__(self, examples):
            x, y = super().__call__(examples)
            return x, y, torch.zeros(x.shape, dtype=torch.int32)

    monkeypatch.setattr(trainer, "CollatorForCLM", OneDocCollator)
    trainer.train(_args(tmp_path / "one", 4))
    assert _losses(tmp_path / "off") == _losses(tmp_path / "one") and len(_losses(tmp_path / "off")) == 4
    _assert_same(_ckpt(tmp_path / "off", 4), _ckpt(tmp_path / "one", 4))

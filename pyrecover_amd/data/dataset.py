"""Datasets and collator (reference dataset.py:10-61) plus synthetic data for benchmarks.

* :class:`ParquetDataset` keeps the reference semantics: memory-mapped parquet with a ``text``
  column, virtual length = ``training_samples``, sample ``idx`` tokenizes ``text[idx % rows]`` with
  right padding / truncation to ``sequence_length + 1``.
* :class:`CollatorForCLM` returns ``(inputs, labels)`` with pad labels set to -100.
* :class:`PackedParquetDataset` (``--pack-sequences``) concatenates the documents into one token
  stream and cuts it into rows, so no position is padding; :class:`CollatorForPackedCLM` returns
  ``(inputs, labels, doc_start)``, the document boundaries the model masks attention with.
* :class:`SyntheticTokenDataset` yields deterministic random token rows (a function of
  ``(seed, idx)`` only, so resuming at any sample reproduces the same stream).
* :func:`make_synthetic_parquet` writes a parquet file of random text for end-to-end runs without
  the reference's cluster dataset.
"""
from __future__ import annotations

import bisect
import os
import random
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset


class ParquetDataset(Dataset):
    def __init__(self, parquet_file: str, tokenizer, sequence_length: int, training_samples: int):
        import pyarrow.parquet as pq

        self.parquet_ds = pq.read_table(parquet_file, memory_map=True)
        self.real_length = len(self.parquet_ds)
        if self.real_length == 0:
            raise ValueError(f"{parquet_file} has no rows")
        self.texts = self.parquet_ds.column("text")
        self.tokenizer = tokenizer
        self.sequence_length = sequence_length
        self.training_samples = training_samples

    def __len__(self):
        return self.training_samples

    def __getitem__(self, idx: int):
        sample_str = str(self.texts[idx % self.real_length])
        return self.tokenizer.encode_plus(sample_str, max_length=self.sequence_length + 1, padding="max_length",
                                          truncation=True, padding_side="right")


def _doc_start_from_lengths(lengths, n: int) -> List[int]:
    """doc_start of a row of n tokens cut into consecutive documents of the given lengths (the last
    one truncated at the row's end): the index of the first token of each token's document."""
    out = np.empty(n, dtype=np.int64)
    p = 0
    for ln in lengths:
        if p >= n:
            break
        out[p:p + ln] = p
        p += ln
    assert p >= n, "document lengths must cover the row"
    return out.tolist()


class PackedParquetDataset(Dataset):
    """Concat-and-chunk packing of a parquet ``text`` column (``--pack-sequences``).

    The token stream is every document's ``tokenizer.encode(text)`` followed by ``eos_token_id``,
    documents taken in file order, cyclically. Sample ``idx`` is tokens
    ``[idx * (S + 1), (idx + 1) * (S + 1))`` of that stream, ``S = sequence_length``: a pure function
    of ``(file, tokenizer, S, idx)``, so the resumable sampler and DataLoader workers need no new
    state. A sample is ``{"input_ids": [S + 1 ids], "doc_start": [S + 1 ints]}``; ``doc_start[p]`` is
    the index within the sample of the first token of the document token ``p`` belongs to. A document
    cut by a sample boundary continues in the next sample as a new document starting at position 0.

    To find a sample, the dataset keeps a prefix-sum index of the documents' token counts. The index
    is extended lazily: it tokenizes only as far as the requested ``idx`` needs (at most once through
    the file; beyond that the stream repeats with a known period), and only the documents a sample
    overlaps are tokenized again to produce it. Each DataLoader worker extends its own copy.
    """

    def __init__(self, parquet_file: str, tokenizer, sequence_length: int, training_samples: int):
        import pyarrow.parquet as pq

        self.parquet_ds = pq.read_table(parquet_file, memory_map=True)
        self.real_length = len(self.parquet_ds)
        if self.real_length == 0:
            raise ValueError(f"{parquet_file} has no rows")
        self.texts = self.parquet_ds.column("text")
        self.tokenizer = tokenizer
        self.eos = tokenizer.eos_token_id
        if self.eos is None:
            raise ValueError("--pack-sequences needs a tokenizer with an eos token")
        self.sequence_length = sequence_length
        self.training_samples = training_samples
        self._cum = [0]  # _cum[k] = tokens of documents 0 .. k-1 (first pass through the file)

    def __len__(self):
        return self.training_samples

    def _doc_tokens(self, k: int) -> List[int]:
        return list(self.tokenizer.encode(str(self.texts[k % self.real_length]))) + [self.eos]

    def _locate(self, pos: int) -> Tuple[int, int]:
        """(document index within the file, offset inside it) of stream position ``pos``."""
        while self._cum[-1] <= pos and len(self._cum) <= self.real_length:
            self._cum.append(self._cum[-1] + len(self._doc_tokens(len(self._cum) - 1)))
        if self._cum[-1] <= pos:  # the whole file is indexed: the stream repeats every _cum[-1] tokens
            pos %= self._cum[-1]
        j = bisect.bisect_right(self._cum, pos) - 1
        return j, pos - self._cum[j]

    def __getitem__(self, idx: int):
        n = self.sequence_length + 1
        j, off = self._locate(int(idx) * n)
        ids: List[int] = []
        lengths: List[int] = []
        while len(ids) < n:
            toks = self._doc_tokens(j)[off:]
            ids.extend(toks)
            lengths.append(len(toks))
            j, off = j + 1, 0
        return {"input_ids": ids[:n], "doc_start": _doc_start_from_lengths(lengths, n)}


class SyntheticTokenDataset(Dataset):
    """Deterministic random token rows of length sequence_length + 1 (no pad tokens).

    ``doc_len_range=(lo, hi)`` (``--synthetic-data --pack-sequences``) also cuts each row into
    documents of lengths drawn uniformly from [lo, hi], a function of ``(seed, idx)`` only, and adds
    their ``doc_start`` (see :class:`PackedParquetDataset`); the tokens are the same with or without it."""

    def __init__(self, vocab_size: int, sequence_length: int, training_samples: int, seed: int = 0,
                 pad_token_id: int = 0, doc_len_range: Optional[Tuple[int, int]] = None):
        self.vocab_size = vocab_size
        self.sequence_length = sequence_length
        self.training_samples = training_samples
        self.seed = seed
        self.pad_token_id = pad_token_id
        if doc_len_range is not None and not 1 <= doc_len_range[0] <= doc_len_range[1]:
            raise ValueError(f"doc_len_range must be 1 <= lo <= hi, got {doc_len_range}")
        self.doc_len_range = doc_len_range

    def __len__(self):
        return self.training_samples

    def __getitem__(self, idx: int):
        rng = np.random.default_rng([self.seed, int(idx)])
        lo = 1 if self.pad_token_id == 0 else 0
        ids = rng.integers(lo, self.vocab_size, size=self.sequence_length + 1, dtype=np.int64)
        if self.pad_token_id != 0:
            ids[ids == self.pad_token_id] = (self.pad_token_id + 1) % self.vocab_size
        if self.doc_len_range is None:
            return {"input_ids": ids.tolist()}
        n = self.sequence_length + 1
        lo, hi = self.doc_len_range
        lens = np.random.default_rng([self.seed, int(idx), 1]).integers(lo, hi + 1, size=n // lo + 1)
        return {"input_ids": ids.tolist(), "doc_start": _doc_start_from_lengths(lens.tolist(), n)}


@dataclass
class CollatorForCLM:
    sequence_length: int
    pad_token_id: int

    def __call__(self, examples: List[Dict[str, List[int]]]):
        input_ids = torch.as_tensor(np.asarray([e["input_ids"] for e in examples], dtype=np.int64))
        inputs = input_ids[:, :-1].clone()
        labels = input_ids[:, 1:].clone()
        labels[labels == self.pad_token_id] = -100
        assert inputs.shape[1] == labels.shape[1] == self.sequence_length
        assert inputs.shape == labels.shape
        return inputs, labels


@dataclass
class CollatorForPackedCLM:
    """``(inputs, labels, doc_start)`` of packed samples (``input_ids`` and ``doc_start`` of length
    S + 1). ``doc_start`` is int32 [B, S]. The label of a document's last position is -100: its next
    token belongs to another document. Packed rows hold no padding, so no label is masked for being
    the pad token (eos, which many tokenizers also use as pad, is a real target)."""

    sequence_length: int
    pad_token_id: int

    def __call__(self, examples: List[Dict[str, List[int]]]):
        input_ids = torch.as_tensor(np.asarray([e["input_ids"] for e in examples], dtype=np.int64))
        ds = torch.as_tensor(np.asarray([e["doc_start"] for e in examples], dtype=np.int32))
        inputs = input_ids[:, :-1].clone()
        labels = input_ids[:, 1:].clone()
        S = self.sequence_length
        assert inputs.shape[1] == S and ds.shape == input_ids.shape
        starts_doc = ds[:, 1:] == torch.arange(1, S + 1, dtype=torch.int32)  # the next token opens a document
        labels[starts_doc] = -100
        return inputs, labels, ds[:, :-1].contiguous()


_WORDS = ("the of and to in is was for on that with as by at from his her an were are which this be "
          "or has had not but one all their they it its been more also who would two new first after "
          "time may other some these only such when than most into over many both then use while where "
          "state city year world during later known under since made part between work").split()


def make_synthetic_parquet(path: str, n_docs: int = 256, min_words: int = 50, max_words: int = 2000,
                           seed: int = 0) -> str:
    """Write a parquet file with a ``text`` column of random word sequences."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    rnd = random.Random(seed)
    texts = [" ".join(rnd.choice(_WORDS) for _ in range(rnd.randint(min_words, max_words))) for _ in range(n_docs)]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    pq.write_table(pa.table({"text": texts}), path)
    return path

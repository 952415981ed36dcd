"""``generate.py`` command line: sample from a checkpoint written by ``train.py``.

    python generate.py --checkpoint-dir checkpoints/ --model-preset llama2-7b --sequence-length 2048 \
        --prompt "Once upon a time" --max-new-tokens 64 --temperature 0.8 --top-p 0.95 --output-jsonl out.jsonl \
        [--sampler philox --decode-graph] [--kv-cache-dtype fp8] [--prefill-chunk 512]

The model flags (``--model-preset``, ``--n-layers``, ``--vocab-size``, ``--sequence-length``,
``--model-dtype``, ``--tokenizer-name-or-path``) and the checkpoint flags (``--checkpoint-dir``,
``--resume-from-checkpoint``, ``--use-torch-distributed-ckpt``, ``--verify-checkpoints``) carry the names
and defaults of ``train.py`` and must describe the run that wrote the checkpoint. Only the parameters
are read (:func:`pyrecover_amd.ckpt.model_only.load_model_only`); generation runs on the KV-cache path of
:mod:`pyrecover_amd.inference`.
"""
from __future__ import annotations

import argparse
import json
import logging
import sys
from typing import List

import torch

from .ckpt.model_only import load_model_only
from .cli import PRECISION_STR_TO_DTYPE, build_parser as train_parser, set_default_dtype
from .config import get_preset
from .data.tokenizer import load_tokenizer
from .inference import KV_DTYPES, generate
from .models.llama import Transformer

logger = logging.getLogger("pyrecover")

_SHARED = ("checkpoint_dir", "resume_from_checkpoint", "use_torch_distributed_ckpt", "verify_checkpoints",
           "model_preset", "n_layers", "vocab_size", "sequence_length", "model_dtype", "tokenizer_name_or_path",
           "seed")


def _token_list(v: str) -> List[int]:
    try:
        ids = [int(x) for x in v.split(",") if x.strip() != ""]
    except ValueError:
        ids = []
    if not ids or min(ids) < 0:
        raise argparse.ArgumentTypeError(f"{v!r}: expected a comma list of token ids, e.g. 1,2,3")
    return ids


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="pyrecover_amd generation from a train.py checkpoint (KV cache, "
                                            "HIP decode attention)")
    shared = {a.dest: a for a in train_parser()._actions}
    for dest in _SHARED:  # same spellings, types, defaults and help as train.py
        a = shared[dest]
        kw = {"dest": a.dest, "default": a.default, "help": a.help}
        if isinstance(a, argparse._StoreTrueAction):
            kw["action"] = "store_true"
        else:
            kw.update(type=a.type, choices=a.choices)
        p.add_argument(*a.option_strings, **kw)
    p.add_argument("--prompt", action="append", default=[], metavar="TEXT", help="a text prompt (repeatable)")
    p.add_argument("--prompt-tokens", action="append", default=[], type=_token_list, metavar="1,2,3",
                   help="a prompt as token ids (repeatable)")
    p.add_argument("--max-new-tokens", type=int, default=32)
    p.add_argument("--temperature", type=float, default=0.0, help="0: greedy (ties to the lowest token id)")
    p.add_argument("--top-k", type=int, default=0, help="0: off")
    p.add_argument("--top-p", type=float, default=1.0, help="1: off")
    p.add_argument("--sampler", choices=("torch", "philox"), default="torch",
                   help="torch: torch.multinomial with a seeded generator. philox: the stateless rule of "
                        "csrc/kernels/sample.hip, a draw is a function of (seed, prompt, position); one kernel "
                        "launch per token on a bf16 / fp16 GPU model")
    p.add_argument("--decode-graph", action="store_true",
                   help="replay sample + decode step as one hipGraph per token (needs --sampler philox or "
                        "--temperature 0, and a bf16 / fp16 GPU model)")
    p.add_argument("--kv-cache-dtype", choices=KV_DTYPES, default="model",
                   help="model: the cache holds k / v in the model's dtype. fp8: e4m3fn bytes with one "
                        "power-of-two scale per (token, kv head), about half the cache memory; the prompt's "
                        "attention stays unquantized, so the first generated token does not change")
    p.add_argument("--prefill-chunk", type=int, default=0, metavar="N",
                   help="feed the prompt through in pieces of N tokens, each appended to the cache so far "
                        "(csrc/kernels/attention_extend.hip): the prefill's activation memory scales with N, not "
                        "with the prompt. 0 (default): one pass over the whole prompt. Not with --kv-cache-dtype fp8")
    p.add_argument("--no-kv-cache", action="store_true",
                   help="naive path: a full forward over the whole prefix per new token (debugging aid)")
    p.add_argument("--output-jsonl", type=str, default=None,
                   help="write one JSON line per prompt: prompt ids, generated ids, text, finish reason, prefill "
                        "and per-token decode milliseconds")
    return p


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if not args.prompt and not args.prompt_tokens:
        raise SystemExit("generate.py: give at least one --prompt or --prompt-tokens")
    device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    tokenizer = load_tokenizer(args.tokenizer_name_or_path) if args.prompt else None
    preset = get_preset(args.model_preset)
    vocab = args.vocab_size or (tokenizer.vocab_size if tokenizer is not None else preset.vocab_size)
    cfg = get_preset(args.model_preset, seq_len=args.sequence_length, vocab_size=vocab, n_layers=args.n_layers)
    with set_default_dtype(PRECISION_STR_TO_DTYPE[args.model_dtype]), torch.device(device):
        model = Transformer(cfg)
    model.eval()
    step = load_model_only(model, args.checkpoint_dir, args.resume_from_checkpoint or "latest",
                           distributed=args.use_torch_distributed_ckpt, verify=args.verify_checkpoints)
    model.flatten_(shadows=False)  # fused QKV / W1|W3 weights as views of one buffer, no transposed copies

    prompts = [tokenizer.encode(t) if hasattr(tokenizer, "encode") else tokenizer(t)["input_ids"]
               for t in args.prompt] + list(args.prompt_tokens)
    bad = [t for p in prompts for t in p if t >= vocab]
    if bad:
        raise SystemExit(f"generate.py: prompt token ids {bad[:5]} are outside the vocabulary ({vocab})")
    eos = getattr(tokenizer, "eos_token_id", None)  # text prompts stop at the tokenizer's end-of-sequence id
    stats = {}
    tokens, reasons = generate(model, prompts, args.max_new_tokens, temperature=args.temperature, top_k=args.top_k,
                               top_p=args.top_p, seed=args.seed, eos_id=eos, use_cache=not args.no_kv_cache,
                               stats=stats, sampler=args.sampler, graph=args.decode_graph,
                               kv_cache_dtype=args.kv_cache_dtype, prefill_chunk=args.prefill_chunk)
    records = []
    for p, ids, why in zip(prompts, tokens, reasons):
        text = tokenizer.decode(ids) if tokenizer is not None else None
        records.append({"prompt_ids": list(p), "generated_ids": ids, "text": text, "finish_reason": why,
                        "prefill_ms": stats["prefill_ms"], "decode_ms_per_token": stats["decode_ms_per_token"],
                        "checkpoint_step": step, "sampler": args.sampler, "decode_graph": args.decode_graph,
                        "kv_cache_dtype": args.kv_cache_dtype, "prefill_chunks": stats["prefill_chunks"]})
        logger.info(f"[{why}] {ids if text is None else text!r}")
    if args.output_jsonl:
        with open(args.output_jsonl, "w", encoding="utf-8") as f:
            for r in records:
                f.write(json.dumps(r) + "\n")
    else:
        for r in records:
            sys.stdout.write(json.dumps(r) + "\n")
    return 0

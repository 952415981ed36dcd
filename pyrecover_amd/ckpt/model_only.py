"""Load only the parameters of a checkpoint (inference: ``generate.py``).

A training checkpoint is mostly optimizer state (at 7B the AdamW moments are 25 of the 37.65 GiB).
:func:`load_model_only` reads the ``model.*`` entries alone, of a vanilla archive or a sharded
directory, needs no optimizer and never allocates or reads a moment:

* vanilla: the archive is memory-mapped (``torch.load(mmap=True)``), so only the pages of the tensors
  that are copied into the model are ever read from the file;
* sharded: the metadata lists every entry; everything outside ``model.`` is passed to
  :func:`pyrecover_amd.ckpt.sharded.read_sharded_state` as ``skip`` and is not opened.

The training loaders (``load_ckpt_vanilla`` / ``load_ckpt_distributed``) are untouched.
"""
from __future__ import annotations

import logging
from pathlib import Path
from typing import Any, Dict, Tuple

import torch

from . import core, sharded
from .vanilla import verify_checkpoint

logger = logging.getLogger("pyrecover")


def resolve_checkpoint(checkpoint_dir: str, which: str = "latest", distributed: bool = False) -> str:
    """``which``: "latest" (newest under ``checkpoint_dir``, searched recursively for vanilla archives),
    a path, or a name relative to ``checkpoint_dir``."""
    if which == "latest":
        base = Path(checkpoint_dir)
        path = core.get_latest_checkpoint(str(base), distributed=distributed)
        if path is None and distributed:  # checkpoint_dir/<experiment>/ckpt_*
            found = [p for d in sorted(base.glob("*")) if d.is_dir()
                     for p in [core.get_latest_checkpoint(str(d), distributed=True)] if p is not None]
            found.sort(key=lambda p: (Path(p).stat().st_mtime, core.ckpt_step(Path(p))))
            path = found[-1] if found else None
        if path is None:
            raise RuntimeError(f"No checkpoint found in {checkpoint_dir}")
        return path
    p = Path(which)
    if not p.exists() and (Path(checkpoint_dir) / which).exists():
        p = Path(checkpoint_dir) / which
    if not p.exists():
        raise RuntimeError(f"checkpoint {which} not found")
    return str(p)


def read_model_state(path: str, distributed: bool = False) -> Tuple[Dict[str, Any], int]:
    """(model state dict with unprefixed keys, step) of the checkpoint at ``path``."""
    if distributed:
        md = sharded.read_metadata(path)
        keys = [idx.fqn for idx in md.storage_data]
        skip = {k for k in keys if not (k.startswith("model.") or k.startswith("metadata."))}
        st = sharded.read_sharded_state(path, skip=skip)
        return core.strip_prefixes(st.get("model", {})), int(st.get("metadata", {}).get("step", 0) or 0)
    ckpt = torch.load(path, map_location="cpu", mmap=True, weights_only=True)
    return core.strip_prefixes(ckpt["model"]), int(ckpt.get("step", 0) or 0)


def load_model_only(model, checkpoint_dir: str, which: str = "latest", distributed: bool = False,
                    verify: bool = False) -> int:
    """Restore ``model``'s parameters from a checkpoint under ``checkpoint_dir`` and return its step.

    ``distributed``: the checkpoint is a sharded directory (train.py --use-torch-distributed-ckpt).
    ``verify``: check a vanilla archive against its ``.md5`` sidecar first (this reads the whole file;
    sharded directories carry no whole-checkpoint digest)."""
    core.wait_all()
    if distributed:
        sharded.finalize_pending()
    path = resolve_checkpoint(checkpoint_dir, which, distributed)
    if verify and not distributed:
        ok, err = verify_checkpoint(path)
        if not ok:
            raise RuntimeError(err)
    sd, step = read_model_state(path, distributed)
    m = core.unwrap(model)
    with torch.no_grad():
        missing, unexpected = m.load_state_dict(sd, strict=False)
    if missing or unexpected:
        raise RuntimeError(f"checkpoint/model key mismatch: missing={missing[:5]} unexpected={unexpected[:5]}")
    logger.info(f"Model parameters loaded from {path} (step {step})")
    return step

#!/usr/bin/env python
"""Sample from a checkpoint written by ``train.py`` (KV cache + HIP decode attention; see ``--help``).

    python generate.py --checkpoint-dir checkpoints/ --model-preset llama2-7b --prompt "Once upon a time" \
        --max-new-tokens 64 --temperature 0.8 --top-p 0.95 --output-jsonl out.jsonl
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pyrecover_amd.cli import init_logger  # noqa: E402
from pyrecover_amd.generate import main  # noqa: E402

if __name__ == "__main__":
    init_logger()
    sys.exit(main())

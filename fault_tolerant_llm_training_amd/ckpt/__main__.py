"""``python -m fault_tolerant_llm_training_amd.ckpt verify FILE...``

Checks each checkpoint's flat state storages against the digests its writer recorded
(:mod:`.verify`), on the CPU and from the file alone: no model, no GPU. Exit status 0 if every
file matches, 1 if a buffer does not, 2 if a file carries no digest record (and none mismatched).
"""
from __future__ import annotations

import argparse
import sys

from .verify import verify_file


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m fault_tolerant_llm_training_amd.ckpt")
    sub = ap.add_subparsers(dest="cmd", required=True)
    v = sub.add_parser("verify", help="compare the state storages of checkpoints with their digest records")
    v.add_argument("files", nargs="+", metavar="FILE")
    a = ap.parse_args(argv)
    worst = 0
    for path in a.files:
        try:
            st = verify_file(path)
        except OSError as e:
            print(f"{path}: {e}")
            st = 1
        # a mismatch (1) outranks a missing record (2)
        worst = st if worst == 0 else (1 if 1 in (worst, st) else worst)
    return worst


if __name__ == "__main__":
    sys.exit(main())

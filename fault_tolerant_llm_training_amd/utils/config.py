"""Command-line surface.

The 16 reference flags are kept byte-for-byte (names, types, defaults, help):
reference ``utils.py:112-203`` (table in SURVEY.md §2.6). Everything after the
``# --- additive flags ---`` marker is new and defaults to the reference's
behaviour.
"""
from __future__ import annotations

import argparse
import os

import torch

PRECISION_STR_TO_DTYPE = {
    "fp16": torch.float16,
    "bf16": torch.bfloat16,
    "fp32": torch.float32,
    "fp64": torch.float64,
}


def workdir() -> str:
    """``$WORKDIR`` (reference ``utils.py:11``)."""
    return os.getenv("WORKDIR", "")


def jobid() -> str | None:
    """``$SLURM_JOB_ID`` (reference ``utils.py:12``; read at call time, not import time)."""
    return os.environ.get("SLURM_JOB_ID")


def build_parser() -> argparse.ArgumentParser:
    wd = workdir()
    parser = argparse.ArgumentParser()
    parser.add_argument(
        "--dataset",
        type=str,
        default="/capstor/store/cscs/ethz/large-sc/datasets/train_data.parquet",
        help="Path to a parquet file containing a 'text' column with documents (`str`)",
    )
    parser.add_argument(
        "--checkpoint-path",
        type=str,
        default=f"{wd}/checkpoints",
        help="Path to a checkpoint file to save the model and optimizer state dicts",
    )
    parser.add_argument(
        "--checkpoint-id",
        type=str,
        default="",
        help="Path to a checkpoint file to save the model and optimizer state dicts",
    )
    parser.add_argument(
        "--tokenizer-name-or-path",
        type=str,
        default="unsloth/Mistral-Nemo-Base-2407-bnb-4bit",
        help="A path to a directory containing vocabulary files required by the tokenizer or the model id of a predefined tokenizer hosted inside a model repo on the Hugging Face Hub.",
    )
    parser.add_argument("--sequence-length", type=int, default=4096)
    parser.add_argument("--batch-size", type=int, default=1)
    parser.add_argument(
        "--fused-optimizer",
        action="store_true",
        help="Set to fuse the optimizer for increased performance or not",
    )
    parser.add_argument("--learning-rate", type=float, default=1e-5)
    parser.add_argument("--lr-warmup-steps", type=int, default=10)
    parser.add_argument("--training-steps", type=int, default=1000)
    parser.add_argument(
        "--logging-frequency", type=int, default=5, help="Log every `--logging-frequency` steps"
    )
    parser.add_argument("--grad-max-norm", type=float, default=1)
    parser.add_argument(
        "--model-dtype",
        type=str,
        default="bf16",
        help="Model dtype for parameters, gradients and optimizer states. Default: bf16",
    )
    parser.add_argument(
        "--compile", action="store_true", help="Set to compile the model with `torch.compile`"
    )
    parser.add_argument(
        "--raise-error",
        action="store_true",
        help="Set to raise an error in the training loop at the error_step parameter",
    )
    parser.add_argument(
        "--error-step",
        type=int,
        default=100,
        help="Step at which to raise an error if --raise-error is set",
    )
    # --- additive flags (not in the reference; defaults keep its behaviour) ---
    parser.add_argument(
        "--model",
        type=str,
        default="llama3-8b",
        help="Architecture preset: llama3-8b (reference train.py:43-53), gpt2-small, gpt2-medium, tiny",
    )
    parser.add_argument(
        "--vocab-size",
        type=int,
        default=0,
        help="Override the vocabulary size (0: tokenizer's, or 131072 with --synthetic-data)",
    )
    parser.add_argument(
        "--synthetic-data",
        action="store_true",
        help="Deterministic synthetic token stream instead of parquet+tokenizer (offline boxes)",
    )
    parser.add_argument(
        "--iterable-dataset",
        action="store_true",
        help="Use the packing IterableParquetDataset (resumable mid-shard) instead of ParquetDataset",
    )
    parser.add_argument("--seed", type=int, default=1234, help="RNG seed for init and data")
    parser.add_argument(
        "--state-digest",
        action="store_true",
        help="At 'Training completed', log bit-level digests of the parameters, AdamW moments and "
        "data-loader position (resume-equivalence checks without a second checkpoint on disk)",
    )
    parser.add_argument(
        "--device", type=str, default="cuda", choices=["cuda", "cpu"], help="Run on GPU (default) or CPU"
    )
    parser.add_argument(
        "--save-every",
        type=int,
        default=-1,
        help="Periodic asynchronous checkpoint every N steps (0 disables; default: 200 under data "
        "parallelism, so a lost rank costs at most that many steps, else 0)",
    )
    parser.add_argument(
        "--no-async-checkpoint",
        action="store_true",
        help="Block the training loop until each periodic checkpoint is durable",
    )
    parser.add_argument(
        "--checkpoint-mode",
        type=str,
        default="auto",
        choices=["auto", "hbm", "host"],
        help="Snapshot path: hbm = D2D copy into reserved HBM then background D2H; host = D2H "
        "straight into pinned host memory; auto = hbm when free HBM allows",
    )
    parser.add_argument(
        "--checkpoint-alt-path",
        type=str,
        default="",
        help="A second checkpoint directory (another filesystem): a job that resumed from a file in one "
        "of the two directories writes its own checkpoints to the other, so the file it resumed from "
        "stays intact until its own is durable (a disk with room for ONE checkpoint, e.g. the 48 GB 8B "
        "file on 79 GB). --checkpoint-id is looked up in both",
    )
    parser.add_argument(
        "--prune-consumed",
        action="store_true",
        help="Delete the checkpoint this job resumed from once this job's own checkpoint is durable "
        "(periodic or exit save): the chain keeps at least one complete checkpoint at every moment",
    )
    parser.add_argument(
        "--no-checkpoint-prealloc",
        action="store_true",
        help="Pin the checkpoint host buffers at the first save instead of in a background thread at startup",
    )
    parser.add_argument(
        "--no-checkpoint-digest",
        action="store_true",
        help="Write checkpoints without the state_digest record (the per-buffer digests a resume and "
        "`python -m fault_tolerant_llm_training_amd.ckpt verify` check the state against)",
    )
    parser.add_argument(
        "--no-verify-checkpoint",
        action="store_true",
        help="On resume, do not compare the restored parameters and AdamW moments with the digests "
        "recorded in the checkpoint (by default a mismatch stops the job before it trains)",
    )
    parser.add_argument(
        "--checkpoint-writer-threads", type=int, default=8, help="Parallel pwrite threads of the checkpoint writer"
    )
    parser.add_argument(
        "--prefetch", type=int, default=2, help="Batches prepared ahead by the data-loader thread (0: inline)"
    )
    parser.add_argument(
        "--optimizer-state-dtype",
        type=str,
        default="",
        help="AdamW moment dtype (bf16/fp16/fp32); default = --model-dtype like the reference (fp32 for fp16 models: fp16 moments underflow)",
    )
    parser.add_argument(
        "--dp-bucket-mb",
        type=float,
        default=None,
        help="Gradient bucket size in MiB: the all-reduce / reduce-scatter unit under data parallelism "
             "(default 256) and the optimizer's launch / gating unit on one GPU (default 64)",
    )
    parser.add_argument(
        "--dp-mode",
        type=str,
        default="",
        choices=["", "allreduce", "zero1"],
        help="Data-parallel gradient mode (default zero1: reduce-scatter + sharded AdamW + all-gather)",
    )
    parser.add_argument(
        "--dp-reduce-dtype",
        type=str,
        default="native",
        choices=["native", "fp32"],
        help="Data-parallel gradient reduction dtype: native (the gradient dtype, bf16 by default; the "
        "error bound is in docs/PERFORMANCE.md) or fp32 (reduce an fp32 copy of each bucket: 2x the "
        "bytes on the links, one rounding)",
    )
    parser.add_argument(
        "--grad-accum",
        type=int,
        default=1,
        help="Gradient accumulation: micro-batches of --batch-size per optimizer step (collectives only "
        "in the last micro-batch's backward)",
    )
    parser.add_argument(
        "--hip-graph",
        action="store_true",
        help="Replay each step (optimizer of the previous step + forward/backward) as one HIP graph; "
        "1 GPU, no gradient accumulation. For launch-bound small models (gpt2-small: -18%% step time)",
    )
    parser.add_argument(
        "--peer-timeout",
        type=float,
        default=60.0,
        help="Seconds a rank waits at the per-step vote for a silent peer before declaring it lost "
        "(a dead peer is detected at once); well under Slurm's 120 s USR1 lead",
    )
    parser.add_argument(
        "--flash-bwd",
        type=str,
        default="deterministic",
        choices=["deterministic", "atomic"],
        help="Flash-attention backward: atomic-free dQ kernel (bit-reproducible, default) or fp32 atomics",
    )
    parser.add_argument(
        "--activation-checkpointing",
        type=int,
        default=0,
        help="Recompute this many transformer blocks (from the first; -1 = all) in backward instead of "
        "storing their activations (long sequences / larger batches per GPU)",
    )
    parser.add_argument(
        "--recompute-attention",
        action="store_true",
        help="With --activation-checkpointing: also re-run the flash-attention forward in backward "
        "(default keeps each recomputed block's attention output: one T x Hq x D tensor per block)",
    )
    parser.add_argument(
        "--document-mask",
        action="store_true",
        help="Attention within each packed document only: every BOS token (the tokenizer's id, 1 if it has "
        "none) starts a document and a token attends from its document's BOS up to itself (default: plain "
        "causal attention across the whole sample, as the reference)",
    )
    parser.add_argument(
        "--stochastic-rounding",
        action="store_true",
        help="AdamW stores its bf16 parameters and moments with stochastic rounding instead of "
        "round-to-nearest, so updates below half a bf16 spacing accumulate in expectation instead of "
        "being dropped. The random bits are a pure function of (--seed key, optimizer step, buffer, flat "
        "element index): a resume and every data-parallel mode stay bit-reproducible. "
        "bf16 parameters only (--model-dtype bf16); not with --hip-graph / --compile",
    )
    parser.add_argument(
        "--eval-every",
        type=int,
        default=0,
        help="Held-out evaluation every N steps (at each step boundary with training_step %% N == 0 and "
        "training_step > 0) and once more after the last step: a forward-only pass over a fixed set that "
        "leaves the training state untouched bit for bit (0: off). Needs --eval-dataset unless "
        "--synthetic-data",
    )
    parser.add_argument(
        "--eval-sequences",
        type=int,
        default=32,
        help="Size of the fixed evaluation set, in sequences of --sequence-length (default 32); a multiple "
        "of --batch-size: the set runs as micro-batches of --batch-size sequences, micro-batch i on rank "
        "i %% world size",
    )
    parser.add_argument(
        "--eval-dataset",
        type=str,
        default="",
        help="Parquet file or directory of the held-out set, read from its beginning with the same kind of "
        "dataset as training (map-style, or the packing dataset under --iterable-dataset). Optional with "
        "--synthetic-data: the set is then a synthetic stream whose seed the training stream never uses",
    )
    parser.add_argument(
        "--tensor-stats-every",
        type=int,
        default=0,
        help="Per-parameter statistics every N steps (at each step boundary with training_step %% N == 0 and "
        "training_step > 0, the final one included; never at the first boundary of a process, where no "
        "backward has run): sum of squares, absmax, non-finite count and zero count of every parameter's "
        "weights, gradient (of the step just taken, unclipped), exp_avg and exp_avg_sq, one read-only pass per "
        "flat buffer; one log line, and one JSON line in --metrics-file. A non-finite stop then also names "
        "the parameters whose gradient holds NaN / Inf (0: off)",
    )
    parser.add_argument(
        "--sample-every",
        type=int,
        default=0,
        help="Generate a text sample every N steps (at each step boundary with training_step %% N == 0 and "
        "training_step > 0) and once more after the last step, after a periodic save, an evaluation and the "
        "tensor statistics: rank 0 alone decodes --sample-tokens tokens from --sample-prompt with the KV-cache "
        "kernels; a read-only pass that leaves the training state untouched bit for bit (0: off). The other "
        "ranks wait in the next vote, so a sample has to stay far below --peer-timeout",
    )
    parser.add_argument(
        "--sample-prompt",
        type=str,
        default=None,
        help="Prompt of --sample-every (default: the BOS token alone); needs the tokenizer, so not with "
        "--synthetic-data",
    )
    parser.add_argument(
        "--sample-tokens",
        type=int,
        default=64,
        help="Tokens generated per sample (1 .. 1024; prompt + tokens may not exceed --sequence-length)",
    )
    parser.add_argument(
        "--sample-temperature",
        type=float,
        default=0.0,
        help="Sampling temperature of --sample-every (0: greedy). The sampler is stateless: its key comes from "
        "--seed and its step is the training step, so a resumed chain prints the sample an uninterrupted run prints",
    )
    parser.add_argument("--sample-top-k", type=int, default=0, help="Top-k of --sample-every (0: all tokens)")
    parser.add_argument(
        "--sample-top-p",
        type=float,
        default=1.0,
        help="Top-p (nucleus) of --sample-every, in (0, 1]: after top-k, only the most probable tokens whose "
        "probabilities add up to P are drawn from (1: off). No effect on greedy samples",
    )
    parser.add_argument(
        "--sample-count",
        type=int,
        default=1,
        help="Samples per --sample-every boundary (1 .. 16). Above 1, rank 0 decodes N copies of --sample-prompt "
        "in one batch with the multi-row decode kernels (one pass over the weights per token for all of them): "
        "sample 0 is the sample of --sample-count 1, the others are further draws, so use a --sample-temperature "
        "above 0 (greedy copies are identical)",
    )
    parser.add_argument(
        "--sample-graph",
        action="store_true",
        help="Decode the samples of --sample-every by replaying one captured HIP graph per token "
        "(generation.DecodeGraph) instead of launching every kernel from Python: the trainer captures it once, at "
        "the first sample, sized from --sample-count, the prompt and --sample-tokens, and reuses it at every "
        "boundary. The sample lines and records are those of a run without the flag and the training state stays "
        "bit-identical; independent of --hip-graph. Needs --device cuda, a bf16/fp16/fp32 model and a vocabulary that is a "
        "multiple of 8 (elsewhere the samples are decoded eagerly)",
    )
    parser.add_argument(
        "--ema-decay",
        type=float,
        default=0.0,
        help="Keep an exponential moving average of the parameters with this decay per optimizer step "
        "(0: off; otherwise 0 < D < 1, e.g. 0.999): an fp32 flat buffer updated behind each AdamW launch, "
        "sharded under ZeRO-1, saved in the checkpoint as the `ema` entry with a digest. Read-only to "
        "training: parameters, moments and losses are bit-identical to a run without the flag",
    )
    parser.add_argument(
        "--ema-every",
        type=int,
        default=1,
        help="Update the average every K optimizer steps (steps K, 2K, ...) with decay D ** K (default 1). "
        "K > 1 not with --hip-graph / --compile: the captured launch would run at every replay",
    )
    parser.add_argument(
        "--eval-ema",
        action="store_true",
        help="Run each --eval-every evaluation a second time on the averaged weights; its loss, perplexity and "
        "accuracy are added to the same record as ema_* fields. Needs --eval-every and --ema-decay",
    )
    parser.add_argument(
        "--sample-ema",
        action="store_true",
        help="Generate the --sample-every samples from the averaged weights (same sampler key and step). "
        "Needs --sample-every and --ema-decay",
    )
    parser.add_argument(
        "--profile-steps",
        type=str,
        default="",
        help="torch.profiler window 'START:STOP' (steps); Chrome trace written to --profile-dir",
    )
    parser.add_argument("--profile-dir", type=str, default="profiles/torch", help="Output dir for --profile-steps")
    parser.add_argument(
        "--metrics-file", type=str, default="", help="Append per-step JSON metrics to this file"
    )
    parser.add_argument(
        "--sbatch-script",
        type=str,
        default="",
        help="Job script resubmitted on SIGUSR1 (default: $WORKDIR/train.sh)",
    )
    return parser


def get_args(argv=None) -> argparse.Namespace:
    """Parse flags (reference ``utils.py:112-203``)."""
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.stochastic_rounding and args.model_dtype != "bf16":
        parser.error(f"--stochastic-rounding supports bf16 parameters only (--model-dtype bf16), "
                     f"got --model-dtype {args.model_dtype}")
    if args.stochastic_rounding and (args.hip_graph or args.compile):
        parser.error("--stochastic-rounding is not supported under whole-step graph replay "
                     "(--hip-graph / --compile): run the step eagerly")
    if not (args.ema_decay == 0.0 or 0.0 < args.ema_decay < 1.0):
        parser.error(f"--ema-decay must be 0 (off) or in (0, 1), got {args.ema_decay}")
    if args.ema_every < 1:
        parser.error(f"--ema-every must be >= 1, got {args.ema_every}")
    if args.ema_every > 1 and args.ema_decay == 0.0:
        parser.error("--ema-every needs --ema-decay")
    if args.ema_decay > 0 and args.ema_every > 1 and (args.hip_graph or args.compile):
        parser.error("--ema-every above 1 is not supported under whole-step graph replay (--hip-graph / "
                     "--compile): the captured update would run at every replay; use --ema-every 1")
    if args.eval_ema and not (args.eval_every > 0 and args.ema_decay > 0):
        parser.error("--eval-ema needs --eval-every and --ema-decay")
    if args.sample_ema and not (args.sample_every > 0 and args.ema_decay > 0):
        parser.error("--sample-ema needs --sample-every and --ema-decay")
    if args.eval_every < 0:
        parser.error(f"--eval-every must be >= 0, got {args.eval_every}")
    if args.tensor_stats_every < 0:
        parser.error(f"--tensor-stats-every must be >= 0, got {args.tensor_stats_every}")
    if args.sample_every < 0:
        parser.error(f"--sample-every must be >= 0, got {args.sample_every}")
    if not 1 <= args.sample_count <= 16:
        parser.error(f"--sample-count must be in 1 .. 16, got {args.sample_count}")
    if args.sample_count > 1 and args.sample_every == 0:
        parser.error("--sample-count needs --sample-every")
    try:  # NaN and a value that rounds to 0 in float32 fail too
        from .sampling import check_top_p

        check_top_p(args.sample_top_p)
    except ValueError:
        parser.error(f"--sample-top-p must be in (0, 1], got {args.sample_top_p}")
    if args.sample_graph and args.sample_every == 0:
        parser.error("--sample-graph needs --sample-every")
    if args.sample_every > 0:
        if not 1 <= args.sample_tokens <= 1024:
            parser.error(f"--sample-tokens must be in 1 .. 1024, got {args.sample_tokens}")
        if args.sample_temperature < 0 or args.sample_top_k < 0:
            parser.error("--sample-temperature and --sample-top-k must be >= 0")
        if args.sample_prompt is not None and args.synthetic_data:
            parser.error("--sample-prompt needs the tokenizer: not with --synthetic-data (the default prompt, "
                         "the BOS token alone, needs none)")
        # a text prompt is counted in tokens once the tokenizer is loaded (trainer.py); the BOS-only
        # default is one token
        if 1 + args.sample_tokens > args.sequence_length:
            parser.error(f"--sample-every: prompt (1 token) + --sample-tokens ({args.sample_tokens}) exceed "
                         f"--sequence-length ({args.sequence_length})")
    if args.eval_every > 0:
        if not args.eval_dataset and not args.synthetic_data:
            parser.error("--eval-every needs a held-out set: give --eval-dataset (only --synthetic-data runs "
                         "can do without one)")
        if args.eval_sequences <= 0 or args.eval_sequences % args.batch_size:
            parser.error(f"--eval-sequences ({args.eval_sequences}) must be a positive multiple of "
                         f"--batch-size ({args.batch_size})")
    return args

"""``python -m fault_tolerant_llm_training_amd.generate``: text from a training checkpoint.

Loads only the ``model`` entry of the file (``ckpt.format.load_checkpoint`` maps the storages, so
the AdamW moments are never read) into a model of the given preset (``ckpt.state.restore_model``,
strict), generates with ``generation.generate`` and prints the decoded text; ``--json`` prints one
line with the prompt ids, the generated ids, the text, the seconds and the tokens per second.
A file that does not fit the model is reported as one error line and a non-zero exit code.

Several sequences at once: ``--num-samples N`` draws N samples of the prompt, ``--prompts-file`` reads
one prompt per line (``--prompt-ids-file``: comma-separated ids per line); with both, every prompt is
repeated N times. More than one row goes through ``generation.generate_batch`` (one pass over the
weights per token for all rows): ``--json`` then prints one line per row with a ``row`` field, the
text mode a line ``--- sample b ---`` before each row. One row without these flags prints what it
always printed.

``--use-ema`` reads the ``ema`` entry of a ``--ema-decay`` run instead of ``model``: the fp32 parameter
average, rounded to nearest in ``--model-dtype``.

``--decode-graph`` decodes with ``generation.DecodeGraph``: one captured HIP graph per token, replayed,
instead of about nine launches per layer issued from Python. The ids are the same.
"""
from __future__ import annotations

import argparse
import json
import sys
import time

import torch


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m fault_tolerant_llm_training_amd.generate", description=__doc__)
    p.add_argument("--checkpoint", type=str, required=True, help="Checkpoint file written by train.py")
    p.add_argument("--model", type=str, default="llama3-8b", help="Architecture preset, as in train.py")
    p.add_argument("--vocab-size", type=int, default=0,
                   help="Vocabulary size the model was trained with (0: the tokenizer's, as in train.py)")
    p.add_argument("--tokenizer-name-or-path", type=str, default="unsloth/Mistral-Nemo-Base-2407-bnb-4bit",
                   help="Tokenizer, as in train.py (`byte`: the built-in byte-level tokenizer)")
    p.add_argument("--model-dtype", type=str, default="bf16", help="Model dtype (bf16/fp16/fp32/fp64)")
    p.add_argument("--device", type=str, default="cuda", choices=["cuda", "cpu"])
    p.add_argument("--sequence-length", type=int, default=0,
                   help="Length of the RoPE tables and the longest prompt + generation (0: the checkpoint's)")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--prompt", type=str, default=None, help="Prompt text (needs the tokenizer)")
    g.add_argument("--prompt-ids", type=str, default=None, help="Prompt as comma-separated token ids, e.g. 1,2,3")
    g.add_argument("--prompts-file", type=str, default=None,
                   help="File with one prompt per line (text, or comma-separated ids with --prompt-ids-file)")
    p.add_argument("--prompt-ids-file", action="store_true", help="The lines of --prompts-file are token ids")
    p.add_argument("--num-samples", type=int, default=1,
                   help="Samples per prompt, generated as one batch (at most 64 rows in all); use a --temperature "
                   "above 0, greedy samples of one prompt are identical")
    p.add_argument("--max-new-tokens", type=int, default=64)
    p.add_argument("--temperature", type=float, default=0.0, help="0: greedy")
    p.add_argument("--top-k", type=int, default=0, help="0: all tokens")
    p.add_argument("--top-p", type=float, default=1.0,
                   help="Nucleus sampling, in (0, 1]: after --top-k, draw only from the most probable tokens whose "
                   "probabilities add up to P (1: off; no effect on greedy decoding)")
    p.add_argument("--seed", type=int, default=1234, help="Seed of the sampler key")
    p.add_argument("--sampler-step", type=int, default=0,
                   help="Step of the stateless sampler (default 0); train.py's --sample-every samples use the "
                   "training step, so the boundary's step reproduces its sample from that step's checkpoint")
    p.add_argument("--decode-graph", action="store_true",
                   help="Decode by replaying one captured HIP graph per token instead of launching every kernel "
                   "from Python (the same ids; GPU models of a kernel dtype with a vocabulary that is a multiple of 8, elsewhere ignored)")
    p.add_argument("--use-ema", action="store_true",
                   help="Generate from the file's `ema` entry (the parameter average of a --ema-decay run), rounded "
                   "to nearest in --model-dtype, instead of `model`; an error if the file has none")
    p.add_argument("--json", action="store_true", help="Print one JSON line instead of the text")
    return p


def _fail(msg: str) -> int:
    print(f"generate: error: {msg}", file=sys.stderr, flush=True)
    return 2


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from .ckpt.format import load_checkpoint
    from .ckpt.state import restore_model
    from .generation import MAX_BATCH, generate, generate_batch
    from .models.llama import PRESETS, build_model, model_args_for
    from .utils.config import PRECISION_STR_TO_DTYPE
    from .utils.sround import key_from_seed

    if args.model not in PRESETS:
        return _fail(f"unknown --model {args.model!r}; choose from {sorted(PRESETS)}")
    if args.model_dtype not in PRECISION_STR_TO_DTYPE:
        return _fail(f"unknown --model-dtype {args.model_dtype!r}")
    if args.max_new_tokens < 1 or args.temperature < 0 or args.top_k < 0:
        return _fail("--max-new-tokens must be >= 1, --temperature and --top-k >= 0")
    try:  # NaN and a value that rounds to 0 in float32 fail too
        from .utils.sampling import check_top_p

        check_top_p(args.top_p)
    except ValueError:
        return _fail(f"--top-p must be in (0, 1], got {args.top_p}")
    if args.num_samples < 1:
        return _fail("--num-samples must be >= 1")
    if args.prompt_ids_file and args.prompts_file is None:
        return _fail("--prompt-ids-file needs --prompts-file")
    lines = None
    if args.prompts_file is not None:
        try:
            with open(args.prompts_file) as f:
                lines = [ln.rstrip("\n") for ln in f if ln.strip()]
        except OSError as e:
            return _fail(f"cannot read {args.prompts_file}: {e!r}")
        if not lines:
            return _fail(f"{args.prompts_file} holds no prompt")
    ids_given = args.prompt_ids is not None or (lines is not None and args.prompt_ids_file)
    tok = None
    if not ids_given or not args.vocab_size:
        from .data.tokenizer import load_tokenizer

        try:
            tok = load_tokenizer(args.tokenizer_name_or_path)
        except Exception as e:  # noqa: BLE001 - reported as the one error line
            return _fail(f"cannot load the tokenizer {args.tokenizer_name_or_path!r} ({e!r}); "
                         "give --prompt-ids and --vocab-size to do without one")
    try:
        if lines is not None and args.prompt_ids_file:
            prompts = [[int(s) for s in ln.split(",") if s.strip()] for ln in lines]
        elif lines is not None:
            from .data.tokenizer import encode

            prompts = [encode(tok, ln) for ln in lines]
        if lines is not None:
            prompt = prompts[0]
        elif args.prompt_ids is not None:
            prompt = [int(s) for s in args.prompt_ids.split(",") if s.strip()]
        elif args.prompt is not None:
            from .data.tokenizer import encode

            prompt = encode(tok, args.prompt)
        else:
            bos = getattr(tok, "bos_token_id", None)
            prompt = [1 if bos is None else int(bos)]
    except ValueError as e:
        return _fail(f"--prompt-ids: {e}")
    if lines is None:
        prompts = [prompt]
    if not all(prompts):
        return _fail("the prompt is empty")
    prompts = [p for p in prompts for _ in range(args.num_samples)]
    if len(prompts) > MAX_BATCH:
        return _fail(f"{len(prompts)} rows (prompts x --num-samples) exceed the batch limit of {MAX_BATCH}")
    batched = lines is not None or args.num_samples > 1
    vocab = args.vocab_size or int(tok.vocab_size)
    try:
        ckpt = load_checkpoint(args.checkpoint)
    except Exception as e:  # noqa: BLE001
        return _fail(f"cannot read {args.checkpoint}: {e!r}")
    meta = ckpt.get("meta") or {}
    seq_len = args.sequence_length or int((meta.get("model_args") or {}).get("seq_len", 0)) or 2048
    device = torch.device(args.device)
    dtype = PRECISION_STR_TO_DTYPE[args.model_dtype]
    margs = model_args_for(args.model, vocab_size=vocab, seq_len=seq_len)
    rec = meta.get("model_args") or {}
    diff = [f"{f}: file {rec[f]!r}, --model {getattr(margs, f)!r}"
            for f in ("dim", "n_layers", "n_heads", "n_kv_heads", "multiple_of", "ffn_dim_multiplier", "norm_type",
                      "vocab_size") if f in rec and rec[f] != getattr(margs, f)]
    if diff:  # before anything is allocated for the wrong architecture
        return _fail(f"{args.checkpoint} does not fit --model {args.model} with vocabulary {vocab} ({'; '.join(diff)})")
    entry = "model"
    if args.use_ema:
        if not isinstance(ckpt.get("ema"), dict):
            return _fail(f"{args.checkpoint} has no ema entry (it was written without --ema-decay); "
                         "drop --use-ema to generate from its model entry")
        entry = "ema"  # fp32 tensors: restore_model's per-tensor copies round them to nearest in --model-dtype
    try:
        model = build_model(margs, device, dtype)
        restore_model(model, ckpt[entry])
    except Exception as e:  # noqa: BLE001 - a layout mismatch: keys, shapes or sizes
        return _fail(f"{args.checkpoint} does not fit --model {args.model} with vocabulary {vocab}: "
                     f"{type(e).__name__}: {str(e).splitlines()[0] if str(e) else ''}")
    del ckpt
    model.eval()
    eos = getattr(tok, "eos_token_id", None) if tok is not None else None
    if device.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        if batched:
            rows = generate_batch(model, prompts, args.max_new_tokens, temperature=args.temperature, top_k=args.top_k,
                                  key=key_from_seed(args.seed), eos_id=eos, step=args.sampler_step,
                                  graph=args.decode_graph, top_p=args.top_p)
        else:
            ids = generate(model, prompt, args.max_new_tokens, temperature=args.temperature, top_k=args.top_k,
                           key=key_from_seed(args.seed), eos_id=eos, step=args.sampler_step,
                           graph=args.decode_graph, top_p=args.top_p)
    except ValueError as e:
        return _fail(str(e))
    dt = time.perf_counter() - t0  # generate() returns host integers: the device work is finished
    if batched:
        total = sum(len(r) for r in rows)
        for b, (p, r) in enumerate(zip(prompts, rows)):
            text = tok.decode(r) if tok is not None else ""
            if args.json:  # seconds: the whole batch; tokens_per_s: all rows' tokens over it
                print(json.dumps({"row": b, "prompt_ids": p, "ids": r, "text": text, "seconds": dt,
                                  "tokens_per_s": total / dt if dt > 0 else 0.0}), flush=True)
            else:
                print(f"--- sample {b} ---", flush=True)
                print(text if tok is not None else ",".join(str(i) for i in r), flush=True)
        return 0
    text = tok.decode(ids) if tok is not None else ""
    if args.json:
        print(json.dumps({"prompt_ids": prompt, "ids": ids, "text": text, "seconds": dt,
                          "tokens_per_s": len(ids) / dt if dt > 0 else 0.0}), flush=True)
    else:
        print(text if tok is not None else ",".join(str(i) for i in ids), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

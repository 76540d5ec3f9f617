"""Text generation from the flat-buffer model: KV cache, prefill, one-token decode, sampling.

The reference has no generation path. Here the prompt runs once through the training forward
kernels (:func:`prefill`, which also fills the cache), then every new token costs one pass over the
weights with the one-row kernels of csrc/kernels/decode.hip (:func:`decode_step`): per layer
``norm`` / ``add_norm`` on one row, ``gemv`` for ``wqkv``, ``decode_qkv_append_`` (RoPE at the
token's position, K and V into the cache), ``decode_attn`` over the cache, ``gemv`` for ``wo``,
``add_norm``, ``gemv_swiglu`` on ``[w1; w3]``, ``gemv`` for ``w2``; then the final norm, the head
``gemv`` and the sampler. CPU tensors and fp64 models take the composed-PyTorch path of the same ops
(``ops/decode.py``): a cache of rotated K and V with the math of ``attention_reference``. That path
is the definition; tests compare it with ``Transformer.forward``.

Several sequences at once (:func:`generate_batch`): every prompt is prefilled on its own into its row
of a :class:`BatchKVCache`, then one :func:`decode_step_rows` per token serves all B rows with the
multi-row kernels (``gemv_rows``, ``gemv_swiglu_rows``, ``decode_qkv_append_rows_``,
``decode_attn_rows``), which read every weight once for up to 8 rows. Each of those returns for a row
the bits the one-row op returns for it alone, so a row's tokens do not depend on its batch: under
greedy decoding ``generate_batch(model, prompts, ...)[b] == generate(model, prompts[b], ...)``.

Generation always uses plain causal attention: a model with a document mask set generates one
continuing document. Everything runs under ``torch.no_grad()`` and writes nothing of the training
state (no gradient buffer, no sink, no optimizer state).

Sampling is stateless (``utils/sampling.py``): new token ``t`` of a call is drawn with the key
``token_key(key, t)`` and the sampler step ``step``, so a call is a pure function of
(parameters, prompt, temperature, top_k, key, step).

A pass issues about nine short launches per layer from Python. :class:`DecodeGraph` (``graph=True`` of
:func:`generate` / :func:`generate_batch`) captures one token -- sample, the pass of
:func:`decode_step_rows`, the head -- as one HIP graph and replays it, which removes the host's launch
cost. That cost is the bound only on small models (3x per token on the ``tiny`` preset); on Llama-3-8B
the GPU is the bound and the replay gains nothing (``profiles/generate_graph.md``), so the default is the
eager loop. Everything that changes from token to token lives in device memory: the sampled
token, each row's start position ``pos0`` and a control block ``ctl`` with the step counter ``t`` and
the sampling arguments, which the device-step ops of ``ops/decode.py`` read and a last one-thread
launch advances. The attention grid covers the cache's capacity, not the current key count, so the
captured launches are right for any token of any call that fits the capacity; the results are those
of the eager loop bit for bit.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import torch

from ._native import native
from .ops import decode as D
from .ops import functional as Fx
from .utils.sampling import token_key  # noqa: F401 - part of this module's interface


class KVCache:
    """Rotated K and V of the tokens seen so far: ``k`` / ``v`` ``[layers, Hkv, max_len, D]`` in the
    model dtype; ``length`` tokens are valid. ``max_len`` may not exceed ``model_args.seq_len``, the
    length of the model's RoPE tables."""

    def __init__(self, model_args, max_len: int, device, dtype):
        max_len = int(max_len)
        if max_len < 1 or max_len > model_args.seq_len:
            raise ValueError(f"KVCache: max_len {max_len} outside [1, {model_args.seq_len}] "
                             "(the model's sequence length, which sizes its RoPE tables)")
        shape = (model_args.n_layers, model_args.kv_heads, max_len, model_args.head_dim)
        self.k = torch.zeros(shape, dtype=dtype, device=device)
        self.v = torch.zeros(shape, dtype=dtype, device=device)
        self.max_len = max_len
        self.length = 0


class _CacheRow:
    """Row ``b`` of a :class:`BatchKVCache` behind :class:`KVCache`'s interface: ``k`` / ``v`` are the
    views ``[layers, Hkv, max_len, D]`` of that row (``k[i]`` is contiguous), ``length`` is the row's
    entry of the batch's ``lengths``."""

    def __init__(self, cache: "BatchKVCache", b: int):
        self._cache, self._b = cache, b
        self.k, self.v = cache.k[:, b], cache.v[:, b]
        self.max_len = cache.max_len

    @property
    def length(self) -> int:
        return self._cache.lengths[self._b]

    @length.setter
    def length(self, n: int) -> None:
        self._cache.set_length(self._b, n)


class BatchKVCache:
    """The caches of ``batch`` sequences: ``k`` / ``v`` ``[layers, B, Hkv, max_len, D]``, so ``k[i]`` is
    the contiguous per-layer operand of the multi-row kernels and ``k[i, b]`` that of the one-row ones.
    ``lengths`` (host) and ``pos0`` (the same numbers, int32 on the device) hold every row's token
    count when batched decoding starts; decode step ``t`` then works at position ``pos0[b] + t`` of
    row ``b``, and ``steps`` counts the steps taken. ``row(b)`` is the row as a :class:`KVCache`, which
    :func:`prefill` fills."""

    def __init__(self, model_args, batch: int, max_len: int, device, dtype):
        batch, max_len = int(batch), int(max_len)
        if batch < 1:
            raise ValueError(f"BatchKVCache: batch {batch} must be >= 1")
        if max_len < 1 or max_len > model_args.seq_len:
            raise ValueError(f"BatchKVCache: max_len {max_len} outside [1, {model_args.seq_len}] "
                             "(the model's sequence length, which sizes its RoPE tables)")
        shape = (model_args.n_layers, batch, model_args.kv_heads, max_len, model_args.head_dim)
        self.k = torch.zeros(shape, dtype=dtype, device=device)
        self.v = torch.zeros(shape, dtype=dtype, device=device)
        self.batch, self.max_len = batch, max_len
        self.lengths = [0] * batch
        self.steps = 0
        self._pos0: Optional[torch.Tensor] = None

    def row(self, b: int) -> _CacheRow:
        if not 0 <= b < self.batch:
            raise IndexError(f"row {b} outside the batch of {self.batch}")
        return _CacheRow(self, b)

    def set_length(self, b: int, n: int) -> None:
        if self.steps:
            raise ValueError("a row's length is fixed once batched decoding has started")
        self.lengths[b] = int(n)
        self._pos0 = None

    def copy_row(self, dst: int, src: int) -> None:
        """Row ``dst`` becomes a copy of row ``src`` (an identical prompt is prefilled once)."""
        n = self.lengths[src]
        self.k[:, dst, :, :n] = self.k[:, src, :, :n]
        self.v[:, dst, :, :n] = self.v[:, src, :, :n]
        self.set_length(dst, n)

    def reset(self) -> None:
        """Every row empty again, for another batch of prompts. The tensors are kept and not cleared:
        keys beyond a row's count are never loaded."""
        self.lengths = [0] * self.batch
        self.steps = 0
        self._pos0 = None

    @property
    def pos0(self) -> torch.Tensor:
        if self._pos0 is None:
            self._pos0 = torch.tensor(self.lengths, dtype=torch.int32, device=self.k.device)
        return self._pos0


def _final_logits(model, h: torch.Tensor, d: Optional[torch.Tensor]) -> torch.Tensor:
    """Final norm and LM head on one row: h, d [1, dim] -> logits [V]."""
    a = model.model_args
    ln = a.norm_type == "layernorm"
    model._wait(model._ranges[2])
    if d is None:
        hn = Fx.norm(h, model.norm.weight, None, a.norm_eps, ln)
    else:
        _, hn = Fx.add_norm(h, d, model.norm.weight, None, a.norm_eps, ln)
    return D.gemv(hn.reshape(-1), model.output.weight)


@torch.no_grad()
def prefill(model, tokens: Union[Sequence[int], torch.Tensor], cache: KVCache) -> torch.Tensor:
    """Run the prompt (P >= 1 tokens) through the training forward kernels -- embedding, add_norm,
    QKV projection, flash forward, FFN, with the per-layer parameter-gate waits, as
    ``Transformer.evaluate`` does -- into an empty ``cache``; returns the logits [V] after the last
    prompt token. Only that row goes through the head, so no [P, V] logits are formed."""
    dev = cache.k.device
    tok = torch.as_tensor(tokens, dtype=torch.int64).reshape(1, -1).to(dev)
    P = tok.shape[1]
    if cache.length != 0:
        raise ValueError("prefill needs an empty cache")
    if P < 1 or P > cache.max_len:
        raise ValueError(f"prompt of {P} tokens does not fit the cache (1 .. {cache.max_len})")
    a = model.model_args
    ln = a.norm_type == "layernorm"
    hq, hkv, hd = a.n_heads, a.kv_heads, a.head_dim
    emb_r, layer_r, _ = model._ranges
    model._wait(emb_r)
    h = Fx.embedding(tok, model.tok_embeddings.weight, None)
    cos, sin = model.rope_cos, model.rope_sin
    d = None
    for i, layer in enumerate(model.layers.values()):
        model._wait(layer_r[i])
        at, ff = layer.attention, layer.feed_forward
        if d is None:
            xn = Fx.norm(h, layer.attention_norm.weight, None, a.norm_eps, ln)
        else:
            h, xn = Fx.add_norm(h, d, layer.attention_norm.weight, None, a.norm_eps, ln)
        o, k, v = Fx.qkv_rope_attention_kv(xn, at.wqkv, cos, sin, P, hq, hkv, hd)
        cache.k[i, :, :P] = k.reshape(P, hkv, hd).transpose(0, 1)
        cache.v[i, :, :P] = v.reshape(P, hkv, hd).transpose(0, 1)
        da = Fx.linear(o.view(1, P, -1), at.wo.weight, None)
        h, hn = Fx.add_norm(h, da, layer.ffn_norm.weight, None, a.norm_eps, ln)
        d = Fx.feed_forward(hn, ff.w13, ff.w2.weight, None, None)
    cache.length = P
    return _final_logits(model, h[0, -1:].contiguous(), None if d is None else d[0, -1:].contiguous())


@torch.no_grad()
def decode_step(model, token: Union[int, torch.Tensor], cache: KVCache) -> torch.Tensor:
    """Append one token at position ``cache.length``; returns the logits [V] after it."""
    pos = cache.length
    if pos >= cache.max_len:
        raise ValueError(f"the cache is full ({cache.max_len} tokens)")
    dev = cache.k.device
    tok = torch.as_tensor(token, dtype=torch.int64).reshape(1, 1).to(dev)
    a = model.model_args
    ln = a.norm_type == "layernorm"
    hq, hd = a.n_heads, a.head_dim
    emb_r, layer_r, _ = model._ranges
    model._wait(emb_r)
    h = Fx.embedding(tok, model.tok_embeddings.weight, None).view(1, -1)
    cos, sin = model.rope_cos, model.rope_sin
    d = None
    for i, layer in enumerate(model.layers.values()):
        model._wait(layer_r[i])
        at, ff = layer.attention, layer.feed_forward
        if d is None:
            xn = Fx.norm(h, layer.attention_norm.weight, None, a.norm_eps, ln)
        else:
            h, xn = Fx.add_norm(h, d, layer.attention_norm.weight, None, a.norm_eps, ln)
        qkv = D.gemv(xn.reshape(-1), at.wqkv)
        D.qkv_append_(qkv, cos, sin, pos, cache.k[i], cache.v[i])
        o = D.attn(qkv[: hq * hd], cache.k[i], cache.v[i], pos + 1)
        da = D.gemv(o, at.wo.weight)
        h, hn = Fx.add_norm(h, da.view(1, -1), layer.ffn_norm.weight, None, a.norm_eps, ln)
        d = D.gemv(D.gemv_swiglu(hn.reshape(-1), ff.w13), ff.w2.weight).view(1, -1)
    cache.length = pos + 1
    return _final_logits(model, h, d)


def _rows_pass(model, tok: torch.Tensor, append, attend, wait) -> torch.Tensor:
    """One pass over the weights for the B rows of ``tok`` [B, 1]: embedding, the layers, final norm and
    head; returns the logits [B, V]. The two ops that touch the cache are the caller's: ``append(i, qkv)``
    rotates Q in place and stores layer i's K and V, ``attend(i, q)`` returns its attention output
    [B, Hq D]. ``wait(range)`` is the parameter-gate wait before each range of weights (None: the caller
    has waited for all of them). :func:`decode_step_rows` and :class:`DecodeGraph` share this loop."""
    a = model.model_args
    ln = a.norm_type == "layernorm"
    hq, hd = a.n_heads, a.head_dim
    emb_r, layer_r, final_r = model._ranges
    if wait is not None:
        wait(emb_r)
    h = Fx.embedding(tok, model.tok_embeddings.weight, None).view(tok.shape[0], -1)
    d = None
    for i, layer in enumerate(model.layers.values()):
        if wait is not None:
            wait(layer_r[i])
        at, ff = layer.attention, layer.feed_forward
        if d is None:
            xn = Fx.norm(h, layer.attention_norm.weight, None, a.norm_eps, ln)
        else:
            h, xn = Fx.add_norm(h, d, layer.attention_norm.weight, None, a.norm_eps, ln)
        qkv = D.gemv_rows(xn, at.wqkv)
        append(i, qkv)
        o = attend(i, qkv[:, : hq * hd])
        da = D.gemv_rows(o, at.wo.weight)
        h, hn = Fx.add_norm(h, da, layer.ffn_norm.weight, None, a.norm_eps, ln)
        d = D.gemv_rows(D.gemv_swiglu_rows(hn, ff.w13), ff.w2.weight)
    if wait is not None:
        wait(final_r)
    if d is None:
        hn = Fx.norm(h, model.norm.weight, None, a.norm_eps, ln)
    else:
        _, hn = Fx.add_norm(h, d, model.norm.weight, None, a.norm_eps, ln)
    return D.gemv_rows(hn, model.output.weight)


@torch.no_grad()
def decode_step_rows(model, tokens: Union[Sequence[int], torch.Tensor], cache: BatchKVCache, t: int) -> torch.Tensor:
    """Decode step ``t`` (0, 1, ...) of a batch: append ``tokens[b]`` at position ``pos0[b] + t`` of
    row ``b``; returns the logits [B, V] after them. The loop of :func:`decode_step` on B rows."""
    B, t = cache.batch, int(t)
    if t != cache.steps:
        raise ValueError(f"decode step {t} out of order (the cache has taken {cache.steps})")
    if min(cache.lengths) < 1:
        raise ValueError("every row needs a prefilled prompt")
    if max(cache.lengths) + t >= cache.max_len:
        raise ValueError(f"the cache is full ({cache.max_len} tokens)")
    dev = cache.k.device
    tok = torch.as_tensor(tokens, dtype=torch.int64).reshape(B, 1).to(dev)
    cos, sin = model.rope_cos, model.rope_sin
    pos0, lengths = cache.pos0, cache.lengths
    logits = _rows_pass(
        model, tok,
        lambda i, qkv: D.qkv_append_rows_(qkv, cos, sin, pos0, t, cache.k[i], cache.v[i], lengths),
        lambda i, q: D.attn_rows(q, cache.k[i], cache.v[i], pos0, t, lengths), model._wait)
    cache.steps = t + 1
    return logits


def _prefill_rows(model, rows: List[List[int]], cache: BatchKVCache) -> torch.Tensor:
    """Every prompt into its row of ``cache`` (identical prompts prefilled once, then copied); the
    logits [B, V] after each row's last prompt token."""
    first, first_logits = {}, []
    for b, p in enumerate(rows):
        src = first.setdefault(tuple(p), b)
        if src == b:
            first_logits.append(prefill(model, p, cache.row(b)))
        else:
            cache.copy_row(b, src)
            first_logits.append(first_logits[src])
    return torch.stack(first_logits)


def graph_supported(model) -> bool:
    """Whether :class:`DecodeGraph` can decode for ``model``: every op of the captured body must take its
    kernel route, since a composed route reads the control block on the host, which a capture cannot do.
    That is a GPU model of a kernel dtype (CPU and fp64 models compose everything) whose vocabulary is a
    multiple of 8 (``sample_dev_``; the eager sampler takes other vocabularies to its float64
    definition). ``graph=True`` decodes eagerly where this is False."""
    return native(model.flat.params) and model.model_args.vocab_size % 8 == 0


class DecodeGraph:
    """One decoded token for ``batch`` rows as one captured HIP graph, replayed per token.

    Owns a :class:`BatchKVCache` of capacity ``max_len`` and the static buffers the captured launches
    name: ``tok`` [B, 1] (the token the pass embeds), ``logits`` [B, V], ``out`` [B, max_len] (the call's
    tokens, column t = new token t), ``pos0`` [B], the attention workspace ``part`` and output ``o``, and
    the control block ``ctl``. The body is ``sample_dev_`` from ``logits`` into ``tok`` / ``out[:, t]``,
    the layer loop of :func:`decode_step_rows` on ``tok`` with the device-step ops, the head into
    ``logits``, then ``t += 1``: a single chain of launches on one stream.

    The capture happens here, once (``captures`` counts them), so build the object when the parameters'
    addresses are final. :meth:`run` serves any request of up to ``batch`` rows that fits ``max_len``."""

    EOS_CHECK_EVERY = 16  # tokens between two looks at the generated ids (one copy to the host each)

    def __init__(self, model, batch: int, max_len: int):
        flat, a = model.flat, model.model_args
        if not graph_supported(model):  # before anything is allocated or a capture opens
            raise ValueError("DecodeGraph needs a GPU model of a kernel dtype (bf16, fp16 or fp32) whose vocabulary "
                             f"is a multiple of 8 (the device sampler's rows), got {flat.device.type} / {flat.dtype} "
                             f"/ vocabulary {a.vocab_size}")
        dev = flat.device
        self.model = model
        self.cache = BatchKVCache(a, batch, max_len, dev, flat.dtype)
        self.batch, self.max_len = self.cache.batch, self.cache.max_len
        B = self.batch
        self.tok = torch.zeros(B, 1, dtype=torch.int64, device=dev)
        self.logits = torch.zeros(B, a.vocab_size, dtype=flat.dtype, device=dev)
        self.out = torch.zeros(B, self.max_len, dtype=torch.int64, device=dev)
        self.pos0 = torch.zeros(B, dtype=torch.int32, device=dev)
        self.part = D.attn_part(B, a.n_heads, self.max_len, a.head_dim, dev)
        self.o = torch.empty(B, a.n_heads * a.head_dim, dtype=flat.dtype, device=dev)
        self.ctl = D.new_ctl(dev)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.stream: Optional[torch.cuda.Stream] = None
        self.captures = 0
        self.replays = 0
        self._longest, self._t = 0, 0  # the current call's longest prompt and its passes so far
        self._capture()

    def _wait_params(self) -> None:
        """The parameter-gate waits of a pass, all of them, on the current stream: the captured body
        holds none."""
        emb_r, layer_r, final_r = self.model._ranges
        for r in (emb_r, *layer_r, final_r):
            self.model._wait(r)

    def _body(self) -> None:
        model, cache, ctl, pos0 = self.model, self.cache, self.ctl, self.pos0
        cos, sin = model.rope_cos, model.rope_sin
        D.sample_dev_(self.logits, ctl, self.tok, self.out)
        logits = _rows_pass(
            model, self.tok,
            lambda i, qkv: D.qkv_append_rows_dev_(qkv, cos, sin, pos0, ctl, cache.k[i], cache.v[i]),
            lambda i, q: D.attn_rows_dev(q, cache.k[i], cache.v[i], pos0, ctl, self.part, self.o), None)
        self.logits.copy_(logits)
        D.ctl_advance_(ctl)

    @torch.no_grad()
    def _capture(self) -> None:
        # one eager pass first, so that every kernel is loaded before the capture opens. It runs on
        # the fresh buffers (token 0 of all-zero logits at position 0 of empty rows); what it leaves
        # in the cache and in `out` is overwritten by the first call's prefill and tokens
        self._wait_params()
        D.write_ctl(self.ctl, 0, 0.0, 0, 0, 0)
        self._body()
        torch.cuda.synchronize()
        self.stream = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        # thread-local capture on a private stream, as graphs.GraphedStep: the trainer's RCCL watchdog
        # and checkpoint threads make HIP calls of their own while the capture is open
        with torch.cuda.graph(g, stream=self.stream, capture_error_mode="thread_local"):
            self._body()
        self.graph = g
        self.captures += 1

    @torch.no_grad()
    def begin(self, prompts: Sequence[Sequence[int]], max_new_tokens: int, temperature: float = 0.0, top_k: int = 0,
              key: int = 0, step: int = 0, top_p: float = 1.0) -> int:
        """Start a call: check the request, prefill every row (fewer prompts than ``batch`` are padded with
        copies of the first one: a row's tokens do not depend on the other rows), and write ``logits``,
        ``pos0`` and ``ctl`` (t = 0). Returns the number of prompts. Nothing is replayed."""
        rows = [[int(t) for t in p] for p in prompts]
        n_new = int(max_new_tokens)
        if not 1 <= len(rows) <= self.batch:
            raise ValueError(f"this DecodeGraph takes 1 .. {self.batch} prompts, got {len(rows)}")
        for p in rows:
            _check_request(self.model.model_args, p, n_new, "DecodeGraph")
        self._longest = max(len(p) for p in rows)
        if self._longest + n_new > self.max_len:
            raise ValueError(f"prompt ({self._longest}) + new tokens ({n_new}) exceed this DecodeGraph's capacity "
                             f"{self.max_len}")
        self.cache.reset()
        padded = rows + [rows[0]] * (self.batch - len(rows))
        logits = _prefill_rows(self.model, padded, self.cache)  # waits for the parameters as it goes
        self._wait_params()
        self.logits.copy_(logits)
        self.pos0.copy_(self.cache.pos0)
        D.write_ctl(self.ctl, 0, temperature, top_k, key, step, top_p=top_p)
        self._t = 0  # the host's count of the passes of this call: ctl's t, which is never read back
        return len(rows)

    def replay(self) -> None:
        """One token: sample new token t from ``logits`` into ``tok`` / ``out[:, t]``, append it, leave the
        logits after it in ``logits``, t += 1. The capacity check of :func:`decode_step_rows`, made here
        because the captured launches cannot make it."""
        if self._longest + self._t >= self.max_len:
            raise ValueError(f"the cache is full ({self.max_len} tokens)")
        self.graph.replay()
        self._t += 1
        self.replays += 1

    @torch.no_grad()
    def run(self, prompts: Sequence[Sequence[int]], max_new_tokens: int, temperature: float = 0.0, top_k: int = 0,
            key: int = 0, step: int = 0, eos_id: Optional[int] = None, top_p: float = 1.0) -> List[List[int]]:
        """What :func:`generate_batch` returns for these arguments."""
        n_new = int(max_new_tokens)
        n_rows = self.begin(prompts, n_new, temperature, top_k, key, step, top_p=top_p)
        seen = 0  # tokens of every row the host has looked at
        done = [False] * n_rows
        t = 0
        while t < n_new:
            if t == n_new - 1:  # the last token needs the sampler alone, no pass after it
                D.sample_dev_(self.logits, self.ctl, self.tok, self.out)
            else:
                self.replay()
            t += 1
            if eos_id is not None and t < n_new and t % self.EOS_CHECK_EVERY == 0:
                for b, r in enumerate(self.out[:n_rows, seen:t].tolist()):
                    done[b] = done[b] or eos_id in r
                seen = t
                if all(done):  # up to EOS_CHECK_EVERY - 1 tokens were computed for nothing
                    break
        ids = self.out[:n_rows, :t].tolist()
        if eos_id is not None:  # a row ends with its first EOS; the eager loop ends with the last row's
            ids = [r[: r.index(eos_id) + 1] if eos_id in r else r for r in ids]
        return ids


def _check_request(a, prompt: List[int], n_new: int, who: str) -> None:
    if not prompt:
        raise ValueError(f"{who} needs a prompt of at least one token")
    if n_new < 0 or len(prompt) + n_new > a.seq_len:
        raise ValueError(f"prompt ({len(prompt)}) + new tokens ({n_new}) exceed the model's sequence length "
                         f"{a.seq_len}")
    bad = [t for t in prompt if not 0 <= t < a.vocab_size]
    if bad:
        raise ValueError(f"prompt id {bad[0]} outside the vocabulary [0, {a.vocab_size})")


MAX_BATCH = 64


@torch.no_grad()
def generate_batch(model, prompts: Sequence[Sequence[int]], max_new_tokens: int, temperature: float = 0.0,
                   top_k: int = 0, key: int = 0, eos_id: Optional[int] = None, step: int = 0,
                   graph: bool = False, top_p: float = 1.0) -> List[List[int]]:
    """:func:`generate` for B prompts at once: the ids generated after each of ``prompts``. New token
    ``t`` of every row comes from one ``D.sample(logits[B, V], ..., token_key(key, t), step)``, row
    ``b``'s draw being the sampler's row ``b``: row 0 equals ``generate`` with the same arguments, and
    copies of one prompt give different samples. A row that has emitted ``eos_id`` ends there (the id
    included) and keeps its batch slot -- its further tokens are computed and dropped, so no other
    row's draw or position shifts. Identical prompts are prefilled once. ``graph=True`` decodes with a
    :class:`DecodeGraph` built for this request (the same ids; keep the object yourself to reuse its
    capture)."""
    rows = [[int(t) for t in p] for p in prompts]
    n_new = int(max_new_tokens)
    a = model.model_args
    B = len(rows)
    if not 1 <= B <= MAX_BATCH:
        raise ValueError(f"generate_batch takes 1 .. {MAX_BATCH} prompts, got {B}")
    for p in rows:
        _check_request(a, p, n_new, "generate_batch")
    if n_new == 0:
        return [[] for _ in rows]
    flat = model.flat
    if graph and graph_supported(model):
        return DecodeGraph(model, B, max(len(p) for p in rows) + n_new).run(
            rows, n_new, temperature=temperature, top_k=top_k, key=key, step=step, eos_id=eos_id, top_p=top_p)
    cache = BatchKVCache(a, B, max(len(p) for p in rows) + n_new, flat.device, flat.dtype)
    logits = _prefill_rows(model, rows, cache)
    out: List[List[int]] = [[] for _ in rows]
    live = [True] * B
    for t in range(n_new):
        nxt = D.sample(logits, temperature, top_k, token_key(key, t), step, top_p=top_p)
        for b, tok in enumerate(nxt.tolist()):
            if live[b]:
                out[b].append(tok)
                live[b] = eos_id is None or tok != eos_id
        if not any(live) or t == n_new - 1:
            break
        logits = decode_step_rows(model, nxt, cache, t)
    return out


@torch.no_grad()
def generate(model, prompt_ids: Sequence[int], max_new_tokens: int, temperature: float = 0.0, top_k: int = 0,
             key: int = 0, eos_id: Optional[int] = None, step: int = 0, graph: bool = False,
             top_p: float = 1.0) -> List[int]:
    """The ids generated after ``prompt_ids`` (at most ``max_new_tokens``; ends after ``eos_id``,
    which is included). ``temperature == 0`` is greedy; otherwise temperature / top-k / top-p sampling
    (``top_p`` in (0, 1], 1: off) with the stateless sampler under ``(key, step)``. ``graph=True`` decodes with a one-row
    :class:`DecodeGraph` (the multi-row kernels at B = 1 return the one-row kernels' bits)."""
    prompt = [int(t) for t in prompt_ids]
    n_new = int(max_new_tokens)
    a = model.model_args
    if not prompt:
        raise ValueError("generate needs a prompt of at least one token")
    if n_new < 0 or len(prompt) + n_new > a.seq_len:
        raise ValueError(f"prompt ({len(prompt)}) + new tokens ({n_new}) exceed the model's sequence length "
                         f"{a.seq_len}")
    bad = [t for t in prompt if not 0 <= t < a.vocab_size]
    if bad:
        raise ValueError(f"prompt id {bad[0]} outside the vocabulary [0, {a.vocab_size})")
    if n_new == 0:
        return []
    flat = model.flat
    if graph and graph_supported(model):
        return DecodeGraph(model, 1, len(prompt) + n_new).run(
            [prompt], n_new, temperature=temperature, top_k=top_k, key=key, step=step, eos_id=eos_id,
            top_p=top_p)[0]
    cache = KVCache(a, len(prompt) + n_new, flat.device, flat.dtype)
    logits = prefill(model, prompt, cache)
    out: List[int] = []
    for t in range(n_new):
        nxt = D.sample(logits, temperature, top_k, token_key(key, t), step, top_p=top_p)
        out.append(int(nxt[0]))
        if (eos_id is not None and out[-1] == eos_id) or t == n_new - 1:
            break
        logits = decode_step(model, nxt, cache)
    return out

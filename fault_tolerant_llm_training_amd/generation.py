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

Generation always uses plain causal attention: a model with a document mask set generates one
continuing document. Everything runs under ``torch.no_grad()`` and writes nothing of the training
state (no gradient buffer, no sink, no optimizer state).

Sampling is stateless (``utils/sampling.py``): new token ``t`` of a call is drawn with the key
``token_key(key, t)`` and the sampler step ``step``, so a call is a pure function of
(parameters, prompt, temperature, top_k, key, step).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import torch

from .ops import decode as D
from .ops import functional as Fx

_MASK63 = (1 << 63) - 1


def token_key(key: int, t: int) -> int:
    """The sampler key of the ``t``-th new token of a call (63 bits: a signed operator argument)."""
    return (int(key) + (int(t) + 1) * 0x9E3779B97F4A7C15) & _MASK63


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


@torch.no_grad()
def generate(model, prompt_ids: Sequence[int], max_new_tokens: int, temperature: float = 0.0, top_k: int = 0,
             key: int = 0, eos_id: Optional[int] = None, step: int = 0) -> List[int]:
    """The ids generated after ``prompt_ids`` (at most ``max_new_tokens``; ends after ``eos_id``,
    which is included). ``temperature == 0`` is greedy; otherwise temperature / top-k sampling with
    the stateless sampler under ``(key, step)``."""
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
    cache = KVCache(a, len(prompt) + n_new, flat.device, flat.dtype)
    logits = prefill(model, prompt, cache)
    out: List[int] = []
    for t in range(n_new):
        nxt = D.sample(logits, temperature, top_k, token_key(key, t), step)
        out.append(int(nxt[0]))
        if (eos_id is not None and out[-1] == eos_id) or t == n_new - 1:
            break
        logits = decode_step(model, nxt, cache)
    return out

"""Held-out evaluation on the GPU: the ``xent_eval_`` kernel against its definition
(utils/evalacc.py) and against the training kernel's arithmetic, the forward-only head and
``Transformer.evaluate``, the training state left untouched, and ``--eval-every`` runs of
train.py against runs without it.
"""
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FX = 2 ** 24


@pytest.fixture(scope="module")
def K():
    from fault_tolerant_llm_training_amd._native import kernels

    return kernels()


def _acc():
    return torch.zeros(4, dtype=torch.int64, device="cuda")


def _twin(logits, labels):
    """The CPU definition on the same (already rounded) logits."""
    from fault_tolerant_llm_training_amd.utils.evalacc import xent_eval_reference_

    return xent_eval_reference_(logits.cpu(), labels.cpu(), torch.zeros(4, dtype=torch.int64))


def _logits(T, V, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (3 * torch.randn(T, V, device="cuda", generator=g)).to(dtype)


def _check_against_definition(K, logits, labels):
    acc = _acc()
    K.xent_eval_(logits, labels, acc, -100)
    want = _twin(logits, labels)
    got = acc.cpu()
    print(f"T={logits.shape[0]} V={logits.shape[1]} {logits.dtype}: kernel {got.tolist()} twin {want.tolist()}")
    assert got[1:].tolist() == want[1:].tolist()  # tokens, hits, left-out rows: exact
    n = int(got[1])
    # float64 cross-entropy of the same logits; the tolerance xent_fwd is held to per row
    # (tests/test_kernels_gpu.py test_xent: atol 2e-3, rtol 1e-3) holds for the mean of the rows
    ref = F.cross_entropy(logits.double(), labels, reduction="sum", ignore_index=-100).item() / n
    mean = got[0].item() / FX / n
    print(f"  mean NLL {mean:.6f} float64 {ref:.6f} diff {abs(mean - ref):.2e}")
    assert abs(mean - ref) <= 2e-3 + 1e-3 * abs(ref)


# V = 8: most lanes idle, -inf partials in the merges; 2056: one vector into the second sweep; 50304
# and 131072: the real vocabularies. T = 70000 (> the 32768-block grid) runs the row grid-stride.
@pytest.mark.parametrize("V,T", [(8, 1), (8, 3), (2056, 1), (2056, 3), (50304, 1), (50304, 3), (131072, 1),
                                 (131072, 3), (8, 70000)])
def test_kernel_matches_definition_bf16(K, V, T):
    logits = _logits(T, V, torch.bfloat16, V + T)
    labels = torch.randint(0, V, (T,), device="cuda")
    labels[0], labels[-1] = 0, V - 1
    _check_against_definition(K, logits, labels)
    if T == 1:  # the single row with the other end of the vocabulary
        _check_against_definition(K, logits, torch.zeros(1, dtype=torch.int64, device="cuda"))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("V,T", [(8, 3), (2056, 3), (50304, 3), (8, 70000)])
def test_kernel_matches_definition_fp16_fp32(K, V, T, dtype):
    logits = _logits(T, V, dtype, V + T + 1)
    labels = torch.randint(0, V, (T,), device="cuda")
    labels[0], labels[-1] = 0, V - 1
    _check_against_definition(K, logits, labels)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("V,T", [(8, 70000), (2056, 300), (50304, 33), (131072, 5)])
def test_same_arithmetic_as_the_training_kernel(K, V, T, dtype):
    logits = _logits(T, V, dtype, V * 3 + T)
    labels = torch.randint(0, V, (T,), device="cuda")
    labels[::5] = -100
    keep = logits.clone()
    loss, _ = K.xent_fwd(logits, labels, -100)
    live = (labels != -100).cpu()
    want = torch.round(loss.cpu() * float(FX)).to(torch.int64)[live].sum().item()  # the fp32 product is exact
    acc = _acc()
    K.xent_eval_(logits, labels, acc, -100)
    assert acc[0].item() == want
    assert acc[1].item() == int(live.sum()) and acc[3].item() == 0
    first = acc.clone()
    K.xent_eval_(logits, labels, acc, -100)  # accumulated, not overwritten
    assert torch.equal(acc, 2 * first)
    assert torch.equal(logits, keep)  # read-only


def test_edge_rows(K):
    V = 2056
    logits = _logits(6, V, torch.bfloat16, 5)
    labels = torch.tensor([7, -100, 11, 300, 2055, 0], device="cuda")
    base = _acc()
    K.xent_eval_(logits, labels, base, -100)
    assert base[1].item() == 5 and base[3].item() == 0
    # an ignored row adds nothing: the same rows without it
    sel = torch.tensor([0, 2, 3, 4, 5], device="cuda")
    acc = _acc()
    K.xent_eval_(logits[sel].contiguous(), labels[sel], acc, -100)
    assert torch.equal(acc, base)
    # all rows ignored: acc unchanged
    K.xent_eval_(logits, torch.full((6,), -100, device="cuda"), acc, -100)
    assert torch.equal(acc, base)
    # +inf at a non-label column (a bad batch): the row goes to acc[3] and nowhere else
    bad = logits.clone()
    bad[2, 1000] = float("inf")
    acc = _acc()
    K.xent_eval_(bad, labels, acc, -100)
    rest = _acc()
    sel = torch.tensor([0, 3, 4, 5], device="cuda")
    K.xent_eval_(logits[sel].contiguous(), labels[sel], rest, -100)
    assert acc[3].item() == 1 and acc[:3].tolist() == rest[:3].tolist()
    assert acc[1:].tolist() == _twin(bad, labels)[1:].tolist()


@pytest.mark.parametrize("lo,hi", [(3, 9), (5, 2051), (0, 2055), (2047, 2048)])
def test_ties_go_to_the_lowest_index(K, lo, hi):
    """Two columns share the row maximum in bf16 (different threads, waves and sweeps): the label at
    the lower index is a hit, the label at the higher index is not."""
    V = 2056
    logits = _logits(2, V, torch.bfloat16, lo + hi).clamp_(max=4.0)
    logits[:, lo] = 8.0
    logits[:, hi] = 8.0
    labels = torch.tensor([lo, hi], device="cuda")
    acc = _acc()
    K.xent_eval_(logits[:1].contiguous(), labels[:1], acc, -100)
    assert acc[1:3].tolist() == [1, 1]
    acc = _acc()
    K.xent_eval_(logits[1:].contiguous(), labels[1:], acc, -100)
    assert acc[1:3].tolist() == [1, 0]
    acc = _acc()
    K.xent_eval_(logits, labels, acc, -100)
    assert acc[1:].tolist() == [2, 1, 0] == _twin(logits, labels)[1:].tolist()  # (counts: the twin's NLL is torch's)


def test_order_independence(K):
    T, V = 4096, 2056
    logits = _logits(T, V, torch.bfloat16, 77)
    labels = torch.randint(0, V, (T,), device="cuda")
    labels[::9] = -100
    whole = _acc()
    K.xent_eval_(logits, labels, whole, -100)
    acc = _acc()
    order = torch.randperm(T // 256, generator=torch.Generator().manual_seed(3)).tolist()
    assert order != sorted(order)
    for c in order:
        K.xent_eval_(logits[c * 256:(c + 1) * 256], labels[c * 256:(c + 1) * 256], acc, -100)
    assert torch.equal(acc, whole)


# ------------------------------------------------------------------------------- head and model
def test_lm_head_eval_equals_kernel_on_materialised_logits(K, monkeypatch):
    from fault_tolerant_llm_training_amd.ops import functional as Fx

    T, D, V = 1024, 256, 1024  # the tiny preset's width; 4 chunks of 256 rows
    monkeypatch.setattr(Fx, "_HEAD_CHUNK_MB", 0.25)
    rows = Fx._head_rows(T, V)
    assert rows == 256
    torch.manual_seed(2)
    h = torch.randn(T, D, device="cuda").bfloat16()
    w = (torch.randn(V, D, device="cuda") * 0.05).bfloat16()
    lab = torch.randint(0, V, (T,), device="cuda")
    lab[::7] = -100
    acc = _acc()
    Fx.lm_head_eval(h.view(4, 256, D), w, lab.view(4, 256), acc)
    logits = torch.cat([Fx._head_fwd(h[r:r + rows], w) for r in range(0, T, rows)])
    want = _acc()
    K.xent_eval_(logits, lab, want, -100)
    assert torch.equal(acc, want) and acc[1].item() == int((lab != -100).sum())


def _tiny(seed=0, vocab=1024, seq=128):
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for
    from fault_tolerant_llm_training_amd.optim.adamw import FlatAdamW
    from fault_tolerant_llm_training_amd.parallel.ddp import GradReducer

    model = build_model(model_args_for("tiny", vocab_size=vocab, seq_len=seq), "cuda:0", torch.bfloat16, seed=seed)
    red = GradReducer(model.flat, model.sinks_in_backward_order(), bucket_mb=1.0)
    opt = FlatAdamW(model.parameters(), model.flat, lr=1e-3, max_grad_norm=1.0, reducer=red)
    model.gate = opt.gate
    return model, red, opt


def _batch(vocab=1024, seq=128, B=2, seed=1):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(2, vocab, (B, seq), generator=g)
    tok[:, 0] = 1
    tok[0, 40] = tok[1, 77] = tok[1, 100] = 1  # BOS: document starts under the mask
    lab = torch.randint(0, vocab, (B, seq), generator=g)
    lab[0, :5] = -100
    return tok.cuda(), lab.cuda()


@pytest.mark.parametrize("doc_mask", [False, True])
def test_evaluate_equals_the_training_forward(K, doc_mask):
    model, _, _ = _tiny()
    if doc_mask:
        model.set_document_mask(1)
    tok, lab = _batch()
    acc = _acc()
    model.evaluate(tok, lab, acc)
    with torch.no_grad():
        logits = model(tok)  # the training forward's logits
    loss, _ = K.xent_fwd(logits.view(-1, logits.shape[-1]), lab.view(-1), -100)
    live = (lab.view(-1) != -100).cpu()
    want = torch.round(loss.cpu() * float(FX)).to(torch.int64)[live].sum().item()
    assert acc[0].item() == want and acc[1].item() == int(live.sum())
    # ... and the scalar loss the training step itself reports (fp32 sum of the same rows)
    inv = torch.full((1,), 1.0 / int(live.sum()), device="cuda")
    train_loss = model(tok, lab, inv).item()
    assert abs(acc[0].item() / FX / acc[1].item() - train_loss) <= 1e-4 * max(1.0, abs(train_loss))
    if doc_mask:  # the mask is in effect: not the causal result
        model.set_document_mask(None)
        plain = _acc()
        model.evaluate(tok, lab, plain)
        assert plain[0].item() != acc[0].item()


def _all_sinks(model):
    return list(model.flat.sinks.values()) + model.sinks_in_backward_order()


def _step(model, red, opt, tok, lab):
    loss = model(tok, lab)
    loss.backward()
    red.finish()
    opt.clip_grad_norm_(1.0)
    opt.step()
    torch.cuda.synchronize()
    return loss.item()


@pytest.mark.parametrize("ckpt_layers", [0, 1])
def test_evaluate_touches_nothing_of_the_training_state(ckpt_layers):
    model, red, opt = _tiny(seed=3)
    if ckpt_layers:
        model.set_activation_checkpointing(ckpt_layers)
    tok, lab = _batch()
    n = model.flat.grads.numel()
    model.flat.grads.copy_((torch.arange(n, device="cuda") % 251).to(model.flat.grads.dtype))
    red.partials.copy_(torch.arange(red.partials.numel(), device="cuda").float() + 0.5)
    sinks = _all_sinks(model)
    parts = [None if s.part is None else s.part.clone() for s in sinks]
    assert any(p is not None for p in parts)
    flags = [(s.sq_done, s.accumulate, s.defer, len(s.stash)) for s in sinks]
    buckets = [(b.filled, b.launched) for b in red.buckets]
    grads, partials, params = model.flat.grads.clone(), red.partials.clone(), model.flat.params.clone()
    keeps = [(l.attn_keep.gen, l.attn_keep.o) for l in model.layers.values()]
    acc = _acc()
    model.evaluate(tok, lab, acc)
    torch.cuda.synchronize()
    assert acc[1].item() > 0
    assert torch.equal(model.flat.grads, grads) and torch.equal(red.partials, partials)
    assert torch.equal(model.flat.params, params)
    for s, p in zip(sinks, parts):
        assert p is None or torch.equal(s.part, p)
    assert flags == [(s.sq_done, s.accumulate, s.defer, len(s.stash)) for s in sinks]
    assert buckets == [(b.filled, b.launched) for b in red.buckets]
    for l, (g, o) in zip(model.layers.values(), keeps):  # the kept-attention store got no generation
        assert l.attn_keep.gen == g and l.attn_keep.o is o
    assert model.flat.grads.grad_fn is None and not acc.requires_grad


def test_a_step_after_evaluate_equals_the_step_of_a_model_that_never_evaluated():
    tok, lab = _batch()
    a, ra, oa = _tiny(seed=4)
    b, rb, ob = _tiny(seed=4)
    a.evaluate(tok, lab, _acc())
    la = [_step(a, ra, oa, tok, lab)]
    a.evaluate(tok, lab, _acc())  # between two steps: behind the pipelined AdamW of the first
    la.append(_step(a, ra, oa, tok, lab))
    lb = [_step(b, rb, ob, tok, lab) for _ in range(2)]
    assert la == lb
    assert torch.equal(a.flat.params, b.flat.params)
    assert torch.equal(oa.exp_avg, ob.exp_avg) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)


# ------------------------------------------------------------------------------- train.py
GPU = ["--device", "cuda", "--model", "tiny", "--synthetic-data", "--vocab-size", "1024", "--sequence-length", "128",
       "--batch-size", "2", "--training-steps", "6", "--logging-frequency", "1", "--state-digest", "--prefetch", "1",
       "--eval-sequences", "6"]
MODES = {"eager": [], "graph": ["--hip-graph"], "sr": ["--stochastic-rounding"]}


@pytest.fixture(scope="module")
def train_runs(tmp_path_factory):
    """(mode, eval_every) -> (log, evaluation records) of one 6-step run; each run happens once."""
    from helpers import run_train

    cache = {}

    def get(mode, every):
        if (mode, every) not in cache:
            d = str(tmp_path_factory.mktemp(f"{mode}{every}"))
            rc, out = run_train(d, "1", GPU + MODES[mode] + ["--eval-every", str(every), "--metrics-file", "m.jsonl",
                                                             "--checkpoint-path", os.path.join(d, "ck")], timeout=240)
            assert rc == 0, out
            recs = [json.loads(ln) for ln in open(os.path.join(d, "m.jsonl")).read().splitlines() if ln.strip()]
            cache[(mode, every)] = (out, [r for r in recs if "eval_step" in r])
        return cache[(mode, every)]

    return get


def _losses(out):
    return re.findall(r"Training step: (\d+) \| Loss: ([-\d.naninf]+) .*?grad_norm: ([-\d.naninf]+)", out)


def _digest(out):
    m = re.search(r"State digest at step 6: (params=\w+ exp_avg=\w+ exp_avg_sq=\w+ optimizer_step=\d+ data_loader=.*)",
                  out)
    assert m, out
    return m.group(1)


@pytest.mark.parametrize("mode", ["eager", "graph", "sr"])
def test_training_is_unchanged_by_evaluation(train_runs, mode):
    off, none = train_runs(mode, 0)
    on, recs = train_runs(mode, 2)
    assert none == [] and "Evaluation" not in off
    assert len(_losses(off)) == 6 and _losses(off) == _losses(on)
    assert _digest(off) == _digest(on)
    assert [r["eval_step"] for r in recs] == [2, 4, 6]
    for r in recs:
        assert r["eval_tokens"] == 6 * 128 and r["eval_nonfinite"] == 0
        assert r["eval_loss"] == r["eval_loss_fx"] / FX / r["eval_tokens"]
        assert f"Evaluation at step {r['eval_step']} | Loss: {r['eval_loss']:.4f} | Perplexity: " in on


def test_eager_and_graph_runs_log_the_same_evaluation(train_runs):
    _, eager = train_runs("eager", 2)
    _, graph = train_runs("graph", 2)
    assert [r["eval_loss_fx"] for r in eager] == [r["eval_loss_fx"] for r in graph]
    assert [r["eval_correct"] for r in eager] == [r["eval_correct"] for r in graph]

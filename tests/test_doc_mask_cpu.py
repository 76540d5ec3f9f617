"""Document-masked attention for packed sequences (--document-mask), the layers that run without a
GPU: the boundary composition, the model's CPU path, activation checkpointing, the CLI flag and a
train.py run on the packing dataset (start-up line, different loss, bit-exact resume)."""
import os
import re

import pytest
import torch

from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for
from fault_tolerant_llm_training_amd.ops.attention import doc_bounds

BOS = 1


def loop_bounds(tokens, bos):
    B, S = tokens.shape
    ds = torch.zeros(B, S, dtype=torch.int32)
    de = torch.zeros(B, S, dtype=torch.int32)
    for b in range(B):
        last = 0
        for i in range(S):
            if tokens[b, i] == bos:
                last = i
            ds[b, i] = last
        nxt = S
        for i in reversed(range(S)):
            de[b, i] = nxt
            if tokens[b, i] == bos:
                nxt = i
    return ds, de


def row(S, pos, seed=0):
    t = torch.randint(2, 50, (S,), generator=torch.Generator().manual_seed(seed))
    for p in pos:
        t[p] = BOS
    return t


@pytest.mark.parametrize("pos", [[], [0], [3, 4, 5], [15], [0, 1, 7, 15]])
def test_doc_bounds_composition_matches_loop(pos):
    tok = row(16, pos).view(1, 16)
    ds, de = doc_bounds(tok, BOS)
    rs, re_ = loop_bounds(tok, BOS)
    assert ds.dtype == de.dtype == torch.int32
    assert torch.equal(ds, rs) and torch.equal(de, re_)
    i = torch.arange(16)
    assert (ds[0] <= i).all() and (i < de[0]).all()
    assert (ds[0, 1:] >= ds[0, :-1]).all() and (de[0, 1:] >= de[0, :-1]).all()


def test_doc_bounds_two_rows_with_different_layouts():
    tok = torch.stack([row(33, [0, 10, 32], 1), row(33, [5], 2)])
    ds, de = doc_bounds(tok, BOS)
    rs, re_ = loop_bounds(tok, BOS)
    assert torch.equal(ds, rs) and torch.equal(de, re_)
    assert ds[0, 31] == 10 and de[0, 31] == 32 and ds[0, 32] == 32 and de[0, 32] == 33
    assert ds[1, 4] == 0 and de[1, 4] == 5 and ds[1, 5] == 5 and de[1, 32] == 33


LENS = (37, 64, 27)
V = 300


def packed():
    """[docA | docB | docC], each starting with BOS; A and C draw from ids docB never uses."""
    g = torch.Generator().manual_seed(0)
    a = torch.randint(200, V, (LENS[0],), generator=g)
    b = torch.randint(2, 100, (LENS[1],), generator=g)
    c = torch.randint(100, 200, (LENS[2],), generator=g)
    for d in (a, b, c):
        d[0] = BOS
    return torch.cat([a, b, c]).view(1, -1), b.view(1, -1)


def tiny(seed=3):
    return build_model(model_args_for("tiny", vocab_size=V, seq_len=sum(LENS)), "cpu", torch.float32, seed=seed)


def test_packed_document_logits_equal_the_document_alone():
    """With the mask the logits over docB's positions equal docB run alone at positions 0.. (RoPE
    positions are not reset: rotary scores depend on i - j only), at the fp32 tolerance of
    tests/test_model_cpu.py; without the mask they differ by far more (the test sees the feature)."""
    tok, b = packed()
    m = tiny()
    lo, hi = LENS[0], LENS[0] + LENS[1]
    with torch.no_grad():
        alone = m(b)
        plain = m(tok)[:, lo:hi]
        m.set_document_mask(BOS)
        masked = m(tok)[:, lo:hi]
        assert torch.equal(m(b), alone)  # one document: the mask changes nothing
    assert torch.allclose(masked, alone, atol=1e-4, rtol=1e-4)
    assert (plain - alone).abs().max().item() > 100 * 1e-4
    m.set_document_mask(None)
    with torch.no_grad():
        assert torch.equal(m(tok)[:, lo:hi], plain)


def test_gradients_do_not_cross_documents():
    """Labels on docB only: the embedding-gradient rows of tokens that occur only in docA / docC
    are exactly zero with the mask (and not without it)."""
    tok, _ = packed()
    lab = torch.full_like(tok, -100)
    lo, hi = LENS[0], LENS[0] + LENS[1]
    lab[:, lo:hi] = torch.randint(2, 100, (1, LENS[1]), generator=torch.Generator().manual_seed(1))
    only_ac = sorted(set(tok[0, :lo].tolist() + tok[0, hi:].tolist()) - set(tok[0, lo:hi].tolist()))
    assert len(only_ac) > 20
    grads = {}
    for on in (True, False):
        m = tiny()
        m.set_document_mask(BOS if on else None)
        m(tok, lab).backward()
        grads[on] = m.tok_embeddings.weight.grad[only_ac].clone()
    assert torch.count_nonzero(grads[True]) == 0
    assert grads[False].abs().max().item() > 0


@pytest.mark.parametrize("recompute_attention", [False, True])
def test_activation_checkpointing_same_loss_and_grads_with_mask(recompute_attention):
    tok, _ = packed()
    lab = torch.randint(2, V, tok.shape, generator=torch.Generator().manual_seed(2))
    out = []
    for k in (0, -1):
        m = tiny(seed=5)
        m.set_document_mask(BOS)
        m.set_activation_checkpointing(k, recompute_attention=recompute_attention)
        loss = m(tok, lab)
        loss.backward()
        out.append((loss.detach(), m.flat.grads.clone()))
    assert torch.equal(out[0][0], out[1][0])
    assert torch.allclose(out[0][1], out[1][1], rtol=0, atol=1e-6)


def test_cli_flag_parses_and_defaults_off():
    from fault_tolerant_llm_training_amd.utils.config import get_args

    import sys
    argv = sys.argv
    try:
        sys.argv = ["train.py"]
        assert get_args().document_mask is False
        sys.argv = ["train.py", "--document-mask"]
        assert get_args().document_mask is True
    finally:
        sys.argv = argv


@pytest.mark.slow
def test_train_py_document_mask_on_the_packing_dataset(tmp_path):
    """train.py --iterable-dataset --document-mask on a tiny parquet file: the start-up line, a
    loss different from the run without the flag at the same seed, and save -> resume bit-exact
    (in the manner of tests/test_ft_e2e.py)."""
    from helpers import TINY, make_parquet, run_train, write_fake_sbatch

    d = str(tmp_path)
    write_fake_sbatch(d)
    pq = os.path.join(d, "data.parquet")
    make_parquet(pq, n_docs=30)
    base = TINY + ["--dataset", pq, "--tokenizer-name-or-path", "byte", "--iterable-dataset", "--checkpoint-path",
                   os.path.join(d, "ck"), "--training-steps", "9", "--lr-warmup-steps", "3", "--logging-frequency", "1",
                   # large enough for the two runs' losses to part within the log's two decimals
                   "--learning-rate", "1e-2"]
    end = ["--raise-error", "--error-step", "8"]
    losses = lambda out: re.findall(r"Training step: (\d+) \| Loss: ([0-9.]+)", out)  # noqa: E731

    rc, plain = run_train(d, "10", base + end)
    assert rc == 0 and "Document mask" not in plain, plain[-3000:]
    rc, out = run_train(d, "20", base + end + ["--document-mask"])
    assert rc == 0 and "Checkpoint saved at step 8" in out, out[-3000:]
    assert "Document mask: on" in out and "token id 1 (BOS) starts a document" in out
    assert losses(out) and losses(out) != losses(plain)

    rc, out = run_train(d, "30", base + ["--document-mask", "--raise-error", "--error-step", "4"])
    assert rc == 0 and "Checkpoint saved at step 4" in out, out[-3000:]
    rc, out = run_train(d, "40", base + end + ["--document-mask", "--checkpoint-id", "30"])
    assert rc == 0 and "Resuming training from training_step 4" in out, out[-3000:]
    load = lambda j: torch.load(os.path.join(d, "ck", f"checkpoint_{j}.ckpt"), map_location="cpu",  # noqa: E731
                                weights_only=True)
    a, b = load(20), load(40)
    assert a["training_step"] == b["training_step"] == 8
    for k in a["model"]:
        assert torch.equal(a["model"][k], b["model"][k]), k
    for i in a["optimizer"]["state"]:
        for f in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(a["optimizer"]["state"][i][f], b["optimizer"]["state"][i][f]), (i, f)
    assert a["lr_scheduler"] == b["lr_scheduler"]
    assert a["data_loader"] == b["data_loader"]

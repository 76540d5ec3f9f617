"""``mma=True`` without a GPU: on the CPU it changes nothing, and the CLI refuses what no kernel serves."""
import pytest
import torch

PROMPTS = [[1, 5, 9, 200, 3, 77, 410, 8, 2], [7, 7, 300], [511, 0, 42, 42, 19]]


@pytest.mark.parametrize("graph", [False, True])
def test_on_the_cpu_mma_changes_nothing(graph):
    from fault_tolerant_llm_training_amd.generation import generate_batch
    from fault_tolerant_llm_training_amd.models.llama import build_model, model_args_for

    model = build_model(model_args_for("tiny", vocab_size=512, seq_len=64), "cpu", torch.float32, seed=3)
    assert generate_batch(model, PROMPTS, 6, mma=True, graph=graph) == generate_batch(model, PROMPTS, 6, graph=graph)


def test_cli_refuses_decode_mma_for_fp32_on_the_gpu_before_loading(tmp_path, capsys):
    from fault_tolerant_llm_training_amd.generate import main

    code = main(["--checkpoint", str(tmp_path / "absent.pt"), "--model", "tiny", "--vocab-size", "512", "--prompt-ids",
                 "1,2,3", "--num-samples", "2", "--decode-mma", "--model-dtype", "fp32", "--device", "cuda"])
    err = capsys.readouterr().err.strip().splitlines()
    assert code == 2 and len(err) == 1 and "--decode-mma needs --model-dtype bf16 or fp16" in err[0]

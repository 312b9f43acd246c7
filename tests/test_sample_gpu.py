"""csrc/sample.hip on MI355X against the fp64 reference of
sample_common.py, and GPT2.generate(top_p=, seed=) through the kernel."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

import sample_common as sc  # noqa: E402
from ray_lightning_amd import ops as _ops  # noqa: E402
from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,  # noqa: E402
                                           to_bf16_training)
from ray_lightning_amd.ops import sample as sm  # noqa: E402

assert _ops._load_ext() is not None, "HIP extension failed to load"
DEV = "cuda"


@pytest.fixture(autouse=True)
def kernel_calls(monkeypatch):
    """The gate on, and a count of the kernel's launches."""
    monkeypatch.setenv("RLA_FUSED_SAMPLE", "1")
    calls = []
    ext = _ops._load_ext()

    class Spy:
        def sample_fwd(self, *args):
            calls.append(1)
            return ext.sample_fwd(*args)

        def __getattr__(self, name):
            return getattr(ext, name)

    monkeypatch.setattr(sm, "_load_ext", lambda: Spy())
    return calls


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", sc.VS)
def test_kernel_against_fp64(V, B, dtype, kernel_calls):
    got = sc.run_cases(sm.sample_tokens, sc.make_rows(V, B, dtype), DEV)
    assert len(kernel_calls) == len(got), "the kernel did not run"


def test_all_neg_inf_row_is_token_zero(kernel_calls):
    rows = torch.full((2, 100), -torch.inf, device=DEV)
    rows[1, 40] = 1.0
    seeds = torch.zeros(2, dtype=torch.int64, device=DEV)
    for t in (0.0, 1.0):
        assert sm.sample_tokens(rows, seeds, 0, temperature=t,
                                top_p=0.9).tolist() == [0, 40]
    assert len(kernel_calls) == 2


@pytest.mark.parametrize("V,dtype", [(4097, torch.float32),
                                     (50257, torch.bfloat16)])
def test_bitwise_and_row_alone(V, dtype):
    """V = 50257 in bf16: the rows of a batch sit at other offsets from
    a 16-byte boundary than the row alone."""
    sc.check_rows_alone(sm.sample_tokens, sc.make_rows(V, 3, dtype), DEV)


def test_epilogue(kernel_calls):
    sc.check_epilogue(sm.sample_tokens, DEV)
    assert len(kernel_calls) == 2


_BAD_NAMES = sorted(sc.bad_operands("cpu")[1])


@pytest.mark.parametrize("name", _BAD_NAMES)
def test_rejected_operand(name):
    ok, bad = sc.bad_operands(DEV)
    kw = dict(ok, **bad[name])
    with pytest.raises((ValueError, RuntimeError)):
        sm.sample_tokens(kw.pop("logits"), kw.pop("seeds"), kw.pop("step"),
                         **kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("top_p,top_k", [(0.9, 40), (1.0, None)])
def test_generate_tokens_in_their_intervals(top_p, top_k, kernel_calls):
    torch.manual_seed(0)
    m = to_bf16_training(GPT2(GPT2Config(
        n_layer=2, n_embd=128, n_head=2, vocab_size=256,
        n_positions=128))).to(DEV).eval()
    idx = torch.randint(0, 256, (3, 12)).to(DEV)
    lens, new, seed = [5, 1, 12], 32, 1234
    kw = dict(prompt_lens=lens, top_p=top_p, top_k=top_k, seed=seed,
              return_logits=True)
    out, logits = m.generate(idx, new, **kw)
    assert len(kernel_calls) == new, "the kernel did not run"
    assert torch.equal(out, m.generate(idx, new, **kw)[0])
    out, logits = out.cpu(), logits.cpu()
    for b, n in enumerate(lens):
        for s in range(new):
            sc.Ref(logits[b, s], 1.0, top_k, top_p).check(
                int(out[b, n + s]), seed + b, s)

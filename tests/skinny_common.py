"""Operands, references and the model check shared by the skinny-linear
tests (CPU and GPU)."""
import copy
import math

import torch
import torch.nn.functional as F

from ray_lightning_amd.models.gpt2 import GPT2, GPT2Config, to_bf16_training

BF16 = torch.bfloat16
EPS = 1e-5


def operands(M, N, K, mode, bias, device, seed=0):
    """x = big[:M] and W = tall[:N]: every row after the slice is NaN, so
    a read past M or N shows in the result."""
    g = torch.Generator().manual_seed(seed)

    def sliced(rows, cols, std):
        t = torch.randn(rows + 3, cols, generator=g) * std
        t[rows:] = math.nan
        return t.to(BF16).to(device)[:rows]

    op = dict(x=sliced(M, K, 1.0), weight=sliced(N, K, 0.02), bias=None,
              residual=None, ln_weight=None, ln_bias=None)
    if bias:
        op["bias"] = (torch.randn(N, generator=g) * 0.02).to(BF16).to(device)
    if mode != "plain":
        op["ln_weight"] = (1 + 0.1 * torch.randn(K, generator=g)).to(device)
        op["ln_bias"] = (0.1 * torch.randn(K, generator=g)).to(device)
    if mode == "add_ln":
        op["residual"] = sliced(M, K, 1.0)
    return op


def reference(op, gelu):
    """fp64 from the same bf16 operands, no intermediate rounding."""
    h = op["x"].double()
    if op["residual"] is not None:
        h = h + op["residual"].double()
    if op["ln_weight"] is not None:
        h = F.layer_norm(h, h.shape[-1:], op["ln_weight"].double(),
                         op["ln_bias"].double(), EPS)
    y = h @ op["weight"].double().t()
    if op["bias"] is not None:
        y = y + op["bias"].double()
    return F.gelu(y, approximate="tanh") if gelu else y


def composed(op, gelu):
    """The path the model takes without the op: add + LayerNorm, then
    F.linear, then F.gelu, every step in bf16."""
    from ray_lightning_amd.ops.fused_ln import dropout_add_layer_norm
    h = op["x"]
    if op["ln_weight"] is not None:
        _, h = dropout_add_layer_norm(h, op["residual"], op["ln_weight"],
                                      op["ln_bias"], EPS, 0.0)
    y = F.linear(h, op["weight"], op["bias"])
    return F.gelu(y, approximate="tanh") if gelu else y


def err(y, ref):
    assert torch.isfinite(y).all()
    return (y.double() - ref).abs().max().item()


def tiny_models(vocab, device):
    torch.manual_seed(0)
    m32 = GPT2(GPT2Config(n_layer=2, n_embd=128, n_head=2, vocab_size=vocab,
                          n_positions=128)).to(device).eval()
    m16 = to_bf16_training(copy.deepcopy(m32)).eval()
    m32.load_state_dict({k: v.float() for k, v in m16.state_dict().items()})
    return m16, m32


def decode_errors(m16, m32, vocab, device, monkeypatch, sl):
    """B = 3 ragged prompts, a prefill and 8 decode steps, once with the
    gate off and once with it on: the logit errors against the fp32 copy
    (e_off, e_on) and the number of decode_layer calls with the gate on.
    Tokens must equal the fp32 argmax wherever its top-1/top-2 margin
    exceeds 4 * e_off."""
    lens, new = [5, 1, 12], 9
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, vocab, (3, 12), generator=g).to(device)
    calls = []
    monkeypatch.setattr(sl, "decode_layer", lambda *a, _f=sl.decode_layer:
                        (calls.append(1), _f(*a))[1])
    runs = {}
    for gate in ("0", "1"):
        monkeypatch.setenv("RLA_SKINNY_LINEAR", gate)
        del calls[:]
        out, logits = m16.generate(idx, new, prompt_lens=lens,
                                   temperature=0.0, return_logits=True)
        e, rows = 0.0, []
        with torch.no_grad():
            for b, n in enumerate(lens):
                ref = m32(out[b, :n + new][None])[0][0, n - 1:n - 1 + new]
                e = max(e, (logits[b] - ref.float()).abs().max().item())
                rows.append((out[b, n:n + new], ref.float()))
        runs[gate] = (e, rows, len(calls))
    e_off, e_on = runs["0"][0], runs["1"][0]
    for tok, ref in runs["1"][1]:
        top2 = ref.topk(2, dim=-1).values
        clear = (top2[:, 0] - top2[:, 1]) > 4 * e_off
        assert torch.equal(tok[clear], ref.argmax(dim=-1)[clear])
    print(f"vocab {vocab}: e_off {e_off:.3e}  e_on {e_on:.3e}")
    assert runs["0"][2] == 0
    return e_off, e_on, runs["1"][2]

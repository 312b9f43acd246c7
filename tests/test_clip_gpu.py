"""Global-norm gradient clipping on the GPU: the HIP sum-of-squares and
scale kernels, the gradient multiplier inside the fused optimizers, and
the trainer path that strings them together without a host read."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from torch.utils.data import DataLoader, TensorDataset  # noqa: E402

from ray_lightning_amd import (Callback, LightningModule,  # noqa: E402
                               Trainer, ops, seed_everything)
from ray_lightning_amd.optim import (FusedAdamW, FusedSGD,  # noqa: E402
                                     ShardedFusedAdam)

assert ops._load_ext() is not None, "HIP extension must be built"

SIZES = [1, 3, 17, 256, 1000, 4096, 65536, 100003]
F32, BF16 = torch.float32, torch.bfloat16


def _rand(n, dtype, gen):
    return torch.randn(n, device="cuda", generator=gen).to(dtype)


def _gen(seed=0):
    return torch.Generator(device="cuda").manual_seed(seed)


def _segments(kind, seed=0):
    g = _gen(seed)
    if kind == "f32":
        return [_rand(s, F32, g) for s in SIZES]
    if kind == "bf16":
        return [_rand(s, BF16, g) for s in SIZES]
    if kind == "mixed":
        return [_rand(s, BF16 if i % 2 else F32, g)
                for i, s in enumerate(SIZES)]
    if kind == "many_small":  # 100 odd lengths: crosses kMaxSeg (48)
        return [_rand(2 * i + 1, BF16 if i % 3 == 0 else F32, g)
                for i in range(100)]
    if kind in ("offset1", "offset3"):  # misaligned base pointers
        off = int(kind[-1])
        out = []
        for dt in (F32, BF16):
            flat = _rand(70000, dt, g)
            out += [flat[off:off + 5], flat[100 + off:100 + off + 1001],
                    flat[2000 + off:2000 + off + 65537]]
        return out
    if kind == "slots":  # the engines' 8-element-aligned bucket slots
        out = []
        for dt in (F32, BF16):
            total = sum((s + 7) & ~7 for s in SIZES)
            flat = _rand(total, dt, g)
            off = 0
            for s in SIZES:
                out.append(flat[off:off + s])
                off += (s + 7) & ~7
        return out
    if kind == "zero_len":
        return [torch.empty(0, device="cuda"), _rand(17, F32, g),
                torch.empty(0, device="cuda", dtype=BF16)]
    if kind == "only_zero_len":
        return [torch.empty(0, device="cuda")]
    if kind == "empty":
        return []
    raise ValueError(kind)


KINDS = ["f32", "bf16", "mixed", "many_small", "offset1", "offset3",
         "slots", "zero_len", "only_zero_len", "empty"]


@pytest.mark.parametrize("kind", KINDS)
def test_sumsq_matches_fp64(kind):
    """norm rtol 1e-5: all terms are non-negative, so a blocked fp32 sum
    is off by at most (longest sequential chain + tree depth) * 2^-24
    relative; chains here are <= 16 terms per level."""
    ts = _segments(kind)
    got = ops.grad_sumsq(ts, device=torch.device("cuda"))
    assert got.shape == (1,) and got.dtype == F32 and got.is_cuda
    ref = sum((t.double().pow(2).sum() for t in ts),
              torch.zeros((), dtype=torch.float64, device="cuda"))
    got_norm, ref_norm = got.double().sqrt().item(), ref.sqrt().item()
    print(f"{kind}: norm {got_norm!r} ref {ref_norm!r} "
          f"rel {abs(got_norm - ref_norm) / max(ref_norm, 1e-300):.3e}")
    assert got_norm == pytest.approx(ref_norm, rel=1e-5, abs=0.0)


@pytest.mark.parametrize("kind", ["mixed", "many_small", "offset3"])
def test_sumsq_is_deterministic(kind):
    ts = _segments(kind)
    assert torch.equal(ops.grad_sumsq(ts), ops.grad_sumsq(ts))


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_norm_propagates_like_torch(bad):
    ours = _segments("f32", seed=3)[2:6]
    ours[1][5] = bad
    theirs = [t.clone() for t in ours]
    for t in theirs:
        t.grad = t.clone()
    ref_norm = torch.nn.utils.clip_grad_norm_(theirs, 1.0)
    norm, coef = ops.clip_coef(ops.grad_sumsq(ours), 1.0)
    ops.scale_grads_(ours, coef)
    ref_coef = torch.clamp(1.0 / (ref_norm + 1e-6), max=1.0)
    assert torch.equal(norm.reshape(()).isnan(), ref_norm.isnan())
    assert torch.allclose(coef.reshape(()), ref_coef, rtol=0, atol=0,
                          equal_nan=True)
    if bad == float("inf"):
        assert coef.item() == 0.0
    for a, b in zip(ours, theirs):
        assert torch.allclose(a, b.grad, rtol=0, atol=0, equal_nan=True)


@pytest.mark.parametrize("kind", ["mixed", "many_small", "offset1",
                                  "offset3", "slots"])
def test_scale_grads_matches_fp32_multiply(kind):
    ts = _segments(kind, seed=4)
    c = torch.tensor([0.3127], device="cuda")
    ref = [(t.float() * c).to(t.dtype) for t in ts]
    ops.scale_grads_(ts, c)
    for a, b in zip(ts, ref):
        assert torch.equal(a, b)


def test_scale_grads_by_one_leaves_bits_alone():
    ts = _segments("mixed", seed=5)
    ts[0][0] = float("nan")  # NaN * 1 would still be NaN, -0.0 stays -0.0
    ts[2][1] = -0.0
    before = [t.clone().view(torch.int32 if t.dtype == F32
                             else torch.int16) for t in ts]
    ops.scale_grads_(ts, torch.ones(1, device="cuda"))
    for a, b in zip(ts, before):
        assert torch.equal(a.view(b.dtype), b)


# ------------------------------------------------------------------ #
# fused optimizers with a device coefficient vs their eager fallback
# on fp32 copies fed g.float() * c
# ------------------------------------------------------------------ #
# A different coefficient at every step: Adam's update m/(sqrt(v)+eps) is
# unchanged when every gradient of every step is multiplied by one
# constant, so a single c could be dropped from a kernel unnoticed. With
# the scales mixed inside the moments it cannot. Each test also runs the
# same optimizer without the coefficient and asserts that it lands far
# outside the tolerance, separately for the elements the vector body
# handles and for the ones the scalar tail handles.
CS = [0.9, 0.05, 0.4]
FAR = 1e-4  # >= 33x the largest atol below


def _coef(step):
    return torch.tensor([CS[step]], device="cuda")


def _opt_inputs(pdtype, gdtype, seed):
    g = _gen(seed)
    params = [torch.nn.Parameter(_rand(s, pdtype, g)) for s in SIZES]
    grads = [[_rand(s, gdtype, g) for s in SIZES] for _ in range(3)]
    return params, grads


def _twin(params):
    return [torch.nn.Parameter(p.detach().clone()) for p in params]


def _assert_coefficient_matters(scaled, unscaled):
    """The kernels take 4 elements per lane: a tensor's last numel % 4
    elements go through the scalar tail, the rest through the vector
    body. Both must have moved with the coefficient."""
    body, tail = [], []
    for a, u in zip(scaled, unscaled):
        d = (a.detach().float() - u.detach().float()).abs().reshape(-1)
        cut = d.numel() - d.numel() % 4
        body.append(d[:cut])
        tail.append(d[cut:])
    body, tail = torch.cat(body), torch.cat(tail)
    assert tail.numel() == 8  # sizes 1, 3, 17 and 100003
    print(f"unscaled run differs: body max {float(body.max()):.3e} "
          f"tail max {float(tail.max()):.3e}")
    assert float(body.max()) > FAR and float(tail.max()) > FAR


def test_fused_sgd_with_coefficient():
    params, grads = _opt_inputs(F32, F32, 10)
    plain = _twin(params)
    ref = [p.detach().clone() for p in params]
    mom = [torch.zeros_like(p) for p in ref]
    opt = FusedSGD(params, lr=0.1, momentum=0.9, weight_decay=1e-4)
    opt_plain = FusedSGD(plain, lr=0.1, momentum=0.9, weight_decay=1e-4)
    group = opt.param_groups[0]
    for step in range(3):
        c = _coef(step)
        for p, u, g in zip(params, plain, grads[step]):
            p.grad = g.clone()
            u.grad = g.clone()
        opt.set_grad_scale(c)
        opt.step()
        opt_plain.step()
        FusedSGD._eager_step(ref, [g.float() * c for g in grads[step]],
                             mom, group, step == 0)
    for a, b in zip(params, ref):
        assert torch.allclose(a, b, atol=1e-6, rtol=1e-5), \
            f"max diff {(a - b).abs().max()}"
    _assert_coefficient_matters(params, plain)


def test_fused_adamw_with_coefficient():
    params, grads = _opt_inputs(F32, F32, 11)
    plain = _twin(params)
    ref = [p.detach().clone() for p in params]
    avgs = [torch.zeros_like(p) for p in ref]
    sqs = [torch.zeros_like(p) for p in ref]
    opt = FusedAdamW(params, lr=1e-3, weight_decay=0.01)
    opt_plain = FusedAdamW(plain, lr=1e-3, weight_decay=0.01)
    group = opt.param_groups[0]
    for step in range(3):
        c = _coef(step)
        for p, u, g in zip(params, plain, grads[step]):
            p.grad = g.clone()
            u.grad = g.clone()
        opt.set_grad_scale(c)
        opt.step()
        opt_plain.step()
        FusedAdamW._eager_step(ref, [g.float() * c for g in grads[step]],
                               avgs, sqs, group, step + 1)
    for a, b in zip(params, ref):
        assert torch.allclose(a, b, atol=2e-6, rtol=1e-5), \
            f"max diff {(a - b).abs().max()}"
    _assert_coefficient_matters(params, plain)


@pytest.mark.parametrize("gdtype", [BF16, F32], ids=["bf16", "f32"])
def test_sharded_adam_with_coefficient(gdtype):
    params, grads = _opt_inputs(BF16, gdtype, 12)
    plain = _twin(params)
    if gdtype != BF16:  # bf16 params holding fp32 grads
        for p in params + plain:
            p.grad_dtype = gdtype
    ref16 = [p.detach().clone() for p in params]
    masters = [p.detach().float().clone() for p in params]
    avgs = [torch.zeros_like(m) for m in masters]
    sqs = [torch.zeros_like(m) for m in masters]
    opt = ShardedFusedAdam(params, lr=1e-3, weight_decay=0.01)
    opt_plain = ShardedFusedAdam(plain, lr=1e-3, weight_decay=0.01)
    group = opt.param_groups[0]
    for step in range(3):
        c = _coef(step)
        for p, u, g in zip(params, plain, grads[step]):
            p.grad = g.clone()
            u.grad = g.clone()
        opt.set_grad_scale(c)
        opt.step()
        opt_plain.step()
        ShardedFusedAdam._eager_bf16(
            ref16, masters, [g.float() * c for g in grads[step]], avgs,
            sqs, group, step + 1)
    for p, m in zip(params, masters):
        got = opt.state[p]["master"]
        assert torch.allclose(got, m, atol=3e-6, rtol=1e-5), \
            f"max diff {(got - m).abs().max()}"
        assert torch.equal(p.detach(), got.to(BF16))
    _assert_coefficient_matters(
        [opt.state[p]["master"] for p in params],
        [opt_plain.state[u]["master"] for u in plain])


def test_other_dtypes_take_the_torch_math():
    """fp16/fp64 grads are outside the kernels' contract: same answers
    through torch instead of an error."""
    g = _gen(30)
    for dt in (torch.float16, torch.float64):
        ts = [_rand(1000, dt, g), _rand(17, dt, g)]
        ref = sum(t.double().pow(2).sum() for t in ts)
        got = ops.grad_sumsq(ts)
        assert got.dtype == F32 and got.shape == (1,)
        assert got.double().sqrt().item() == pytest.approx(
            ref.sqrt().item(), rel=1e-5)
        c = torch.tensor([0.25], device="cuda")
        want = [t * 0.25 for t in ts]  # a power of two: exact
        ops.scale_grads_(ts, c)
        for a, b in zip(ts, want):
            assert torch.equal(a, b)


def test_clip_and_step_never_read_back_to_the_host():
    params, grads = _opt_inputs(BF16, BF16, 13)
    params.append(torch.nn.Parameter(_rand(1000, F32, _gen(14))))
    opt = ShardedFusedAdam(params, lr=1e-3)
    for p in params:
        p.grad = torch.randn_like(p)
    opt.step()  # state allocation is not part of the hot path
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        sumsq = ops.grad_sumsq([p.grad for p in params])
        norm, coef = ops.clip_coef(sumsq, 0.5)
        opt.set_grad_scale(coef)
        opt.step()
        ops.scale_grads_([p.grad for p in params], coef)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert float(norm) > 0.5


# ------------------------------------------------------------------ #
# trainer on one GPU: tiny bf16 GPT-2, ShardedFusedAdam
# ------------------------------------------------------------------ #
GPT_CLIP = 0.05
# The reference clips in place, which rounds g*c to bf16 (2^-9 relative)
# and takes c from torch's bf16 norm (up to ~2^-9 more); the deferred
# path keeps g*c in fp32. Adam's update is at most ~lr per step and moves
# by about that relative amount, so at lr=1e-4 two steps differ by
# < 1e-6, inside the 3e-6 the sharded-Adam tests allow.
GPT_LR = 1e-4
# Adam with its usual eps=1e-8 barely sees a coefficient that is almost
# the same at both steps: m/(sqrt(v)+eps) cancels it. The clipped
# gradient has norm 0.05 over 3.3e5 elements, an rms of 9e-5, so eps=1e-4
# puts the update g*c/(|g*c|+eps) on its slope, where clipped and
# unclipped gradients give clearly different steps. The test asserts
# that against an unclipped reference.
GPT_EPS = 1e-4


class _TinyGPT(LightningModule):
    def __init__(self):
        super().__init__()
        from ray_lightning_amd.models.gpt2 import (GPT2, GPT2Config,
                                                   to_bf16_training)
        torch.manual_seed(21)
        self.cfg = GPT2Config(vocab_size=512, n_positions=64, n_embd=128,
                              n_layer=2, n_head=2)
        self.net = to_bf16_training(GPT2(self.cfg))
        self.seen_grads = []

    def training_step(self, batch, batch_idx):
        x, y = batch
        _, loss = self.net(x, y)
        return loss

    def on_after_backward(self):
        # the very grads the trainer is about to clip
        self.seen_grads.append([p.grad.clone() for p in self.parameters()])

    def configure_optimizers(self):
        return ShardedFusedAdam(self.parameters(), lr=GPT_LR,
                                eps=GPT_EPS, weight_decay=0.01)

    def train_dataloader(self):
        g = torch.Generator().manual_seed(22)
        x = torch.randint(0, 512, (4, 64), generator=g)
        y = torch.randint(0, 512, (4, 64), generator=g)
        return DataLoader(TensorDataset(x, y), batch_size=2)


class _KeepNorm(Callback):
    def __init__(self):
        self.norms = []

    def on_train_batch_end(self, trainer, pl_module, outputs, batch,
                           batch_idx):
        self.norms.append(trainer.last_grad_norm)


def test_trainer_gpt2_clip_matches_torch_clip(tmp_path):
    """Two trainer steps (HIP norm, coefficient deferred into the sharded
    Adam kernel) against torch clipping in place and then stepping.

    The reference is fed the gradients the trainer saw rather than
    running its own forward/backward. Two independent bf16 runs do not
    stay comparable past the first step: ~1e-7 differences in the
    masters flip a few bf16 roundings of the parameters, the second
    backward then differs in its noise-level gradient elements, and Adam
    turns a sign flip there into an lr-sized difference. Measured on an
    MI355X: 1.2e-4 between two runs that both clip with torch in place
    and differ only in whether the coefficient came from a bf16 or an
    fp32 norm, while their first steps agree to 1.9e-7. With the same
    gradients on both sides the comparison measures the clip and the
    step, at the tolerances the sharded-Adam tests use.

    ``last_grad_norm`` is compared at rtol=1e-3 with
    ``torch.nn.utils.clip_grad_norm_`` over the same gradient values held
    in fp32. Over the bf16 tensors themselves torch rounds every
    per-tensor norm to bf16, half an ulp of which is up to 2^-8 = 3.9e-3
    relative, so that figure can miss 1e-3 on its own account: measured
    here, 2.881778 against 2.884799 from the kernel (1.05e-3), where the
    kernel agrees with an fp64 sum to 1e-7 in the sum-of-squares tests.
    It is printed, and it is still what clips the reference in place."""
    seed_everything(20)
    model = _TinyGPT()
    init = [p.detach().clone() for p in model.parameters()]
    rec = _KeepNorm()
    trainer = Trainer(default_root_dir=str(tmp_path), max_epochs=1,
                      limit_train_batches=2, enable_checkpointing=False,
                      num_sanity_val_steps=0, callbacks=[rec],
                      gradient_clip_val=GPT_CLIP)
    trainer.fit(model)
    opt = trainer.optimizers[0]
    assert len(rec.norms) == 2 and len(model.seen_grads) == 2

    ref = [torch.nn.Parameter(t.cuda()) for t in init]
    ref_opt = ShardedFusedAdam(ref, lr=GPT_LR, eps=GPT_EPS,
                               weight_decay=0.01)
    raw = [torch.nn.Parameter(t.cuda()) for t in init]  # never clipped
    raw_opt = ShardedFusedAdam(raw, lr=GPT_LR, eps=GPT_EPS,
                               weight_decay=0.01)
    for ours, grads in zip(rec.norms, model.seen_grads):
        for q, u, g in zip(ref, raw, grads):
            q.grad = g.clone()
            u.grad = g.clone()
        # torch's norm of the same gradient values, held in fp32
        twins = []
        for g in grads:
            t = torch.empty_like(g, dtype=F32)
            t.grad = g.float()
            twins.append(t)
        theirs = torch.nn.utils.clip_grad_norm_(twins, float("inf"))
        theirs16 = torch.nn.utils.clip_grad_norm_(ref, GPT_CLIP)
        ref_opt.step()
        raw_opt.step()
        print(f"norm ours {float(ours)!r} torch {float(theirs)!r} "
              f"torch on bf16 {float(theirs16)!r}")
        assert float(theirs) > GPT_CLIP  # clipping is active
        assert float(ours) == pytest.approx(float(theirs), rel=1e-3)

    worst = 0.0
    n_far = 0
    for p, q, u in zip(model.parameters(), ref, raw):
        a = opt.state[p].get("master", p.detach()).cpu()
        b = ref_opt.state[q].get("master", q.detach()).cpu()
        c = raw_opt.state[u].get("master", u.detach()).cpu()
        worst = max(worst, float((a - b).abs().max()))
        assert torch.allclose(a, b, atol=3e-6, rtol=1e-5), \
            f"max diff {(a - b).abs().max()}"
        # the same steps without clipping are nowhere near: every
        # tensor, bf16 or fp32, moved with the coefficient
        far = float((a - c).abs().max())
        assert far > 10 * 3e-6, f"unclipped run within {far:.3e}"
        n_far += 1
    print(f"max master diff {worst:.3e} over {n_far} tensors")

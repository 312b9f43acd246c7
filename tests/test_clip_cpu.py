"""Global-norm gradient clipping on CPU: the sharded engine clips by the
norm of the WHOLE model on every rank (world-2 gloo), the trainer
dispatches to it, and the fused optimizers' deferred coefficient equals
pre-scaled gradients."""
import json
import multiprocessing as mp
import os

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from ray_lightning_amd import (Callback, LightningModule, RayShardedStrategy,
                               RayStrategy, Trainer, seed_everything)
from ray_lightning_amd.strategies import SingleDeviceStrategy
from ray_lightning_amd.optim import FusedAdamW, FusedSGD, ShardedFusedAdam
from ray_lightning_amd.util import find_free_port

_MP = mp.get_context("spawn")
WORLD = 2
LR = 0.1


# ------------------------------------------------------------------ #
# engine level, world-2 gloo
# ------------------------------------------------------------------ #
def _make_model(seed: int = 0) -> torch.nn.Sequential:
    g = torch.Generator().manual_seed(seed)
    m = torch.nn.Sequential(
        torch.nn.Linear(16, 32), torch.nn.ReLU(),
        torch.nn.Linear(32, 4))
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return m


def _make_single_param_model(seed: int = 0) -> torch.nn.Module:
    g = torch.Generator().manual_seed(seed)
    m = torch.nn.Linear(16, 4, bias=False)
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 0.1)
    return m


def _rank_batch(rank: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(100 + rank)
    return torch.randn(8, 16, generator=g)


def _reference(make_model):
    """Single process: average both ranks' grads, measure the total
    norm, clip to half of it with torch, plain SGD step."""
    model = make_model()
    grads = None
    for r in range(WORLD):
        model.zero_grad()
        model(_rank_batch(r)).pow(2).mean().backward()
        cur = [p.grad.clone() for p in model.parameters()]
        grads = cur if grads is None else [a + b
                                           for a, b in zip(grads, cur)]
    for p, g in zip(model.parameters(), grads):
        p.grad = g / WORLD
    total = torch.linalg.vector_norm(torch.stack(
        [torch.linalg.vector_norm(p.grad) for p in model.parameters()]))
    max_norm = float(total) / 2
    # where the same step lands without clipping: the tests assert that
    # this is far outside the tolerance, so a dropped coefficient fails
    unclipped = [p.detach() - LR * p.grad for p in model.parameters()]
    norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
    torch.optim.SGD(model.parameters(), lr=LR).step()
    expected = [p.detach() for p in model.parameters()]
    assert all((e - u).abs().max() > 1e-4
               for e, u in zip(expected, unclipped))
    return max_norm, float(norm), expected


def _worker(rank: int, port: int, single: bool, inner: str,
            max_norm: float, out_q) -> None:
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        from ray_lightning_amd.engine.comm import (TorchDistCommunicator,
                                                   init_control_plane)
        from ray_lightning_amd.engine.sharded import (ShardedDDP,
                                                      ShardedOptimizer)
        init_control_plane(rank, WORLD)
        comm = TorchDistCommunicator()
        make = _make_single_param_model if single else _make_model
        model = make(seed=rank)  # wrap-time broadcast equalizes replicas
        opt = (FusedSGD(model.parameters(), lr=LR) if inner == "fused_sgd"
               else torch.optim.SGD(model.parameters(), lr=LR))
        oss = ShardedOptimizer(opt, comm, bucket_cap_mb=0.0001)
        sddp = ShardedDDP(model, comm, oss, bucket_cap_mb=0.0001)
        model(_rank_batch(rank)).pow(2).mean().backward()
        sddp.finalize_backward()
        owned = sum(p.grad is not None for p in model.parameters())
        before = [None if p.grad is None else p.grad.clone()
                  for p in model.parameters()]
        norm = oss.clip_grad_norm(max_norm)
        # deferred: the coefficient waits in the inner optimizer and the
        # grads are untouched; otherwise they were scaled in place
        deferred = getattr(oss.optim, "_grad_scale", None) is not None
        untouched = all(b is None or torch.equal(b, p.grad)
                        for b, p in zip(before, model.parameters()))
        oss.step()
        out_q.put((rank, "ok", {
            "norm": float(norm), "owned": owned,
            "deferred": deferred, "untouched": untouched,
            "params": [p.detach().clone().numpy()
                       for p in model.parameters()]}))
    except BaseException as e:  # noqa: BLE001
        import traceback
        out_q.put((rank, "err", f"{e}\n{traceback.format_exc()}"))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()


def _run_workers(single: bool, inner: str, max_norm: float):
    port = find_free_port()
    q = _MP.Queue()
    procs = [_MP.Process(target=_worker,
                         args=(r, port, single, inner, max_norm, q))
             for r in range(WORLD)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(WORLD):
            rank, status, payload = q.get(timeout=120)
            assert status == "ok", f"rank {rank} failed:\n{payload}"
            results[rank] = payload
        for p in procs:
            p.join(30)
            assert not p.is_alive(), "worker did not exit"
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    return results


@pytest.mark.parametrize("inner", ["sgd", "fused_sgd"])
def test_sharded_clip_matches_whole_model_clip(inner):
    """torch SGD takes the in-place scale; FusedSGD has set_grad_scale,
    so the coefficient is deferred into its step."""
    max_norm, ref_norm, expected = _reference(_make_model)
    assert ref_norm > max_norm  # clipping is active by construction
    results = _run_workers(False, inner, max_norm)
    for rank in range(WORLD):
        assert results[rank]["owned"] > 0
        assert results[rank]["deferred"] == (inner == "fused_sgd")
        assert results[rank]["untouched"] == (inner == "fused_sgd")
        assert results[rank]["norm"] == pytest.approx(ref_norm, rel=1e-5)
        for got, e in zip(results[rank]["params"], expected):
            assert torch.allclose(torch.from_numpy(got), e, atol=1e-6), \
                f"rank {rank} param mismatch"
    assert results[0]["norm"] == results[1]["norm"]


def test_rank_without_grads_still_joins_the_collective():
    max_norm, ref_norm, expected = _reference(_make_single_param_model)
    assert ref_norm > max_norm
    results = _run_workers(True, "sgd", max_norm)
    assert sorted(r["owned"] for r in results.values()) == [0, 1]
    assert results[0]["norm"] == results[1]["norm"]
    for rank in range(WORLD):
        assert results[rank]["norm"] == pytest.approx(ref_norm, rel=1e-5)
        for got, e in zip(results[rank]["params"], expected):
            assert torch.allclose(torch.from_numpy(got), e, atol=1e-6)


# ------------------------------------------------------------------ #
# trainer level
# ------------------------------------------------------------------ #
class _ClipModel(LightningModule):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.net = torch.nn.Sequential(
            torch.nn.Linear(32, 16), torch.nn.ReLU(),
            torch.nn.Linear(16, 2))
        with torch.no_grad():
            for p in self.net.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)

    def forward(self, x):
        return self.net(x)

    def training_step(self, batch, batch_idx):
        (x,) = batch
        out = self(x)
        return torch.nn.functional.mse_loss(out, torch.ones_like(out))

    def configure_optimizers(self):
        return torch.optim.SGD(self.parameters(), lr=0.05)

    def train_dataloader(self):
        g = torch.Generator().manual_seed(11)
        return DataLoader(TensorDataset(torch.randn(64, 32, generator=g)),
                          batch_size=4)


class _NormRecorder(Callback):
    """Writes each step's ``trainer.last_grad_norm`` to a per-rank file
    (callbacks run inside the workers)."""

    def __init__(self, out_dir: str):
        self.out_dir = out_dir
        self.norms = []

    def on_train_batch_end(self, trainer, pl_module, outputs, batch,
                           batch_idx):
        n = trainer.last_grad_norm
        self.norms.append(None if n is None else float(n))

    def on_train_end(self, trainer, pl_module):
        path = os.path.join(self.out_dir,
                            f"norms_rank{trainer.global_rank}.json")
        with open(path, "w") as f:
            json.dump(self.norms, f)


CLIP_VAL = 0.05
STEPS = 8


def _fit(tmp_path, name, strategy, clip):
    out_dir = tmp_path / name
    out_dir.mkdir()
    seed_everything(5)
    model = _ClipModel()
    trainer = Trainer(default_root_dir=str(out_dir), max_epochs=1,
                      limit_train_batches=STEPS, strategy=strategy,
                      callbacks=[_NormRecorder(str(out_dir))],
                      enable_checkpointing=False, num_sanity_val_steps=0,
                      gradient_clip_val=clip)
    trainer.fit(model)
    weights = torch.cat([p.detach().flatten() for p in model.parameters()])
    norms = []
    for r in range(WORLD):
        with open(out_dir / f"norms_rank{r}.json") as f:
            norms.append(json.load(f))
    return weights, norms


def test_trainer_ddp_and_sharded_agree_under_clipping(tmp_path):
    """RayStrategy and RayShardedStrategy end at the same weights when
    both clip by the whole model's norm.

    Unclipped (``_fit(..., clip=None)`` for each strategy, then the max
    abs difference of the two weight vectors), the two strategies differ
    by exactly 0.0: same averaged grads, same SGD. So atol=1e-5 stands
    for the clipped comparison."""
    w_ddp, n_ddp = _fit(tmp_path, "ddp", RayStrategy(num_workers=WORLD),
                        CLIP_VAL)
    w_sh, n_sh = _fit(tmp_path, "sharded",
                      RayShardedStrategy(num_workers=WORLD), CLIP_VAL)
    for norms in n_ddp + n_sh:
        assert len(norms) == STEPS
        # clipping is active at every step
        assert all(n is not None and n > CLIP_VAL for n in norms), norms
    # every rank saw the same global norm, under both strategies
    assert n_sh[0] == n_sh[1]
    for a, b in zip(n_ddp[0], n_sh[0]):
        assert a == pytest.approx(b, rel=1e-4)
    assert torch.allclose(w_ddp, w_sh, atol=1e-5), \
        f"max diff {(w_ddp - w_sh).abs().max()}"


# ------------------------------------------------------------------ #
# unit tests
# ------------------------------------------------------------------ #
SIZES = [3, 17, 256, 1000]


def _params(dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(dtype))
            for s in SIZES]


def _grads(step, dtype=torch.float32, seed=1):
    g = torch.Generator().manual_seed(seed + step)
    return [torch.randn(s, generator=g).to(dtype) for s in SIZES]


# A different coefficient at every step: Adam's update m/(sqrt(v)+eps) is
# unchanged when every gradient of every step is multiplied by one
# constant, so a single c could be dropped unnoticed. With the scales
# mixed inside the moments it cannot, and each test also asserts that the
# result without the coefficient is far outside the tolerance.
CS = [0.9, 0.05, 0.4]
FAR = 1e-4  # 100x the atol below


@pytest.mark.parametrize("make_opt", [
    lambda ps: FusedSGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-4),
    lambda ps: FusedAdamW(ps, lr=1e-3, weight_decay=0.01),
    lambda ps: ShardedFusedAdam(ps, lr=1e-3, weight_decay=0.01),
], ids=["sgd", "adamw", "sharded_adam_f32"])
def test_eager_coefficient_equals_prescaled_grads(make_opt):
    pa, pb, pu = _params(), _params(), _params()
    oa, ob, ou = make_opt(pa), make_opt(pb), make_opt(pu)
    for step in range(3):
        c = torch.tensor([CS[step]])
        for p, q, u, g in zip(pa, pb, pu, _grads(step)):
            p.grad = g.clone()
            q.grad = g * c
            u.grad = g.clone()
        oa.set_grad_scale(c)
        oa.step()
        ob.step()
        ou.step()  # the same grads with the coefficient left out
    for a, b, u in zip(pa, pb, pu):
        assert torch.allclose(a, b, atol=1e-6, rtol=1e-5)
        assert (a - u).abs().max() > FAR


def _bf16_twin(coefs):
    """``_eager_bf16`` fed pre-scaled fp32 grads (bf16 grads cannot hold
    g*c, so the twin bypasses .grad). Returns the masters."""
    pb = _params(torch.bfloat16)
    masters = [p.detach().float().clone() for p in pb]
    avgs = [torch.zeros_like(m) for m in masters]
    sqs = [torch.zeros_like(m) for m in masters]
    group = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.01, adamw=True)
    for step in range(3):
        pre = [g.float() * coefs[step]
               for g in _grads(step, torch.bfloat16)]
        ShardedFusedAdam._eager_bf16(
            [p.data for p in pb], masters, pre, avgs, sqs, group,
            step + 1)
    return masters


def test_eager_bf16_coefficient_equals_prescaled_fp32_grads():
    pa = _params(torch.bfloat16)
    oa = ShardedFusedAdam(pa, lr=1e-3, weight_decay=0.01)
    for step in range(3):
        for p, g in zip(pa, _grads(step, torch.bfloat16)):
            p.grad = g.clone()
        oa.set_grad_scale(torch.tensor([CS[step]]))
        oa.step()
    for p, m, u in zip(pa, _bf16_twin(CS), _bf16_twin([1.0] * 3)):
        got = oa.state[p]["master"]
        assert torch.allclose(got, m, atol=1e-6, rtol=1e-5)
        assert (got - u).abs().max() > FAR


@pytest.mark.parametrize("cls", [FusedSGD, FusedAdamW, ShardedFusedAdam])
def test_grad_scale_is_cleared_after_one_step(cls):
    pa, pb = _params(), _params()
    oa, ob = cls(pa, lr=0.01), cls(pb, lr=0.01)
    for p, q, g in zip(pa, pb, _grads(0)):
        p.grad = g.clone()
        q.grad = g.clone()
    oa.set_grad_scale(torch.tensor([0.5]))
    oa.step()
    assert oa._grad_scale is None
    for p, q in zip(pa, pb):      # restart both from the same point
        q.data.copy_(p.data)
    oa.state.clear()
    ob.state.clear()
    oa.step()                     # no coefficient set: must not reuse 0.5
    ob.step()
    for p, q in zip(pa, pb):
        assert torch.equal(p, q)


def _one_param_step(tmp_path, **trainer_kwargs):
    seed_everything(9)
    model = _ClipModel()
    # explicitly the CPU: the default strategy picks cuda:0 when one is
    # visible, and these tests are about the CPU branch
    trainer = Trainer(default_root_dir=str(tmp_path), max_epochs=1,
                      strategy=SingleDeviceStrategy(torch.device("cpu")),
                      limit_train_batches=3, enable_checkpointing=False,
                      num_sanity_val_steps=0, **trainer_kwargs)
    trainer.fit(model)
    return trainer, model


def _manual_steps(clip_fn):
    """The trainer's three SGD steps by hand, with ``clip_fn(params)``
    between backward and step."""
    seed_everything(9)
    model = _ClipModel()
    opt = model.configure_optimizers()
    for i, batch in enumerate(model.train_dataloader()):
        if i >= 3:
            break
        loss = model.training_step(batch, i)
        loss.backward()
        clip_fn(list(model.parameters()))
        opt.step()
        opt.zero_grad(set_to_none=True)
    return model


def test_cpu_single_process_clip_is_bit_identical_to_torch(tmp_path):
    trainer, model = _one_param_step(tmp_path, gradient_clip_val=CLIP_VAL)
    ref = _manual_steps(
        lambda ps: torch.nn.utils.clip_grad_norm_(ps, CLIP_VAL))
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.equal(p, q)
    assert float(trainer.last_grad_norm) > CLIP_VAL


def test_clip_by_value_clamps(tmp_path):
    clip = 0.01
    trainer, model = _one_param_step(tmp_path, gradient_clip_val=clip,
                                     gradient_clip_algorithm="value")
    ref = _manual_steps(
        lambda ps: torch.nn.utils.clip_grad_value_(ps, clip))
    unclipped = _manual_steps(lambda ps: None)
    for p, q, u in zip(model.parameters(), ref.parameters(),
                       unclipped.parameters()):
        assert torch.equal(p, q)
    assert any(not torch.equal(q, u) for q, u in
               zip(ref.parameters(), unclipped.parameters()))
    # lr * clip bounds every element's per-step movement
    init = _ClipModel()
    for p, p0 in zip(model.parameters(), init.parameters()):
        assert (p - p0).abs().max() <= 3 * 0.05 * clip + 1e-7


def test_bad_clip_algorithm_raises():
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        Trainer(gradient_clip_val=1.0, gradient_clip_algorithm="nope")

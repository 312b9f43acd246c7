"""Sharded data-parallel engine (ZeRO-1/2-style).

MI355X-native replacement for the FairScale OSS + ShardedDataParallel
stack the reference reaches through PTL's ``DDPSpawnShardedStrategy``
(reference ray_ddp_sharded.py:11-13):

- ``ShardedOptimizer`` (OSS): parameters are greedily partitioned across
  ranks by numel; each rank instantiates the inner optimizer *only for
  its owned shard*, so optimizer state is 1/N per GPU — the memory
  reduction the reference claims qualitatively (README.md:127-128).
- ``ShardedDDP``: gradients are bucketed **by owner rank** and
  asynchronously *reduced to the owner* during backward (RCCL reduce
  over xGMI on the comm side stream); after the owner's optimizer step,
  updated params are broadcast back owner->all in flat buckets
  (the reduce-scatter + all-gather message pattern of SURVEY.md N6).
- On GPU the owner's step can use the fused sharded Adam HIP kernel via
  the optimizer passed in (see ``ray_lightning_amd.optim``).
"""
from __future__ import annotations

import contextlib
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from .comm import Communicator, Work


def partition_params(params: List[nn.Parameter],
                     world_size: int) -> List[List[nn.Parameter]]:
    """Greedy balanced partition by numel (stable across ranks: inputs are
    iterated in registration order)."""
    shards: List[List[nn.Parameter]] = [[] for _ in range(world_size)]
    sizes = [0] * world_size
    for p in sorted(params, key=lambda p: -p.numel()):
        i = sizes.index(min(sizes))
        shards[i].append(p)
        sizes[i] += p.numel()
    return shards


class ShardedOptimizer(torch.optim.Optimizer):
    """OSS-style wrapper: rebuilds the user's optimizer over only the
    params this rank owns; ``step`` then broadcasts updated params from
    their owners in flat buckets."""

    def __init__(self, optimizer: torch.optim.Optimizer,
                 comm: Communicator, bucket_cap_mb: float = 25.0):
        self.comm = comm
        self.world_size = comm.world_size
        self.rank = comm.rank
        self._all_params: List[nn.Parameter] = [
            p for g in optimizer.param_groups for p in g["params"]]
        # Original group membership as global indices — consolidated
        # checkpoints must keep the param→group assignment (per-group
        # lr/weight_decay) like torch/fairscale, not claim every index in
        # every group.
        _gidx = {p: i for i, p in enumerate(self._all_params)}
        self._group_global_indices: List[List[int]] = [
            [_gidx[p] for p in g["params"]] for g in optimizer.param_groups]
        self._shards = partition_params(self._all_params, self.world_size)
        self._owner: Dict[nn.Parameter, int] = {}
        for r, shard in enumerate(self._shards):
            for p in shard:
                self._owner[p] = r

        # Rebuild the inner optimizer with only owned params (keep group
        # hyperparameters; empty groups are preserved so LR schedulers
        # keep working).
        owned = set(self._shards[self.rank])
        inner_groups = []
        for g in optimizer.param_groups:
            ng = {k: v for k, v in g.items() if k != "params"}
            ng["params"] = [p for p in g["params"] if p in owned]
            inner_groups.append(ng)
        self.optim = type(optimizer)(inner_groups, **optimizer.defaults)

        # Flat broadcast buckets per owner rank.
        self._bcast_buckets: List[Tuple[int, List[nn.Parameter],
                                        torch.Tensor]] = []
        cap = int(bucket_cap_mb * 1024 * 1024)
        for r, shard in enumerate(self._shards):
            cur: List[nn.Parameter] = []
            cur_bytes = 0
            for p in shard:
                nbytes = p.numel() * p.element_size()
                if cur and (cur_bytes + nbytes > cap
                            or p.dtype != cur[0].dtype
                            or p.device != cur[0].device):
                    self._seal_bucket(r, cur)
                    cur, cur_bytes = [], 0
                cur.append(p)
                cur_bytes += nbytes
            if cur:
                self._seal_bucket(r, cur)

        super().__init__([{"params": self._all_params,
                           **optimizer.defaults}], optimizer.defaults)
        # expose the inner groups for LR schedulers. They hold only this
        # rank's shard, so a norm taken over them is a per-shard norm:
        # global-norm clipping goes through clip_grad_norm() below.
        self.param_groups = self.optim.param_groups

    def _seal_bucket(self, rank: int, params: List[nn.Parameter]) -> None:
        numel = sum(p.numel() for p in params)
        flat = torch.empty(numel, dtype=params[0].dtype,
                           device=params[0].device)
        self._bcast_buckets.append((rank, list(params), flat))

    def owner_of(self, p: nn.Parameter) -> int:
        return self._owner[p]

    @torch.no_grad()
    def step(self, closure=None):
        loss = self.optim.step(closure)
        self._broadcast_params()
        return loss

    @torch.no_grad()
    def clip_grad_norm(self, max_norm: float,
                       defer: bool = True) -> torch.Tensor:
        """Clip to the L2 norm of the WHOLE model's gradient and return
        that norm (FairScale OSS ``clip_grad_norm``). Call it after
        ``ShardedDDP.finalize_backward``: each rank then holds exactly
        the reduced grads of the shard it owns, so the global sum of
        squares is the all-reduced sum of the per-rank ones.

        Every rank issues the all-reduce exactly once per call — a rank
        that owns no gradient contributes zero — so the collective order
        never diverges. The coefficient stays on the device; an inner
        optimizer with ``set_grad_scale`` folds it into its next step,
        otherwise (or with ``defer=False``, e.g. under a GradScaler that
        inspects the grads itself) the owned grads are scaled in place.
        """
        from .. import ops
        grads = [p.grad for g in self.optim.param_groups
                 for p in g["params"] if p.grad is not None]
        device = (grads[0].device if grads else
                  self._all_params[0].device if self._all_params else None)
        sumsq = ops.grad_sumsq(grads, device=device)
        if self.world_size > 1:
            self.comm.all_reduce_(sumsq, op="sum")
        norm, coef = ops.clip_coef(sumsq, max_norm)
        if defer and hasattr(self.optim, "set_grad_scale"):
            self.optim.set_grad_scale(coef)
        else:
            ops.scale_grads_(grads, coef)
        return norm.reshape(())

    def _broadcast_params(self) -> None:
        if self.world_size <= 1:
            return
        works: List[Work] = []
        for r, params, flat in self._bcast_buckets:
            if r == self.rank:
                off = 0
                for p in params:
                    flat[off:off + p.numel()].copy_(p.data.reshape(-1))
                    off += p.numel()
            works.append(self.comm.broadcast_(flat, src=r, async_op=True))
        for (r, params, flat), w in zip(self._bcast_buckets, works):
            w.wait()
            if r != self.rank:
                off = 0
                for p in params:
                    p.data.copy_(
                        flat[off:off + p.numel()].view_as(p))
                    off += p.numel()

    def zero_grad(self, set_to_none: bool = True):
        for p in self._all_params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    # -- checkpoint support -------------------------------------------------
    def state_dict(self) -> Dict:
        """Consolidated state dict: every rank contributes its shard via
        the control plane so rank 0 can checkpoint the full optimizer
        (FairScale consolidate_state_dict equivalent)."""
        local = self.optim.state_dict()
        if self.world_size <= 1:
            return {"consolidated": local, "world_size": 1}
        # Map local param indices to global indices. NOTE: local
        # indices follow the INNER optimizer's group order (the greedy
        # shard order differs — using it mislabels every entry).
        gidx = {p: i for i, p in enumerate(self._all_params)}
        inner_params = [p for g in self.optim.param_groups
                        for p in g["params"]]
        local_to_global = [gidx[p] for p in inner_params]
        shard_payload = {"state": local["state"],
                         "local_to_global": local_to_global}
        gathered = [None] * self.world_size
        try:
            import torch.distributed as dist
            dist.all_gather_object(gathered, shard_payload)
        except Exception:
            gathered = [shard_payload]
        state: Dict = {}
        for payload in gathered:
            if payload is None:
                continue
            for li, gi in enumerate(payload["local_to_global"]):
                if li in payload["state"]:
                    state[gi] = payload["state"][li]
                elif str(li) in payload["state"]:
                    state[gi] = payload["state"][str(li)]
        return {"consolidated": {"state": state,
                                 "param_groups": [
                                     {**g, "params": list(gi)}
                                     for g, gi in zip(
                                         self.optim.param_groups,
                                         self._group_global_indices)]},
                "world_size": self.world_size}

    def load_state_dict(self, state_dict: Dict) -> None:
        full = state_dict.get("consolidated", state_dict)
        gstate = full.get("state", {})
        # Select this rank's shard out of the consolidated state
        # (local indices = inner-optimizer group order).
        gidx = {p: i for i, p in enumerate(self._all_params)}
        inner_params = [p for g in self.optim.param_groups
                        for p in g["params"]]
        local_state = {}
        for li, p in enumerate(inner_params):
            gi = gidx[p]
            if gi in gstate:
                local_state[li] = gstate[gi]
            elif str(gi) in gstate:
                local_state[li] = gstate[str(gi)]
        inner = self.optim.state_dict()
        inner["state"] = local_state
        try:
            self.optim.load_state_dict(inner)
        except (ValueError, KeyError) as e:
            from ..util import rank_zero_warn
            rank_zero_warn(
                f"Sharded optimizer state restore dropped for "
                f"{type(self.optim).__name__} ({type(e).__name__}: {e}); "
                "continuing with fresh state (expected only on "
                "world-size-change resume).")


class ShardedDDP(nn.Module):
    """Gradient engine for the sharded path: buckets grouped by owner
    rank, async reduce-to-owner overlapped with backward."""

    def __init__(self, module: nn.Module, comm: Communicator,
                 sharded_optimizer: ShardedOptimizer,
                 bucket_cap_mb: float = 25.0, average: bool = True,
                 **_ignored):
        super().__init__()
        self.module = module
        self.comm = comm
        self.oss = sharded_optimizer
        self.average = average
        self._sync_enabled = True
        self._hooks = []
        self._next_bucket = 0

        cap = int(bucket_cap_mb * 1024 * 1024)
        self._buckets = []  # (owner, params, flat, offsets, ready)
        self._param_to_bucket: Dict[nn.Parameter, list] = {}
        for r, shard in enumerate(self.oss._shards):
            cur: List[nn.Parameter] = []
            cur_bytes = 0
            for p in [p for p in shard if p.requires_grad][::-1]:
                nbytes = p.numel() * p.element_size()
                if cur and (cur_bytes + nbytes > cap
                            or p.dtype != cur[0].dtype
                            or p.device != cur[0].device):
                    self._seal(r, cur)
                    cur, cur_bytes = [], 0
                cur.append(p)
                cur_bytes += nbytes
            if cur:
                self._seal(r, cur)

        self._sync_initial_state()
        for p in self._param_to_bucket:
            self._hooks.append(
                p.register_post_accumulate_grad_hook(self._grad_ready))

    def _seal(self, owner: int, params: List[nn.Parameter]) -> None:
        from .ddp import _align8
        offsets = {}
        off = 0
        for p in params:
            offsets[p] = off
            off += _align8(p.numel())
        numel = off
        flat = torch.zeros(numel, dtype=params[0].dtype,
                           device=params[0].device)
        bucket = {"owner": owner, "params": params, "flat": flat,
                  "offsets": offsets, "ready": set(), "work": None,
                  "reduced": False}
        self._buckets.append(bucket)
        for p in params:
            self._param_to_bucket[p] = bucket

    def _sync_initial_state(self) -> None:
        if self.comm.world_size <= 1:
            return
        for t in self.module.state_dict().values():
            if isinstance(t, torch.Tensor) and t.numel() > 0:
                self.comm.broadcast_(t.data, src=0)

    def _grad_ready(self, param: nn.Parameter) -> None:
        if not self._sync_enabled or self.comm.world_size <= 1:
            return
        b = self._param_to_bucket[param]
        b["ready"].add(param)
        if len(b["ready"]) == len(b["params"]):
            # launch strictly in bucket-index order: RCCL requires a
            # uniform collective issue order across ranks (see
            # NativeDDP._maybe_launch_in_order).
            self._maybe_launch_in_order()

    def _maybe_launch_in_order(self) -> None:
        while self._next_bucket < len(self._buckets):
            b = self._buckets[self._next_bucket]
            if b["reduced"]:
                self._next_bucket += 1
                continue
            if len(b["ready"]) == len(b["params"]):
                self._launch(b)
                self._next_bucket += 1
            else:
                break

    def _launch(self, b) -> None:
        from .. import ops
        grads, slots = [], []
        for p in b["params"]:
            off = b["offsets"][p]
            slot = b["flat"][off:off + p.numel()]
            if p.grad is None:
                slot.zero_()
            else:
                grads.append(p.grad)
                slots.append(slot)
        ops.pack_grads(slots, grads)
        b["work"] = self.comm.reduce_(b["flat"], dst=b["owner"], op="sum",
                                      async_op=True)
        b["reduced"] = True

    def finalize_backward(self) -> None:
        if self.comm.world_size <= 1 or not self._sync_enabled:
            return
        rank = self.comm.rank
        for b in self._buckets:
            if not b["reduced"]:
                self._launch(b)
        for b in self._buckets:
            if b["work"] is not None:
                b["work"].wait()
                b["work"] = None
        scale = 1.0 / self.comm.world_size if self.average else 1.0
        for b in self._buckets:
            if b["owner"] == rank:
                if scale != 1.0:
                    b["flat"].mul_(scale)
                for p in b["params"]:
                    off = b["offsets"][p]
                    p.grad = b["flat"][off:off + p.numel()].view_as(p)
            else:
                # ZeRO-2: non-owners drop their grads (grad memory 1/N).
                for p in b["params"]:
                    p.grad = None
            b["ready"].clear()
            b["reduced"] = False
        self._next_bucket = 0

    @contextlib.contextmanager
    def no_sync(self):
        old = self._sync_enabled
        self._sync_enabled = False
        try:
            yield
        finally:
            self._sync_enabled = old

    def forward(self, batch, batch_idx):
        return self.module.training_step(batch, batch_idx)

    def state_dict(self, *args, **kwargs):
        return self.module.state_dict(*args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        return self.module.load_state_dict(*args, **kwargs)

    def train(self, mode: bool = True):
        self.module.train(mode)
        return self

    def eval(self):
        self.module.eval()
        return self

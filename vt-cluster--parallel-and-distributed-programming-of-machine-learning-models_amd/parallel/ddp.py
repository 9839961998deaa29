"""Data-parallel gradient reduction over the flat LoRA arena (RCCL over xGMI).

Replaces HF Trainer -> torch DDP (reference C16, X6/X7) with a design sized
for LoRA on MI355X:
  * no parameter broadcast at construction: every rank builds identical
    weights from the same seed / file, and ``verify_replicas`` checks a
    checksum (all-reduce of MAX-MIN) instead of broadcasting 329 MB (X6);
  * the gradient arena is split into buckets in *reverse* module order;
    readiness is counted per tensor and each bucket's async all-reduce (SUM —
    the loss is already normalised by the global token count) launches as
    soon as its last tensor is done, overlapping the rest of backward;
    ``finish()`` waits for all handles.  Readiness comes from two sources:
    the fused GPU blocks write LoRA grads straight into the arena and call
    ``arena.grad_ready(offsets)`` after queueing an adapter's wgrad kernels
    (mift.ops.fused), the eager path from post-accumulate-grad hooks.  A tensor
    the fused forward claimed (``arena.grad_claim``) counts through the first
    source only: PyTorch also runs its hook, and counting both launched buckets
    before the last layers' grads existed (eager DP replicas diverged);
  * ``no_sync()`` for accumulation micro-steps (reference ``no_sync`` on
    steps 1..accum-1, verified in SURVEY C16);
  * default bucket 25 MB: distilgpt2 LoRA (1.6 MB fp32) and OPT-2.7B
    (47 MB, 11.8 MB per PP stage) are latency-bound on xGMI, so one or two
    buckets — one-shot all-reduce in RCCL — beat many small ones.
"""
import contextlib

import torch
import torch.distributed as dist

from ..obs.profiler import rng
from ..utils.faults import maybe_inject


class GradReducer:
    def __init__(self, arena, group=None, bucket_mb: float = 25.0, overlap: bool = True, world: int = None):
        self.arena = arena
        self.group = group
        self.world = world if world is not None else (dist.get_world_size(group) if dist.is_initialized() else 1)
        self.enabled = self.world > 1
        self.overlap = overlap and self.enabled
        self._sync = True
        self.handles = []
        # buckets over reverse module order (backward produces last layers first)
        cap = int(bucket_mb * 1024 * 1024 / 4)
        named = list(zip(arena.named, arena.offsets))
        buckets, cur, cur_n = [], [], 0
        for (n, p), off in reversed(named):
            cur.append((p, off))
            cur_n += p.numel()
            if cur_n >= cap:
                buckets.append(cur)
                cur, cur_n = [], 0
        if cur:
            buckets.append(cur)
        self.buckets = []
        for b in buckets:
            lo = min(off for _, off in b)
            hi = max(off + p.numel() for p, off in b)
            self.buckets.append({"params": [p for p, _ in b], "lo": lo, "hi": hi, "pending": len(b),
                                 "idx": len(self.buckets)})
        self._p2b = {}
        for i, b in enumerate(self.buckets):
            for p in b["params"]:
                self._p2b[id(p)] = i
        self._off2p = {off: p for (_, p), off in named}
        self._fused = set()  # ids of tensors whose grads the fused backward reports (hooks ignored)
        self.step = 0        # optimizer step being reduced (set by begin_step; fault injection only)
        self._hooks = []
        self.launch_log = []  # (bucket index, "backward" | "finish") per launch of the last step
        if self.overlap:
            for _, p in arena.named:
                self._hooks.append(p.register_post_accumulate_grad_hook(self._on_grad))
            arena.grad_ready = self._on_ready_offsets
            arena.grad_claim = self._on_claim

    @contextlib.contextmanager
    def no_sync(self):
        old = self._sync
        self._sync = False
        try:
            yield
        finally:
            self._sync = old

    def _launch(self, b, where="finish"):
        sl = self.arena.grad[b["lo"]:b["hi"]]
        maybe_inject(dist.get_rank(), self.step, "grads", grads=sl)
        with rng(f"mift.comm.bucket{b['idx']}.{where}"):
            self.handles.append(dist.all_reduce(sl, group=self.group, async_op=True))
        b["launched"] = True
        self.launch_log.append((b["idx"], where))

    def _ready(self, p):
        if not self._sync or not self.overlap:
            return
        b = self.buckets[self._p2b[id(p)]]
        b["pending"] -= 1
        if b["pending"] == 0 and not b.get("launched"):
            self._launch(b, "backward")

    def _on_grad(self, p):
        if id(p) in self._fused:
            return  # its readiness comes from the fused backward's notification (_on_ready_offsets)
        self._ready(p)

    def _on_claim(self, offsets):
        """Fused-forward claim: these arena slices are reported by ``_on_ready_offsets`` only."""
        for off in offsets:
            p = self._off2p.get(off)
            if p is not None:
                self._fused.add(id(p))

    def _on_ready_offsets(self, offsets):
        """Fused-backward notification: the arena slices at ``offsets`` hold this micro-step's grads."""
        for off in offsets:
            p = self._off2p.get(off)
            if p is not None:
                self._ready(p)

    def finish(self):
        """Call after the last micro-batch's backward of an optimizer step."""
        if not self.enabled:
            return
        for b in self.buckets:
            if not b.get("launched"):  # no overlap, or params that got no grad this step
                self._launch(b)
        for h in self.handles:
            h.wait()
        self.handles = []
        for b in self.buckets:
            b["pending"] = len(b["params"])
            b["launched"] = False

    def begin_step(self, step=None):
        """Start an optimizer step.  Claims are per step: the fused forward re-claims its tensors in
        every micro-step it runs, so a tensor whose backward this step takes a non-fused path (a shape
        or flag the fused Functions do not handle) counts through its hook again."""
        self.launch_log = []
        self._fused.clear()
        if step is not None:
            self.step = step

    def remove(self):
        for h in self._hooks:
            h.remove()
        self._hooks = []
        if getattr(self.arena, "grad_ready", None) == self._on_ready_offsets:
            self.arena.grad_ready = None
        if getattr(self.arena, "grad_claim", None) == self._on_claim:
            self.arena.grad_claim = None


@torch.no_grad()
def replica_checksum(tensors):
    """[n, 2] int64: per tensor, the wrapping sums of its raw bit patterns and of the bit patterns
    weighted by position — exact (no float rounding), sensitive to sign-symmetric drift and to a
    small tensor differing next to large ones."""
    rows = []
    chunk = 1 << 24  # bounded int64 temporaries (OPT-6.7B frozen weights are 6.7 G elements)
    for t in tensors:
        t = t.detach().contiguous().reshape(-1)
        ib = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
        flat = t.view(ib)
        acc = torch.zeros(2, dtype=torch.int64, device=t.device)
        for c0 in range(0, flat.numel(), chunk):
            bits = flat[c0:c0 + chunk].to(torch.int64)
            w = (torch.arange(c0, c0 + bits.numel(), device=bits.device, dtype=torch.int64) % 65521) + 1
            acc += torch.stack([bits.sum(), (bits * w).sum()])
        rows.append(acc)
    return torch.stack(rows) if rows else torch.zeros(0, 2, dtype=torch.int64)


@torch.no_grad()
def verify_replicas(tensors, group=None, rtol=0.0, resync=False, slices=None, companions=None):
    """Checksum every tensor across the group; True when all replicas are bit-identical.

    Replaces DDP's construction-time broadcast: identical init by seed, verified with one
    all-reduce of [max, -min] of the exact per-tensor checksums — there any difference raises.

    Assumption for the periodic check in training (``TrainConfig.consistency_every``): replicas
    stay bit-identical only if every rank receives the SAME all-reduce result.  Ring and tree
    all-reduce compute each output element once and forward it, so they do; a one-shot / low-latency
    algorithm that RCCL may select for a small bucket (distilgpt2's 1.6 MB of LoRA grads) sums the
    peers' inputs on every rank, and nothing guarantees the same summation order on every rank.
    With ``rtol > 0`` a checksum mismatch is therefore measured instead of raised: within each
    parameter slice (``slices[i]``: the (offset, numel) segments of tensor i, e.g. the LoRA arena's
    per-parameter views; default: the whole tensor) the element-wise spread (max - min over ranks)
    relative to the SLICE's largest magnitude — a small-magnitude parameter such as LoRA B early in
    training is judged against its own scale, not the arena's — within ``rtol`` is an
    ulp-level replica drift: reported, and with ``resync`` healed by broadcasting the group's first
    rank's tensor together with its ``companions[i]`` (tensors of the same layout that evolve with
    it, e.g. the AdamW moments, so the healed replicas keep identical optimizer state); a larger
    spread (a lost update, a skipped step on one rank) raises."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return True
    cs = replica_checksum(tensors)
    both = torch.stack([cs, -cs])
    dist.all_reduce(both, op=dist.ReduceOp.MAX, group=group)
    spread = both[0] + both[1]
    if not bool((spread != 0).any()):
        return True
    bad = [i for i in range(spread.shape[0]) if bool((spread[i] != 0).any())]
    if rtol <= 0:
        raise RuntimeError(f"replica divergence detected: {len(bad)} tensor(s) differ, first index {bad[0]}")
    worst = 0.0
    for i in bad:
        t = tensors[i].detach().reshape(-1)
        hi, lo = t.float().clone(), t.float().clone()
        dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=group)
        dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=group)
        segs = (slices[i] if slices is not None and slices[i] else None) or [(0, t.numel())]
        for off, n in segs:
            h, l_ = hi[off:off + n], lo[off:off + n]
            d = float((h - l_).max()) if n else 0.0
            if d == 0.0:
                continue
            scale = float(torch.maximum(h.abs().max(), l_.abs().max()))
            rel = d / max(scale, 1e-30)
            worst = max(worst, rel)
            if rel > rtol:
                raise RuntimeError(f"replica divergence detected: tensor {i} slice [{off}, {off + n}) spread "
                                   f"{rel:.3e} of its scale (> rtol {rtol:g})")
    first = dist.get_global_rank(group, 0) if group is not None else 0
    if dist.get_rank() == first:
        print(f"[DDP] replica drift {worst:.3e} (<= rtol {rtol:g}) in {len(bad)} tensor(s)"
              + ("; re-synchronised from the first replica" if resync else ""), flush=True)
    if resync:
        for i in bad:
            dist.broadcast(tensors[i], src=first, group=group)
            for c in (companions[i] if companions is not None and companions[i] else ()):
                dist.broadcast(c, src=first, group=group)
    return False

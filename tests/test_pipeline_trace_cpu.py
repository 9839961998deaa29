"""Event order of one pipeline rank: what is posted on which communicator, and when, relative to the
compute launches.

On RCCL a p2p waits for the compute stream at POST time, so the position of every ``post`` among
the forward / backward launches decides what a transfer overlaps.  This test drives a
``PipelineEngine`` for one rank with no process group (recording stand-ins for ``P2P``, a stub stage
model, a stub ``ctx`` — the way tools/stage_time.py's ``LocalP2P`` stands in for ``P2P``) and compares
the ordered events with traces recorded from the engine before plain and interleaved 1F1B were
merged into one scheduler (tests/golden/pp_event_traces.json):

  post_recv <comm> <peer> | post_send <comm> <peer> | F <chunk> <micro-batch> <micro_step> | B <chunk> <micro-batch>

Waits are not recorded: moving a post across a wait on another receive of the same communicator
changes nothing on an in-order stream.  The fixture is rewritten by

  python tests/test_pipeline_trace_cpu.py --write
"""
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pp_event_traces.json")
MICRO_STEP0 = 10
COMMS = ("rx_f", "tx_f", "rx_b", "tx_b", "rx_wf", "tx_wf", "rx_wb", "tx_wb")


def cases():
    for S in (2, 3, 4):
        for s in range(S):
            for M in sorted({1, S - 1, S, 2 * S + 1}):
                for mode in ("link", "blocking", "shared"):
                    yield S, s, 1, M, mode
            for M in (S, 2 * S):
                for mode in ("link", "blocking"):
                    yield S, s, 2, M, mode


def case_id(S, s, V, M, mode):
    return f"S{S}_s{s}_V{V}_M{M}_{mode}"


class RecordingP2P:
    """Stands in for ``parallel.comm.P2P``: records every posted receive and send, completes at once."""

    def __init__(self, name, events):
        self.name, self.events = name, events

    def post(self, sends=(), recvs=()):
        from mift.parallel.comm import Pending
        for t, peer in recvs:
            t.zero_()
            self.events.append(f"post_recv {self.name} {peer}")
        for _, peer in sends:
            self.events.append(f"post_send {self.name} {peer}")
        return Pending([], [t for t, _ in recvs], [], None)


class _Mark(torch.autograd.Function):
    """Identity whose backward records B(chunk, micro-batch)."""

    @staticmethod
    def forward(ctx, h, model, c, i):
        ctx.rec = (model, c, i)
        return h.clone()

    @staticmethod
    def backward(ctx, g):
        model, c, i = ctx.rec
        model.events.append(f"B {c} {i}")
        return g, None, None, None


class StubStage:
    """Stage model: hidden states in (or the embedding of ``input_ids``), hidden states or a summed
    loss out.  The micro-batch index travels in the attention mask, which every stage is given."""

    def __init__(self, S, s, V, d, events):
        self.has_embed, self.has_head = s == 0, s == S - 1
        self.chunk_ranges = [None] * V
        self.active_chunk = None
        self.micro_step = 0
        self.d, self.events = d, events
        self.w = torch.ones((), requires_grad=True)

    @property
    def embed_here(self):
        return self.has_embed and self.active_chunk in (None, 0)

    @property
    def head_here(self):
        return self.has_head and self.active_chunk in (None, len(self.chunk_ranges) - 1)

    def __call__(self, input_ids=None, attention_mask=None, labels=None, hidden_states=None, reduction="sum",
                 return_logits=False):
        c, i = self.active_chunk or 0, int(attention_mask[0, 0])
        assert (input_ids is not None) == self.embed_here and (labels is not None) == self.head_here
        assert (hidden_states is None) == self.embed_here
        self.events.append(f"F {c} {i} {self.micro_step}")
        h = input_ids.float().unsqueeze(-1).expand(*input_ids.shape, self.d) if self.embed_here else hidden_states
        h = _Mark.apply(h * self.w, self, c, i)
        return {"loss": h.sum()} if self.head_here else {"hidden_states": h}


def make_engine(S, s, V, M, mode):
    """-> (engine of rank ``s`` with recording communicators, its micro-batches, the event list)."""
    from mift.parallel.pipeline import PipelineEngine
    old = os.environ.get("MIFT_PP_P2P")
    os.environ["MIFT_PP_P2P"] = mode
    try:
        events, d = [], 2
        ctx = SimpleNamespace(pp=S, pp_rank=s, pp_ranks=list(range(S)), pp_virtual=V, device=torch.device("cpu"))
        eng = PipelineEngine(StubStage(S, s, V, d, events), ctx, torch.float32, d, graph=False)
    finally:
        if old is None:
            del os.environ["MIFT_PP_P2P"]
        else:
            os.environ["MIFT_PP_P2P"] = old
    by_obj = {}
    for name in COMMS:  # one recorder per communicator object ("shared": rx_f and tx_f are the same one)
        if hasattr(eng, name):
            by_obj.setdefault(id(getattr(eng, name)), []).append(name)
    for names in by_obj.values():
        rec = RecordingP2P("+".join(names), events)
        for name in names:
            setattr(eng, name, rec)
    mbs = [{"input_ids": torch.full((1, 3), i + 1), "attention_mask": torch.full((1, 3), i),
            "labels": torch.full((1, 3), i + 1)} for i in range(M)]
    return eng, mbs, events


def record(S, s, V, M, mode):
    """Ordered events of one eager ``train_batch`` on rank ``s``."""
    eng, mbs, events = make_engine(S, s, V, M, mode)
    loss = eng.train_batch(mbs, torch.ones(()), MICRO_STEP0)
    assert (loss is not None) == (s == S - 1)
    assert eng.stats["fwd"] == eng.stats["bwd"] == M * V
    return events


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(case_id(*c) for c in cases())


@pytest.mark.parametrize("case", list(cases()), ids=lambda c: case_id(*c))
def test_event_order_matches_recorded_trace(golden, case):
    assert record(*case) == golden[case_id(*case)]


def test_eager_interleaved_run_checks_ring_reuse():
    """The eager interleaved run receives into rings of K_c slots per chunk (``slot_counts``), like
    the stage graphs: handing a slot to micro-batch i + K_c before ``release_x`` of micro-batch i
    (its backward queued) raises instead of letting a receive overwrite a live activation."""
    from mift.parallel.pipeline import _EagerRun, slot_counts
    S, s, V, M, c = 2, 1, 2, 4, 1  # chunk 1 of the last rank: the last virtual stage
    K = slot_counts(S, s, M, V)[c]
    assert K < M
    eng, mbs, _ = make_engine(S, s, V, M, "link")
    run = _EagerRun(eng, mbs, torch.ones(()), MICRO_STEP0)
    slots = [run.x_buffer(c, i)[1] for i in range(K)]
    with pytest.raises(RuntimeError, match="reused before"):
        run.x_buffer(c, K)
    eng.model.active_chunk = c
    run.forward(c, 0, slots[0])
    run.backward(c, 0, None)
    run.release_x(c, 0)
    assert run.x_buffer(c, K)[1] == slots[0]


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    sys.path.insert(0, ROOT)
    traces = {case_id(*c): record(*c) for c in cases()}
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in traces.items()) + "\n}\n")
    print(f"{len(traces)} traces -> {GOLDEN}")

"""The pieces every single-launch family shares (vcnf_amd.stacks) where they need no GPU: the affine family's plans on
the shared memo and the out-of-place log-det epilogue."""
import pytest
import torch

import vcnf_amd as nf
from vcnf_amd import derived, fused_affine
from vcnf_amd.stacks import add_log_det


def _block(d_out=4):
    return nf.flows.AffineCouplingBlock(nf.nets.MLP([2, 8, 8, d_out]))


def _reseed(perm):
    with torch.no_grad():
        perm.perm.copy_(perm.perm.flip(0))
        perm.inv_perm[perm.perm] = torch.arange(len(perm.perm))


# the structural edits after which the old per-model memo planned again, each made in place on order[at] (a block at
# even positions, the Permute behind it at odd ones)
EDITS = {
    "module replaced": lambda order, at: order.__setitem__(at, _block()),
    "fused toggled": lambda order, at: setattr(order[at], "fused", False),
    "param_map swapped": lambda order, at: setattr(order[at].flows[1], "param_map", nf.nets.MLP([2, 8, 8, 4])),
    "scale changed": lambda order, at: setattr(order[at].flows[1], "scale", False),
    "scale_map changed": lambda order, at: setattr(order[at].flows[1], "scale_map", "sigmoid"),
    "split_mode changed": lambda order, at: setattr(order[at], "split_mode", "channel_inv"),
    "Permute re-seeded": lambda order, at: _reseed(order[at + 1]),
}


def _order():
    order = []
    for _ in range(5):
        order += [_block(), nf.flows.Permute(4, mode="shuffle")]
    return order


@pytest.fixture
def planner(monkeypatch):
    """fused_affine.plan_stack replaced by a counter that reports the run order[start:start + 4], ended by the flow
    behind it."""
    calls = []

    def plan_stack(order, start, z, inverse):
        calls.append(start)
        return start + 4, "steps", None
    monkeypatch.setattr(fused_affine, "plan_stack", plan_stack)
    return calls


def test_affine_cached_plan_reuses_a_plan_per_position(planner):
    owner, order, z = torch.nn.Module(), _order(), torch.zeros(33, 4)
    with torch.no_grad():
        assert fused_affine.cached_plan(owner, order, 0, z, True) == (4, "steps", None)
        assert fused_affine.cached_plan(owner, order, 0, z, True) == (4, "steps", None)
        assert planner == [0]
        assert fused_affine.cached_plan(owner, order, 4, z, True) == (8, "steps", None)
        assert fused_affine.cached_plan(owner, order, 4, z, True) == (8, "steps", None)
        assert planner == [0, 4]
        fused_affine.cached_plan(owner, order, 0, z, False)              # the other direction is another plan
        fused_affine.cached_plan(owner, order, 0, z.double(), True)      # so is another dtype
        assert planner == [0, 4, 0, 0]
    assert len(derived.plans(owner, "_stack_plans")) == 4              # on the shared plan memo, one per key
    with torch.enable_grad():                                           # autograd on: every call plans
        for _ in range(3):
            fused_affine.cached_plan(owner, order, 0, z, True)
    assert planner == [0, 4, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("edit", list(EDITS), ids=[e.replace(" ", "_") for e in EDITS])
def test_affine_cached_plan_drops_a_plan_after_a_structural_edit(planner, edit):
    """Seen by the plan from position 0: the run order[0:4] and order[4], the flow that ended it."""
    owner, order, z = torch.nn.Module(), _order(), torch.zeros(33, 4)
    with torch.no_grad():
        fused_affine.cached_plan(owner, order, 0, z, True)
        EDITS[edit](order, 6)                                           # order[6] / order[7]: beyond the flow that ended the run
        fused_affine.cached_plan(owner, order, 0, z, True)
        assert planner == [0], "an edit the plan cannot depend on dropped it"
        for n, at in enumerate((2, 4) if edit != "Permute re-seeded" else (2,)):      # inside the run; the flow that ended it
            EDITS[edit](order, at)
            fused_affine.cached_plan(owner, order, 0, z, True)
            assert planner == [0] * (n + 2), "order[%d]: %s, the plan was kept" % (at, edit)
            fused_affine.cached_plan(owner, order, 0, z, True)
            assert planner == [0] * (n + 2)


def test_affine_cached_plan_watches_what_was_read_when_there_is_no_run(monkeypatch):
    """Without a run plan_stack has read at most a Permute, a block, a Permute and the flow that stopped it: a switch
    toggled on any of the four plans again (the old memo keyed on every flow of the model)."""
    calls = []
    monkeypatch.setattr(fused_affine, "plan_stack", lambda order, start, z, inverse: calls.append(start))
    owner, z = torch.nn.Module(), torch.zeros(33, 4)
    order = [nf.flows.Permute(4, mode="shuffle")] + _order()
    with torch.no_grad():
        assert fused_affine.cached_plan(owner, order, 0, z, True) is None
        assert fused_affine.cached_plan(owner, order, 0, z, True) is None and calls == [0]
        order[4].fused = False
        assert fused_affine.cached_plan(owner, order, 0, z, True) is None and calls == [0]
        order[3].fused = False
        assert fused_affine.cached_plan(owner, order, 0, z, True) is None and calls == [0, 0]


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_add_log_det_is_the_expression_it_replaces(sign):
    g = torch.Generator().manual_seed(5)
    out, ld, log_q = (torch.randn(33, generator=g) for _ in range(3))
    before = log_q.clone()
    got_out, got = add_log_det(out, ld, log_q, sign)
    assert got_out is out and torch.equal(got, log_q + sign * ld)
    assert got is not log_q and torch.equal(log_q, before)              # the given log_q is not written
    got_out, got = add_log_det(out, ld, None, sign)
    assert got_out is out and torch.equal(got, ld if sign == 1.0 else sign * ld)
    assert (got is ld) == (sign == 1.0)                                 # ld itself, not 1.0 * ld


def test_add_log_det_keeps_the_graph():
    ld = torch.randn(5, requires_grad=True)
    log_q = torch.randn(5, requires_grad=True)
    add_log_det(None, ld, log_q, -1.0)[1].sum().backward()
    assert torch.equal(ld.grad, -torch.ones(5)) and torch.equal(log_q.grad, torch.ones(5))

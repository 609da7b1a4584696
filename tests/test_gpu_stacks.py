"""The contract of the single-launch families (vcnf_amd.stacks) on the GPU: the affine family's plans on the shared memo
after structural edits, and every family's launch inside NormalizingFlow against its layers called one by one.  B = 33
throughout: a 32-sample tile and a ragged second one.  The bounds are those of each family's own single-launch and
gradient tests (named where they are used); nothing here has a bound of its own."""
import pytest
import torch
from torch import nn

import stochastic_ref as sref
import vcnf_amd as nf
from helpers import assert_close
from vcnf_amd import derived, fused, fused_affine, fused_masked, fused_planar, fused_stochastic

pytestmark = pytest.mark.gpu

B = 33
F32, F64 = torch.float32, torch.float64


# ---------------------------------------------------------------- affine family: plans on the shared memo
D, WIDTHS = 2, [1, 32, 32, 2]          # the smallest case of test_affine_stack_single_launch_matches_per_layer, with
                                       # shuffling Permutes: a 'swap' Permute has no buffers to re-seed


def _affine_model():
    flows = []
    for _ in range(8):
        flows += [nf.flows.AffineCouplingBlock(nf.nets.MLP(WIDTHS, init_zeros=False)), nf.flows.Permute(D, mode="shuffle")]
    return nf.NormalizingFlow(nf.distributions.DiagGaussian(D), flows).cuda().eval()


def _fresh(model):
    """A newly constructed model with the structure and the parameters ``model`` has now; nothing is cached on it."""
    flows = []
    for f in model.flows:
        if isinstance(f, nf.flows.Permute):
            flows.append(nf.flows.Permute(D, mode=f.mode))
            continue
        core = f.flows[1]
        linears = [m for m in core.param_map.net if isinstance(m, nn.Linear)]
        blk = nf.flows.AffineCouplingBlock(nf.nets.MLP([m.in_features for m in linears] + [linears[-1].out_features]),
                                           scale=core.scale, scale_map=core.scale_map, split_mode=f.split_mode)
        blk.fused = f.fused
        flows.append(blk)
    new = nf.NormalizingFlow(nf.distributions.DiagGaussian(D), flows)
    new.load_state_dict(model.state_dict())
    return new.cuda().eval()


def _reseed(perm):
    with torch.no_grad():
        perm.perm.copy_(perm.perm.flip(0))
        perm.inv_perm[perm.perm] = torch.arange(D, device=perm.perm.device)


def _no_scale(block):
    block.flows[1].scale = False                   # a pure shift takes half the conditioner outputs
    block.flows[1].param_map = nf.nets.MLP(WIDTHS[:-1] + [1], init_zeros=False).cuda()


# in place on the model, each on a block (or the Permute) of its own inside the run that the first calls planned
AFFINE_EDITS = [
    ("module replaced", lambda m: m.flows.__setitem__(2, nf.flows.AffineCouplingBlock(nf.nets.MLP(WIDTHS, init_zeros=False)).cuda())),
    ("fused toggled", lambda m: setattr(m.flows[4], "fused", False)),
    ("param_map swapped", lambda m: setattr(m.flows[6].flows[1], "param_map", nf.nets.MLP(WIDTHS, init_zeros=False).cuda())),
    ("scale changed", lambda m: _no_scale(m.flows[8])),
    ("scale_map changed", lambda m: setattr(m.flows[10].flows[1], "scale_map", "sigmoid")),
    ("split_mode changed", lambda m: setattr(m.flows[12], "split_mode", "channel_inv")),
    ("Permute re-seeded", lambda m: _reseed(m.flows[13])),
]


def test_affine_plan_memo_follows_structural_edits(hip):
    """The second call at each position takes its plan from the memo; after each in-place structural edit the model
    gives, bit for bit, what a newly constructed model with the same structure and parameters gives."""
    torch.manual_seed(43)
    model = _affine_model()
    x, eps = torch.randn(B, D, device="cuda"), torch.randn(B, D, device="cuda")

    def both(m):
        with torch.no_grad():
            return (m.log_prob(x),) + tuple(m.sample_from(eps))
    first = both(model)
    plans = dict(derived.plans(model, "_stack_plans"))
    assert len(plans) == 2 and all(hit[0][0] == 16 for hit in plans.values())           # one run per direction, all 16 flows
    again = both(model)
    assert all(derived.plans(model, "_stack_plans")[k] is v for k, v in plans.items()), "the second call planned again"
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for what, edit in AFFINE_EDITS:
        edit(model)
        got, want = both(model), both(_fresh(model))
        assert all(torch.isfinite(t).all() for t in want), what
        for name, a, b in zip(("log_prob", "sample z", "sample log_q"), got, want):
            assert torch.equal(a, b), "%s: %s differs from a fresh model's by up to %.3e" % (what, name, float((a - b).abs().max()))
        if what != "fused toggled":                 # (that one changes the path, not the function)
            assert not all(torch.equal(a, b) for a, b in zip(got, first)), what + ": the edit changed nothing"
        first = got


# ---------------------------------------------------------------- every family: the launch inside NormalizingFlow
def _perturb(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    return model


def _const(d):
    f = nf.flows.AffineConstFlow((d,))
    with torch.no_grad():
        f.s.normal_(0, 0.3)
        f.t.normal_(0, 0.3)
    return f


def _masked_pairs(d, h, pairs):
    b = torch.tensor([1.0 if i % 2 == 0 else 0.0 for i in range(d)])
    flows = []
    for i in range(pairs):
        s, t = nf.nets.MLP([d, h, d], init_zeros=True), nf.nets.MLP([d, h, d], init_zeros=True)
        flows += [nf.flows.MaskedAffineFlow(b if i % 2 == 0 else 1 - b, t, s), nf.flows.ActNorm(d)]
    return flows


def _target(d, dtype):
    target = nf.distributions.DiagGaussian(d, trainable=False)
    target.loc.copy_(torch.linspace(-1.0, 1.0, d).reshape(1, d))
    target.log_scale.fill_(0.3)
    return target.to(dtype).cuda()


def _family(name, dtype, training=False):
    """(model, switch, the module and the name of the function that launches a run, d): the family's run with a flow of no
    family (of this family, at least) before and after it, so that a flow ends the run in either direction."""
    torch.manual_seed(17)
    if name == "affine":                # as in test_affine_stack_single_launch_matches_per_layer: exact fp32 matrix path
        d, run = 2, []
        for _ in range(2):
            run += [nf.flows.AffineCouplingBlock(nf.nets.MLP(WIDTHS, init_zeros=False)), nf.flows.Permute(2, mode="swap")]
        for f in run:
            f.fused_precision = "fp32"
        flows, switch, launcher = [_const(d)] + run + [_const(d)], "fuse_affine_stacks", (fused_affine, "run_stack")
    elif name == "rqs":
        d = 32
        run = [nf.flows.CoupledRationalQuadraticSpline(d, 1, 128, 8, reverse_mask=bool(i % 2)) for i in range(2)]
        flows, switch, launcher = [_const(d)] + run + [_const(d)], "fuse_rqs_stacks", (fused, "run_stack")
    elif name == "masked":
        d = 2
        flows = [nf.flows.Permute(d, mode="swap")] + _masked_pairs(d, 16, 2) + [nf.flows.Permute(d, mode="swap")]
        switch, launcher = "fuse_masked_stacks", (fused_masked, "run")
    elif name == "planar":              # a density pass inverts leaky_relu Planar layers only; sampling takes every kind
        d = 4
        run = [nf.flows.Planar(d), nf.flows.Radial(d), nf.flows.Planar(d, act="leaky_relu")] if training else \
            [nf.flows.Planar(d, act="leaky_relu") for _ in range(3)]
        flows = [nf.flows.Permute(d, mode="swap")] + run + [nf.flows.Permute(d, mode="swap")]
        switch, launcher = "fuse_planar_stacks", (fused_planar, "run")
    else:
        d = 2
        target = nf.distributions.TwoMoons()
        run = [nf.flows.HamiltonianMonteCarlo(target, 5, ls.float(), lm.float()) for ls, lm in sref.hmc_parameters(0.05, 3)]
        flows = [nf.flows.Permute(d, mode="swap")] + run + [nf.flows.Permute(d, mode="swap")]
        switch, launcher = "fuse_stochastic_stacks", (fused_stochastic, "run")
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(d), flows)
    if name in ("rqs", "masked"):
        _perturb(model, 23)
    model = model.to(dtype).cuda()
    if name == "stochastic":
        model.p = (target.double() if dtype == F64 else target).cuda()
    elif training:
        model.p = _target(d, dtype)
    if name == "masked":
        with torch.no_grad():
            model.log_prob(torch.randn(B, d, device="cuda", dtype=dtype))          # the first batch initialises ActNorm
            for f in model.flows:
                if isinstance(f, nf.flows.ActNorm):
                    f.s.add_(0.05 * torch.randn_like(f.s))
                    f.t.add_(0.05 * torch.randn_like(f.t))
    return model, switch, launcher, d


def _count_runs(monkeypatch, launcher):
    """The list that receives the length of every run of two or more layers the family launches (a Planar, Radial or HMC
    layer called on its own launches a run of one)."""
    mod, name = launcher
    real, calls = getattr(mod, name), []
    monkeypatch.setattr(mod, name, lambda steps, *a: (calls.extend([len(steps)] * (len(steps) > 1)), real(steps, *a))[1])
    return calls


def _close_log_prob(name, dtype, got, want):
    """Each family's own bound of its single-launch test against the per-layer path."""
    print("%s %s: max |log_prob run - layers| %.3e" % (name, dtype, float((got - want).abs().max())))
    assert torch.isfinite(want).all()
    if name == "affine":                # test_affine_stack_single_launch_matches_per_layer
        assert_close(got, want.cpu(), rtol=2e-6, atol=2e-5, what="affine run log_prob")
    elif name == "rqs":                 # test_rqs_stack_single_launch_matches_per_layer
        assert bool(((got - want).abs() <= 1e-4).all())
    elif name == "stochastic":          # test_model_runs_and_trains
        eps = torch.finfo(dtype).eps
        assert bool(((got - want).abs() <= 64 * eps * (1 + want.abs())).all())
    else:                               # test_masked_affine_stack_single_launch_matches_per_layer,
        tol = dict(rtol=2e-5, atol=2e-5) if dtype == F32 else dict(rtol=1e-11, atol=1e-11)      # test_mixed_model_plans_...
        assert torch.allclose(got, want, **tol)


@pytest.mark.parametrize("name,dtype", [("affine", F32), ("rqs", F32), ("masked", F32), ("masked", F64), ("planar", F32),
                                        ("planar", F64), ("stochastic", F32), ("stochastic", F64)],
                         ids=lambda v: v if isinstance(v, str) else str(v).split(".")[-1])
def test_family_launch_in_log_prob_matches_the_layers_one_by_one(hip, name, dtype, monkeypatch):
    """log_prob with the family's run in one launch against the sum over the layers' own ``inverse`` calls."""
    model, switch, launcher, d = _family(name, dtype)
    calls = _count_runs(monkeypatch, launcher)
    x = torch.randn(B, d, device="cuda", dtype=dtype)
    with torch.no_grad():
        torch.manual_seed(5)
        got = model.log_prob(x)
        assert len(calls) == 1, "the run was not one launch: %s" % calls
        setattr(model, switch, False)
        torch.manual_seed(5)
        z, want = x, torch.zeros(B, device="cuda", dtype=dtype)
        for f in reversed(model.flows):
            z, ld = f.inverse(z)
            want = want + ld
        want = want + model.q0.log_prob(z)
    assert len(calls) == 1
    _close_log_prob(name, dtype, got, want)


def _same_gradients(model, switch, loss_of, dtype, what, calls, launches):
    """The comparator of test_masked_affine_stack_vjp_matches_per_layer_autograd: loss and every gradient within tol of
    the per-layer path's, relative to the gradient's largest entry; tol 1e-9 in fp64, 3e-4 in fp32."""
    out = {}
    for on in (True, False):
        setattr(model, switch, on)
        model.zero_grad(set_to_none=True)
        del calls[:]
        torch.manual_seed(9)
        loss = loss_of()
        loss.backward()
        assert len(calls) == (launches if on else 0), (what, on, calls)
        out[on] = (float(loss.detach()), {n: None if p.grad is None else p.grad.clone() for n, p in model.named_parameters()})
    setattr(model, switch, True)
    tol = 1e-9 if dtype == F64 else 3e-4
    (l1, g1), (l0, g0) = out[True], out[False]
    assert l0 == l0 and abs(l1 - l0) <= tol * (1 + abs(l0)), (what, l1, l0)
    assert any(g is not None and bool(g.any()) for g in g0.values()), what + ": no gradient at all"
    for n in g0:
        assert (g1[n] is None) == (g0[n] is None), (what, n)
        if g0[n] is not None:
            err, scale = float((g1[n] - g0[n]).abs().max()), float(g0[n].abs().max())
            print("%s %s: |grad run - layers| %.3e of %.3e" % (what, n, err, scale))
            assert err <= tol * (scale + 1e-3), (what, n, err, scale)


# fp32 only where a family's own tests bound an fp32 gradient against the per-layer path (the masked family's); the
# Planar / Radial and HMC tests judge fp32 gradients by the noise of a CPU restatement, which this comparison has not
@pytest.mark.parametrize("name,dtype", [("masked", F32), ("masked", F64), ("planar", F64), ("stochastic", F64)],
                         ids=lambda v: v if isinstance(v, str) else str(v).split(".")[-1])
def test_differentiable_family_trains_like_the_layers_one_by_one(hip, name, dtype, monkeypatch):
    """reverse_kld(...).backward() with the family's switch on and off: the same loss and parameter gradients.  The masked
    family is not offered to the plain walk (its planner is not marked ``differentiable``), so reverse_kld takes its layers
    one by one either way; its run as one autograd node is what forward_kld trains through, compared the same way."""
    model, switch, launcher, d = _family(name, dtype, training=True)
    calls = _count_runs(monkeypatch, launcher)
    beta = 0.5 if name == "stochastic" else 1.0          # at beta = 1 the HMC parameters' gradient is zero by construction
    _same_gradients(model, switch, lambda: model.reverse_kld(B, beta=beta), dtype, name + " reverse_kld", calls,
                    0 if name == "masked" else 1)
    if name == "masked":
        x = torch.randn(B, d, device="cuda", dtype=dtype)
        _same_gradients(model, switch, lambda: model.forward_kld(x), dtype, "masked forward_kld", calls, 1)


def test_training_path_of_the_composed_coupling_keeps_its_autograd_nodes(hip):
    """d = 4, K = 8: the channel partition, the transform spline and the merge of the composed coupling are the nodes
    SplitColumnsFn, RqsPackedFn and MergeColumnsFn."""
    torch.manual_seed(3)
    cp = _perturb(nf.flows.CoupledRationalQuadraticSpline(4, 1, 16, 8), 3).cuda().prqct
    x = torch.randn(B, 4, device="cuda", requires_grad=True)        # (the partition of inputs without a gradient is no node)
    for fn in (cp.forward, cp.inverse):
        out, lad = fn(x)
        seen, todo = set(), [out.grad_fn, lad.grad_fn]
        while todo:
            node = todo.pop()
            if node is not None and node not in seen:
                seen.add(node)
                todo += [n for n, _ in node.next_functions]
        names = {type(n).__name__ for n in seen}
        assert {"SplitColumnsFnBackward", "RqsPackedFnBackward", "MergeColumnsFnBackward"} <= names, names
        assert type(out.grad_fn).__name__ == "MergeColumnsFnBackward"

"""Batches beyond every stream kernel's grid cap: the second and later trips of a workgroup's loop.

The shapes come from tests/grid_caps.py (B = 2 trips of the whole grid + a ragged third one); the references and the
comparators are those of each unit's own test file, evaluated in fp64 and - as the noise yardstick of helpers.parity - in
fp32.  Per case:
  a. every row against the reference;
  b. row independence, bitwise: the last full trip with the ragged tail, and 257 rows across the boundary between
     trip 1 and trip 2, run again as batches of their own give the same bits: there the rows that were on a later trip
     of the large call are on the first trip (the r rows after a window's first full trip on the second) - a stale
     register, LDS value or barrier of a later trip shows here;
  c. parameter sums of the VJPs: against the reference, twice the same bits, and with the cotangents of every trip but
     the last (but the first) set to zero against the reference's sums over that trip's rows alone - an overwrite
     instead of an add, or a dropped trip, fails one of the two outright;
  d. HMC / MH decisions on the rows outside the near-tie band, whose share is asserted under stochastic_ref.BAND_CAP.
The matrix kernels (conv1x1, conv3x3 + conv1x1, channel mixing, fused affine layer and stack) follow at the end with
(a), (b) and the fp16 saturation / range counters.
Each test prints the figures that profiles/grid_caps.md records."""
import copy
import math
import time
import zlib

import pytest
import torch

import grid_caps as gc
import heavy_tail_ref as tail_ref
import mvn_ref
import planar_radial_ref as pr_ref
import spline_edge_ref as edge_ref
import stochastic_ref as sref
import target_ref as tref
import vcnf_amd as nf
from helpers import assert_close, parity
from test_gpu_f64_grad import tight
from test_gpu_grad import close
from vcnf_amd import _lib, fused_planar, fused_stochastic

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DTYPES = [F32, F64]
IDS = ["f32", "f64"]
TOL64 = dict(rtol=1e-10, atol=1e-10)          # the fp64 figure of the base, target and Planar / Radial tests
AFFINE64 = dict(rtol=1e-11, atol=1e-12)       # test_gpu_f64.close64


def tname(dtype):
    return "f64" if dtype == F64 else "f32"


def case_of(stem, dtype):
    return gc.CASES["%s.%s" % (stem, tname(dtype))]


def seeded(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def cast(t, dtype, device="cuda"):
    if isinstance(t, dict):
        return {k: cast(v, dtype, device) for k, v in t.items()}
    if isinstance(t, (list, tuple)):
        return [cast(v, dtype, device) for v in t]
    if not torch.is_tensor(t):
        return t
    return t.to(device=device, dtype=dtype if t.is_floating_point() else None)


def report(case, what, got, r32, r64):
    """One line of profiles/grid_caps.md: the kernel's error against fp64 next to the reference's own fp32 noise."""
    err = float((got.detach().double().cpu() - r64.double().cpu()).abs().max()) if got.numel() else 0.0
    noise = float((r32.double().cpu() - r64.double().cpu()).abs().max()) if r32 is not None and got.numel() else float("nan")
    print("GRIDCAP %-34s %-28s max|got - ref64| %.3e  ref32 noise %.3e  of %.3e" % (
        case.name, what, err, noise, float(r64.abs().max()) if r64.numel() else 0.0))


def check(case, what, got, r32, r64, dtype, tol64=TOL64, noise_floor=0.0, rows=None):
    """fp32: helpers.parity against the reference's fp32 run with its fp32-vs-fp64 noise; fp64: assert_close."""
    got, r64 = got.detach().cpu(), r64.detach().cpu()
    r32 = None if r32 is None else r32.detach().cpu()
    if rows is not None:
        got, r64, r32 = got[rows], r64[rows], None if r32 is None else r32[rows]
    assert got.dtype == dtype and got.shape == r64.shape, "%s %s: %s %s vs %s" % (case.name, what, got.dtype, tuple(got.shape), tuple(r64.shape))
    report(case, what, got, r32, r64)
    if dtype == F32:
        parity(got, r32, r64, what="%s %s" % (case.name, what), noise_floor=noise_floor)
    else:
        assert_close(got, r64, what="%s %s" % (case.name, what), **tol64)


def narrow(t, dim, lo, hi):
    return t.narrow(dim, lo, hi - lo).contiguous()


def rows_again(case, call, inputs, outs):
    """(b): ``call`` on the windows of the batch as batches of their own.  inputs / outs: [(tensor, batch dim)]; call
    takes the input tensors and returns the output tensors."""
    for lo, hi in case.windows():
        sub = call(*[narrow(t, d, lo, hi) for t, d in inputs])
        for i, ((o, d), s) in enumerate(zip(outs, sub)):
            same = torch.equal(narrow(o, d, lo, hi), s)
            assert same, "%s: output %d of the rows %d..%d differs when they are a batch of their own (%d elements)" % (
                case.name, i, lo, hi, int((narrow(o, d, lo, hi) != s).sum()))


def trip_masks(case):
    """The row ranges whose cotangents stay in the two masked calls of (c): the last trip alone, the first alone."""
    return (("last trip", case.trip_rows(case.trips - 1)), ("first trip", case.trip_rows(0)))


def masked(t, rows, dim=0):
    """t with everything outside the rows (lo, hi) along ``dim`` zero; None: t."""
    if rows is None:
        return t
    out = torch.zeros_like(t)
    out.narrow(dim, rows[0], rows[1] - rows[0]).copy_(t.narrow(dim, rows[0], rows[1] - rows[0]))
    return out


def sl(rows):
    return slice(None) if rows is None else slice(rows[0], rows[1])


# ================================================================ 2-D targets
TARGETS = [("two_moons", 0), ("circular", 8), ("ring", 2)]
target_id = lambda c: "%s-%d" % c


def target_of(family, n, dtype):
    D = nf.distributions
    t = D.TwoMoons() if family == "two_moons" else D.CircularGaussianMixture(n) if family == "circular" else D.RingMixture(n)
    return (t.double() if dtype == F64 else t).cuda()


def target_rows(b, *key):
    """z [b, 2] in fp64 as target_ref.inputs draws it: the fixed rows (r == 0, on the crest, far out, ...), then
    randn * 1.5 and randn * 3 by halves, none within 1e-3 of r == 0 (the only kink)."""
    g = seeded("grid caps target", *key)
    fixed = torch.tensor(tref.FIXED_ROWS, dtype=F64)
    z = randn(g, b - len(fixed), 2)
    z[: len(z) // 2] *= 1.5
    z[len(z) // 2:] *= 3.0
    near = torch.norm(z, dim=1) < 1e-3
    z[near] = 1.0
    return torch.cat([fixed, z], 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tgt", TARGETS, ids=target_id)
def test_target_density(hip, tgt, dtype):
    family, n = tgt
    case = case_of("target.narrow", dtype)
    t0 = time.time()
    target = target_of(family, n, dtype)
    z = target_rows(case.B, family, n).to(dtype).cuda()
    table, scale = target._operands(z)
    call = lambda x: _lib.target_log_prob(x, target._family, table, scale, want_score=True)
    lp, score = call(z)
    want = {}
    for d in DTYPES:
        zd = z.to(d)
        want[d] = (tref.log_prob(family, n, zd).detach(), tref.score(family, n, zd))
        assert all(torch.isfinite(t).all() for t in want[d])
    check(case, "log_prob", lp, want[F32][0], want[F64][0], dtype)
    if dtype == F32:
        check(case, "score", score, want[F32][1], want[F64][1], dtype)
    else:                                                       # test_gpu_target.judge(gradient=True)
        report(case, "score", score, None, want[F64][1])
        bound = 1e-9 * float(want[F64][1].abs().max())
        assert torch.isfinite(score).all() and float((score - want[F64][1]).abs().max()) <= bound
    rows_again(case, call, [(z, 0)], [(lp, 0), (score, 0)])
    assert torch.equal(_lib.target_log_prob(z, target._family, table, scale)[0], lp), "the scoreless path differs"
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


# ================================================================ HMC and MH
HMC_STEPS, HMC_STEP, HMC_LAYERS = 2, 0.05, 2
MH_STEPS, MH_SCALE = 2, (0.3, 0.24)


def hmc_inputs(family, n, b):
    g = seeded("grid caps hmc", family, n, b)
    z = target_rows(b, "hmc", family, n)
    return z, randn(g, HMC_LAYERS, b, 2), torch.rand(HMC_LAYERS, b, generator=g, dtype=F64)


def hmc_layers(target, params, dtype):
    return [nf.flows.HamiltonianMonteCarlo(target, HMC_STEPS, ls.to(dtype), lm.to(dtype)).cuda() for ls, lm in params]


def stoch_judge(case, what, got, r32, r64, dtype, yardstick):
    """test_gpu_stochastic.judge: fp64 within 16 x the difference of the restatement's two fp64 runs (autograd and
    closed-form scores) + 1e-12 of the largest entry.  The two runs are taken on the case's own rows, as that file's
    B = 1000 cases take them on theirs."""
    got, r32, r64 = got.detach().cpu(), r32.detach().cpu(), r64.detach().cpu()
    assert got.dtype == dtype and got.shape == r64.shape, what
    report(case, what, got, r32, r64)
    if dtype == F32:
        parity(got, r32, r64, what="%s %s" % (case.name, what))
    else:
        bound = 16.0 * yardstick + 1e-12 * float(r64.abs().max())
        err = float((got - r64).abs().max())
        assert torch.isfinite(got).all() and err <= bound, "%s %s: %.3e > %.3e" % (case.name, what, err, bound)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tgt", TARGETS, ids=target_id)
def test_hmc_run(hip, tgt, dtype):
    family, n = tgt
    case = case_of("stoch.hmc_fwd.narrow", dtype)
    t0 = time.time()
    b = case.B
    z64, noise64, unif64 = (t.cuda() for t in hmc_inputs(family, n, b))
    params = sref.hmc_parameters(HMC_STEP, HMC_LAYERS)
    run = lambda d, score=tref.score: sref.hmc_run(family, n, z64.to(d), noise64.to(d), unif64.to(d),
                                                    [(ls.to(d).cuda(), lm.to(d).cuda()) for ls, lm in params], HMC_STEPS, score=score)
    r64, r32 = run(F64), run(F32)
    closed = run(F64, sref.closed_form_score)
    assert all(torch.isfinite(t).all() for r in (r64, r32) for t in r[:2])
    yard = [float((closed[j] - r64[j]).abs().max()) for j in (0, 1)]
    near = ((torch.clamp(r64[3], max=2.0) - unif64).abs() < sref.HMC_BAND).any(0).cpu()
    assert float(near.double().mean()) <= sref.BAND_CAP and sref.few_near(near, HMC_LAYERS), "%d rows in the band" % int(near.sum())
    keep = ~near
    target = target_of(family, n, dtype)
    layers = hmc_layers(target, params, dtype)
    z, noise, unif = (t.to(dtype).cuda() for t in (z64, noise64, unif64))
    table, scale = target._operands(z)
    with torch.no_grad():
        step, mass, sqm = fused_stochastic.operands(layers)
    call = lambda x, e, u: _lib.hmc_stack(x, e, u, step, mass, sqm, HMC_STEPS, target._family, table, scale, want_trace=True)
    out, ld, trace, accept = call(z, noise, unif)
    assert all(torch.equal(x, y) for x, y in zip((out, ld, trace, accept), call(z, noise, unif))), "two calls differ"
    differ = (accept.bool() != r64[2]).any(0).cpu() & keep
    assert not differ.any(), "%d rows outside the band decided differently" % int(differ.sum())
    for j, (name, got) in enumerate((("z_out", out), ("log_det", ld))):
        stoch_judge(case, name, got.cpu()[keep], r32[j].cpu()[keep], r64[j].cpu()[keep], dtype, yard[j])
    rows_again(case, call, [(z, 0), (noise, 1), (unif, 1)], [(out, 0), (ld, 0), (trace, 1), (accept, 1)])
    print("GRIDCAP %-34s wall %.2f s  band %.4f" % (case.name, time.time() - t0, float(near.double().mean())))


def hmc_ref_grads(family, n, z64, noise64, unif64, params, accept, gz, gl, dtype, rows, score=tref.score):
    """(g_z, [g_log_step_size, g_log_mass per layer]) by autograd of the restatement on the rows ``rows`` with the
    kernel's decisions imposed (test_gpu_stochastic.restatement_gradients)."""
    s = sl(rows)
    z = z64[s].to(dtype).clone().requires_grad_(True)
    leaves = [tuple(t.to(device=z64.device, dtype=dtype).clone().requires_grad_(True) for t in pair) for pair in params]
    out, ld, _, _ = sref.hmc_run(family, n, z, noise64[:, s].to(dtype), unif64[:, s].to(dtype), leaves, HMC_STEPS, score=score,
                                 accept=accept[:, s])
    flat = [z] + [t for pair in leaves for t in pair]
    return torch.autograd.grad((out * gz[s].to(dtype)).sum() + (ld * gl[s].to(dtype)).sum(), flat)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tgt", TARGETS, ids=target_id)
def test_hmc_vjp(hip, tgt, dtype):
    family, n = tgt
    case = case_of("stoch.hmc_bwd.narrow", dtype)
    t0 = time.time()
    b = case.B
    groups = min((b + _lib.HMC_BLOCK - 1) // _lib.HMC_BLOCK, _lib.HMC_MAX_BWD_GROUPS)
    assert groups == case.cap == gc.constant("stoch.bwd_cap") and case.tiles >= 2 * groups + 1
    z64, noise64, unif64 = (t.cuda() for t in hmc_inputs(family, n, b))
    params = sref.hmc_parameters(HMC_STEP, HMC_LAYERS)
    g = seeded("grid caps hmc cotangent", family, n)
    gz64, gl64 = randn(g, b, 2).cuda(), randn(g, b).cuda()
    target = target_of(family, n, dtype)
    layers = hmc_layers(target, params, dtype)
    z, noise, unif = (t.to(dtype).cuda() for t in (z64, noise64, unif64))
    table, scale = target._operands(z)
    names = ["g_z"] + ["%s[%d]" % (p, i) for i in range(HMC_LAYERS) for p in ("log_step_size", "log_mass")]

    def kernel(rows, zs=z, es=noise, us=unif, gz=gz64, gl=gl64):
        x = zs.clone().requires_grad_(True)
        for layer in layers:
            layer.zero_grad(set_to_none=True)
        step, mass, sqm = fused_stochastic.operands(layers)
        out, ld = nf.autograd.HmcStackFn.apply(x, step, mass, sqm, es, us, HMC_STEPS, target._family, table, scale)
        ((out * masked(gz.to(dtype), rows)).sum() + (ld * masked(gl.to(dtype), rows)).sum()).backward()
        return [x.grad.clone()] + [p.grad.clone() for layer in layers for p in (layer.log_step_size, layer.log_mass)]

    with torch.no_grad():
        step, mass, sqm = fused_stochastic.operands(layers)
        accept = _lib.hmc_stack(z, noise, unif, step, mass, sqm, HMC_STEPS, target._family, table, scale, want_trace=True)[3].bool()
    assert 0.2 < float(accept.double().mean()) <= 1.0
    ref = lambda d, rows, score=tref.score: hmc_ref_grads(family, n, z64, noise64, unif64, params, accept, gz64, gl64, d, rows, score)

    def judge_all(got, rows, label):
        w32, w64, c64 = ref(F32, rows), ref(F64, rows), ref(F64, rows, sref.closed_form_score)
        for name, x, a, c, e in zip(names, got, w32, w64, c64):
            if name == "g_z":
                x = x[sl(rows)]
            assert bool((x != 0).any()), name
            stoch_judge(case, "%s%s" % (name, label), x, a, c, dtype, float((e - c).abs().max()))

    first, again = kernel(None), kernel(None)
    assert all(torch.equal(a, c) for a, c in zip(first, again)), "two backward calls differ"
    judge_all(first, None, "")
    for label, rows in trip_masks(case):
        judge_all(kernel(rows), rows, ", %s only" % label)
    # (b) for g_z: the windows as batches of their own
    for lo, hi in case.windows():
        sub = kernel(None, narrow(z, 0, lo, hi), narrow(noise, 1, lo, hi), narrow(unif, 1, lo, hi), gz64[lo:hi], gl64[lo:hi])
        assert torch.equal(sub[0], first[0][lo:hi]), "g_z of the rows %d..%d differs when they are a batch of their own" % (lo, hi)
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tgt", TARGETS, ids=target_id)
def test_mh_walk(hip, tgt, dtype):
    family, n = tgt
    case = case_of("stoch.mh.narrow", dtype)
    t0 = time.time()
    b = case.B
    g = seeded("grid caps mh", family, n)
    z64 = target_rows(b, "mh", family, n).cuda()
    eps64, w64 = randn(g, MH_STEPS, b, 2).cuda(), torch.rand(MH_STEPS, b, generator=g, dtype=F64).cuda()
    with torch.no_grad():
        r = {d: sref.mh_walk(family, n, z64.to(d), eps64.to(d), w64.to(d), torch.tensor(MH_SCALE, dtype=d, device="cuda")) for d in DTYPES}
    near = ((r[F64][3] - w64).abs() < sref.MH_BAND).any(0).cpu()
    assert float(near.double().mean()) <= sref.BAND_CAP and sref.few_near(near), "%d rows in the band" % int(near.sum())
    keep = ~near
    target = target_of(family, n, dtype)
    z, eps, w = (t.to(dtype) for t in (z64, eps64, w64))
    prop = torch.tensor(MH_SCALE, dtype=dtype, device="cuda")
    table, tscale = target._operands(z)
    call = lambda x, e, u: _lib.mh_walk(x, e, u, prop, target._family, table, tscale, want_accept=True)
    out, accept = call(z, eps, w)
    assert torch.equal(out, _lib.mh_walk(z, eps, w, prop, target._family, table, tscale))
    differ = (accept.bool() != r[F64][2]).any(0).cpu() & keep
    assert not differ.any(), "%d rows outside the band decided differently" % int(differ.sum())
    stoch_judge(case, "z_out", out.cpu()[keep], r[F32][0].cpu()[keep], r[F64][0].cpu()[keep], dtype, 0.0)
    stay = ~accept.bool().any(0)
    assert torch.equal(out[stay], z[stay])
    rows_again(case, call, [(z, 0), (eps, 1), (w, 1)], [(out, 0), (accept, 1)])
    print("GRIDCAP %-34s wall %.2f s  band %.4f" % (case.name, time.time() - t0, float(near.double().mean())))


# ================================================================ Planar / Radial
def pr_module(p, d, dtype):
    if p["kind"] == "radial":
        f = nf.flows.Radial(d, z_0=p["z_0"].to(dtype))
        f.alpha.data = p["alpha"].to(dtype)
        f.beta.data = p["beta"].to(dtype)
        return f.cuda()
    return nf.flows.Planar(d, act=p["kind"], u=p["u"].to(dtype), w=p["w"].to(dtype), b=p["b"].to(dtype)).cuda()


def pr_inputs(stack, d, k, b):
    g = seeded("grid caps planar radial", stack, d, k, b)
    layers = [pr_ref.make_layer(kind, (d,), g) for kind in pr_ref.kinds_of(stack, k)]
    return layers, randn(g, b, d), randn(g, b, d), randn(g, b)


def pr_keep(trace64, layers, b):
    keep = ~pr_ref.kink_rows(trace64, layers)
    assert int((~keep).sum()) <= 0.02 * b, "%d of %d rows near a kink" % (int((~keep).sum()), b)
    return keep


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["narrow", "ckpt", "wide"])
def test_planar_radial_forward_and_inverse(hip, which, dtype):
    case = case_of("pr.fwd." + which, dtype)
    t0 = time.time()
    d, k, b = case.shape["D"], case.shape["K"], case.B
    for stack, inverse in (("mixed", False), ("leaky_relu", True)):
        layers, z64, _, _ = pr_inputs(stack, d, k, b)
        flows = [pr_module(p, d, dtype) for p in layers]
        z = z64.to(dtype).cuda()
        with torch.no_grad():
            # operand rows in the order the layers are applied: the inverse walks them last to first
            kinds, va, vb, sc = fused_planar.operands(flows[::-1] if inverse else flows, z.device, dtype)
            call = lambda x: _lib.planar_radial_stack(x, kinds, va, vb, sc, inverse=inverse)
            out, ld = call(z)
            want = {}
            for t in DTYPES:
                dev = pr_ref.cast(layers, t, "cuda")
                if inverse:
                    want[t] = pr_ref.inverse(z.to(t), dev)
                else:
                    want[t] = pr_ref.forward(z.to(t), dev)
            if inverse:                                        # test_gpu_planar_radial.inverse_keep
                keep, x = torch.ones(b, dtype=torch.bool, device="cuda"), z.to(F64)
                for p in reversed(pr_ref.cast(layers, F64, "cuda")):
                    keep &= (pr_ref._sum(p["w"] * x) + p["b"]).abs() >= pr_ref.KINK
                    x, _ = pr_ref.planar_inverse(x, p)
                keep = keep.cpu()
                assert int((~keep).sum()) <= 0.02 * b
            else:
                keep = pr_keep(want[F64][2], layers, b)
            tag = "inverse" if inverse else "forward"
            check(case, tag + " z", out, want[F32][0], want[F64][0], dtype, rows=keep)
            check(case, tag + " log_det", ld, want[F32][1], want[F64][1], dtype, rows=keep)
            rows_again(case, call, [(z, 0)], [(out, 0), (ld, 0)])
            if not inverse:
                # what the VJP reads: trace and checkpoints are written by the same trips
                full = _lib.planar_radial_stack(z, kinds, va, vb, sc, want_trace=True)
                assert torch.equal(full[0], out) and torch.equal(full[1], ld)
                assert (full[3] is not None) == ((k - 1) // gc.pr_checkpoint_every(d) >= 1)
                outs = [(full[2], 1)] + ([(full[3], 1)] if full[3] is not None else [])
                rows_again(case, lambda x: [t for t in _lib.planar_radial_stack(x, kinds, va, vb, sc, want_trace=True)[2:] if t is not None],
                           [(z, 0)], outs)
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["narrow", "ckpt", "wide"])
def test_planar_radial_vjp(hip, which, dtype):
    case = case_of("pr.bwd." + which, dtype)
    t0 = time.time()
    d, k, b = case.shape["D"], case.shape["K"], case.B
    groups = int(nf.lib().vcnf_planar_radial_bwd_groups(b, d, k))
    assert groups == case.cap and case.tiles >= 2 * groups + 1, (groups, case.describe())
    layers, z64, gz64, gl64 = pr_inputs("mixed", d, k, b)
    dev64 = pr_ref.cast(layers, F64, "cuda")
    with torch.no_grad():
        keep = pr_keep(pr_ref.forward(z64.cuda(), dev64)[2], layers, b)
    gz64, gl64 = gz64.clone(), gl64.clone()
    gz64[~keep] = 0
    gl64[~keep] = 0
    flows = [pr_module(p, d, dtype) for p in layers]
    z = z64.to(dtype).cuda()

    def kernel(rows, zs=z, gz=gz64, gl=gl64):
        for f in flows:
            f.zero_grad(set_to_none=True)
        x = zs.clone().requires_grad_(True)
        out, ld = fused_planar.run(flows, x, False, None, 1.0)
        ((out * masked(gz.to(dtype).cuda(), rows)).sum() + (ld * masked(gl.to(dtype).cuda(), rows)).sum()).backward()
        grads = {"%s[%d]" % (name, i): p.grad.clone() for i, f in enumerate(flows) for name, p in f.named_parameters()}
        return x.grad, grads

    def reference(rows):
        s = sl(rows)
        out = []
        for t in DTYPES:
            res = pr_ref.gradients(pr_ref.cast(layers, F64, "cuda"), z64[s].cuda(), gz64[s].cuda(), gl64[s].cuda(), t)
            out.append((res[3], {"%s[%d]" % (name, i): g for i, layer in enumerate(res[4]) for name, g in layer.items()}))
        return out

    def layer_noise(r32, r64, name):
        """test_gpu_planar_radial.layer_noise: a layer's one-element gradients take the noise of all the layer's entries"""
        i = name[name.index("["):]
        return max(float((r32[n].double() - r64[n]).abs().max()) for n in r64 if n.endswith(i))

    def judge(name, got, r32, r64, what, all32, all64):
        got = got.detach()
        report(case, what, got, r32, r64)
        assert got.shape == r64.shape and got.dtype == dtype
        if dtype == F32:
            parity(got, r32.cpu(), r64.cpu(), what="%s %s" % (case.name, what),
                   noise_floor=layer_noise(all32, all64, name) if got.numel() == 1 else 0.0)
        else:
            bound = 1e-9 * float(r64.abs().max())
            assert float((got - r64).abs().max()) <= bound, "%s %s: %.3e > %.3e" % (case.name, what, float((got - r64).abs().max()), bound)

    (gx, gp), (gx2, gp2) = kernel(None), kernel(None)
    assert torch.equal(gx, gx2) and all(torch.equal(gp[n], gp2[n]) for n in gp), "two backward calls differ"
    (x32, p32), (x64, p64) = reference(None)
    judge("d z", gx, x32, x64, "d z", p32, p64)
    for n in sorted(gp):
        judge(n, gp[n], p32[n], p64[n], "d " + n, p32, p64)
    for label, rows in trip_masks(case):
        _, got = kernel(rows)
        (_, m32), (_, m64) = reference(rows)
        for n in sorted(got):
            judge(n, got[n], m32[n], m64[n], "d %s, %s only" % (n, label), m32, m64)
    for lo, hi in case.windows():
        sub, _ = kernel(None, narrow(z, 0, lo, hi), gz64[lo:hi], gl64[lo:hi])
        assert torch.equal(sub, gx[lo:hi]), "d z of the rows %d..%d differs when they are a batch of their own" % (lo, hi)
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


# ================================================================ base distributions: heavy tail, full covariance, mixture
def weights_of(b):
    return torch.linspace(0.5, 1.5, b, dtype=F64)                  # the cotangent of log p in the units' gradient tests


def z_cotangent(b, d):
    return torch.cos(0.37 * torch.arange(b * d, dtype=F64)).reshape(b, d)      # unit scale, fixed (test_gpu_mvn)


def base_loss(outs, w, gz):
    """sum_b w_b log p_b, plus sum z . gz when the call returns (z, log p)."""
    loss = (outs[-1] * w).sum()
    return loss + (outs[0] * gz).sum() if len(outs) == 2 else loss


def leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_()


def run_base(case, dtype, q, params, xs64, kernel, restated, direction):
    """One direction of a base distribution past its caps.  q: the module on the GPU in ``dtype``; params: its fp64
    parameters {name: tensor}; xs64: the per-row inputs in fp64 (integer tensors pass through); kernel(q, *xs) and
    restated(p, *xs) -> (log p,) or (z, log p).  Values (a), rows again (b), and the gradients of base_loss: per row
    (a, b) and summed over the batch into the parameters (c)."""
    t0 = time.time()
    b = case.B
    xs = [cast(x, dtype) for x in xs64]
    seen = cast(cast(params, dtype), F64)                          # the parameters as the module holds them
    names = ("log_p",) if direction == "log_prob" else ("z", "log_p")
    with torch.no_grad():
        call = lambda *a: kernel(q, *a)
        outs = call(*xs)
        precisions = DTYPES if dtype == F32 else [F64]             # the fp32 run is the yardstick of the fp32 kernels only
        want = {t: restated(cast(seen, t), *[cast(x, t) for x in xs]) for t in precisions}
    for t in precisions:
        assert all(torch.isfinite(o).all() for o in want[t]), "the reference output is not finite"
    none = (None,) * len(names)
    for name, o, a, c in zip(names, outs, want.get(F32, none), want[F64]):
        check(case, "%s %s" % (direction, name), o, a, c, dtype)
    rows_again(case, call, [(x, 0) for x in xs], [(o, 0) for o in outs])

    w64, gz64 = weights_of(b).cuda(), z_cotangent(b, xs[0][0].numel()).reshape(xs[0].shape).cuda()
    floats = [i for i, x in enumerate(xs) if x.is_floating_point()]

    def grads(rows, sub=None):
        """({input i: per-row gradient}, {parameter: gradient}) through the kernels; rows: cotangents elsewhere are zero;
        sub = (lo, hi): those rows as a batch of their own."""
        q.zero_grad(set_to_none=True)
        pick = (lambda t: t) if sub is None else (lambda t: narrow(t, 0, *sub))
        ins = [pick(x).clone().requires_grad_() if i in floats else pick(x) for i, x in enumerate(xs)]
        base_loss(kernel(q, *ins), pick(masked(w64.to(dtype), rows)), pick(masked(gz64.to(dtype), rows))).backward()
        return {i: ins[i].grad for i in floats}, {k: v.grad.clone() for k, v in q.named_parameters()}

    def ref_grads(rows, t):
        s = sl(rows)
        p = {k: leaf(v, t) for k, v in seen.items()}
        ins = [leaf(x[s], t) if i in floats else x[s] for i, x in enumerate(xs)]
        base_loss(restated(p, *ins), w64[s].to(t), gz64[s].to(t)).backward()
        out = ({i: ins[i].grad for i in floats}, {k: v.grad for k, v in p.items()})
        assert all(torch.isfinite(v).all() for part in out for v in part.values()), "the reference gradient is not finite"
        return out

    (gi, gp), (gi2, gp2) = grads(None), grads(None)
    assert all(torch.equal(gi[i], gi2[i]) for i in gi) and all(torch.equal(gp[k], gp2[k]) for k in gp), "two backward calls differ"
    class Absent(dict):
        __missing__ = lambda self, key: None
    both = lambda rows: ((ref_grads(rows, F32) if dtype == F32 else (Absent(), Absent())), ref_grads(rows, F64))
    (i32, p32), (i64, p64) = both(None)
    assert sorted(gp) == sorted(p64)
    mul = lambda t_, f: None if t_ is None else t_ * f
    for i in gi:
        # a gamma draw reaches far below 1: compared as the gradient with respect to its logarithm (the units' tests)
        scale = (lambda t_: xs[i].to(t_)) if i == 1 and direction == "sample" and len(floats) > 1 else (lambda t_: 1.0)
        check(case, "%s d/d input %d" % (direction, i), gi[i] * scale(dtype), mul(i32[i], scale(F32)), i64[i] * scale(F64), dtype)
    for k in sorted(gp):
        check(case, "%s d/d%s" % (direction, k), gp[k], p32[k], p64[k], dtype)
    for label, rows in trip_masks(case):
        _, got = grads(rows)
        (_, m32), (_, m64) = both(rows)
        for k in sorted(got):
            check(case, "%s d/d%s, %s only" % (direction, k, label), got[k], m32[k], m64[k], dtype)
    for lo, hi in case.windows():
        sub, _ = grads(None, (lo, hi))
        for i in sub:
            assert torch.equal(sub[i], gi[i][lo:hi]), "%s: d/d input %d of the rows %d..%d differs when they are a batch of their own" % (
                case.name, i, lo, hi)
    print("GRIDCAP %-34s %-10s wall %.2f s" % (case.name, direction, time.time() - t0))


TAIL_CLASSES = {"student_t": "StudentT", "gen_gaussian": "GeneralizedGaussian"}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("direction", ["log_prob", "sample"])
@pytest.mark.parametrize("which", ["narrow", "wide"])
@pytest.mark.parametrize("family", tail_ref.FAMILIES)
def test_heavy_tail(hip, family, which, direction, dtype):
    fwd, bwd = case_of("tail.fwd." + which, dtype), case_of("tail.bwd." + which, dtype)
    assert fwd.shape == bwd.shape and bwd.B >= fwd.B               # one shape is past both caps
    case = bwd
    assert case.tiles * case.per_block >= 2 * fwd.cap * fwd.per_block + 1
    d, b = case.shape["D"], case.B
    groups = int(nf.lib().vcnf_tail_bwd_groups(b, d))
    assert groups == case.cap and case.tiles >= 2 * groups + 1, (groups, case.describe())
    p, eps, gamma, z = tail_ref.inputs(family, d, b)
    q = getattr(nf.distributions, TAIL_CLASSES[family])(d).to(dtype)
    q.load_state_dict(tail_ref.cast(p, dtype))
    q = q.cuda()
    if direction == "log_prob":
        run_base(case, dtype, q, p, [z], lambda m, x: (m.log_prob(x),), lambda pp, x: (tail_ref.log_prob(family, x, pp),), direction)
    else:
        run_base(case, dtype, q, p, [eps, gamma], lambda m, e, g: m.from_noise(e, g),
                 lambda pp, e, g: tail_ref.sample(family, e, g, pp), direction)


MVN_CLASSES = {"gaussian": "MultivariateGaussian", "student_t": "MultivariateStudentT"}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d", [3, 17])
@pytest.mark.parametrize("family", mvn_ref.FAMILIES)
def test_mvn(hip, family, d, dtype):
    for stem in ("mvn.fwd.D%d" % d, "mvn.bwd.D%d" % d):
        case = case_of(stem, dtype)
        b = case.B
        if stem.startswith("mvn.bwd"):
            groups = int(nf.lib().vcnf_mvn_bwd_groups(b, d))
            assert groups == case.cap and case.tiles >= 2 * groups + 1, (groups, case.describe())
        p, eps, gamma, z = mvn_ref.inputs(family, d, b)
        q = getattr(nf.distributions, MVN_CLASSES[family])(d).to(dtype)
        q.load_state_dict(mvn_ref.cast(p, dtype))
        q = q.cuda()
        run_base(case, dtype, q, p, [z], lambda m, x: (m.log_prob(x),), lambda pp, x: (mvn_ref.log_prob(family, x, pp),), "log_prob")
        if gamma is None:
            run_base(case, dtype, q, p, [eps], lambda m, e: m.from_noise(e), lambda pp, e: mvn_ref.sample(family, e, None, pp), "sample")
        else:
            run_base(case, dtype, q, p, [eps, gamma], lambda m, e, g: m.from_noise(e, g),
                     lambda pp, e, g: mvn_ref.sample(family, e, g, pp), "sample")


def gmm_log_prob(z, p):
    """test_gpu_gmm.ref_log_prob; p: loc, log_scale [1, M, D], weight_scores [1, M]"""
    w = torch.softmax(p["weight_scores"], 1)
    u = (z[:, None, :] - p["loc"]) / torch.exp(p["log_scale"])
    a = -0.5 * z.shape[1] * math.log(2 * math.pi) + torch.log(w) - 0.5 * torch.sum(u ** 2, 2) - torch.sum(p["log_scale"], 2)
    return torch.logsumexp(a, 1)


def gmm_sample(eps, mode, p):
    z = eps * torch.exp(p["log_scale"][0, mode]) + p["loc"][0, mode]
    return z, gmm_log_prob(z, p)


def gmm_inputs(m, d, b):
    """As test_gpu_gmm.inputs: z the mixture's own draw, the first b // 8 rows x 25 (far tails)."""
    g = seeded("grid caps gmm", m, d)
    p = {"loc": 2.0 * randn(g, 1, m, d), "log_scale": 0.3 * randn(g, 1, m, d), "weight_scores": randn(g, 1, m)}
    mode = torch.multinomial(torch.softmax(p["weight_scores"], 1)[0], b, replacement=True, generator=g)
    eps = randn(g, b, d)
    z = gmm_sample(eps, mode, p)[0].clone()
    z[: b // 8] *= 25.0
    return p, mode, eps, z


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("stem", ["gmm.fwd.narrow", "gmm.fwd.wide", "gmm.bwd.narrow"])
def test_gaussian_mixture(hip, stem, dtype):
    case = case_of(stem, dtype)
    m, d, b = case.shape["M"], case.shape["D"], case.B
    if stem.startswith("gmm.bwd"):
        groups = int(nf.lib().vcnf_gmm_bwd_groups(b, d, m))
        assert groups == case.cap and case.tiles >= 2 * groups + 1, (groups, case.describe())
    p, mode, eps, z = gmm_inputs(m, d, b)
    assert len(torch.unique(mode)) == m
    q = nf.distributions.GaussianMixture(m, d).to(dtype)
    q.load_state_dict(cast(p, dtype, "cpu"))
    q = q.cuda()
    run_base(case, dtype, q, p, [z], lambda mod, x: (mod.log_prob(x),), lambda pp, x: (gmm_log_prob(x, pp),), "log_prob")
    run_base(case, dtype, q, p, [eps, mode], lambda mod, e, k: mod.from_noise(e, k), lambda pp, e, k: gmm_sample(e, k, pp), "sample")


# ================================================================ class-conditional Gaussian (plain torch reference)
CC_CLASSES, CC_TEMPERATURE = 10, 0.7


def cc_tables(p, idx, pixels):
    """Per-sample loc, log_scale [B, C, 1] (+ log T) of the table rows idx"""
    return p["loc"][idx][:, :, None], p["ls"][idx][:, :, None] + math.log(CC_TEMPERATURE)


def cc_log_prob(p, z, idx):
    loc, ls = cc_tables(p, idx, z.shape[2])
    d = z[0].numel()
    return (-0.5 * d * math.log(2 * math.pi) - z.shape[2] * ls.sum((1, 2)) - 0.5 * (((z - loc) / torch.exp(ls)) ** 2).sum((1, 2)),)


def cc_sample(p, eps, idx):
    loc, ls = cc_tables(p, idx, eps.shape[2])
    d = eps[0].numel()
    return loc + torch.exp(ls) * eps, -0.5 * d * math.log(2 * math.pi) - eps.shape[2] * ls.sum((1, 2)) - 0.5 * (eps ** 2).sum((1, 2))


def cc_inputs(c, p, b):
    g = seeded("grid caps class cond", c, p)
    tables = {"loc": 0.3 * randn(g, CC_CLASSES, c), "ls": 0.3 * randn(g, CC_CLASSES, c)}
    idx = torch.randint(CC_CLASSES, (b,), generator=g)
    return tables, idx, randn(g, b, c, p)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["narrow", "wide"])
def test_class_cond_gaussian_forward(hip, which, dtype):
    case = case_of("cc.fwd." + which, dtype)
    t0 = time.time()
    c, p, b = case.shape["C"], case.shape["P"], case.B
    tables, idx, x64 = cc_inputs(c, p, b)
    t = cast(tables, dtype)
    x, i32, i64 = x64.to(dtype).cuda(), idx.to(torch.int32).cuda(), idx.cuda()
    log_prob = lambda z, k: (_lib.cc_gaussian_log_prob(z, t["loc"], t["ls"], k, p, CC_TEMPERATURE),)
    sample = lambda e, k: _lib.cc_gaussian_sample(e, t["loc"], t["ls"], k, p, CC_TEMPERATURE)
    precisions = DTYPES if dtype == F32 else [F64]
    for name, call, restated in (("log_prob", log_prob, cc_log_prob), ("sample", sample, cc_sample)):
        outs = call(x, i32)
        want = {d: restated(cast(cast(tables, dtype), d), x.to(d), i64) for d in precisions}
        for j, o in enumerate(outs):
            check(case, "%s %d" % (name, j), o, want[F32][j] if dtype == F32 else None, want[F64][j], dtype)
        rows_again(case, call, [(x, 0), (i32, 0)], [(o, 0) for o in outs])
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("direction", ["log_prob_bwd", "sample_bwd"])
@pytest.mark.parametrize("which", ["narrow", "narrow_pixels", "wide"])
def test_class_cond_gaussian_vjps_and_reduce_rows(hip, which, direction, dtype):
    case = case_of("cc.bwd." + which, dtype)
    t0 = time.time()
    c, p, b = case.shape["C"], case.shape["P"], case.B
    tables, idx, x64 = cc_inputs(c, p, b)
    t = cast(tables, dtype)
    x, i32, i64 = x64.to(dtype).cuda(), idx.to(torch.int32).cuda(), idx.cuda()
    w = weights_of(b).to(dtype).cuda()
    gz = z_cotangent(b, c * p).reshape(b, c, p).to(dtype).cuda()
    lp_bwd = lambda z, k, g_, gz_: _lib.cc_gaussian_log_prob_bwd(z, t["loc"], t["ls"], k, p, CC_TEMPERATURE, g_)
    s_bwd = lambda e, k, g_, gz_: _lib.cc_gaussian_sample_bwd(e, t["ls"], k, p, CC_TEMPERATURE, gz_, g_)
    precisions = DTYPES if dtype == F32 else [F64]

    def reference(restated, d):
        """(d input, per-sample d loc [B, C], d log_scale [B, C], table gradients [R, C] x 2) by autograd"""
        tab = {k: leaf(v, d) for k, v in cast(cast(tables, dtype), F64).items()}
        rows = {k: v[i64].detach().clone().requires_grad_() for k, v in tab.items()}           # per-sample table rows
        xin = leaf(x, d)
        loc, ls = rows["loc"][:, :, None], rows["ls"][:, :, None] + math.log(CC_TEMPERATURE)
        if restated is cc_log_prob:
            lp = -p * ls.sum((1, 2)) - 0.5 * (((xin - loc) / torch.exp(ls)) ** 2).sum((1, 2))
            loss = (lp * w.to(d)).sum()
        else:
            z = loc + torch.exp(ls) * xin
            lp = -p * ls.sum((1, 2)) - 0.5 * (xin ** 2).sum((1, 2))
            loss = (lp * w.to(d)).sum() + (z * gz.to(d)).sum()
        loss.backward()
        per_class = [torch.zeros(CC_CLASSES, c, dtype=d, device="cuda").index_add_(0, i64, rows[k].grad) for k in ("loc", "ls")]
        return [xin.grad, rows["loc"].grad, rows["ls"].grad] + per_class

    for name, call, restated in ((("log_prob_bwd", lp_bwd, cc_log_prob),) if direction == "log_prob_bwd" else (("sample_bwd", s_bwd, cc_sample),)):
        outs = call(x, i32, w, gz)
        want = {d: reference(restated, d) for d in precisions}
        for j, (o, what) in enumerate(zip(outs, ("d input", "d loc per sample", "d log_scale per sample"))):
            check(case, "%s %s" % (name, what), o, want[F32][j] if dtype == F32 else None, want[F64][j], dtype)
        rows_again(case, call, [(x, 0), (i32, 0), (w, 0), (gz, 0)], [(o, 0) for o in outs])
        # the per-sample gradients onto the table rows: a fixed-order sum over the whole batch
        for j, what in ((1, "d loc rows"), (2, "d log_scale rows")):
            summed = _lib.cc_gaussian_reduce_rows(outs[j], i32, CC_CLASSES)
            assert torch.equal(summed, _lib.cc_gaussian_reduce_rows(outs[j], i32, CC_CLASSES)), "two calls differ"
            check(case, "%s %s" % (name, what), summed, want[F32][j + 2] if dtype == F32 else None, want[F64][j + 2], dtype)
            for label, rows in trip_masks(case):                 # only one trip's samples carry a gradient
                part = _lib.cc_gaussian_reduce_rows(masked(outs[j], rows), i32, CC_CLASSES)
                s = sl(rows)
                r = {d: torch.zeros(CC_CLASSES, c, dtype=d, device="cuda").index_add_(0, i64[s], want[d][j][s]) for d in precisions}
                check(case, "%s %s, %s only" % (name, what, label), part, r[F32] if dtype == F32 else None, r[F64], dtype)
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


# ================================================================ affine family (plain torch references)
def affine_ref(z, param, t_off, d_t, scale_map, inverse):
    """flows/affine/coupling.py: the transformed columns t_off .. t_off + d_t, shift = param[:, 0::2], scale = param[:, 1::2]"""
    out = z.clone()
    v = z[:, t_off:t_off + d_t]
    shift, sc = param[:, 0::2], param[:, 1::2]
    if scale_map == _lib.SCALE_EXP:
        out[:, t_off:t_off + d_t] = (v - shift) * torch.exp(-sc) if inverse else v * torch.exp(sc) + shift
        ld = sc.sum(1)
        return out, -ld if inverse else ld
    sg = torch.sigmoid(sc + 2)
    lg = torch.log(sg)
    divide = (scale_map == _lib.SCALE_SIGMOID) != bool(inverse)
    if inverse:
        out[:, t_off:t_off + d_t] = (v - shift) / sg if divide else (v - shift) * sg
    else:
        out[:, t_off:t_off + d_t] = v / sg + shift if divide else v * sg + shift
    return out, (-lg if divide else lg).sum(1)


def affine_case(case, dtype, name, call, restated, xs64, tol64=AFFINE64, exact=False):
    """Values against the plain-torch reference (a), rows again (b); exact maps by torch.equal."""
    xs = [cast(x, dtype) for x in xs64]
    outs = call(*xs)
    outs = outs if isinstance(outs, (tuple, list)) else (outs,)
    precisions = DTYPES if dtype == F32 and not exact else [F64 if not exact else dtype]
    want = {d: restated(*[cast(x, d) for x in xs]) for d in precisions}
    want = {d: v if isinstance(v, (tuple, list)) else (v,) for d, v in want.items()}
    for j, o in enumerate(outs):
        if exact:
            assert torch.equal(o, want[dtype][j]), "%s %s: output %d is not the exact map" % (case.name, name, j)
        else:
            check(case, "%s %d" % (name, j), o, want[F32][j] if dtype == F32 else None, want[F64][j], dtype, tol64=tol64)
    tup = lambda r: r if isinstance(r, (tuple, list)) else (r,)
    rows_again(case, lambda *a: tup(call(*a)), [(x, 0) for x in xs], [(o, 0) for o in outs])


AFFINE_KERNELS = ["coupling-exp", "coupling-sigmoid", "masked", "maf", "diag_gaussian"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["narrow", "wide"])
@pytest.mark.parametrize("kernel", AFFINE_KERNELS)
def test_affine_row_kernels(hip, kernel, which, dtype):
    """Both directions of one row kernel of affine_kernels.hip."""
    t0 = time.time()
    case = case_of("affine.%s.%s" % (kernel.split("-")[0], which), dtype)
    d, b = case.shape["D"], case.B
    g = seeded("grid caps affine", kernel, which)
    if kernel.startswith("coupling"):
        t_off, d_t = case.shape["t_off"], case.shape["d_t"]
        code = _lib.SCALE_EXP if kernel == "coupling-exp" else _lib.SCALE_SIGMOID
        z, param = randn(g, b, d), torch.stack([randn(g, b, d_t), 0.5 * randn(g, b, d_t)], 2).reshape(b, 2 * d_t)
        for inverse in (False, True):
            affine_case(case, dtype, "%s inverse %d" % (kernel, inverse), lambda x, pr: _lib.affine_coupling(x, pr, t_off, d_t, code, inverse),
                        lambda x, pr: affine_ref(x, pr, t_off, d_t, code, inverse), [z, param])
    elif kernel == "masked":
        z, s, t = randn(g, b, d), 0.5 * randn(g, b, d), randn(g, b, d)
        mask = (torch.arange(d) % 2 == 0).to(F64)
        for inverse in (False, True):
            def restated(x, s_, t_, inverse=inverse):
                m = mask.to(x)
                if inverse:
                    return m * x + (1 - m) * (x - t_) * torch.exp(-s_), -((1 - m) * s_).sum(1)
                return m * x + (1 - m) * (x * torch.exp(s_) + t_), ((1 - m) * s_).sum(1)
            affine_case(case, dtype, "masked inverse %d" % inverse,
                        lambda x, s_, t_: _lib.masked_affine(x, s_, t_, mask.to(x), inverse), restated, [z, s, t])
    elif kernel == "maf":                                          # params [B, D, 2] = (scale logit, shift)
        x, params = randn(g, b, d), randn(g, b, d, 2).reshape(b, 2 * d)
        for inverse in (False, True):
            def restated(v, pr, inverse=inverse):
                pr = pr.reshape(len(v), -1, 2)
                scale = torch.sigmoid(pr[..., 0] + 2) + 1e-3
                ld = torch.log(scale).sum(1)
                return ((v - pr[..., 1]) / scale, -ld) if inverse else (scale * v + pr[..., 1], ld)
            affine_case(case, dtype, "maf inverse %d" % inverse, lambda v, pr: _lib.maf_affine(v, pr, inverse), restated, [x, params])
    else:
        x = randn(g, b, d)
        loc, ls = cast(randn(g, d), dtype), cast(0.3 * randn(g, d), dtype)
        norm = -0.5 * d * math.log(2 * math.pi)
        lt = math.log(CC_TEMPERATURE)
        affine_case(case, dtype, "diag log_prob", lambda v: _lib.diag_gaussian_log_prob(v, loc, ls, CC_TEMPERATURE),
                    lambda v: norm - (ls.to(v) + lt + 0.5 * ((v - loc.to(v)) / torch.exp(ls.to(v) + lt)) ** 2).sum(1), [x])
        affine_case(case, dtype, "diag sample", lambda v: _lib.diag_gaussian_sample(v, loc, ls, CC_TEMPERATURE),
                    lambda v: (loc.to(v) + torch.exp(ls.to(v) + lt) * v, norm - (ls.to(v) + lt + 0.5 * v * v).sum(1)), [x])
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_affine_flat_kernels(hip, dtype):
    t0 = time.time()
    g = seeded("grid caps affine flat")
    case = case_of("affine.const.narrow", dtype)
    c, b = case.shape["D"], case.B
    z = randn(g, b, c)
    s, t = cast(0.3 * randn(g, c), dtype), cast(randn(g, c), dtype)
    for inverse in (False, True):
        affine_case(case, dtype, "const inverse %d" % inverse, lambda x: _lib.affine_const(x, s, t, inverse),
                    lambda x: (x - t.to(x)) * torch.exp(-s.to(x)) if inverse else x * torch.exp(s.to(x)) + t.to(x), [z])
    perm = torch.tensor([2, 0, 1])
    idx32 = perm.to(torch.int32).cuda()
    affine_case(case_of("affine.permute.narrow", dtype), dtype, "permute", lambda x: _lib.permute(x, idx32), lambda x: x[:, perm.to(x.device)],
                [z], exact=True)
    first = 1
    affine_case(case_of("affine.split.narrow", dtype), dtype, "split", lambda x: _lib.split_columns(x, idx32, first),
                lambda x: (x[:, perm.to(x.device)[:first]].contiguous(), x[:, perm.to(x.device)[first:]].contiguous()), [z], exact=True)
    pa, pb = randn(g, b, first), randn(g, b, c - first)
    affine_case(case_of("affine.merge.narrow", dtype), dtype, "merge", lambda a, b_: _lib.merge_columns(a, b_, idx32),
                lambda a, b_: torch.cat([a, b_], 1)[:, perm.to(a.device)], [pa, pb], exact=True)
    print("GRIDCAP %-34s wall %.2f s" % ("affine flat %s" % tname(dtype), time.time() - t0))


# ================================================================ elementwise splines with batch-shared logit rows
SPLINE_BINS, SPLINE_CHUNK = 8, 16384


def spline_inputs(b, period, *key):
    """The well-conditioned logit rows of the spline edge tests (tier A, 8 bins, linear tails) and x uniform on 1.2 x the
    interval, so that a sixth of the elements lies in the tails."""
    assert period == edge_ref.R
    uw, uh, ud = edge_ref.rows("A", SPLINE_BINS, "linear")
    g = seeded("grid caps spline", b, *key)
    x = (torch.rand(b, period, generator=g, dtype=F64) * 2 - 1) * edge_ref.TB * 1.2
    return x, uw, uh, ud


def spline_oracle(x, uw, uh, ud, inverse, dtype, limits=None):
    """The oracle on x [B, period] and logit rows [period, .] in ``dtype`` on the device, in runs of rows (the logits are
    expanded per element): linear tails, or no tails and the tensor interval ``limits`` (four tensors like x)."""
    ys, lads = [], []
    for lo in range(0, len(x), SPLINE_CHUNK):
        xc = x[lo:lo + SPLINE_CHUNK].to(dtype)
        ex = lambda t: t.to(dtype).expand(len(xc), *t.shape).contiguous()
        lims = None if limits is None else [t[lo:lo + SPLINE_CHUNK].to(dtype) for t in limits]
        y, lad = edge_ref.soft_oracle(xc, ex(uw), ex(uh), ex(ud), inverse, None if limits else "linear", lims)
        ys.append(y)
        lads.append(lad)
    return torch.cat(ys), torch.cat(lads)


def spline_values(case, name, got, x, logits, inverse, dtype, limits=None):
    """test_gpu_spline_limits: fp32 within 1e-4 + 8 x the oracle's own fp32 error, fp64 within 1e-10"""
    r64 = spline_oracle(x, *logits, inverse, F64, limits)
    r32 = spline_oracle(x, *logits, inverse, F32, limits) if dtype == F32 else (None, None)
    for what, o, a, c in zip(("y", "logabsdet"), got, r32, r64):
        assert torch.isfinite(c).all() and o.dtype == dtype
        err = float((o.double() - c).abs().max())
        if dtype == F32:
            ok = torch.isfinite(a)
            noise = float((a.double() - c)[ok].abs().max())
            print("GRIDCAP %-34s %-28s max|got - ref64| %.3e  ref32 noise %.3e" % (case.name, "%s %s" % (name, what), err, noise))
            assert err <= 1e-4 + 8 * noise, (case.name, name, what, err, noise)
        else:
            print("GRIDCAP %-34s %-28s max|got - ref64| %.3e" % (case.name, "%s %s" % (name, what), err))
            assert err <= 1e-10, (case.name, name, what, err)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("entry", ["strided", "dense", "limits"])
def test_spline_elementwise_shared_rows(hip, entry, dtype, inverse):
    """The one-element-per-thread loop of the elementwise entry points without a logit row per element (8 bins past the
    cap would be 16.8 M logits per tensor).  "strided": vcnf_rqs_elementwise_strided_* with period = 32, element i reads
    the logit row i % 32.  "dense": vcnf_rqs_elementwise_* with a row stride of 0, every element reads row 0.  "limits":
    vcnf_rqs_elementwise_limits_* (no tails) the same way, with an interval of its own per element, drawn as
    test_gpu_spline_limits draws it.  In fp64 the three are instances of one kernel."""
    case = case_of("rqs.strided.narrow", dtype)
    t0 = time.time()
    period, b, k = case.shape["period"], case.B, SPLINE_BINS
    x64, uw, uh, ud = spline_inputs(b, period, entry, inverse)
    limits = None
    if entry == "limits":
        uw, uh, ud = edge_ref.rows("A", k, None)
        g = seeded("grid caps spline limits", inverse)
        limits = []
        for _ in range(2):                                         # left ~ U(-3, -1), right = left + U(0.5, 4); bottom, top alike
            lo = torch.rand(b, period, generator=g, dtype=F64) * 2 - 3
            limits += [lo.to(dtype).cuda(), (lo + 0.5 + 3.5 * torch.rand(b, period, generator=g, dtype=F64)).to(dtype).cuda()]
        lo, hi = (limits[2], limits[3]) if inverse else (limits[0], limits[1])
        u = (torch.rand(b, period, generator=g, dtype=F64) * 0.998 + 0.001).cuda()
        x64 = lo.double() + (hi.double() - lo.double()) * u
    if entry != "strided":
        uw, uh, ud = (t[:1].expand(period, -1) for t in (uw, uh, ud))
    x, logits = x64.to(dtype).cuda(), [t.to(dtype).cuda().contiguous() for t in (uw, uh, ud)]
    cfg = _lib.make_cfg(k, None if entry == "limits" else "linear", tail_bound=edge_ref.TB)

    # The wrappers of vcnf_amd._lib take one logit row per element; a shared row (stride 0, or a period) is expressed at
    # the entry points only, so the calls below are the wrappers' own (_lib.rqs_elementwise, rqs_elementwise_image,
    # rqs_elementwise_limits) with other strides, through the same private helpers _call, _sfx, _cfg_of, _bad_if,
    # _limit_layouts and _bcast.  If one of those is renamed, this test follows the wrappers.
    def call(xs, *lims):
        y, lad = torch.empty_like(xs), torch.empty_like(xs)
        tail = (y, lad, xs.numel(), _lib._cfg_of(cfg, xs), bool(inverse), _lib._bad_if(inverse, xs.device))
        if entry == "strided":
            _lib._call("vcnf_rqs_elementwise_strided" + _lib._sfx(xs), xs.device, xs, *logits, k, k, k - 1, 1, 1, period, *tail)
        elif entry == "dense":
            _lib._call("vcnf_rqs_elementwise" + _lib._sfx(xs), xs.device, xs, *logits, 0, 0, 0, *tail)
        else:
            lay = _lib._limit_layouts(lims, xs, False)
            assert all(l[0].numel() == xs.numel() and l[1:] == (xs.numel(), 1) for l in lay)
            _lib._call("vcnf_rqs_elementwise_limits" + _lib._sfx(xs), xs.device, xs, *logits, 0, 0, 0, *[l[0] for l in lay],
                       _lib._bcast(lay), *tail)
        return y, lad

    lims = limits or []
    got = call(x, *lims)
    spline_values(case, entry, got, x, logits, inverse, dtype, limits)
    rows_again(case, call, [(x, 0)] + [(t, 0) for t in lims], [(o, 0) for o in got])
    if inverse:
        nf.check_discriminant()
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_spline_shared_table(hip, inverse):
    case = gc.CASES["rqs.shared.narrow.f32"]
    t0 = time.time()
    period, b, k = case.shape["period"], case.B, SPLINE_BINS
    x64, uw, uh, ud = spline_inputs(b, period, "shared", inverse)
    x, logits = x64.float().cuda(), [t.float().cuda() for t in (uw, uh, ud)]
    cfg = _lib.make_cfg(k, "linear", tail_bound=edge_ref.TB)
    call = lambda xs: _lib.rqs_elementwise_shared(xs, *logits, cfg, inverse)
    got = call(x)
    spline_values(case, "shared", got, x, logits, inverse, F32)
    rows_again(case, call, [(x, 0)], [(o, 0) for o in got])
    if inverse:
        nf.check_discriminant()
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_spline_shared_vjp(hip, inverse):
    case = gc.CASES["rqs.shared_bwd.narrow.f32"]
    t0 = time.time()
    period, b, k = case.shape["period"], case.B, SPLINE_BINS
    groups = int(nf.lib().vcnf_rqs_shared_bwd_groups(b, period))
    assert groups == case.cap and b >= 2 * groups + 1, (groups, case.describe())
    x64, uw, uh, ud = spline_inputs(b, period, "shared vjp", inverse)
    g = seeded("grid caps spline cotangent", inverse)
    gy64, gl64 = randn(g, b, period).cuda(), randn(g, b).cuda()
    x, logits = x64.float().cuda(), [t.float().cuda() for t in (uw, uh, ud)]
    cfg = _lib.make_cfg(k, "linear", tail_bound=edge_ref.TB)
    kernel = lambda rows, xs=x, gy=gy64, gl=gl64: _lib.rqs_shared_bwd(xs, *logits, masked(gy.float(), rows), masked(gl.float(), rows), cfg, inverse)

    def reference(rows, dtype):
        """(g_x, g_uw, g_uh, g_ud) by autograd of the oracle over the rows, in runs of rows"""
        s = sl(rows)
        leaves = [leaf(t, dtype) for t in logits]
        xs, gys, gls = x[s].to(dtype), gy64[s].to(dtype), gl64[s].to(dtype)
        gx = []
        for lo in range(0, len(xs), SPLINE_CHUNK):
            xc = xs[lo:lo + SPLINE_CHUNK].clone().requires_grad_()
            ex = lambda t: t.expand(len(xc), *t.shape)
            y, lad = edge_ref.soft_oracle(xc, *[ex(t) for t in leaves], inverse, "linear", None)
            ((y * gys[lo:lo + SPLINE_CHUNK]).sum() + (lad.sum(1) * gls[lo:lo + SPLINE_CHUNK]).sum()).backward()
            gx.append(xc.grad)
        return [torch.cat(gx)] + [t.grad for t in leaves]

    names = ("g_x", "g_uw", "g_uh", "g_ud")
    first, again = kernel(None), kernel(None)
    assert all(torch.equal(a, c) for a, c in zip(first, again)), "two calls differ"
    for label, rows in ((("", None),) + tuple((", %s only" % n, r) for n, r in trip_masks(case))):
        got = first if rows is None else kernel(rows)
        w32, w64 = reference(rows, F32), reference(rows, F64)
        for name, o, a, c in zip(names, got, w32, w64):
            if name == "g_x":
                o = o[sl(rows)]
            print("GRIDCAP %-34s %-28s max|got - ref64| %.3e  ref32 noise %.3e  of %.3e" % (
                case.name, name + label, float((o.double() - c).abs().max()), float((a.double() - c).abs().max()), float(c.abs().max())))
            close(o, c.cpu(), "%s %s%s" % (case.name, name, label), want32=a.cpu())
    for lo, hi in case.windows():
        sub = kernel(None, narrow(x, 0, lo, hi), gy64[lo:hi], gl64[lo:hi])
        assert torch.equal(sub[0], first[0][lo:hi]), "g_x of the rows %d..%d differs when they are a batch of their own" % (lo, hi)
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


# ================================================================ elementwise spline VJPs (one logit row per element)
def spline_vjp_reference(x, uw, uh, ud, gy, gl_of, inverse, tails, limits, dtype):
    """Autograd of the oracle (assertion-free restatement) in ``dtype`` on the device: gradients of x, the three logit
    tensors and, with tensor limits, the four limits.  gl_of(lad) -> the log|det| term of the loss."""
    leaves = [leaf(t, dtype) for t in (x, uw, uh, ud)]
    xl, wl, hl, dl = leaves
    if tails == "linear":
        inside = (xl >= -edge_ref.TB) & (xl <= edge_ref.TB)
        edge = edge_ref.orqs.boundary_derivative_logit()
        y, lad = edge_ref.soft_spline(torch.where(inside, xl, torch.zeros_like(xl)), wl, hl,
                                      torch.nn.functional.pad(dl, (1, 1), value=edge), inverse,
                                      -edge_ref.TB, edge_ref.TB, -edge_ref.TB, edge_ref.TB)
        y, lad = torch.where(inside, y, xl), torch.where(inside, lad, torch.zeros_like(lad))
    else:
        leaves += [leaf(t, dtype) for t in limits]
        y, lad = edge_ref.soft_spline(xl, wl, hl, dl, inverse, *leaves[4:])
    ((y * gy.to(dtype)).sum() + gl_of(lad, dtype)).backward()
    out = [t.grad for t in leaves]
    assert all(torch.isfinite(g).all() for g in out), "the reference gradient is not finite"
    return out


def spline_vjp_judge(case, names, got, w32, w64, dtype):
    """fp32: test_gpu_grad.close (the oracle's fp32 gradients as the yardstick, at most 2e-3 of the elements - the
    bin-boundary cap - outside); fp64: test_gpu_f64_grad.tight (every element)."""
    for name, o, a, c in zip(names, got, w32 or [None] * len(got), w64):
        if c.numel() == 0:                                         # one bin with linear tails has no derivative logit
            assert o.numel() == 0
            continue
        o = o.reshape(c.shape)
        print("GRIDCAP %-34s %-28s max|got - ref64| %.3e  ref32 noise %.3e  of %.3e" % (
            case.name, name, float((o.double() - c).abs().max()), float((a.double() - c).abs().max()) if a is not None else float("nan"),
            float(c.abs().max())))
        if dtype == F32:
            close(o, c.cpu(), "%s %s" % (case.name, name), want32=a.cpu())
        else:
            tight(o, c, "%s %s" % (case.name, name))


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("entry", ["dense-f32", "dense-f64", "limits-f32", "limitgrads-f32", "packed-f32"])
def test_spline_elementwise_vjps(hip, entry, inverse):
    """vcnf_rqs_elementwise_bwd_*, vcnf_rqs_elementwise_limits_bwd_f32 and vcnf_rqs_packed_bwd_* past their caps.  The
    packed fp32 call takes the variant that stages each block of 256 logit rows in LDS and reuses the stage from trip to
    trip; the cotangent of log|det| is per sample of three elements there.  (a), (b) and the two-calls check; the
    gradients are per element, there is no sum over the batch."""
    kind, t = entry.split("-")
    part = slice(4, 8) if kind == "limitgrads" else slice(0, 4)    # the tensor-limit call is judged in two cases
    kind = "limits" if kind == "limitgrads" else kind
    dtype = F64 if t == "f64" else F32
    case = gc.CASES["rqs.bwd.%s.%s" % (kind, t)]
    t0 = time.time()
    k, tails = case.shape["bins"], case.shape["tails"]
    nd = k - 1 if tails == "linear" else k + 1
    c = case.shape.get("C", 1)
    b, n = case.B, case.B * c
    g = seeded("grid caps spline vjp", entry, inverse)
    cfg = _lib.make_cfg(k, tails, tail_bound=edge_ref.TB)
    params = (1.5 * randn(g, b, c, 2 * k + nd)).to(dtype).cuda()
    uw, uh, ud = params[..., :k], params[..., k:2 * k], params[..., 2 * k:]
    gy = randn(g, b, c).to(dtype).cuda()
    limits = None
    if kind == "limits":
        limits = []
        for _ in range(2):                                         # as test_gpu_spline_limits draws them
            lo = torch.rand(b, c, generator=g, dtype=F64) * 2 - 3
            limits += [lo.to(dtype).cuda(), (lo + 0.5 + 3.5 * torch.rand(b, c, generator=g, dtype=F64)).to(dtype).cuda()]
        lo, hi = (limits[2], limits[3]) if inverse else (limits[0], limits[1])
        u = (torch.rand(b, c, generator=g, dtype=F64) * 0.998 + 0.001).cuda()
        x = (lo.double() + (hi.double() - lo.double()) * u).to(dtype)
    else:
        x = ((torch.rand(b, c, generator=g, dtype=F64) * 2 - 1) * edge_ref.TB * 1.2).to(dtype).cuda()
    if kind == "packed":
        assert gc.rqs_bwd_packed(1, k, nd), "the staged variant is not the one launched"
        gl = randn(g, b).to(dtype).cuda()                          # per sample
        gl_of = lambda lad, d: (lad.sum(1) * gl.to(d)).sum()
        flat = params.reshape(b, c * (2 * k + nd))
        call = lambda xs, ps, gys, gls: _lib.rqs_packed_bwd(xs, ps, gys, gls, cfg, inverse)
        ins = [x, flat, gy, gl]
        split = lambda out: [out[0], out[1].reshape(b, c, -1)[..., :k], out[1].reshape(b, c, -1)[..., k:2 * k], out[1].reshape(b, c, -1)[..., 2 * k:]]
    else:
        gl = randn(g, b, c).to(dtype).cuda()                       # per element
        gl_of = lambda lad, d: (lad * gl.to(d)).sum()
        if kind == "dense":
            call = lambda xs, w, h, d_, gys, gls: _lib.rqs_elementwise_bwd(xs, w, h, d_, gys, gls, cfg, inverse)
            ins = [x, uw.contiguous(), uh.contiguous(), ud.contiguous(), gy, gl]
            split = list
        else:
            def call(xs, w, h, d_, gys, gls, *lims):
                out = _lib.rqs_elementwise_limits_bwd(xs, w, h, d_, lims, gys, gls, cfg, inverse)
                return list(out[:4]) + list(out[4])
            ins = [x, uw.contiguous(), uh.contiguous(), ud.contiguous(), gy, gl] + limits
            split = list
    got, again = call(*ins), call(*ins)
    assert all(torch.equal(a, c_) for a, c_ in zip(got, again)), "two calls differ"
    names = ["g_x", "g_uw", "g_uh", "g_ud"] + (["g_left", "g_right", "g_bottom", "g_top"] if limits else [])
    w64 = spline_vjp_reference(x, uw, uh, ud, gy, gl_of, inverse, tails, limits, F64)
    w32 = spline_vjp_reference(x, uw, uh, ud, gy, gl_of, inverse, tails, limits, F32) if dtype == F32 else None
    spline_vjp_judge(case, names[part], split(got)[part], w32 and w32[part], w64[part], dtype)
    rows_again(case, lambda *a_: call(*a_)[part], [(t_, 0) for t_ in ins], [(o, 0) for o in got][part])
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


# ================================================================ a run of masked affine layers with their MLPs
def masked_stack_model(d, h, pairs, dtype, gain):
    """K x [MaskedAffineFlow(b | 1 - b, t, s), ActNorm] with s, t = MLP([d, h, d]), as test_gpu_parity and test_gpu_grad
    build it; the ActNorm layers initialised by a first batch."""
    mask = torch.tensor([1.0 if i % 2 == 0 else 0.0 for i in range(d)])
    flows = []
    for i in range(pairs):
        s, t = nf.nets.MLP([d, h, d], init_zeros=True), nf.nets.MLP([d, h, d], init_zeros=True)
        flows += [nf.flows.MaskedAffineFlow(mask if i % 2 == 0 else 1 - mask, t, s), nf.flows.ActNorm(d)]
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(d), flows)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if ".net.2." in n:
                p.normal_(0.0, gain)
    model = model.to(dtype).cuda()
    with torch.no_grad():
        model.log_prob(torch.randn(512, d, device="cuda", dtype=dtype))
        for f in model.flows:
            if isinstance(f, nf.flows.ActNorm):
                f.s.add_(0.05 * torch.randn_like(f.s))
                f.t.add_(0.05 * torch.randn_like(f.t))
    return model


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_masked_affine_stack(hip, dtype):
    """The one-launch run and its VJP (csrc/masked_affine_stack.hip) against the per-layer path, with the bounds of
    test_gpu_parity.test_masked_affine_stack_single_launch_matches_per_layer and
    test_gpu_grad.test_masked_affine_stack_vjp_matches_per_layer_autograd; rows again, bitwise."""
    from vcnf_amd import fused_masked
    case = case_of("mstack.narrow", dtype)
    t0 = time.time()
    d, h, b = case.shape["D"], case.shape["H"], case.B
    torch.manual_seed(10 * d + h)
    model = masked_stack_model(d, h, 5, dtype, 0.5 / h ** 0.5).eval()
    x, w = torch.randn(b, d, device="cuda", dtype=dtype), torch.randn(b, d, device="cuda", dtype=dtype)
    assert fused_masked.plan(list(reversed(model.flows)), 0, x)[0] == len(model.flows)
    tol = dict(rtol=2e-5, atol=2e-5) if dtype == F32 else dict(rtol=1e-11, atol=1e-11)

    def values(xs):
        with torch.no_grad():
            return (model.log_prob(xs),) + tuple(model.sample_from(xs))
    out = {}
    for stacks in (True, False):
        model.fuse_masked_stacks = stacks
        out[stacks] = values(x)
    model.fuse_masked_stacks = True
    for name, a, c in zip(("log_prob", "sample z", "sample log_q"), out[True], out[False]):
        print("GRIDCAP %-34s %-28s max|run - per layer| %.3e  of %.3e" % (case.name, name, float((a - c).abs().max()), float(c.abs().max())))
        assert torch.isfinite(c).all() and torch.allclose(a, c, **tol), (name, float((a - c).abs().max()))
    assert all(torch.equal(a, c) for a, c in zip(out[True], values(x))), "two calls differ"
    rows_again(case, values, [(x, 0)], [(o, 0) for o in out[True]])

    # The conditioners are ReLU networks.  Where a hidden unit's input is within KINK of 0, one rounding decides the side
    # and the two fp32 paths may take different, equally valid one-sided derivatives (measured at this batch: a handful
    # of rows off by up to 1e-2 of the largest entry in either path against the fp64 per-layer pass, the rest within
    # 2e-6).  As the Planar / Radial tests do at their kinks, such rows - found in the fp64 per-layer pass - carry no
    # cotangent; they may be at most 2 % of the batch.  The band is 2e-5: the hidden inputs are of size 1 and the fp32
    # paths carry them to about 1e-6 (300 hidden units per row: a band of 1e-4 would leave out 5.5 % of the rows).
    kink = 2e-5
    model64 = copy.deepcopy(model).double()
    model64.fuse_masked_stacks = False

    def kink_rows(which, xs):
        near = []
        firsts = [net.net[0] for f in model64.flows if isinstance(f, nf.flows.MaskedAffineFlow) for net in (f.s, f.t)]
        hooks = [m.register_forward_hook(lambda mod, inp, out: near.append((out.abs() < kink).any(1))) for m in firsts]
        with torch.no_grad():
            model64.log_prob(xs.double()) if which == "density" else model64.sample_from(xs.double())
        for hk in hooks:
            hk.remove()
        assert len(near) == len(firsts)
        return torch.stack(near).any(0)

    def grads(stacks, which, keep, xs=x, ws=w, rows=None):
        model.fuse_masked_stacks = stacks
        model.zero_grad(set_to_none=True)
        xin = xs.clone().requires_grad_(True)
        ones = masked(keep.to(dtype), rows)
        if which == "density":
            loss = -(model.log_prob(xin) * ones).sum() / b
        else:
            z, lq = model.sample_from(xin)
            loss = (z * masked(ws * keep.to(dtype)[:, None], rows)).sum() / b + (lq * ones).sum() / b
        loss.backward()
        model.fuse_masked_stacks = True
        return [xin.grad] + [p.grad.clone() for p in model.parameters()]
    bound = 1e-9 if dtype == F64 else 3e-4
    for which in ("density", "sampling"):
        keep = ~kink_rows(which, x)
        assert int((~keep).sum()) <= 0.02 * b, "%d of %d rows near a kink" % (int((~keep).sum()), b)
        first = grads(True, which, keep)
        # the parameter sums of this unit are hardware atomics (no fixed order): only the per-row gradient repeats bitwise
        assert torch.equal(first[0], grads(True, which, keep)[0]), "d x differs between two backward calls"
        for label, rows in (("", None),) + tuple((", %s only" % n, r) for n, r in trip_masks(case)):
            g1, g0 = first if rows is None else grads(True, which, keep, rows=rows), grads(False, which, keep, rows=rows)
            worst = max(float((a - c).abs().max()) / (float(c.abs().max()) + 1e-3) for a, c in zip(g1, g0))
            print("GRIDCAP %-34s %-28s worst error / largest entry %.3e  kink rows %d" % (case.name, which + label, worst, int((~keep).sum())))
            for i, (a, c) in enumerate(zip(g1, g0)):
                err, scale = float((a - c).abs().max()), float(c.abs().max())
                assert err <= bound * (scale + 1e-3), (which, label, i, err, scale)
        for lo, hi in case.windows():
            sub = grads(True, which, keep[lo:hi], narrow(x, 0, lo, hi), narrow(w, 0, lo, hi))
            assert torch.equal(sub[0], first[0][lo:hi]), "d x of the rows %d..%d differs when they are a batch of their own" % (lo, hi)
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


# ================================================================ elementwise maps of the residual block (fp32)
RESBLOCK = {
    0: lambda x, y, z: (x + y * torch.sigmoid(z),),
    1: lambda x, y, z: (x * torch.sigmoid(z), x * y * torch.sigmoid(z) * (1 - torch.sigmoid(z))),
    2: lambda x, y, z: (torch.where(y > 0, x, torch.zeros_like(x)),),
    3: lambda x, y, z: (z + torch.where(y > 0, x, torch.zeros_like(x)),),
}


@pytest.mark.parametrize("op", sorted(RESBLOCK))
@pytest.mark.parametrize("which", ["scalar", "vec"])
def test_resblock_ops(hip, which, op):
    """The four maps of csrc/resblock_ops.hip, one element or one pack of four per thread: the selects exactly, the
    sigmoid gates by helpers.parity against the same formulas in torch."""
    case = gc.CASES["resblock.%s.f32" % which]
    t0 = time.time()
    pack = case.shape["pack"]
    g = seeded("grid caps resblock", which)
    a, b_, c = (randn(g, case.B, pack).float().cuda() for _ in range(3))
    assert (a.numel() % 4 == 0) == (which == "vec")
    tup = lambda r: r if isinstance(r, tuple) else (r,)
    call = lambda x, y, z: tup(_lib.resblock_op(op, x, y, None if op == 2 else z, two_outputs=op == 1))
    got = call(a, b_, c)
    r32 = RESBLOCK[op](a, b_, c)
    for j, o in enumerate(got):
        if op >= 2:
            assert torch.equal(o, r32[j]), "op %d is not the exact map" % op
        else:
            check(case, "op %d output %d" % (op, j), o, r32[j], RESBLOCK[op](a.double(), b_.double(), c.double())[j], F32)
    rows_again(case, call, [(a, 0), (b_, 0), (c, 0)], [(o, 0) for o in got])
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


# ================================================================ the matrix kernels: conv1x1, conv3x3 + conv1x1, channel mixing, fused affine
# A "tile" case of grid_caps.py holds 2 x cap + 1 tiles: every workgroup of the capped grid makes two trips and the
# first one a ragged third.  These kernels keep weights in registers for the whole launch, reuse LDS fragments from
# pass to pass and (conv1x1) request the next pass's rows one pass ahead: what a later trip starts from is what the
# earlier one left.  (a) - (c) as above, with the references and acceptance rules of each kernel's own test in
# test_gpu_parity.py.
SLOPES = (0.1, 0.2)                                               # both LeakyReLUs on: the masked paths run


def by_trip(case, what, got, r32, r64):
    """The GRIDCAP line of the whole batch and one per trip: a trip that is merely worse shows in the log."""
    report(case, what, got, r32, r64)
    assert case.trips == 3
    for t in range(case.trips):
        lo, hi = case.trip_rows(t)
        assert lo < hi
        report(case, "%s, trip %d" % (what, t), got[lo:hi], None if r32 is None else r32[lo:hi], r64[lo:hi])


def accept_matrix(case, what, got, r32, r64, floor):
    """The rule of the conv and channel-mix kernels' own tests: e_got <= 2 e_ref + floor * scale over every element,
    e_ref being torch's fp32 composition against the fp64 one."""
    assert got.shape == r64.shape and got.dtype == F32, (case.name, what, tuple(got.shape), tuple(r64.shape))
    by_trip(case, what, got, r32, r64)
    scale = float(r64.abs().max())
    e_got, e_ref = float((got.double() - r64).abs().max()), float((r32.double() - r64).abs().max())
    assert bool(torch.isfinite(got).all()) and e_got <= 2.0 * e_ref + floor * scale, (case.name, what, e_got, e_ref, scale)


def one_float_past(x):
    """x copied to an address one float past a 16-byte boundary (test_conv1x1_fused_kernel_unaligned_input)"""
    big = torch.empty(x.numel() + 4, device=x.device, dtype=x.dtype)
    at = 1 + (-(big.data_ptr() // 4)) % 4
    xo = big[at:at + x.numel()].view(x.shape)
    xo.copy_(x)
    assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
    return xo


@pytest.mark.parametrize("which", ["dma", "dma_odd", "regs", "regs_rows"])
def test_conv1x1(hip, which):
    """csrc/conv1x1.hip past its cap of 256 passes, in both staging variants with one and three k-steps.  The DMA cases
    are also run on a copy of x one float past a 16-byte boundary, which the launcher stages through registers: the two
    variants feed the same fragments to the same instructions, so the results are the same bits (and the register
    variant makes its three trips at 2 x 2 images too)."""
    from vcnf_amd.nets.cnn import pack_conv1x1
    case = gc.CASES["conv1x1.%s.f32" % which]
    t0 = time.time()
    c_in, c_out, h, w, b = case.shape["c_in"], case.shape["c_out"], case.shape["H"], case.shape["W"], case.B
    g = seeded("grid caps conv1x1", which)
    wgt = (torch.randn(c_out, c_in, generator=g) / c_in ** 0.5).cuda()
    b_in, b_out = torch.randn(c_in, generator=g).cuda(), torch.randn(c_out, generator=g).cuda()
    x = torch.randn(b, c_in, h, w, generator=g).cuda()
    pack = pack_conv1x1(wgt)
    # the launcher's choice: buffer_load ... lds for 16-byte aligned x with H W % 4 == 0, registers otherwise
    assert x.data_ptr() % 16 == 0 and ((h * w) % 4 == 0) == case.shape["dma"]
    call = lambda xs: (_lib.conv1x1_fused(xs, pack, c_out, in_bias=b_in, out_bias=b_out, in_slope=SLOPES[0], out_slope=SLOPES[1]),)
    (got,) = call(x)
    lrelu = torch.nn.functional.leaky_relu

    def ref(dt):
        t = lrelu(x.to(dt) + b_in.to(dt).view(1, -1, 1, 1), SLOPES[0])
        return lrelu(torch.einsum("oc,bchw->bohw", wgt.to(dt), t) + b_out.to(dt).view(1, -1, 1, 1), SLOPES[1])
    accept_matrix(case, "y", got, ref(F32), ref(F64), 2e-6)
    rows_again(case, call, [(x, 0)], [(got, 0)])
    if case.shape["dma"]:
        assert torch.equal(call(one_float_past(x))[0], got), "register staging and DMA staging differ"
    assert nf.check_saturation() == 0
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


def conv31_weights(c_in, c_out, g):
    """w1, w2, w3, b1, b2, b3 as test_conv3x3_1x1_fused_kernel and test_convnet3_fused_taps_and_col2im draw them"""
    w1 = (torch.randn(256, c_in, 3, 3, generator=g) / (3.0 * c_in ** 0.5)).cuda()
    w2 = (torch.randn(256, 256, generator=g) / 16).cuda()
    w3 = (torch.randn(c_out, 256, 3, 3, generator=g) / 48).cuda()
    return (w1, w2, w3) + tuple(torch.randn(n, generator=g).cuda() for n in (256, 256, c_out))


def conv31_packs(w1, w2, w3, c_in, c_out):
    from vcnf_amd.nets.cnn import pack_conv1x1
    k1 = 9 * c_in
    p1 = pack_conv1x1(torch.nn.functional.pad(w1.reshape(256, k1), (0, (-k1) % 16)))
    p3 = pack_conv1x1(w3.permute(2, 3, 0, 1).reshape(9 * c_out, 256), row_blocks=(9 * c_out + 31) // 32)
    return p1, pack_conv1x1(w2), p3


def conv3x3_ref(x, w, b):
    """torch.nn.functional.conv2d(x, w, b, padding=1) composed of nine matrix products, one per tap, over the shifted
    zero-padded image, in the dtype of x.  The convolution library searches its kernels for seconds at every new shape
    and type (measured at these shapes in fp32: 5.2 s for c_in 2 -> 256, 2.7 s for 256 -> 5); in fp64 on the host this sum and conv2d
    differ by 4e-15 at entries of size 10."""
    h, wd = x.shape[2:]
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    out = b.view(1, -1, 1, 1).expand(len(x), -1, h, wd).clone()
    for dy in range(3):
        for dx in range(3):
            out += torch.einsum("oc,bchw->bohw", w[:, :, dy, dx], xp[:, :, dy:dy + h, dx:dx + wd])
    return out


def test_conv3x3_1x1(hip):
    """csrc/conv3x3_1x1.hip (THIRD = false) past its cap: 2 x 3 images, every pixel on a border, every pass of 64
    pixels across image boundaries."""
    Fn = torch.nn.functional
    case = gc.CASES["conv3x3_1x1.f32"]
    t0 = time.time()
    c_in, h, w, b = case.shape["c_in"], case.shape["H"], case.shape["W"], case.B
    g = seeded("grid caps conv3x3_1x1")
    w1, w2, w3, b1, b2, _ = conv31_weights(c_in, 1, g)
    p1, p2, _ = conv31_packs(w1, w2, w3, c_in, 1)
    x = torch.randn(b, c_in, h, w, generator=g).cuda()
    call = lambda xs: (_lib.conv3x3_1x1_fused(xs, p1, p2, b1, b2, *SLOPES),)
    (got,) = call(x)

    def ref(dt):
        t = Fn.leaky_relu(conv3x3_ref(x.to(dt), w1.to(dt), b1.to(dt)), SLOPES[0])
        return Fn.leaky_relu(torch.einsum("oc,bchw->bohw", w2.to(dt), t) + b2.to(dt).view(1, -1, 1, 1), SLOPES[1])
    accept_matrix(case, "y", got, ref(F32), ref(F64), 2e-6)
    rows_again(case, call, [(x, 0)], [(got, 0)])
    assert nf.check_saturation() == 0
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


def test_convnet3(hip):
    """The taps instance (THIRD = true) of csrc/conv3x3_1x1.hip past its cap and the col2im that follows it: the whole
    conditioner against the fp64 composition, and the nine tap results z themselves in the windows."""
    Fn = torch.nn.functional
    case = gc.CASES["convnet3.f32"]
    t0 = time.time()
    c_in, c_out, h, w, b = case.shape["c_in"], case.shape["c_out"], case.shape["H"], case.shape["W"], case.B
    g = seeded("grid caps convnet3")
    w1, w2, w3, b1, b2, b3 = conv31_weights(c_in, c_out, g)
    p1, p2, p3 = conv31_packs(w1, w2, w3, c_in, c_out)
    x = torch.randn(b, c_in, h, w, generator=g).cuda()
    call = lambda xs: (_lib.convnet3_fused(xs, p1, p2, p3, b1, b2, b3, c_out, *SLOPES),)
    (got,) = call(x)

    def ref(dt):
        t = Fn.leaky_relu(conv3x3_ref(x.to(dt), w1.to(dt), b1.to(dt)), SLOPES[0])
        t = Fn.leaky_relu(torch.einsum("oc,bchw->bohw", w2.to(dt), t) + b2.to(dt).view(1, -1, 1, 1), SLOPES[1])
        return conv3x3_ref(t, w3.to(dt), b3.to(dt))
    accept_matrix(case, "y", got, ref(F32), ref(F64), 2e-6)
    rows_again(case, call, [(x, 0)], [(got, 0)])
    assert nf.check_saturation() == 0
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


@pytest.mark.parametrize("which", ["rows", "rows8", "image"])
def test_channel_mix(hip, which):
    """csrc/channel_mix.hip past its cap of 4096 workgroups: the ROWS instances on [B, C] matrices and the image
    instance on 1 x 3 images.  The fp32 yardstick is torch's einsum (a matrix product): a batch of a million images is
    not a shape to hand to the convolution library that test_channel_mix_kernel uses at b <= 257."""
    case = gc.CASES["mix.%s.f32" % which]
    t0 = time.time()
    c, b = case.shape["C"], case.B
    g = seeded("grid caps channel mix", which)
    mat, vec = torch.randn(c, c, generator=g).cuda(), torch.randn(c, generator=g).cuda()
    shape = (b, c) if case.shape["rows"] else (b, c, case.shape["H"], case.shape["W"])
    x = torch.randn(*shape, generator=g).cuda()
    call = lambda xs: (_lib.channel_mix(xs, mat, vec),)
    (got,) = call(x)
    assert got.data_ptr() % 16 == 0                                # what sends a [B, C] matrix to the ROWS instance
    bias = (1, c) + (1,) * (len(shape) - 2)
    ref = lambda dt: torch.einsum("oc,bc...->bo...", mat.to(dt), x.to(dt)) + vec.to(dt).view(bias)
    accept_matrix(case, "y", got, ref(F32), ref(F64), 1e-6)
    rows_again(case, call, [(x, 0)], [(got, 0)])
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


@pytest.mark.parametrize("which", ["layer", "layer_odd"])
def test_fused_affine_layer(hip, which):
    """fused_affine_layer_kernel past its cap of 2048 workgroups, as test_fused_affine_layer_vs_three_step_path_and_oracle
    builds and judges the block: both directions and the accumulate form against the oracle block in fp64 (the
    three-step path is the fp32 yardstick of the GRIDCAP lines)."""
    from oracle import layers as OL, nets as ON
    from vcnf_amd import fused_affine
    case = gc.CASES["faffine.%s.f32" % which]
    t0 = time.time()
    d, hidden, mode, sm, b = case.shape["D"], case.shape["hidden"], case.shape["mode"], case.shape["scale_map"], case.B
    torch.manual_seed(d * 7 + hidden)
    head = d - d // 2
    cin, cout = (head, d - head) if mode == "channel" else (d - head, head)
    blk = nf.flows.AffineCouplingBlock(nf.nets.MLP([cin, hidden, hidden, 2 * cout], leaky=0.1), scale=True, scale_map=sm, split_mode=mode)
    with torch.no_grad():
        blk.flows[1].param_map.net[4].weight.mul_(0.5)
    sd64 = {k: v.detach().clone().double() for k, v in blk.state_dict().items()}
    blk = blk.cuda()
    x = torch.randn(b, d, generator=seeded("grid caps fused affine layer", which))
    xg = x.cuda()
    assert fused_affine.eligible(blk, xg)
    ora = OL.AffineCouplingBlock(lambda z: ON.mlp(sd64, "flows.1.param_map.", z, 0.1), scale=True, scale_map=sm, split_mode=mode)
    tol = dict(rtol=2e-5, atol=2e-5)
    ld_tol = dict(rtol=2e-5, atol=2e-5 * max(1, cout))
    with torch.no_grad():
        for dirn in ("forward", "inverse"):
            call = lambda xs: getattr(blk, dirn)(xs)
            blk.fused = True
            z1, ld1 = call(xg)
            blk.fused = False
            z2, ld2 = call(xg)
            blk.fused = True
            want_z, want_ld = getattr(ora, dirn)(x.double())
            by_trip(case, dirn + " z", z1, z2, want_z)
            by_trip(case, dirn + " log_det", ld1, ld2, want_ld)
            assert_close(z1, want_z, what="%s z %s" % (case.name, dirn), **tol)
            assert_close(ld1, want_ld, what="%s log_det %s" % (case.name, dirn), **ld_tol)
            rows_again(case, call, [(xg, 0)], [(z1, 0), (ld1, 0)])
        # accumulate-into form used by NormalizingFlow (want_z, want_ld: the inverse direction's)
        def into(xs):
            acc = torch.full((len(xs),), 0.25, device="cuda")
            return blk.inverse_into(xs, acc), acc
        z3, lq = into(xg)
        assert torch.equal(z3, z1) and torch.allclose(lq, 0.25 + ld1, rtol=1e-6, atol=1e-6)
        by_trip(case, "inverse_into log_q", lq, 0.25 + ld2, 0.25 + want_ld)
        assert_close(lq, 0.25 + want_ld, what="%s inverse_into log_q" % case.name, **ld_tol)
        rows_again(case, into, [(xg, 0)], [(z3, 0), (lq, 0)])
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_fused_affine_stack(hip, precision):
    """fused_affine_stack_kernel past its cap in both forms, on config C1's stack (D = 2, MLP [1, 32, 32, 2], four
    [coupling, swap] pairs): density and sampling passes against helpers.oracle_affine_stack in fp64 with the tolerances
    of test_affine_stacks_c1_c2.  test_c2_full_size_round_trip crosses the cap too, but compares the kernel with itself.
    The weights are torch's default initialisation, as test_affine_stack_split_half_matrix_path draws them for this
    stack.  The golden fixture's weights (g10_c1_two_moons, final layer x 6) suit its own 64 rows only: among 262 177
    standard-normal rows the fp64 oracle itself samples |z| up to 9e111 with them (measured), where no fp32 result
    exists.  The per-layer path is the fp32 yardstick of the GRIDCAP lines."""
    from helpers import oracle_affine_stack
    from test_gpu_parity import LP, TOL
    from vcnf_amd import fused_affine
    case = gc.CASES["faffine.stack.f32"]
    t0 = time.time()
    d, widths, layers, b = case.shape["D"], list(case.shape["widths"]), case.shape["layers"], case.B
    torch.manual_seed(77 + d)
    flows = []
    for _ in range(layers):
        flows += [nf.flows.AffineCouplingBlock(nf.nets.MLP(widths, init_zeros=False)), nf.flows.Permute(d, mode="swap")]
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(d), flows)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.cuda().eval()
    for f in model.flows:
        f.fused_precision = precision
    g = seeded("grid caps fused affine stack")
    x, eps = torch.randn(b, d, generator=g), torch.randn(b, d, generator=g)
    xg, eg = x.cuda(), eps.cuda()
    with torch.no_grad():                                          # as the passes below: no autograd, so the blocks are fusable
        plan = fused_affine.plan_stack(list(model.flows), 0, xg, False)
    assert plan is not None and len(plan[1]) == layers and model.fuse_affine_stacks      # one launch for the four blocks
    assert fused_affine.h3_ok(model.flows[0]) == (precision == "fp16x3")
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    oracle = oracle_affine_stack(sd64, layers, d)
    want_lp = oracle.log_prob(x.double())
    want_z, want_lq = oracle.sample_from(eps.double())
    density = lambda xs: (model.log_prob(xs),)
    sampling = lambda es: tuple(model.sample_from(es))
    nf.range_redo_count()
    with torch.no_grad():
        (lp,), (z, lq) = density(xg), sampling(eg)
        model.fuse_affine_stacks = False
        (lp0,), (z0, lq0) = density(xg), sampling(eg)
        model.fuse_affine_stacks = True
        assert all(bool(torch.isfinite(t).all()) for t in (want_lp, want_z, want_lq))
        by_trip(case, precision + " log_prob", lp, lp0, want_lp)
        by_trip(case, precision + " sample z", z, z0, want_z)
        by_trip(case, precision + " sample log_q", lq, lq0, want_lq)
        assert_close(lp, want_lp, what="%s log_prob" % precision, **LP)
        assert_close(z, want_z, what="%s sample z" % precision, **TOL)
        assert_close(lq, want_lq, what="%s sample log_q" % precision, **LP)
        rows_again(case, density, [(xg, 0)], [(lp, 0)])
        rows_again(case, sampling, [(eg, 0)], [(z, 0), (lq, 0)])
    assert nf.range_redo_count() == 0, "a wave took the fp32 fallback: the rows are no longer independent of their tile"
    print("GRIDCAP %-34s wall %.2f s" % (case.name, time.time() - t0))

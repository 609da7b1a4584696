"""What a single-launch family is: the contract between ``NormalizingFlow`` and the host modules that evaluate a run of
consecutive layers in ONE kernel launch (fused_affine, fused_masked, fused (RQS), fused_planar, fused_stochastic), and the
pieces every family states the same way.  A new family is a module with the planner below and a row in
``vcnf_amd.core._STACKS`` (which also fixes the order in which families are tried); this module imports none of them.

The planner
    ``stack_run(owner, order, start, z, context, density)`` -> ``None`` or ``(end, launch)``.
    ``order`` is the pass's list of flows (the model's, reversed in a density pass), ``start`` the position the pass is at,
    ``z`` the inputs as they arrive there.  ``None``: no run starts here, the pass goes on to its other forms.  Otherwise
    the run is ``order[start:end]`` and the pass continues at ``end``.  The planner launches nothing.

The launch
    ``launch(z, log_q, sign)`` -> ``(z', log_q')`` with ``log_q' = log_q + sign * log|det|`` of the run (``sign``: 1.0 in
    a density pass, -1.0 when sampling).  Given a ``log_q`` the kernel adds into it and returns that tensor; the caller
    uses what is returned.  A family whose run is one autograd node returns a NEW ``log_q'`` whenever autograd records
    the run and leaves the given tensor as it was; without a ``log_q`` it returns ``sign * log|det|`` alone
    (``add_log_det``).  Setting ``stack_run.differentiable = True`` offers such a family to the plain walk as well, the
    one reverse_kld trains through: it sums out of place, passes ``log_q=None`` and takes the runs of these families only.

Plans
    Finding a run costs more than the launch it saves at small batches, so planners memoise on ``owner`` through
    ``memo_plan``: the key holds what is not a property of a module (position, direction, shape and dtype of the inputs),
    the stamp what a module contributes besides its identity (routing switches, sub-module identities).  A plan is
    dropped when a module it has seen was replaced or its stamp changed.

Run caches
    What a launch needs besides the plan (tables of addresses, concatenated packs, descriptors) lives on the run's first
    module in the dict ``run_cache`` returns, emptied when the run's modules are no longer the ones it was filled for.
    Weights a run packs or concatenates are derived buffers: slots of ``vcnf_amd.derived`` (keyed, rewritten in place -
    the contract is that module's docstring), not entries of the run cache.

Plan memos and run caches live in the containers of ``vcnf_amd.derived``, whose ``refresh_packed`` empties them along
with every derived buffer's key after parameters changed behind autograd's back.
"""
from .derived import plans as _plans, refresh_packed, runs as _runs           # noqa: F401  (refresh_packed stays importable from here)


def memo_plan(owner, attr, key, order, start, make, stamp, seen=None):
    """``make()`` - a run plan (end, ...) or None - memoised on ``owner`` in the plan memo ``attr`` under ``key``.  An entry is
    reused while the modules the plan has seen - the run and the flow that ended it, narrowed by ``seen`` - are the
    same objects at the same positions of ``order`` with the same ``stamp``."""
    plans = _plans(owner, attr)
    hit = plans.get(key)
    if hit is not None:
        plan, mods, stamps = hit
        if all(a is b for a, b in zip(order[start:start + len(mods)], mods)) and stamps == tuple(map(stamp, mods)):
            return plan
    plan = make()
    mods = order[start:(start if plan is None else plan[0]) + 1]
    if seen is not None:
        mods = seen(mods)
    if len(plans) > 64:
        plans.clear()
    plans[key] = (plan, mods, tuple(map(stamp, mods)))
    return plan


def run_cache(first, name, ids):
    """The run cache ``name`` on ``first`` of a run whose identity is ``ids``, emptied (but for ``'ids'``) when it was
    filled for another run."""
    cache = _runs(first, name)
    if cache.get('ids') != ids:
        cache.clear()
        cache['ids'] = ids
    return cache


def add_log_det(out, log_det, log_q, sign):
    """(out, log_q + sign * log_det) with the sum taken OUT of place, or (out, sign * log_det) without a log_q: the
    epilogue of a run that autograd records (``vcnf_amd.flows.base.fold_log_det`` is the in-place form)."""
    if log_q is not None:
        return out, log_q + sign * log_det
    return out, (log_det if sign == 1.0 else sign * log_det)

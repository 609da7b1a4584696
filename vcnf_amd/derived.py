"""What a derived buffer is: a tensor (or tuple of tensors) computed from a module's parameters that a kernel reads in
their place - packed conditioner weights, a composed channel map, an int32 copy of an index buffer - and the one body
of the idiom every such site uses.  A site states a key and a builder; where the result lives, when it is rebuilt,
how it is rebuilt and what forgets it are stated here.  This module imports no family and names none.

Keys
    A key holds everything the builder reads that can change while the owner lives: ``tensor_key`` of the source
    tensors - (data_ptr, _version, device) each, so a re-assigned Parameter, an optimiser step, a ``.to()`` all change
    it - plus whatever else selects the result (direction, precision, the ids of a run's modules).  A key is a tuple,
    never None: None is what a forgotten key looks like.  The caller computes the key (a hot caller computes it once
    and uses it for several slots); the helpers only compare it.

Slots: ``packed(owner, slot, key, make)``
    ONE buffer per (owner, slot), valid while ``key`` equals the key of the last build that succeeded.  ``make(owner)``
    runs under ``torch.no_grad()`` (pass a module-level function, not a closure, on a path that is called per layer
    and evaluation).  The in-place rule: a rebuild whose result has the old one's shapes, dtypes and devices, member by
    member (None matching None), is COPIED INTO the old tensors and those are returned; any other result replaces
    them.  Why: a captured HIP graph (vcnf_amd.graphs) and the address tables of the single-launch families hold the
    buffers' addresses - new weights must appear behind the same address.  The key is recorded after ``make`` has
    returned: a builder that raises leaves key and buffer as they were and the next call builds again.

Memos: ``memo(owner, slot, key, make, limit)``
    Derived tensors nothing holds the address of (index vectors, composed matrices), any number of keys per slot;
    the slot is emptied when it holds more than ``limit`` entries.  ``memos(owner, slot)`` is the slot's dict itself,
    for host-side state that follows the same life cycle without being a tensor (a device flag read once, the
    (module, name) places of a parameter walk).

Plans and run caches (``plans``, ``runs``) are the containers of ``vcnf_amd.stacks.memo_plan`` / ``run_cache``.

``refresh_packed``
    A write through ``.data`` (``p.data.copy_(ema)``, the reference API's initialisation idiom) changes no key.
    ``refresh_packed(module)`` forgets every slot's key - the buffers stay, so the next use rewrites them in place -
    and empties every memo, plan memo and run cache under ``module``.  NormalizingFlow / MultiscaleFlow call it on
    train() / eval() and after load_state_dict(); after a ``.data`` edit call it yourself.

Adding a derived buffer
    Call ``packed`` (address-stable) or ``memo`` with a slot name unique on the owner; keep nothing derived from
    parameters in an attribute of your own.  There is nothing to register: refresh_packed and the GPU sweep of
    tests/test_gpu_derived.py (no module attribute outside these containers may hold a device tensor) find it.
"""
import torch

SLOTS, MEMOS, PLANS, RUNS = '_derived_slots', '_derived_memos', '_derived_plans', '_derived_runs'
CONTAINERS = (SLOTS, MEMOS, PLANS, RUNS)


def tensor_key(tensors, device=True):
    """(data_ptr, _version, device) of each tensor, None for a None.  ``device=False`` leaves the device out, for a key
    that is computed on every evaluation over many tensors and states their device once itself (or never did: the
    run keys)."""
    if device:
        return tuple([None if t is None else (t.data_ptr(), t._version, t.device) for t in tensors])
    return tuple([None if t is None else (t.data_ptr(), t._version) for t in tensors])


def _members(buf):
    return buf if isinstance(buf, tuple) else (buf,)


def _same_layout(old, new):
    if isinstance(old, tuple) != isinstance(new, tuple):
        return False
    old, new = _members(old), _members(new)
    return len(old) == len(new) and all(
        (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and a.dtype == b.dtype
                                      and a.device == b.device) for a, b in zip(old, new))


def packed(owner, slot, key, make):
    """The buffer ``make(owner)`` derives, kept on ``owner`` under ``slot`` while ``key`` is the last built key and
    rewritten in place when a rebuild has the same layout (the contract: this module's docstring)."""
    slots = owner.__dict__.get(SLOTS)
    if slots is None:
        slots = owner.__dict__[SLOTS] = {}
    kept = slots.get(slot)
    if kept is not None and kept[0] == key:
        return kept[1]
    with torch.no_grad():
        buf = make(owner)
        if kept is not None and _same_layout(kept[1], buf):
            for old, new in zip(_members(kept[1]), _members(buf)):
                if old is not None:
                    old.copy_(new)
            buf = kept[1]
    slots[slot] = [key, buf]
    return buf


def _container(owner, name, slot):
    outer = owner.__dict__.get(name)
    if outer is None:
        outer = owner.__dict__[name] = {}
    inner = outer.get(slot)
    if inner is None:
        inner = outer[slot] = {}
    return inner


def memos(owner, slot):
    """The dict of memo ``slot`` on ``owner``."""
    return _container(owner, MEMOS, slot)


def plans(owner, name):
    """The dict of plan memo ``name`` on ``owner`` (vcnf_amd.stacks.memo_plan)."""
    return _container(owner, PLANS, name)


def runs(owner, name):
    """The dict of run cache ``name`` on ``owner`` (vcnf_amd.stacks.run_cache)."""
    return _container(owner, RUNS, name)


def memo(owner, slot, key, make, limit):
    """``make(owner)`` (under no_grad) memoised on ``owner`` under (slot, key); the slot is emptied above ``limit``
    entries.  A None result is not remembered."""
    try:
        kept = owner.__dict__[MEMOS][slot]
    except KeyError:
        kept = memos(owner, slot)
    hit = kept.get(key)
    if hit is None:
        with torch.no_grad():
            hit = make(owner)
        if len(kept) > limit:
            kept.clear()
        kept[key] = hit
    return hit


def buffers(module):
    """(owner, slot, tensor) of every tensor in every slot under ``module``."""
    for m in module.modules():
        for slot, (_, buf) in m.__dict__.get(SLOTS, {}).items():
            for t in _members(buf):
                if t is not None:
                    yield m, slot, t


def refresh_packed(module):
    """Forget every slot's key (the buffers stay and are rewritten in place at the next use, so a captured HIP graph
    keeps its addresses) and empty every memo, plan memo and run cache under ``module``: what a change of parameters
    behind autograd's back (``.data``, load_state_dict, train() / eval()) needs."""
    for m in module.modules():
        d = m.__dict__
        for kept in d.get(SLOTS, {}).values():
            kept[0] = None
        for name in (MEMOS, PLANS, RUNS):
            if name in d:
                d[name].clear()
    return module

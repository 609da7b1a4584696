"""The one body of the derived-buffer idiom (vcnf_amd.derived) on CPU tensors: the keyed in-place slot, the bounded
memo and refresh_packed, which knows containers and no names."""
import pytest
import torch

from vcnf_amd import derived, stacks


class Maker:
    """Builder that counts its calls and returns what ``result`` makes."""

    def __init__(self, result):
        self.result, self.calls = result, 0

    def __call__(self, owner):
        self.calls += 1
        return self.result()


def test_tensor_key_follows_storage_version_and_device():
    a, b = torch.zeros(3), torch.zeros(3)
    key = derived.tensor_key((a, None, b))
    assert key == ((a.data_ptr(), 0, a.device), None, (b.data_ptr(), 0, b.device))
    assert derived.tensor_key((a, None, b), device=False) == ((a.data_ptr(), 0), None, (b.data_ptr(), 0))
    assert derived.tensor_key((a, None, b)) == key
    b.add_(1)                                   # an in-place update bumps _version ...
    assert derived.tensor_key((a, None, b)) != key
    key = derived.tensor_key((a, None, b))
    b.data.add_(1)                              # ... one through .data does not: refresh_packed is for that
    assert derived.tensor_key((a, None, b)) == key


def test_packed_hit_returns_the_same_object_without_building():
    owner, make = torch.nn.Module(), Maker(lambda: torch.arange(4.))
    buf = derived.packed(owner, 's', ('k', 1), make)
    assert make.calls == 1 and torch.equal(buf, torch.arange(4.))
    assert derived.packed(owner, 's', ('k', 1), make) is buf and make.calls == 1
    other = derived.packed(owner, 't', ('k', 1), make)                 # another slot of the same owner is another buffer
    assert other is not buf and make.calls == 2


def test_packed_changed_key_builds_once_into_the_old_tensor():
    owner, value = torch.nn.Module(), [1.0]
    make = Maker(lambda: torch.full((5,), value[0]))
    buf = derived.packed(owner, 's', ('k', 1), make)
    addr = buf.data_ptr()
    value[0] = 2.0
    again = derived.packed(owner, 's', ('k', 2), make)
    assert make.calls == 2
    assert again is buf and again.data_ptr() == addr and torch.equal(buf, torch.full((5,), 2.0))
    assert derived.packed(owner, 's', ('k', 2), make) is buf and make.calls == 2
    assert not buf.requires_grad


def test_packed_builds_under_no_grad():
    owner, w = torch.nn.Module(), torch.nn.Parameter(torch.ones(3))
    with torch.enable_grad():
        buf = derived.packed(owner, 's', ('k',), lambda _: w * 2)
    assert buf.grad_fn is None and not buf.requires_grad


@pytest.mark.parametrize("other", [lambda: torch.zeros(6), lambda: torch.zeros(5, dtype=torch.float64),
                                   lambda: torch.zeros(5, device="meta"), lambda: (torch.zeros(5),)],
                         ids=["shape", "dtype", "device", "tuple"])
def test_packed_another_layout_replaces_the_tensors(other):
    owner = torch.nn.Module()
    buf = derived.packed(owner, 's', ('k', 1), lambda _: torch.zeros(5))
    new = derived.packed(owner, 's', ('k', 2), lambda _: other())
    assert new is not buf
    assert derived.packed(owner, 's', ('k', 2), None) is new           # a hit: the builder is not looked at
    assert torch.equal(buf, torch.zeros(5))                             # the old tensor was not written


def test_packed_tuple_with_a_none_member():
    owner, value = torch.nn.Module(), [1.0]
    make = Maker(lambda: (torch.full((2, 2), value[0]), None, torch.tensor(value[0])))
    buf = derived.packed(owner, 's', ('k', 1), make)
    assert buf[1] is None and [t is None for t in buf] == [False, True, False]
    addrs = [buf[0].data_ptr(), buf[2].data_ptr()]
    value[0] = 3.0
    again = derived.packed(owner, 's', ('k', 2), make)
    assert again is buf and [buf[0].data_ptr(), buf[2].data_ptr()] == addrs
    assert torch.equal(buf[0], torch.full((2, 2), 3.0)) and float(buf[2]) == 3.0
    # a member appears where there was None: the whole result replaces the old one
    new = derived.packed(owner, 's', ('k', 3), lambda _: (torch.zeros(2, 2), torch.zeros(1), torch.tensor(0.)))
    assert new is not buf and new[1] is not None
    assert [(m, s) for m, s, _ in derived.buffers(owner)] == [(owner, 's')] * 3


def test_packed_raising_builder_leaves_key_and_buffer():
    owner = torch.nn.Module()
    buf = derived.packed(owner, 's', ('k', 1), lambda _: torch.ones(3))

    def fail(_):
        raise RuntimeError("out of memory")
    for _ in range(2):                                                  # ... and the next call tries again
        with pytest.raises(RuntimeError):
            derived.packed(owner, 's', ('k', 2), fail)
        assert owner.__dict__[derived.SLOTS]['s'][0] == ('k', 1) and owner.__dict__[derived.SLOTS]['s'][1] is buf
        assert torch.equal(buf, torch.ones(3))
    assert derived.packed(owner, 's', ('k', 1), fail) is buf            # the old key is still the current one
    make = Maker(lambda: torch.zeros(3))
    assert derived.packed(owner, 's', ('k', 2), make) is buf and make.calls == 1 and torch.equal(buf, torch.zeros(3))
    with pytest.raises(RuntimeError):                                   # a first build that raises leaves no slot
        derived.packed(owner, 'new', ('k',), fail)
    assert 'new' not in owner.__dict__[derived.SLOTS]


def test_memo_keeps_entries_up_to_its_limit_then_clears():
    owner, make = torch.nn.Module(), Maker(lambda: torch.zeros(1))
    got = [derived.memo(owner, 'm', (i,), make, 2) for i in range(3)]
    assert make.calls == 3 and len(derived.memos(owner, 'm')) == 3     # the present policy: cleared when ABOVE the limit
    assert all(derived.memo(owner, 'm', (i,), make, 2) is got[i] for i in range(3)) and make.calls == 3
    derived.memo(owner, 'm', (3,), make, 2)
    assert make.calls == 4 and list(derived.memos(owner, 'm')) == [(3,)]
    assert derived.memo(owner, 'm', (0,), make, 2) is not got[0] and make.calls == 5
    assert derived.memos(owner, 'other') == {}                          # slots do not share entries


def test_memo_builds_under_no_grad():
    owner, w = torch.nn.Module(), torch.nn.Parameter(torch.ones(3))
    with torch.enable_grad():
        assert derived.memo(owner, 'm', ('k',), lambda _: w * 2, 4).grad_fn is None


def test_refresh_packed_forgets_keys_keeps_buffers_and_empties_the_rest():
    root = torch.nn.Sequential(torch.nn.Linear(2, 2), torch.nn.Sequential(torch.nn.Linear(2, 2)))
    owners = list(root.modules())
    bufs = {}
    for i, m in enumerate(owners):
        bufs[id(m), 'a'] = derived.packed(m, 'a', ('k',), lambda _: torch.zeros(2))
        bufs[id(m), 'b'] = derived.packed(m, 'b', ('k',), lambda _: (torch.zeros(2), None))
        derived.memo(m, 'm', ('k',), lambda _: torch.zeros(1), 4)
        stacks.memo_plan(m, 'plans', ('k',), owners, i, lambda: None, lambda f: None)
        stacks.run_cache(m, 'run', (id(m),))['table'] = torch.zeros(1)
    assert derived.refresh_packed(root) is root
    for m in owners:
        for slot in ('a', 'b'):
            make = Maker(lambda: torch.ones(2) if slot == 'a' else (torch.ones(2), None))
            key, buf = m.__dict__[derived.SLOTS][slot]
            assert key is None and buf is bufs[id(m), slot]
            assert derived.packed(m, slot, ('k',), make) is buf and make.calls == 1      # same key as before: built again
            assert torch.equal(derived._members(buf)[0], torch.ones(2))
        assert not m.__dict__[derived.MEMOS] and not m.__dict__[derived.PLANS] and not m.__dict__[derived.RUNS]
    assert [t.data_ptr() for _, _, t in derived.buffers(root)] == [t.data_ptr() for b in bufs.values()
                                                                  for t in derived._members(b) if t is not None]

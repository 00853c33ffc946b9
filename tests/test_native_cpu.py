"""The one owner of native objects (iris_amd._lib.Native) and the one staleness key (iris_amd._lib.tensor_key), without a GPU and without libiris_hip.so:
the owner is driven with a counting Python destroy function, the key with CPU tensors."""
import copy
import pickle

import torch
import torch.nn as nn

from iris_amd import _lib as L


class _Counter:
    def __init__(self):
        self.freed = []

    def __call__(self, p):
        self.freed.append(p)


def test_free_twice_destroys_once():
    c = _Counter()
    n = L.Native(1234, c, 0)
    assert n.ptr == 1234 and n.device == 0
    n.free(); n.free()
    assert c.freed == [1234] and n.ptr is None
    del n
    assert c.freed == [1234]
    L.Native().free()                               # an empty owner has nothing to destroy (and no destroy function to call)


def test_del_destroys_once():
    c = _Counter()
    n = L.Native(77, c, 3)
    del n
    assert c.freed == [77]


def test_copies_are_empty_owners():
    c = _Counter()
    n = L.Native(55, c, 1, (L.tensor_key(torch.zeros(2)),))
    for other in (copy.copy(n), copy.deepcopy(n), pickle.loads(pickle.dumps(n))):
        assert type(other) is L.Native and other.ptr is None and other.keys == []
        other.free()
        del other
    assert c.freed == [] and n.ptr == 55
    del n
    assert c.freed == [55]


def test_a_module_copy_has_an_empty_owner_and_a_shallow_copy_shares_the_one_owner():
    c = _Counter()
    m = nn.Linear(2, 2)
    m._native = L.Native(9, c, 0, (L.tensor_key(m.weight),))
    for other in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert other._native.ptr is None and other._native.keys == []
        del other
    s = copy.copy(m)
    assert s._native is m._native                   # shares the tensors and with them the one owner: nothing to free twice
    del s
    assert c.freed == []
    del m
    assert c.freed == [9]


def test_a_raising_destroy_does_not_leave_del():
    def boom(p):
        raise RuntimeError("the library is gone")
    n = L.Native(5, boom, 0)
    n.__del__()                                     # (called directly: an exception that left it would surface here)
    assert n.ptr is None
    seen = []
    import sys
    old, sys.unraisablehook = sys.unraisablehook, lambda u: seen.append(u)
    try:
        n = L.Native(6, boom, 0)
        del n
    finally:
        sys.unraisablehook = old
    assert seen == []


def test_scene_refuses_to_be_copied():
    import pytest
    from iris_amd.utils.path_tracing import Scene
    sc = Scene.__new__(Scene)                       # (no library here: the refusal needs no native object)
    for f in (copy.copy, copy.deepcopy, pickle.dumps):
        with pytest.raises(L.IrisError, match="cannot be copied"):
            f(sc)


# ---- tensor_key ---------------------------------------------------------------------------------------
def test_untouched_tensor_is_fresh():
    t = torch.arange(6.0)
    k = L.tensor_key(t)
    assert k.fresh(t) and k.fresh(t)
    assert not L.tensor_key().fresh(t)              # the empty key matches nothing


def test_in_place_write_is_stale():
    t = torch.arange(6.0)
    k = L.tensor_key(t)
    t.add_(1)
    assert not k.fresh(t)


def test_rebinding_is_stale():
    m = nn.Module()
    m.register_buffer("radiance", torch.ones(4, 3))
    k = L.tensor_key(m.radiance)
    for _ in range(6):                              # freed addresses come back and versions restart at 0: the key holds the object it was made from
        m.radiance = m.radiance / 2.0
        assert not k.fresh(m.radiance)
        k = L.tensor_key(m.radiance)
        assert k.fresh(m.radiance)


def test_data_swap_on_a_parameter_is_stale():
    p = nn.Parameter(torch.zeros(8))
    k = L.tensor_key(p)
    v = p._version
    p.data = torch.ones(8)
    assert p._version == v                          # the swap keeps the object and its version: only data_ptr() tells
    assert not k.fresh(p)


def test_module_to_is_stale():
    m = nn.Linear(3, 2)
    p = m.weight
    k = L.tensor_key(p)
    m.to(torch.float64)
    assert m.weight is p and not k.fresh(m.weight)


class _Holder:
    pass


def test_a_copied_holder_does_not_carry_the_key():
    h = _Holder()
    t = torch.arange(4.0)
    h.t, h.key = t, L.tensor_key(t)
    for other in (copy.deepcopy(h), pickle.loads(pickle.dumps(h))):
        assert other.key.t is None and not other.key.fresh(other.t) and not other.key.fresh(t)
    assert copy.copy(h.key).t is None
    assert h.key.fresh(t)

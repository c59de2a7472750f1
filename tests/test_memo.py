"""bodyfitting_amd/_memo.py, the one statement of "seen before" behind the torch drop-ins' memos: a stamp answers "still this?" by
identity, liveness and `_version` - never by contents, never by an `id` alone - an array by a digest of bytes, shape and dtype, and
a table - a plain dict - keeps `slots` entries, oldest first, closing exactly what it drops.  No GPU, no library, no torch."""
import gc

import numpy as np

from bodyfitting_amd import _memo


class _Tensor:
    """what the memo reads of a tensor: identity and `_version`"""

    def __init__(self, version=0):
        self._version = version


class _Untouchable:
    """a tensor whose every attribute but `_version` raises: a hit must not look at anything else"""
    _version = 3

    def __getattr__(self, name):
        raise AssertionError(f"the memo read .{name}")

    def __eq__(self, other):
        raise AssertionError("the memo compared contents")

    __hash__ = object.__hash__


def _key_of(*objects):
    seen = []
    return tuple(_memo.part(x, seen) for x in objects), seen


# ---- weak stamps ------------------------------------------------------------------------------------------------------------

def _value(entry):
    return None if entry is None else entry["value"]


def _find(table, key, objects=()):
    return _value(_memo.find(table, key, objects))


def _store(table, key, objects, value, slots=4, **kw):
    return _memo.store(table, slots, key, objects, {"value": value}, **kw)


def test_a_weak_stamp_misses_once_its_object_is_gone_whoever_has_its_id_now():
    table = {}
    old = _Tensor()
    key, seen = _key_of(old)
    _store(table, key, seen, "built from old")
    stamp = _memo.Stamp(old)
    ident = id(old)
    assert _find(table, key, seen) == "built from old" and stamp.still(old)
    del old, seen
    gc.collect()
    keep, reused = [], None
    for _ in range(10000):                                   # CPython hands a freed block out again: a new object with the old id
        t = _Tensor()
        if id(t) == ident:
            reused = t
            break
        keep.append(t)
    if reused is not None:
        new_key, new_seen = _key_of(reused)
        assert new_key == key                                # the id alone says "seen before" ...
        assert _memo.find(table, new_key, new_seen) is None  # ... the stamp does not
        assert not stamp.still(reused) and not stamp.still(reused, any_version=True)
    else:                                                    # no reuse in 10,000 tries: the same key, forged
        other = _Tensor()
        assert _memo.find(table, (("tensor", ident),), [other]) is None
        assert not stamp.still(other) and not stamp.still(other, any_version=True)


# ---- held stamps ------------------------------------------------------------------------------------------------------------

def test_a_held_stamp_keeps_its_object_alive_and_no_other_object_hits_its_entry():
    table = {}
    held = _Tensor()
    key, seen = _key_of(held)
    _store(table, key, seen, "built from held", hold=True)
    ident = id(held)
    del held, seen
    gc.collect()
    entry = next(iter(table.values()))
    assert id(entry.stamps[0].held) == ident                 # alive: the id in the key cannot be handed out again
    for _ in range(1000):
        t = _Tensor()
        assert id(t) != ident
        assert _memo.find(table, key, [t]) is None           # not even under the held object's own key
    assert _find(table, key, [entry.stamps[0].held]) == "built from held"
    # a weak stamp does not keep its object
    weak = _memo.Stamp(_Tensor())
    gc.collect()
    assert weak.held is None and weak._ref() is None


def test_hold_is_chosen_per_object():
    table = {}
    a, b = _Tensor(), _Tensor()
    _store(table, "k", [a, b], "v", hold=[False, True])
    stamps = table["k"].stamps
    assert stamps[0].held is None and stamps[1].held is b and _find(table, "k", [a, b]) == "v"


def test_many_held_objects_are_checked_the_same_way():
    """more than four objects, all held, take the look-up's loop-free branch: the same answers"""
    table = {}
    objects = [_Tensor() for _ in range(6)]
    key, seen = _key_of(*objects)
    _store(table, key, seen, "set", hold=True)
    assert table[key].held is not None and _find(table, key, objects) == "set"
    for i in range(6):
        swapped = list(objects)
        swapped[i] = _Tensor()
        assert _memo.find(table, key, swapped) is None
        objects[i]._version += 1
        assert _memo.find(table, key, objects) is None
        objects[i]._version -= 1
    assert _memo.find(table, key, objects[:5]) is None and _find(table, key, objects) == "set"
    assert _memo.find(table, key, objects[:5] + [np.zeros(3)]) is None


# ---- versions ---------------------------------------------------------------------------------------------------------------

def test_a_version_bump_misses():
    table = {}
    t = _Tensor()
    key, seen = _key_of(t)
    _store(table, key, seen, "v0")
    stamp = _memo.Stamp(t)
    t._version += 1                                          # an in-place edit
    assert _memo.find(table, *_key_of(t)) is None and not stamp.still(t)
    assert stamp.still(t, any_version=True)                         # (what tells "edited in place" from "another object")
    _store(table, key, seen, "v1")                           # the stale entry is replaced under its own key
    assert _find(table, key, seen) == "v1" and len(table) == 1


def test_the_same_object_at_the_same_version_hits_without_a_look_at_its_contents():
    t = _Untouchable()
    for hold in (False, True):
        table = {}
        key, seen = _key_of(t)
        _store(table, key, seen, "built", hold=hold)
        assert _find(table, *_key_of(t)) == "built"
        stamp = _memo.Stamp(t, hold=hold)
        assert stamp.still(t) and stamp.still(t, any_version=True) and stamp.version == 3
        assert not stamp.still(_Untouchable()) and _memo.find(table, key, [_Untouchable()]) is None


# ---- array digests ----------------------------------------------------------------------------------------------------------

def test_array_digests_tell_shape_and_dtype_apart_and_know_a_copy():
    a = np.arange(24, dtype=np.int32).reshape(4, 6)
    assert a.tobytes() == a.reshape(6, 4).tobytes() == a.view(np.float32).tobytes()
    assert _memo.digest(a) != _memo.digest(a.reshape(6, 4))                  # equal bytes, another shape
    assert _memo.digest(a) != _memo.digest(a.view(np.float32))               # equal bytes, another dtype
    assert _memo.digest(a) != _memo.digest(a.view(np.uint32))
    assert _memo.digest(a) == _memo.digest(a.copy()) == _memo.digest(np.asfortranarray(a))
    seen = []
    assert _memo.part(a, seen) == _memo.part(a.copy(), seen) == ("array", _memo.digest(a)) and seen == []
    stamp = _memo.Stamp(a)
    assert stamp.still(a.copy()) and not stamp.still(a.reshape(6, 4)) and not stamp.still(a + 1)
    assert not stamp.still(_Tensor()) and not stamp.still(_Tensor(), any_version=True)          # a tensor is never an array
    assert not _memo.Stamp(_Tensor()).still(a)


def test_caller_supplied_bytes_make_int32_and_int64_faces_one_key():
    faces32 = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    faces64 = faces32.astype(np.int64)
    assert _memo.digest(faces32) != _memo.digest(faces64)
    as_int32 = [np.ascontiguousarray(f.reshape(-1, 3), dtype=np.int32).tobytes() for f in (faces32, faces64, faces64.reshape(-1))]
    parts = [_memo.part(f, [], data) for f, data in zip((faces32, faces64, faces64.reshape(-1)), as_int32)]
    assert parts[0] == parts[1] == parts[2]
    other = faces32.copy()
    other[0, 0] = 3
    assert _memo.part(other, [], other.tobytes()) != parts[0]


# ---- the table --------------------------------------------------------------------------------------------------------------

def test_the_table_keeps_its_slots_evicts_oldest_first_and_closes_exactly_what_it_drops():
    closed = []
    table = {}

    def store(key, value):
        return _store(table, key, (), value, slots=3, closed=lambda entry: closed.append(entry["value"]))

    for k in range(3):
        store(k, f"value {k}")
    assert len(table) == 3 and closed == []
    assert [_find(table, k) for k in range(3)] == ["value 0", "value 1", "value 2"]
    store(3, "value 3")                                      # the fourth evicts the first
    assert len(table) == 3 and closed == ["value 0"] and _memo.find(table, 0) is None
    _memo.find(table, 1)                                     # a look-up does not renew: the order is the stores'
    store(4, "value 4")
    assert closed == ["value 0", "value 1"] and [e["value"] for e in table.values()] == ["value 2", "value 3", "value 4"]
    store(3, "value 3 again")                                # replaced under its own key: closed once, and now the youngest
    assert closed == ["value 0", "value 1", "value 3"] and len(table) == 3
    assert [e["value"] for e in table.values()] == ["value 2", "value 4", "value 3 again"]
    for entry in table.values():                             # never on a value that is still stored
        assert entry["value"] not in closed
    _memo.drop(table, 4, lambda entry: closed.append(entry["value"]))
    _memo.drop(table, "never stored", lambda entry: closed.append(entry["value"]))
    assert closed == ["value 0", "value 1", "value 3", "value 4"] and len(table) == 2
    assert len(set(closed)) == len(closed)                   # once per dropped value
    # without a callback the table only forgets
    plain = {}
    _store(plain, "a", (), 1, slots=1)
    _store(plain, "b", (), 2, slots=1)
    assert list(plain) == ["b"] and plain["b"]["value"] == 2
    plain.clear()
    assert len(plain) == 0 and _memo.find(plain, "b") is None


def test_a_look_up_over_several_objects_misses_when_any_one_stamp_fails():
    table = {}
    objects = [_Tensor(), _Tensor(), _Tensor()]
    key, seen = _key_of(*objects)
    assert seen == objects
    _store(table, key, seen, "built")
    assert _find(table, key, objects) == "built"
    for i in range(3):
        swapped = list(objects)
        swapped[i] = _Tensor()
        assert _memo.find(table, key, swapped) is None       # another object in place i
        objects[i]._version += 1
        assert _memo.find(table, key, objects) is None       # object i edited in place
        objects[i]._version -= 1
        assert _find(table, key, objects) == "built"
    assert _memo.find(table, key, objects[:2]) is None and _memo.find(table, key, objects + [_Tensor()]) is None
    assert _memo.find(table, key, [objects[0], np.zeros(3), objects[2]]) is None    # an array where a tensor was stamped


def test_a_look_up_compares_in_order_so_equal_keys_need_seen_in_the_same_order():
    """the contract's ORDER clause: a user that canonicalises its key must collect `seen` in the canonical order too (loss._views_key
    sorts a keypoint dict's items before it calls `part`); the same objects in another order are a miss, never a wrong hit"""
    table = {}
    a, b = _Tensor(), _Tensor()
    key = tuple(sorted(_memo.part(x, []) for x in (a, b)))           # a key that does not depend on the order
    in_key_order = sorted((a, b), key=id)
    _store(table, key, in_key_order, "built")
    assert _find(table, key, in_key_order) == "built"
    assert _memo.find(table, key, in_key_order[::-1]) is None

"""The one statement of "seen before" behind the torch drop-ins' memos (the contract and the users; a new
memo is one more user).  Of a tensor only its identity and its `_version` are read, never its contents.  "Still this" means: the same
object, alive, at the same version.  An `id` alone never answers it: a stamp asks a weak reference with `is`, and with hold=True
keeps the object itself, which is what makes an `id` in a key safe for as long as the entry lives.  An array is told apart by a
digest of its bytes, shape and dtype.  A table is a plain dict, oldest entry first, that `find`, `store`, `room` and `drop` work on.
ORDER: a look-up compares its objects with the stamps one by one, so equal keys must come with `seen` in the same order - a user
that sorts its key parts calls `part` in the sorted order (loss._views_key).  Neither torch nor the library is imported here."""
from __future__ import annotations

import hashlib
import weakref
from operator import attrgetter, is_

import numpy as np

_VERSION = attrgetter("_version")


def digest(a=None, data=None):
    """sha1 of an array's contiguous bytes plus repr((shape, dtype.str)) - equal bytes under another shape or dtype differ - or of
    `data`, the bytes a caller digests instead (topology_for: its converted int32 faces, so that int32 and int64 faces are one)"""
    if data is None:
        a = np.ascontiguousarray(a)
        data = a.tobytes() + repr((a.shape, a.dtype.str)).encode()
    return hashlib.sha1(data).hexdigest()


def part(x, seen, data=None):
    """the hashable key part of `x`: anything with a `_version` by its id - it is appended to `seen`, the objects a look-up checks
    and a store stamps, since the id alone proves nothing - an array by its digest, which says all there is to say"""
    if hasattr(x, "_version"):
        seen.append(x)
        return ("tensor", id(x))
    return ("array", digest(x, data))


class Stamp:
    """one object as it was seen: its key part, its `_version` (None: an array), a weak reference and - hold=True - the object"""
    __slots__ = ("part", "version", "held", "_ref")

    def __init__(self, x, hold=False):
        seen = []
        self.part = part(x, seen)
        self.version, self.held, self._ref = (x._version, x if hold else None, weakref.ref(x)) if seen else (None, None, None)

    def still(self, x, any_version=False):
        """is `x` still this: the same object, alive, at the same version (any_version: at whatever version); an array: the same digest"""
        if self.version is None:
            return not hasattr(x, "_version") and self.part[1] == digest(x)
        return self._ref() is x and (any_version or self.version == x._version)


class Entry(dict):
    """what a table keeps under a key: the caller's fields, and the stamps of the objects the key was made from.  held: the objects
    when all of several are held (a camera set: 96 of them) - `find` then checks them without a Python-level loop"""
    __slots__ = ("stamps", "held", "versions")

    def __init__(self, fields, stamps):
        dict.__init__(self, fields)
        self.stamps, self.versions = stamps, [s.version for s in stamps]
        self.held = [s.held for s in stamps] if len(stamps) > 4 and all(s.held is not None for s in stamps) else None


def find(table, key, objects=()):
    """the entry under `key` when every one of `objects` - those `part` collected for the key, in that order - is still what `store` stamped"""
    entry = table.get(key)
    if entry is None or len(entry.stamps) != len(objects):
        return None
    if entry.held is not None:
        same = all(map(is_, entry.held, objects)) and list(map(_VERSION, objects)) == entry.versions
        return entry if same else None
    for s, x in zip(entry.stamps, objects):
        if s._ref() is not x or s.version != x._version:
            return None
    return entry


def store(table, slots, key, objects, fields, hold=False, closed=None):
    """`fields` under `key` as an Entry, `objects` stamped - hold: kept alive with it (one answer for all, or one per object).  Room
    is made from the oldest entry on; closed(entry) is called on every entry dropped, the one replaced under its key included."""
    stamps = [Stamp(x, h) for x, h in zip(objects, [hold] * len(objects) if isinstance(hold, bool) else hold)]
    room(table, slots, key, closed)
    table[key] = Entry(fields, stamps)
    return table[key]


def room(table, slots, key, closed=None):
    """what `store` does first - the entry under `key` dropped, then the oldest until one more fits - for a user that frees before it builds"""
    drop(table, key, closed)
    while len(table) >= slots:
        drop(table, next(iter(table)), closed)


def drop(table, key, closed=None):
    entry = table.pop(key, None)
    if entry is not None and closed is not None:
        closed(entry)

"""The compiled reference for the tests that compare with it call by call: live where oracle/_ref was built, else its recorded
answers (tests/golden/ref_calls/<module>.<test>.<f64|f32>.npz).

    reference(dtype)    oracle.bindings.Reference(dtype) where oracle/_ref exists; otherwise a stand-in that answers every method
                        call with what the live reference answered to the same call of the same test, and fails if the call's inputs
                        differ from the recorded ones (digest of every array and argument).  Skips where neither exists.
    reference(dtype, replay=False)   the live reference or a skip: for the tests whose subject is a committed fixture (is it
                        what the reference returns?), which a recording cannot answer.

Recording and when to record again: tests/golden/ref_calls/README.md.  A call is stored as the arrays it changed in place
(outputs written into the caller's buffers) and its return value, each array once per file however many calls return it; the
n-th call of a test is looked up by the test's id (module file name :: test name [parameters], the same from any directory
pytest starts in) and n.  Recorded answers are stored in these files only, never read from another fixture.
``apply(fn, *args)`` runs ``fn(lib, *args)`` on the raw ctypes library of the reference (helpers of golden_cases.py that call
its C ABI directly) under the same record / replay."""
import atexit
import glob
import hashlib
import json
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CALLS = os.path.join(GOLD, "ref_calls")
TAGS = {np.float64: "f64", np.float32: "f32"}


def _test_id():
    """module file name :: test name [parameters] -- without the directory, which depends on pytest's rootdir."""
    cur = os.environ.get("PYTEST_CURRENT_TEST", "?").rsplit(" (", 1)[0]
    path, sep, rest = cur.partition("::")
    return os.path.basename(path) + sep + rest


def _module(test_id):
    return os.path.splitext(os.path.basename(test_id.split("::")[0]))[0]


def _path(test_id, tag):
    """One file per test function and precision (every parametrisation of the function in it)."""
    func = test_id.split("::")[-1].split("[")[0]
    return os.path.join(CALLS, "%s.%s.%s.npz" % (_module(test_id), func, tag))


def _arrays(x, out):
    """Every ndarray among the (nested) arguments, in order."""
    if isinstance(x, np.ndarray):
        out.append(x)
    elif isinstance(x, (tuple, list)):
        for y in x:
            _arrays(y, out)
    elif isinstance(x, dict):
        for k in sorted(x):
            _arrays(x[k], out)
    return out


def _digest(name, args, kwargs):
    h = hashlib.sha1(name.encode())
    def walk(x):
        if isinstance(x, np.ndarray):
            a = np.ascontiguousarray(x)
            h.update(("%s%s" % (a.dtype.str, a.shape)).encode()); h.update(a.tobytes())
        elif isinstance(x, (tuple, list)):
            h.update(b"(")
            for y in x:
                walk(y)
            h.update(b")")
        elif isinstance(x, dict):
            for k in sorted(x):
                h.update(str(k).encode()); walk(x[k])
        elif callable(x):
            h.update(getattr(x, "__name__", "?").encode())
        else:
            h.update(repr(x.item() if isinstance(x, np.generic) else x).encode())
    walk(args); walk(kwargs)
    return h.hexdigest()


def _array_hash(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha1(("%s%s" % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def _put(a, store):
    """Descriptor of array `a`: its key in `store` (added once per content)."""
    name = "x" + _array_hash(a)[:24]
    if name not in store:
        store[name] = np.array(a, copy=True)
    return {"x": name}


def _get(desc, z):
    return z[desc["x"]].copy()


def _encode(x, store, inputs=()):
    """JSON description of a return value; an array that is one of the call's input arrays (written in place) is named by its
    position among them."""
    if isinstance(x, np.ndarray):
        same = [i for i, a in enumerate(inputs) if a is x]
        if same:
            return {"i": same[0]}
        return {"a": _put(x, store)}
    if isinstance(x, tuple):
        return {"t": [_encode(y, store, inputs) for y in x]}
    if isinstance(x, list):
        return {"l": [_encode(y, store, inputs) for y in x]}
    if isinstance(x, dict):
        return {"d": {str(k): _encode(v, store, inputs) for k, v in x.items()}}
    if isinstance(x, np.generic):
        return {"s": x.item(), "dt": x.dtype.str}
    return {"v": x}


def _decode(e, z, inputs):
    if "a" in e:
        return _get(e["a"], z)
    if "i" in e:
        return inputs[e["i"]]
    if "t" in e:
        return tuple(_decode(y, z, inputs) for y in e["t"])
    if "l" in e:
        return [_decode(y, z, inputs) for y in e["l"]]
    if "d" in e:
        return {k: _decode(v, z, inputs) for k, v in e["d"].items()}
    if "s" in e:
        return np.dtype(e["dt"]).type(e["s"])
    return e["v"]


_recorded = {}        # file -> {key: array}
_counters = {}        # (test id, precision) -> calls so far


def _next_key(dtype):
    tid = _test_id()
    c = _counters.get((tid, TAGS[dtype]), 0)
    _counters[(tid, TAGS[dtype])] = c + 1
    return tid, "%s#%d" % (hashlib.sha1(tid.encode()).hexdigest()[:20], c)


def _save_recorded():
    os.makedirs(CALLS, exist_ok=True)
    for path, store in _recorded.items():
        np.savez_compressed(path, **store)


class _Recorder:
    def __init__(self, live, dtype):
        self._live, self._dtype = live, dtype
        self.dtype = dtype
        if not _recorded:
            atexit.register(_save_recorded)

    def _record(self, name, fn, args, kwargs):
        tid, key = _next_key(self._dtype)
        digest = _digest(name, args, kwargs)
        arrs = _arrays((args, kwargs), [])
        before = [a.copy() for a in arrs]
        ret = fn()
        store = _recorded.setdefault(_path(tid, TAGS[self._dtype]), {})
        changed = [[i, _put(a, store)] for i, (a, b) in enumerate(zip(arrs, before)) if not np.array_equal(a, b, equal_nan=True)]
        meta = {"name": name, "digest": digest, "changed": changed, "ret": _encode(ret, store, arrs)}
        store[key] = np.array(json.dumps(meta))
        return ret

    def apply(self, fn, *args):
        return self._record(fn.__name__, lambda: fn(self._live.lib, *args), args, {})

    def __getattr__(self, name):
        attr = getattr(self._live, name)
        if not callable(attr) or name.startswith("_"):
            return attr
        return lambda *a, **kw: self._record(name, lambda: attr(*a, **kw), a, kw)


class _Replay:
    def __init__(self, dtype):
        self.dtype = dtype
        self._z = {}

    def _calls(self, path):
        if path not in self._z:
            if not os.path.exists(path):
                raise AssertionError("no recorded reference calls: %s" % os.path.relpath(path, GOLD))
            self._z[path] = np.load(path)
        return self._z[path]

    def _replay(self, name, args, kwargs):
        tid, key = _next_key(self.dtype)
        z = self._calls(_path(tid, TAGS[self.dtype]))
        n = key.rsplit("#", 1)[1]
        if key not in z:
            raise AssertionError("no recorded reference call %s #%s of %s" % (name, n, tid))
        meta = json.loads(str(z[key]))
        assert meta["name"] == name, (tid, meta["name"], name)
        assert meta["digest"] == _digest(name, args, kwargs), \
            "%s: the inputs of reference call %s #%s differ from the recorded ones" % (tid, name, n)
        arrs = _arrays((args, kwargs), [])
        for i, desc in meta["changed"]:
            np.copyto(arrs[i], _get(desc, z))
        return _decode(meta["ret"], z, arrs)

    def apply(self, fn, *args):
        return self._replay(fn.__name__, args, {})

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **kw: self._replay(name, a, kw)


def reference(dtype, replay=True):
    """The reference of precision `dtype` for a test: live, live and recording (CMFREC_REF_RECORD=1), or replayed (not with
    replay=False: the test is skipped instead)."""
    from oracle.bindings import Reference, ref_available
    dtype = np.dtype(dtype).type
    if ref_available(dtype):
        live = Reference(dtype)
        return _Recorder(live, dtype) if replay and os.environ.get("CMFREC_REF_RECORD") == "1" else _Live(live)
    if not replay:
        pytest.skip("checks a committed fixture against the live reference: needs oracle/_ref")
    if glob.glob(os.path.join(CALLS, "%s.*.npz" % _module(_test_id()))):
        return _Replay(dtype)
    pytest.skip("neither oracle/_ref nor recorded reference calls for this module")


class _Live:
    """The live reference with the stand-in's apply()."""
    def __init__(self, live):
        self._live = live

    def apply(self, fn, *args):
        return fn(self._live.lib, *args)

    def __getattr__(self, name):
        return getattr(self._live, name)

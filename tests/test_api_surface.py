"""The public surface of msm_webgpu_amd.api, pinned: every name of the module with its kind, and every attribute of its classes with its
signature and docstring.  tests/golden/api_surface.json is what `python tests/test_api_surface.py` printed before the scalar-field wrappers
left api.py; nothing may change, and what was added or went is listed below by name (ADDED, REPLACED).  inspect only: no library is loaded."""
import hashlib
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "api_surface.json")
CLASSES = ("MsmContext", "MultiGpuMsm", "FrLookup", "FrHash", "FrMatrix", "G1", "MsmHipError")
DUNDERS = ("__init__", "__enter__", "__exit__", "__del__", "__eq__")
# The differences from the golden file, one by one.  Added: the mixin that carries the scalar-field methods and its private helpers; the
# library name each handle class hands to the one base class; and FrMatrix now leaves a `with` block like the other two handles.
ADDED = {"ScalarFieldOps", "MsmContext._fr_call", "MsmContext._scalar_field", "MsmContext._mont256_flag", "MsmContext._new_out",
         "MsmContext._frhash_create", "MsmContext._frhash_out", "FrLookup._library", "FrHash._library", "FrMatrix._library",
         "FrMatrix.__enter__", "FrMatrix.__exit__"}
# Gone, all private: the loader's cache (it lives in _core, and a re-export would be a stale copy) and the helpers that the ones above replace
# (_scalar_field: _frvec_field and _frmle_field; _mont256_flag: the two _flags; scalars._const32 and scalars._pack_terms: the other three)
REPLACED = {"_lib", "MsmContext._frvec_field", "MsmContext._frmle_field", "MsmContext._frpoly_flags", "MsmContext._frmle_flags",
            "MsmContext._frpoly_const", "MsmContext._frmle_terms", "MsmContext._frgate_terms"}


def _kind(v):
    if inspect.isclass(v):
        return "class"
    if inspect.ismodule(v):
        return "module"
    if callable(v):
        return "function"
    return type(v).__name__


def _describe(v):
    if isinstance(v, (staticmethod, classmethod)):
        v = v.__func__
    if isinstance(v, property):
        return {"property": hashlib.sha256((v.__doc__ or "").encode()).hexdigest()}
    if callable(v):
        try:
            signature = str(inspect.signature(v))
        except ValueError:  # (a builtin that inspect cannot read, such as BaseException.with_traceback)
            signature = None
        return {"signature": signature, "doc": hashlib.sha256((v.__doc__ or "").encode()).hexdigest()}
    return {"repr": repr(v)}


def record():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from msm_webgpu_amd import api

    names = {n: _kind(v) for n, v in sorted(vars(api).items()) if not n.startswith("__")}
    classes = {}
    for cls in CLASSES:
        c, attrs = getattr(api, cls), {}
        for n in sorted(dir(c)):
            if n.startswith("__") and n not in DUNDERS:
                continue
            v = inspect.getattr_static(c, n)
            if n in DUNDERS and v in (getattr(object, n, None), getattr(BaseException, n, None)):
                continue  # (not the class's own: object's or BaseException's)
            attrs[n] = _describe(v)
        classes[cls] = attrs
    return {"names": names, "classes": classes}


def test_api_surface_is_the_recorded_one():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = record()
    gone = {n for n in want["names"] if n not in got["names"]}
    gone |= {"%s.%s" % (cls, n) for cls in CLASSES for n in want["classes"][cls] if n not in got["classes"][cls]}
    assert gone == REPLACED
    for n, kind in want["names"].items():
        assert n in gone or got["names"][n] == kind, n
    for cls, attrs in want["classes"].items():
        for n, d in attrs.items():
            assert "%s.%s" % (cls, n) in gone or got["classes"][cls][n] == d, "%s.%s" % (cls, n)
    extra = {n for n in got["names"] if n not in want["names"]}
    extra |= {"%s.%s" % (cls, n) for cls in CLASSES for n in got["classes"][cls] if n not in want["classes"][cls]}
    assert extra == ADDED


if __name__ == "__main__":
    print(json.dumps(record(), indent=1, sort_keys=True))

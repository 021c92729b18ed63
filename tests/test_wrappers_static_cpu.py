"""Static check of the tensor wrappers' launch sites (no library, no GPU).

``kernels._launch("lea_X", *args)`` names its entry point as a string, so nothing at import
time ties it to ``_lib.SIGNATURES`` the way an attribute access on the typed library did.  This
test restores that: it parses ``kernels.py`` and ``training.py`` and checks every launch-helper
call against the signature table, and that no launch goes round the helpers.

A *launch* is an entry point that takes a stream: it returns ``int`` and its last argument is a
pointer.  Everything else (sizes, kernel names, ``*_supported`` queries, tuning setters) is a
host-side query and may be called on the library directly.
"""
import ast
import ctypes
import os

import pytest

from leastereo_amd import _lib

PKG = os.path.dirname(os.path.abspath(_lib.__file__))
FILES = ("kernels.py", "training.py")
HELPERS = ("_launch", "_call")  # both append the current stream as the last argument

LAUNCHES = {name for name, (res, args) in _lib.SIGNATURES.items()
            if res is ctypes.c_int and args and args[-1] is ctypes.c_void_p}


def _calls(fname):
    """Every call in the file, but for the helpers' own bodies (where ``_launch`` forwards to ``_call``)."""
    with open(os.path.join(PKG, fname)) as f:
        tree = ast.parse(f.read(), fname)
    out, todo = [], [tree]
    while todo:
        node = todo.pop()
        if isinstance(node, ast.FunctionDef) and node.name in HELPERS:
            continue
        if isinstance(node, ast.Call):
            out.append(node)
        todo.extend(ast.iter_child_nodes(node))
    return out


def _helper_calls(fname):
    return [c for c in _calls(fname) if isinstance(c.func, ast.Name) and c.func.id in HELPERS]


def test_the_launch_set_is_what_it_should_be():
    """The rule that tells launches from queries picks the stream-taking entries and no other."""
    assert "lea_conv3d_bnrelu" in LAUNCHES and "lea_bn_backward_f32" in LAUNCHES
    for name in _lib.SIGNATURES:
        if name.endswith(("_supported", "_kernel_name", "_bytes", "_floats")) or "_set" in name:
            assert name not in LAUNCHES, name
    assert len(LAUNCHES) >= 60


@pytest.mark.parametrize("fname", FILES)
def test_helper_calls_match_the_signature_table(fname):
    calls = _helper_calls(fname)
    assert calls, fname
    for c in calls:
        where = f"{fname}:{c.lineno}"
        assert c.args and isinstance(c.args[0], ast.Constant) and isinstance(c.args[0].value, str), \
            f"{where}: the entry point must be a string literal"
        entry = c.args[0].value
        assert entry in LAUNCHES, f"{where}: {entry} is not a stream-taking entry of _lib.SIGNATURES"
        assert {k.arg for k in c.keywords} <= {"probe"}, where
        if any(isinstance(a, ast.Starred) for a in c.args):
            continue
        n_args = len(c.args)  # the name does not go to the library, the stream the helper appends does
        assert n_args == len(_lib.SIGNATURES[entry][1]), \
            f"{where}: {entry} takes {len(_lib.SIGNATURES[entry][1])} arguments, the call passes {n_args}"


def test_every_wrapper_module_launch_is_covered():
    """Sanity of the parse: the helpers reach most of the launches (the rest have no wrapper)."""
    seen = {c.args[0].value for f in FILES for c in _helper_calls(f)}
    assert len(seen) >= 60 and seen <= LAUNCHES


@pytest.mark.parametrize("fname", FILES)
def test_no_launch_goes_round_the_helper(fname):
    """No ``lib.lea_X(...)`` / ``_lib.load().lea_X(...)`` call of a launch outside the helpers."""
    for c in _calls(fname):
        if isinstance(c.func, ast.Attribute) and c.func.attr in LAUNCHES:
            raise AssertionError(f"{fname}:{c.lineno}: {c.func.attr} is launched without _launch")

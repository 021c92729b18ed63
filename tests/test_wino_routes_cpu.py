"""The f32 Winograd planner's answers, recorded from the commit before the route refactor
(tools/wino_routes.py -> tests/golden/wino_routes.json), recomputed from the built library: the
kernel names, the F(4,3) x F(4,3) geometry, the four down-sampling queries and the packed size of
360 shapes at the default settings, and a digest of that table under every single tuning value and
every pair of values of two different Winograd hooks.  Host queries only.

Hand corrections of the recording (a query that disagreed with the launch): none."""
import json
import os

import pytest

from leastereo_amd import _lib
from tools import wino_routes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino_routes.json")


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    return wino_routes.record(_lib.load())


def test_default_routes(want, got):
    assert len(wino_routes.SHAPES) == len(want["default"]) == 360
    assert not wino_routes.moved({**want, "single": {}, "pair": {}}, got)


@pytest.mark.parametrize("part", ["single", "pair"])
def test_routes_under_every_setting(want, got, part):
    assert set(got[part]) == set(want[part])
    assert [k for k in want[part] if want[part][k] != got[part][k]] == []


def test_sweep_left_the_hooks_as_found(want, got):
    assert wino_routes.table(_lib.load()) == [got["rows"][i] for i in got["default"]]

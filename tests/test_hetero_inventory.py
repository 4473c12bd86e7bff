"""tests/test_suite_inventory.py guards the GPU tests listed in tests/golden/gpu_test_names.txt against disappearing unnoticed
on a machine without a GPU.  The GPU tests of the per-filter inputs (tests/test_gpu_hetero.py) are listed in a file of their
own, tests/golden/gpu_hetero_test_names.txt, and held to the same check here, with the same parser, as
tests/test_body_inventory.py does for the body update's: every listed function still exists and is still marked gpu, and the
file has no test function that the list does not name.  The routes those functions are parametrised over come from
tests/hetero_cases.py, which needs no GPU either: their number is pinned here too."""
import os

from tests import hetero_cases as hc
from tests.test_suite_inventory import HERE, _test_functions

LIST = os.path.join(HERE, "golden", "gpu_hetero_test_names.txt")


def _listed():
    with open(LIST) as fh:
        return [ln.strip() for ln in fh if ln.strip() and not ln.startswith("#")]


def test_every_listed_hetero_gpu_test_still_exists():
    names = _listed()
    assert len(names) == len(set(names)) and len(names) >= 3
    found = _test_functions(os.path.join(HERE, "test_gpu_hetero.py"))
    for entry in names:
        path, _, func = entry.partition("::")
        assert path == "tests/test_gpu_hetero.py" and func, "malformed entry %r" % entry
        assert func in found, "listed GPU test no longer exists: %s" % entry
        assert found[func], "listed GPU test is no longer marked gpu: %s" % entry
    unlisted = sorted(set(found) - {e.partition("::")[2] for e in names})
    assert not unlisted, "tests/test_gpu_hetero.py has tests that tests/golden/gpu_hetero_test_names.txt does not list: %s" % unlisted


def test_the_number_of_routes():
    """25 resident routes (14 rows at nmax, 9 of them also at nmin, 2 also at N = 5), 9 streaming, 4 tile, 3 chunked"""
    assert (len(hc.resident_routes()), len(hc.STREAM_ROUTES), len(hc.TILE_ROUTES), len(hc.CHUNKED_ROUTES)) == (25, 9, 4, 3)
    ids = [r[0] for r in hc.resident_routes() + hc.STREAM_ROUTES + hc.TILE_ROUTES + hc.CHUNKED_ROUTES]
    assert len(ids) == len(set(ids))

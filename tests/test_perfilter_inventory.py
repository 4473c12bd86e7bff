"""tests/test_suite_inventory.py guards the GPU tests listed in tests/golden/gpu_test_names.txt against disappearing unnoticed
on a machine without a GPU.  The GPU tests of the per-filter parameter sets (tests/test_gpu_perfilter.py) are listed in a file
of their own, tests/golden/gpu_perfilter_test_names.txt, and held to the same check here, with the same parser, as
tests/test_body_inventory.py does for the body-sensor update's: every listed function still exists and is still marked gpu,
and the file has no test function that the list does not name."""
import os

from tests.test_suite_inventory import HERE, _test_functions

LIST = os.path.join(HERE, "golden", "gpu_perfilter_test_names.txt")


def _listed():
    with open(LIST) as fh:
        return [ln.strip() for ln in fh if ln.strip() and not ln.startswith("#")]


def test_every_listed_perfilter_gpu_test_still_exists():
    names = _listed()
    assert len(names) == len(set(names)) and len(names) >= 10
    found = _test_functions(os.path.join(HERE, "test_gpu_perfilter.py"))
    for entry in names:
        path, _, func = entry.partition("::")
        assert path == "tests/test_gpu_perfilter.py" and func, "malformed entry %r" % entry
        assert func in found, "listed GPU test no longer exists: %s" % entry
        assert found[func], "listed GPU test is no longer marked gpu: %s" % entry
    unlisted = sorted(set(found) - {e.partition("::")[2] for e in names})
    assert not unlisted, "tests/test_gpu_perfilter.py has tests that tests/golden/gpu_perfilter_test_names.txt does not list: %s" % unlisted

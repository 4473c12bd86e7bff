"""tests/test_suite_inventory.py guards the GPU tests listed in tests/golden/gpu_test_names.txt against disappearing unnoticed
on a machine without a GPU.  The GPU tests of the PIXEL_VEL measurement (tests/test_gpu_pixvel.py) and of the intake's
pixel-velocity step (tests/test_gpu_pixvel_intake.py) are listed in a file of their own, tests/golden/gpu_pixvel_test_names.txt,
and held to the same check here, with the same parser, as tests/test_depth_inventory.py does for the depth updates': every
listed function still exists and is still marked gpu, and the files have no test function that the list does not name."""
import os

from tests.test_suite_inventory import HERE, _test_functions

LIST = os.path.join(HERE, "golden", "gpu_pixvel_test_names.txt")
FILES = ("tests/test_gpu_pixvel.py", "tests/test_gpu_pixvel_intake.py")


def _listed():
    with open(LIST) as fh:
        return [ln.strip() for ln in fh if ln.strip() and not ln.startswith("#")]


def test_every_listed_pixvel_gpu_test_still_exists():
    names = _listed()
    assert len(names) == len(set(names)) and len(names) >= 16
    found = {f: _test_functions(os.path.join(HERE, os.path.basename(f))) for f in FILES}
    for entry in names:
        path, _, func = entry.partition("::")
        assert path in FILES and func, "malformed entry %r" % entry
        assert func in found[path], "listed GPU test no longer exists: %s" % entry
        assert found[path][func], "listed GPU test is no longer marked gpu: %s" % entry
    for f in FILES:
        unlisted = sorted(set(found[f]) - {e.partition("::")[2] for e in names if e.startswith(f + "::")})
        assert not unlisted, "%s has tests that tests/golden/gpu_pixvel_test_names.txt does not list: %s" % (f, unlisted)

"""The GPU tests cannot run on a CPU box, so one that disappears (renamed, deleted, dropped in a merge) would go unnoticed
there.  tests/golden/gpu_test_names.txt lists every `-m gpu` test function as `file::function`; this checks, by parsing the
test files with ast (no torch, no pytest collection), that each one still exists and is still marked gpu.  Removing a GPU
test therefore means editing the list, and the removal shows in review."""
import ast
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIST = os.path.join(HERE, "golden", "gpu_test_names.txt")


def _is_gpu_mark(node):
    """pytest.mark.gpu, with or without a call"""
    if isinstance(node, ast.Call):
        node = node.func
    return isinstance(node, ast.Attribute) and node.attr == "gpu" and isinstance(node.value, ast.Attribute) \
        and node.value.attr == "mark"


def _test_functions(path):
    """-> {name: marked gpu} for the module-level test functions of one file"""
    tree = ast.parse(open(path).read(), filename=path)
    module_gpu = False
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "pytestmark" for t in node.targets):
            marks = node.value.elts if isinstance(node.value, (ast.List, ast.Tuple)) else [node.value]
            module_gpu |= any(_is_gpu_mark(m) for m in marks)
    out = {}
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) and node.name.startswith("test"):
            out[node.name] = module_gpu or any(_is_gpu_mark(d) for d in node.decorator_list)
    return out


def _listed():
    with open(LIST) as fh:
        return [ln.strip() for ln in fh if ln.strip() and not ln.startswith("#")]


def test_every_listed_gpu_test_still_exists():
    names = _listed()
    assert len(names) == len(set(names)), "duplicate entries in %s" % LIST
    found = {}
    missing, unmarked = [], []
    for entry in names:
        path, _, func = entry.partition("::")
        assert path.startswith("tests/test_") and path.endswith(".py") and func, "malformed entry %r" % entry
        full = os.path.join(os.path.dirname(HERE), path)
        if not os.path.exists(full):
            missing.append(entry)
            continue
        if path not in found:
            found[path] = _test_functions(full)
        if func not in found[path]:
            missing.append(entry)
        elif not found[path][func]:
            unmarked.append(entry)
    assert not missing, "GPU tests listed in tests/golden/gpu_test_names.txt no longer exist: %s" % missing
    assert not unmarked, "listed GPU tests are no longer marked gpu: %s" % unmarked


def test_the_check_sees_the_files_it_parses():
    """the parser finds the module-level mark and a decorated function (guards the check itself against matching nothing)"""
    fs = _test_functions(os.path.join(HERE, "test_gpu_fullbatch.py"))
    assert fs.get("test_per_filter_ring_headline_batch_vs_oracle") is True
    fs = _test_functions(os.path.join(HERE, "test_oracle_structured.py"))
    assert fs.get("test_structured_equals_dense") is False

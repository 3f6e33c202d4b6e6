"""Every entry point of include/zfft.h that takes a `void *hip_stream` -- the calls that are
"enqueued on hip_stream; return without syncing" -- has an ordering case in test_gpu_ordering.py:
its table COVERED maps the entry point to the scenarios that call it.  A new device entry point
cannot land without one.  No GPU."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream_entry_points():
    with open(os.path.join(ROOT, "include", "zfft.h")) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    # a declaration: `int name(args);` with the arguments free of parentheses
    return [m.group(1) for m in re.finditer(r"\b(zfft_\w+)\s*\(([^()]*)\)\s*;", text)
            if re.search(r"\bvoid\s*\*\s*hip_stream\b", m.group(2))]


def covered_table():
    """COVERED of test_gpu_ordering.py, read from its source (importing it needs the references
    the GPU tests use) together with the names of its test functions."""
    with open(os.path.join(ROOT, "tests", "test_gpu_ordering.py")) as fh:
        tree = ast.parse(fh.read())
    table = None
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", "") == "COVERED" for t in node.targets):
            table = ast.literal_eval(node.value)
    tests = [n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")]
    return table, tests


def test_the_header_parse_finds_the_device_entry_points():
    names = stream_entry_points()
    assert len(names) == len(set(names)) >= 11
    assert "zfft_process_device" in names and "zfft_history_view_device" in names
    assert all(n.endswith("_device") for n in names), names


def test_every_device_entry_point_has_an_ordering_case():
    table, tests = covered_table()
    assert isinstance(table, dict)
    missing = [n for n in stream_entry_points() if not table.get(n)]
    assert not missing, f"no ordering scenario in tests/test_gpu_ordering.py COVERED for: {missing}"
    stale = sorted(set(table) - set(stream_entry_points()))
    assert not stale, f"COVERED names entry points the header does not declare: {stale}"


def test_every_scenario_named_in_the_table_is_a_test():
    """A scenario id is a test function's prefix: "a" -> test_a_..., "e_decay" -> test_e_decay_..."""
    table, tests = covered_table()
    for name, scenarios in table.items():
        for s in scenarios:
            assert any(t.startswith(f"test_{s}_") for t in tests), (name, s)


def test_every_scenario_calls_the_entry_points_it_is_listed_for():
    """The method of ZoomFFT that wraps the entry point appears in the source of the test module
    (the scenarios share their sequences, so the search is over the module)."""
    table, _ = covered_table()
    with open(os.path.join(ROOT, "tests", "test_gpu_ordering.py")) as fh:
        src = fh.read()
    for name in table:
        method = name[len("zfft_"):]
        assert re.search(rf"\bplan\.{method}\b", src), f"{name}: no plan.{method} call in test_gpu_ordering.py"

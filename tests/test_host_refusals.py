"""The host layer's argument checks refuse what they refused, with the message they gave, and return what they returned, at
the commit tests/golden/host_refusals.json was recorded from: the table tests/host_refusals.py, replayed and compared
exactly.  The file is the record of that commit (tools/record_host_refusals.py wrote it there); a wanted change of a check
is a change of the file, by hand, in the same commit."""
import json
import os

import host_refusals

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_refusals.json")


def test_the_table_replays_as_recorded():
    with open(GOLDEN) as f:
        recorded = json.load(f)["cases"]
    seen, differ = set(), []
    for case, function, kwargs in host_refusals.cases():
        assert case not in seen, "two cases are called %r" % case
        seen.add(case)
        now = host_refusals.describe(function, kwargs)
        if now != recorded.get(case):
            differ.append("%s\n    recorded %r\n    now      %r" % (case, recorded.get(case), now))
    assert not differ, "%d of %d cases differ:\n%s" % (len(differ), len(seen), "\n".join(differ[:20]))
    assert seen == set(recorded), "recorded but no longer in the table: %r" % sorted(set(recorded) - seen)[:20]


def test_every_refusal_is_a_value_error():
    with open(GOLDEN) as f:
        recorded = json.load(f)["cases"]
    refused = [v for v in recorded.values() if isinstance(v, str)]
    assert len(refused) > 300 and all(v.startswith("ValueError: ") for v in refused)


def test_the_checks_need_no_library():
    """_checks imports numpy and the standard library alone."""
    import ast
    from tls_amd import _checks
    with open(_checks.__file__) as f:
        tree = ast.parse(f.read())
    imported = {a.name for node in ast.walk(tree) if isinstance(node, ast.Import) for a in node.names}
    assert imported == {"numbers", "operator", "numpy"}
    assert not [node for node in ast.walk(tree) if isinstance(node, ast.ImportFrom)]

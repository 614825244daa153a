#!/usr/bin/env python
"""Run the case table tests/host_refusals.py and write tests/golden/host_refusals.json: what every case raises or returns.

    python tools/record_host_refusals.py COMMIT [--tree DIR] [--out FILE]

COMMIT is written into the file as the commit the record was taken from; --tree names the checkout of that commit whose
tls_amd is imported (default: this one).  The file pins the behaviour of that commit: it is recorded once, from the tree
before a change of the checks, and never from the changed tree.

It also prints every `raise ValueError` line of the functions in host_refusals.IN_SCOPE that no case reached (found with ast,
executed lines noted with sys.settrace): a refusal the table does not pin."""
import argparse
import ast
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def raise_lines(path, names):
    """{line: function} of the `raise ValueError` statements inside the functions `names` of the file."""
    with open(path) as f:
        tree = ast.parse(f.read())
    lines = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name in names:
            for sub in ast.walk(node):
                if isinstance(sub, ast.Raise) and isinstance(sub.exc, ast.Call) and getattr(sub.exc.func, "id", "") == "ValueError":
                    lines[sub.lineno] = node.name
    return lines


def main():
    p = argparse.ArgumentParser()
    p.add_argument("commit")
    p.add_argument("--tree", default=REPO)
    p.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "host_refusals.json"))
    args = p.parse_args()
    sys.path[:0] = [os.path.abspath(args.tree), os.path.join(REPO, "tests")]
    import host_refusals
    import tls_amd
    modules = {k: os.path.join(os.path.dirname(os.path.abspath(tls_amd.__file__)), k + ".py") for k in host_refusals.IN_SCOPE}
    wanted = {path: raise_lines(path, host_refusals.IN_SCOPE[k]) for k, path in modules.items()}
    seen = set()

    def tracer(frame, event, arg):
        if frame.f_code.co_filename not in wanted:
            return None
        if event == "line":
            seen.add((frame.f_code.co_filename, frame.f_lineno))
        return tracer

    record = {}
    sys.settrace(tracer)
    try:
        for case, function, kwargs in host_refusals.cases():
            assert case not in record, case
            record[case] = host_refusals.describe(function, kwargs)
    finally:
        sys.settrace(None)
    with open(args.out, "w") as f:
        f.write('{"commit": %s, "cases": {\n' % json.dumps(args.commit))     # (one line a case)
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(record[k], sort_keys=True)) for k in sorted(record)))
        f.write("\n}}\n")
    missed = [(path, line, name) for path, lines in sorted(wanted.items()) for line, name in sorted(lines.items())
              if (path, line) not in seen]
    refused = [k for k, v in record.items() if isinstance(v, str)]
    odd = [k for k in refused if not record[k].startswith("ValueError: ")]
    print("%d cases, %d refused, %d bytes" % (len(record), len(refused), os.path.getsize(args.out)))
    print("%d of %d `raise ValueError` lines not reached" % (len(missed), sum(len(v) for v in wanted.values())))
    for path, line, name in missed:
        print("  %s:%d (%s)" % (os.path.relpath(path, os.path.abspath(args.tree)), line, name))
    for k in odd:
        print("  not a ValueError: %s: %s" % (k, record[k]))
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
